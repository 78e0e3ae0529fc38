"""The accumulator's noise estimate and passes over a subset of its tiles on the GPU (hrt.Accumulator(noise=True),
hrt_accum_noise, hrt_accum_add_tiles): the bit contract of include/hrt/hrt.h.

The device arithmetic equals the host's; the error map meets an f64 evaluation of the oracle's chunk sums; keeping
the noise plane changes no frame; a tile's pixels and errors depend on that tile's passes alone; refine ends where
the policy says; merge keeps the plane's bits; and errors change nothing.

Inputs: A = `random` (scene seed 1, render seed 7) at 64x36 in 16-px tiles: 12 tiles, the top row 4 px high (ragged
tiles, tiles of fewer than 256 px); B = `cornell` at 32x32 in 16-px tiles (the general chunk class)."""
import numpy as np
import pytest

import hrt
from oracle import oracle as O

TOL = 1e-3   # the project's bar (tests/test_gpu_parity.py), here absolute plus relative
SEED = 7
FLOOR = 0.05
F = np.float32
INPUTS = {"A": ("random", 64, 36), "B": ("cornell", 32, 32)}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    def get(name):
        if name not in _scenes:
            s = hrt.preset(name, 1, earth)
            s.commit()
            _scenes[name] = s
        return _scenes[name]

    yield get
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def setup(s, w, h, spp, offset=0, flags=0, seed=SEED):
    cam = hrt.preset_camera(s.info, w, h)
    return cam, hrt.params(w, h, spp, 50, seed, tuple(s.info.background), sample_offset=offset, flags=flags)


def accumulator(s, w, h, ranges, noise=True, tiles="grid", flags=0):
    """An accumulator over the 16-px tile grid holding the given [begin, end) passes, added in that order."""
    a = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16) if tiles == "grid" else tiles, noise=noise)
    for b, e in ranges:
        a.add(*setup(s, w, h, e - b, offset=b, flags=flags))
    return a


def tile_spans(a):
    """[(first pixel, pixels)] of every tile in the packed order."""
    out, off = [], 0
    for _, _, tw, th in a.tiles:
        out.append((off, tw * th))
        off += tw * th
    return out


def chunk_sizes(sched):
    c = sched["chunk"]
    return [sched["first"]] + [c] * (sched["head"] - 1) + [c >> (1 + (j >> 1)) for j in range(sched["tail"])]


# ------------------------------------------------------------------------------------------ 1. device against host
SIZES = {1: [16], 2: [8, 32], 3: [8, 16, 16], 11: [8, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]}


@pytest.mark.gpu
@pytest.mark.parametrize("n_chunks", [1, 2, 3, 11])
@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 6400])
def test_device_noise_equals_host(n_chunks, n):
    rng = np.random.default_rng(100 * n + n_chunks)
    state = {False: (np.zeros((n, 4), F), np.zeros(n, F)), True: (np.zeros((n, 4), F), np.zeros(n, F))}
    N = K = 0
    for sizes, scale in ((SIZES[n_chunks], 1.0), (SIZES[3], 0.5)):   # the second pass: the moment is one addend
        p = np.zeros((len(sizes), n, 4), F)
        for c, nc in enumerate(sizes):
            p[c, :, :3] = (rng.uniform(0.0, 1.0, (n, 3)) * scale * nc).astype(F)
        p[:, 0, :3] = 0   # a black pixel
        N, K = N + sum(sizes), K + len(sizes)
        got = {}
        for dev in (False, True):
            got[dev] = hrt.debug_noise(p, sizes, state[dev][0], state[dev][1], N, K, FLOOR, on_device=dev)
            state[dev] = got[dev][:2]
        for h, d in zip(got[False], got[True]):
            assert np.array_equal(u32(np.asarray(d, F)), u32(np.asarray(h, F)))
        if K < 2:
            assert np.isinf(got[True][2]).all() and np.isinf(got[True][3]) and np.isinf(got[True][4])
        else:
            assert got[True][2][0] == 0 and np.isfinite(got[True][2]).all()


@pytest.mark.gpu
def test_device_noise_equals_host_beyond_one_grid():
    """More pixels than the accumulate kernel's 4096 x 256 lanes: the second trip of its grid-stride loop, and 4097
    trips of accum_noise's per-thread fold."""
    n, sizes = 4096 * 256 + 3, SIZES[3]
    rng = np.random.default_rng(5)
    p = np.zeros((3, n, 4), F)
    for c, nc in enumerate(sizes):
        p[c, :, :3] = (rng.uniform(0.0, 1.0, (n, 3)) * nc).astype(F)
    zero, zero_m = np.zeros((n, 4), F), np.zeros(n, F)
    host = hrt.debug_noise(p, sizes, zero, zero_m, 40, 3, FLOOR, on_device=False)
    dev = hrt.debug_noise(p, sizes, zero, zero_m, 40, 3, FLOOR, on_device=True)
    for h, d in zip(host, dev):
        assert np.array_equal(u32(np.asarray(d, F)), u32(np.asarray(h, F)))
    assert np.isfinite(dev[2]).all() and dev[2][-1] > 0


# ------------------------------------------------------------------------------------------ 2. against the oracle
PASSES = {"A": [(0, 40), (40, 110), (110, 126)], "B": [(0, 40), (40, 110)]}


def oracle_statistic(s, name, w, h, passes, earth, a):
    """The statistic in f64 from the oracle's chunk sums, packed as the accumulator's tiles are: every chunk of every
    pass is one oracle render of its samples, and its sum is rgb^2 * n_c."""
    osc = O.OracleScene(hrt.PRESETS[name], 1, earth)
    Y, m2, K = np.zeros((h, w)), np.zeros((h, w)), 0
    for b, e in passes:
        at = b
        for nc in chunk_sizes(hrt.sample_chunks(s, setup(s, w, h, e - b, offset=b)[1])):
            rgb, _ = osc.render(w, h, nc, 50, seed=SEED, sample_offset=at)
            yc = (rgb[..., :3].astype(np.float64) ** 2 * nc).sum(axis=2)
            Y, m2, K, at = Y + yc, m2 + yc * yc / nc, K + 1, at + nc
        assert at == e
    N = passes[-1][1]
    var = np.maximum((m2 - Y * Y / N) / (K - 1), 0)
    err = np.sqrt(var / N) / np.maximum(Y / N, FLOOR)
    packed = np.concatenate([err[y:y + th, x:x + tw].reshape(-1) for x, y, tw, th in a.tiles])
    return packed, N, K


@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
def test_noise_against_oracle(scene, earth, inp):
    """Measured on an MI355X, largest |gpu - oracle f64|:
      A: error map 8.9e-5 (on a sky pixel whose true error is 9.5e-9), 2.4e-4 relative where err > 1e-3;
         tile means 4.9e-5, tile maxima 1.2e-7;
      B: error map 3.9e-6, 7.5e-4 relative where err > 1e-3; tile means 3.0e-8, tile maxima 6.7e-9.
    The absolute figure is the f32 rounding floor of m2 - Y^2 / N (csrc/accum.h), not a difference in the paths."""
    name, w, h = INPUTS[inp]
    s = scene(name)
    a = accumulator(s, w, h, PASSES[inp])
    rec, err = a.noise(FLOOR, error_map=True)
    ref, N, K = oracle_statistic(s, name, w, h, PASSES[inp], earth, a)
    assert err.shape == ref.shape and np.isfinite(err).all()
    d = np.abs(err - ref)
    worst = int(np.argmax(d))
    print(f"\n{inp}: error map max |gpu - oracle| = {d.max():.3e} at err {ref[worst]:.3e}; "
          f"max relative where err > 1e-3 = {(d / np.maximum(ref, 1e-30))[ref > 1e-3].max():.3e}")
    assert (d <= TOL + TOL * np.abs(ref)).all(), f"{inp}: {d.max()}"
    dm = dx = 0.0
    for (off, n), r in zip(tile_spans(a), rec):
        assert r.samples == N and r.chunks == K
        mean, mx = ref[off:off + n].mean(), ref[off:off + n].max()
        dm, dx = max(dm, abs(r.mean - mean)), max(dx, abs(r.max - mx))
        assert abs(r.mean - mean) <= TOL + TOL * mean and abs(r.max - mx) <= TOL + TOL * mx
        assert r.max == err[off:off + n].max()
    print(f"{inp}: tile mean max diff {dm:.3e}, tile max max diff {dx:.3e}")
    a.close()


# ------------------------------------------------------------------------------------------ 3. no side effect
@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
def test_noise_plane_changes_no_frame(scene, inp):
    name, w, h = INPUTS[inp]
    s = scene(name)
    with_plane, plain = accumulator(s, w, h, PASSES[inp]), accumulator(s, w, h, PASSES[inp], noise=False)
    assert with_plane.samples == plain.samples == PASSES[inp][-1][1]
    assert np.array_equal(u32(with_plane.download()[0]), u32(plain.download()[0]))
    assert with_plane.download()[1] == plain.download()[1]
    for fmt in ("f32", "rgba8"):
        assert np.array_equal(with_plane.resolve(fmt).view(np.uint8), plain.resolve(fmt).view(np.uint8))
    # one pass into a whole-frame accumulator equals hrt.render, and so does its fused preview
    cam, p = setup(s, w, h, 40)
    one = hrt.Accumulator(s, w, h, noise=True)
    pre = one.add(cam, p, preview=True)
    ref = hrt.render(s, cam, p)
    assert np.array_equal(u32(one.resolve()), u32(ref)) and np.array_equal(u32(pre), u32(ref))
    for x in (with_plane, plain, one):
        x.close()


# ------------------------------------------------------------------------------------------ 4. subset passes
@pytest.mark.gpu
@pytest.mark.parametrize("inp,subset,flags", [("A", [1, 4, 11], 0), ("A", [11, 1, 4], hrt.RENDER_NO_LDS), ("B", [1, 3], 0)])
def test_subset_pass_touches_its_tiles_alone(scene, inp, subset, flags):
    name, w, h = INPUTS[inp]
    s = scene(name)
    first = accumulator(s, w, h, [(0, 40)], flags=flags)
    both = accumulator(s, w, h, [(0, 40), (40, 80)], flags=flags)
    sub = accumulator(s, w, h, [(0, 40)], flags=flags)
    st = sub.add(*setup(s, w, h, 40, offset=40, flags=flags), stats=True, tiles=subset)
    spans = tile_spans(sub)
    assert st.pixels == sum(spans[t][1] for t in subset) and st.samples == 40 * st.pixels
    assert sub.tile_samples == [80 if t in subset else 40 for t in range(len(spans))]
    with pytest.raises(hrt.HrtError) as e:
        sub.samples
    assert e.value.status == hrt.ERR_STATE
    px, m2 = sub.resolve(), sub.moments()
    rec, err = sub.noise(FLOOR, error_map=True)
    want = {True: (both.resolve(), both.moments()) + both.noise(FLOOR, error_map=True),
            False: (first.resolve(), first.moments()) + first.noise(FLOOR, error_map=True)}
    for t, (off, n) in enumerate(spans):
        wpx, wm2, wrec, werr = want[t in subset]
        sl = slice(off, off + n)
        assert np.array_equal(u32(px[sl]), u32(wpx[sl])), t
        assert np.array_equal(u32(m2[sl]), u32(wm2[sl])), t
        assert np.array_equal(u32(err[sl]), u32(werr[sl])), t
        assert u32(F(rec[t].mean)) == u32(F(wrec[t].mean)) and u32(F(rec[t].max)) == u32(F(wrec[t].max))
        assert (rec[t].samples, rec[t].chunks) == (wrec[t].samples, wrec[t].chunks)
    # the remaining tiles catch up: the accumulator is an ordinary one again, with the bits of `both`
    rest = [t for t in range(len(spans)) if t not in subset]
    sub.add(*setup(s, w, h, 40, offset=40, flags=flags), tiles=rest)
    assert sub.samples == 80
    assert np.array_equal(u32(sub.download()[0]), u32(both.download()[0]))
    assert np.array_equal(u32(sub.moments()), u32(both.moments()))
    # a plain accumulator takes subset passes too
    plain = accumulator(s, w, h, [(0, 40)], noise=False, flags=flags)
    plain.add(*setup(s, w, h, 40, offset=40, flags=flags), tiles=subset)
    assert np.array_equal(u32(plain.resolve()), u32(px))
    for x in (first, both, sub, plain):
        x.close()


# ------------------------------------------------------------------------------------------ 5. refine
@pytest.mark.gpu
def test_refine(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    cam, p = setup(s, w, h, 1)
    runs = []
    for _ in range(2):
        a = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16), noise=True)
        log = []
        rec = a.refine(cam, p, target=0.05, pass_spp=40, max_spp=400, floor=FLOOR, on_pass=lambda t, r: log.append(list(t)))
        runs.append((a, rec, log))
    a, rec, log = runs[0]
    held = a.tile_samples
    print(f"\nrefine: samples per tile {held}, {len(log)} passes, tile means {[round(r.mean, 4) for r in rec]}")
    assert all(r.mean <= 0.05 for r in rec) and max(held) < 400
    assert held == [r.samples for r in rec] and all(n % 40 == 0 for n in held)
    assert min(held) == 40 and max(held) >= 120
    assert log[0] == list(range(12)) and all(set(y) <= set(x) for x, y in zip(log, log[1:]))
    assert sum(len(t) for t in log) * 40 == sum(held)
    # a second run: identical bits
    b = runs[1][0]
    assert b.tile_samples == held
    px, err = a.resolve(), a.noise(FLOOR, error_map=True)[1]
    assert np.array_equal(u32(px), u32(b.resolve()))
    assert np.array_equal(u32(err), u32(b.noise(FLOOR, error_map=True)[1]))
    assert np.array_equal(u32(a.moments()), u32(b.moments()))
    # each tile's pixels are those of a uniform accumulator given that tile's pass schedule
    spans = tile_spans(a)
    for n in sorted(set(held)):
        uni = accumulator(s, w, h, [(k, k + 40) for k in range(0, n, 40)])
        upx, uerr = uni.resolve(), uni.noise(FLOOR, error_map=True)[1]
        for t, (off, cnt) in enumerate(spans):
            if held[t] == n:
                assert np.array_equal(u32(px[off:off + cnt]), u32(upx[off:off + cnt])), (n, t)
                assert np.array_equal(u32(err[off:off + cnt]), u32(uerr[off:off + cnt])), (n, t)
        uni.close()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------ 6. merge
@pytest.mark.gpu
def test_merge_adds_the_plane_and_the_chunks(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    lo, hi = accumulator(s, w, h, [(0, 40)]), accumulator(s, w, h, [(40, 80)])
    both = accumulator(s, w, h, [(0, 40), (40, 80)])
    lo.merge(hi)
    assert lo.samples == 80 and lo.download()[1] == [(0, 80)]
    assert np.array_equal(u32(lo.download()[0]), u32(both.download()[0]))
    assert np.array_equal(u32(lo.moments()), u32(both.moments()))
    ra, ea = lo.noise(FLOOR, error_map=True)
    rb, eb = both.noise(FLOOR, error_map=True)
    assert [(r.samples, r.chunks) for r in ra] == [(r.samples, r.chunks) for r in rb] == [(80, 6)] * 12
    assert np.array_equal(u32(ea), u32(eb))
    for x in (lo, hi, both):
        x.close()


# ------------------------------------------------------------------------------------------ 7. device errors
def _raises(status, fn):
    with pytest.raises(hrt.HrtError) as e:
        fn()
    assert e.value.status == status, e.value


@pytest.mark.gpu
def test_errors_change_nothing(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    a = accumulator(s, w, h, [(0, 40)])
    plain = accumulator(s, w, h, [(40, 80)], noise=False)
    sums, held = a.download()
    m2 = a.moments()

    def unchanged():
        got, ranges = a.download()
        assert ranges == held == [(0, 40)] and a.samples == 40 and a.tile_samples == [40] * 12
        assert np.array_equal(u32(got), u32(sums)) and np.array_equal(u32(a.moments()), u32(m2))

    nxt = setup(s, w, h, 40, offset=40)
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*nxt, tiles=[]))              # n == 0
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*nxt, tiles=[0, 12]))         # out of range
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*nxt, tiles=[1, 2, 1]))       # given twice
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*setup(s, w, h, 40, offset=20), tiles=[1]))   # [20, 60) overlaps
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*setup(s, w, h, 40, offset=40, seed=SEED + 1), tiles=[1]))  # identity
    unchanged()
    for floor in (0.0, -0.05, float("nan")):
        _raises(hrt.ERR_INVALID_ARG, lambda: a.noise(floor))
    _raises(hrt.ERR_STATE, lambda: plain.noise(FLOOR))                       # created without the plane
    _raises(hrt.ERR_STATE, lambda: plain.moments())
    empty = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16), noise=True)
    _raises(hrt.ERR_STATE, lambda: empty.noise(FLOOR))                       # no samples
    _raises(hrt.ERR_INVALID_ARG, lambda: a.merge(plain))                     # NOISE with non-NOISE, both ways
    _raises(hrt.ERR_INVALID_ARG, lambda: plain.merge(a))
    _raises(hrt.ERR_UNSUPPORTED, lambda: a.upload(*nxt, plain.download()[0], [(40, 80)]))
    _raises(hrt.ERR_UNSUPPORTED, lambda: empty.upload(*nxt, sums, held))
    unchanged()
    assert plain.download()[1] == [(40, 80)]

    # tiles that hold different passes
    a.add(*nxt, tiles=[1])
    want = [80 if t == 1 else 40 for t in range(12)]
    px, m2b = a.resolve(), a.moments()

    def unchanged_adaptive():
        assert a.tile_samples == want
        assert np.array_equal(u32(a.resolve()), u32(px)) and np.array_equal(u32(a.moments()), u32(m2b))

    _raises(hrt.ERR_STATE, lambda: a.samples)
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*setup(s, w, h, 40, offset=60)))             # [60, 100) overlaps tile 1's
    _raises(hrt.ERR_INVALID_ARG, lambda: a.add(*nxt, tiles=[0, 1]))                          # ... of ANY selected tile
    _raises(hrt.ERR_UNSUPPORTED, lambda: a.add(*setup(s, w, h, 40, offset=80), preview=True))
    other = accumulator(s, w, h, [(200, 240)])
    _raises(hrt.ERR_UNSUPPORTED, lambda: a.merge(other))
    _raises(hrt.ERR_UNSUPPORTED, lambda: other.merge(a))
    _raises(hrt.ERR_UNSUPPORTED, lambda: a.download())
    assert other.download()[1] == [(200, 240)]
    unchanged_adaptive()
    a.add(*setup(s, w, h, 40, offset=80))                                                    # allowed: every tile is free there
    assert a.tile_samples == [n + 40 for n in want]
    rec = a.noise(FLOOR)
    assert [r.chunks for r in rec] == [9 if t == 1 else 6 for t in range(12)]
    # reset clears the plane, the chunks and the per-tile ranges
    a.reset()
    assert a.samples == 0 and a.tile_samples == [0] * 12 and not a.moments().any() and not a.download()[0].any()
    _raises(hrt.ERR_STATE, lambda: a.noise(FLOOR))
    a.add(*setup(s, w, h, 16))
    assert [(r.samples, r.chunks) for r in a.noise(FLOOR)] == [(16, 1)] * 12
    assert all(np.isinf(r.mean) and np.isinf(r.max) for r in a.noise(FLOOR))
    for x in (a, plain, empty, other):
        x.close()
