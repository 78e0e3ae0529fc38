"""The filtered noise estimate on the GPU (hrt_accum_noise_filtered, Accumulator.noise_filtered / refine_filtered;
include/hrt/hrt.h, "noise estimate of the FILTERED frame"): the kernels against the host's arithmetic; the public call
against the numpy restatement (tests/noise_filtered_restated.py) from the state a snapshot and features() give, bit for
bit; the tile cut; the frame it describes; that it writes nothing; hrt_accum_noise's unchanged reduction; refusals; and
the refinement loop.

Inputs: A = `random` (scene seed 1, render seed 7) at 64x36, 126 spp in three 42-spp passes, in 16-px tiles (12 tiles, the
top row 4 px high) or one tile; B = `cornell` at 32x32, 110 spp in two passes, in 16-px tiles (4) or one tile.  The mixed
states give two tiles one further pass."""
import ctypes
import struct

import numpy as np
import pytest

import filter_restated as FR
import guided_restated as GR
import hrt
import noise_filtered_restated as NF

SEED = 7
FLOOR = 0.05
DEMOD_FLOOR = 0.01
F = np.float32
INPUTS = {"A": ("random", 64, 36, 42, 3), "B": ("cornell", 32, 32, 55, 2)}   # scene, width, height, pass spp, passes
EXTRA = {"A": [1, 6], "B": [0, 3]}                                             # the tiles of the mixed state's extra pass
TOL = dict(normal=0.1, albedo=0.1, depth=0.1)
SETTINGS = {"variance": dict(), "guided": dict(guide=TOL), "demodulated": dict(guide=hrt.DEMOD_DEFAULTS, demodulate=DEMOD_FLOOR)}


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


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


def setup(s, w, h, spp, offset=0):
    cam = hrt.preset_camera(s.info, w, h)
    return cam, hrt.params(w, h, spp, 50, SEED, tuple(s.info.background), sample_offset=offset)


def build(get, inp, cut="grid", mixed=False, features=True):
    name, w, h, spp, passes = INPUTS[inp]
    s = get(name)
    a = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16) if cut == "grid" else None, noise=True, features=features)
    for k in range(passes):
        a.add(*setup(s, w, h, spp, offset=spp * k))
    if mixed:
        a.add(*setup(s, w, h, spp, offset=spp * passes), tiles=EXTRA[inp])
    if features:
        a.add_features(*setup(s, w, h, 8))
    return a


_states = {}


@pytest.fixture(scope="module")
def states(scene):
    """The accumulators of this module, built once: states(inp, cut, mixed)."""
    def get(inp, cut="grid", mixed=False):
        key = (inp, cut, mixed)
        if key not in _states:
            _states[key] = build(scene, inp, cut, mixed)
        return _states[key]

    yield get
    for a in _states.values():
        a.close()
    _states.clear()


def snapshot_planes(blob):
    """(sums (n_pixels, 4), m2 (n_pixels,)) of a snapshot, by the layout of include/hrt/hrt.h."""
    flags, _, _, n_tiles = struct.unpack_from("<4I", blob, 16)
    (n_px,) = struct.unpack_from("<Q", blob, 32)
    _, n_records, n_f, _ = struct.unpack_from("<4I", blob, 40)
    at = 184 + 16 * n_tiles
    for _ in range(n_records):
        at += 16 + 16 * struct.unpack_from("<2Q", blob, at)[1]
    at = (at + 16 * n_f + 15) & ~15
    sums = np.frombuffer(blob, F, 4 * n_px, at).reshape(n_px, 4)
    assert flags & hrt.ACCUM_NOISE
    return sums, np.frombuffer(blob, F, n_px, at + 16 * n_px)


def state_of(a):
    """What the restatement starts from: the snapshot's sums and m2, the tiles' scales and the mean feature planes."""
    sums, m2 = snapshot_planes(a.snapshot())
    scales = [FR.tile_scales(r.samples, r.chunks) for r in a.noise(FLOOR)]
    al, no = a.features()
    return sums, m2, scales, al.reshape(-1, 4), no.reshape(-1, 4)


def restated(a, setting, it=3, sigma=4.0, floor=FLOOR):
    sums, m2, scales, al, no = state_of(a)
    kw = SETTINGS[setting]
    return NF.accumulator_noise_filtered(sums, m2, a.tiles, scales, al, no, a.width, a.height, it, sigma, floor, tol=kw.get("guide"),
                                         demod_floor=kw.get("demodulate"))


def unpack(a, px):
    plane = np.zeros((a.height, a.width), px.dtype)
    off = 0
    for x, y, tw, th in a.tiles:
        plane[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw)
        off += tw * th
    return plane


def pass_chunks(s, w, h, spp, offset):
    """The chunks one pass adds to K, from the schedule hrt_debug_sample_chunks gives for it."""
    sc = hrt.sample_chunks(s, setup(s, w, h, spp, offset)[1])
    return 1 + (sc["head"] - 1) + sc["tail"]


@pytest.mark.gpu
def test_the_inputs_hold_two_chunks_per_tile(scene, states):
    """K of every tile is the sum of its passes' chunks (hrt_debug_sample_chunks), and at least 2."""
    for inp, (name, w, h, spp, passes) in INPUTS.items():
        k = [pass_chunks(scene(name), w, h, spp, spp * i) for i in range(passes + 1)]
        a = states(inp, "grid", True)
        for t, r in enumerate(a.noise(FLOOR)):
            assert r.chunks == sum(k[:passes + (t in EXTRA[inp])]) >= 2, (inp, t)


# ------------------------------------------------------------------------------------------ 4. device against host
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["37x23", "1xN", "Nx1", "257"])
def test_device_equals_host(case):
    """The last-iteration kernels (staged steps 1, 2, 4 and the global steps 8, 16 as the LAST iteration) and the reduce
    kernel against the host's arithmetic on the rasters of tests/test_noise_filtered_host.py: err plane and mean / max."""
    import test_noise_filtered_host as TH

    w, h, tiles = TH.CASES[case]
    r, a, n = TH.rasters(w, h, tiles)
    for it in (1, 2, 3, 4, 5):
        for k in (dict(), TH.ALL, dict(ka=10.0)):
            for demod in (False, DEMOD_FLOOR):
                host = hrt.debug_noise_filtered(r, a, n, it, 4.0, tiles, demodulate=demod, floor=FLOOR, **k)
                dev = hrt.debug_noise_filtered(r, a, n, it, 4.0, tiles, demodulate=demod, floor=FLOOR, on_device=True, **k)
                assert np.array_equal(u32(dev[0]), u32(host[0])), (case, it, k, demod)
                assert np.array_equal(u32(dev[1]), u32(host[1])), (case, it, k, demod)


@pytest.mark.gpu
def test_staging_variants_are_bit_identical(monkeypatch):
    """The staging knobs reach the err kernels too: features from global memory, and nothing staged."""
    import test_noise_filtered_host as TH

    w, h, tiles = TH.CASES["37x23"]
    r, a, n = TH.rasters(w, h, tiles)
    for demod in (False, DEMOD_FLOOR):
        want = hrt.debug_noise_filtered(r, a, n, 3, 4.0, tiles, demodulate=demod, **TH.ALL)
        for knob, v in (("HRT_GUIDED_LDS_STEP", "0"), ("HRT_GUIDED_LDS_STEP", "2"), ("HRT_FILTER_LDS_STEP", "0")):
            monkeypatch.setenv(knob, v)
            got = hrt.debug_noise_filtered(r, a, n, 3, 4.0, tiles, demodulate=demod, on_device=True, **TH.ALL)
            assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1])), (knob, v)
            monkeypatch.delenv(knob)


# ------------------------------------------------------------------------------------------ 5. the public call
@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed"])
def test_public_call_equals_the_restatement(states, inp, mixed):
    a = states(inp, "grid", mixed)
    held = a.noise(FLOOR)
    assert all(r.chunks >= 2 for r in held) and (len({r.samples for r in held}) == 2) == mixed
    for setting, kw in SETTINGS.items():
        rec, err = a.noise_filtered(FLOOR, error_map=True, **kw)
        want_err, want_mm = restated(a, setting)
        assert err.dtype == F and err.shape == (a.n_pixels,)
        assert np.array_equal(u32(err), u32(want_err)), (inp, mixed, setting)
        assert np.array_equal(u32([[r.mean, r.max] for r in rec]), u32(want_mm)), (inp, mixed, setting)
        assert [(r.samples, r.chunks) for r in rec] == [(r.samples, r.chunks) for r in held]
        # without an error map the records are the same (the accumulator's own plane)
        assert [(r.mean, r.max, r.samples, r.chunks) for r in a.noise_filtered(FLOOR, **kw)] == \
               [(r.mean, r.max, r.samples, r.chunks) for r in rec]
    # 1 and 5 iterations, another sigma and floor
    for it, sigma, floor, setting in ((1, 4.0, 0.05, "guided"), (5, 2.0, 0.2, "variance"), (4, 4.0, 0.01, "demodulated")):
        rec, err = a.noise_filtered(floor, denoise=dict(iterations=it, sigma=sigma), error_map=True, **SETTINGS[setting])
        want_err, want_mm = restated(a, setting, it, sigma, floor)
        assert np.array_equal(u32(err), u32(want_err)) and np.array_equal(u32([[r.mean, r.max] for r in rec]), u32(want_mm)), (it, setting)
    # the estimates differ from each other and from the raw one
    raw = a.noise(FLOOR, error_map=True)[1]
    var = a.noise_filtered(FLOOR, error_map=True)[1]
    assert not np.array_equal(var, raw) and not np.array_equal(var, a.noise_filtered(FLOOR, guide=TOL, error_map=True)[1])


@pytest.mark.gpu
def test_a_noise_only_accumulator_is_accepted_with_every_term_off(scene, states):
    """hrt_accum_resolve_guided_ex refuses an accumulator without HRT_ACCUM_FEATURES even at all-zero tolerances; the
    estimate of the variance-only frame needs none, and is the one a features accumulator gives."""
    a = build(scene, "A", features=False)
    with pytest.raises(hrt.HrtError) as e:
        a.resolve_guided(guide=dict(normal=0, albedo=0, depth=0))
    assert e.value.status == hrt.ERR_STATE
    rec, err = a.noise_filtered(FLOOR, error_map=True)
    want = states("A").noise_filtered(FLOOR, error_map=True)
    assert np.array_equal(u32(err), u32(want[1])) and [r.mean for r in rec] == [r.mean for r in want[0]]
    a.close()


# ------------------------------------------------------------------------------------------ 6. the tile cut
@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
def test_per_pixel_err_does_not_depend_on_the_tile_cut(states, inp):
    tiled, whole = states(inp, "grid"), states(inp, "one")
    assert len(tiled.tiles) == (12 if inp == "A" else 4) and len(whole.tiles) == 1
    for setting, kw in SETTINGS.items():
        et = tiled.noise_filtered(FLOOR, error_map=True, **kw)[1]
        rec, ew = whole.noise_filtered(FLOOR, error_map=True, **kw)
        assert np.array_equal(u32(unpack(tiled, et)), u32(ew.reshape(whole.height, whole.width))), (inp, setting)
        assert np.array_equal(u32([rec[0].mean, rec[0].max]), u32(NF.tile_reduce(ew)))


# ------------------------------------------------------------------------------------------ 7. the frame it describes
@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
def test_the_estimate_describes_the_frame_that_is_shown(states, inp):
    """The frame of resolve_guided is sqrtf(c') per channel.  Squared it gives c' back only up to the squaring's rounding,
    so BOTH cases apply: on the pixels where the square of every channel IS c' (checked against hrt_debug_guided's c' on
    the same state) err is sqrtf(v') / at_least(l', floor) with l' from the squared frame, to the last bit; elsewhere it
    agrees to the relative deviation of the squared frame's l' from c''s, which is measured here with the numpy
    restatement's c' on the CPU, plus the two roundings of the quotient (2^-23)."""
    a = states(inp, "grid", True)
    sums, m2, scales, al, no = state_of(a)
    w, h = a.width, a.height
    kn, ka, kz = GR.terms(**TOL)
    raster = FR.gather(sums, m2, a.tiles, scales, w, h)
    planes = GR.unpack_plane(al, a.tiles, w, h), GR.unpack_plane(no, a.tiles, w, h)
    lib = FR.pack(hrt.debug_guided(raster, *planes, 3, 4.0, kn=float(kn), ka=float(ka), kz=float(kz), on_device=True), a.tiles)
    ref = FR.pack(GR.guided_raster(raster, *planes, 3, 4.0, kn, ka, kz), a.tiles)
    frame = a.resolve_guided(guide=TOL)
    err = a.noise_filtered(FLOOR, guide=TOL, error_map=True)[1]
    with np.errstate(all="ignore"):
        sq = frame[:, :3] * frame[:, :3]
        exact = (u32(sq) == u32(lib[:, :3])).all(axis=1)
        want = np.sqrt(lib[:, 3]) / NF.at_least(FR.luma(sq), FLOOR)
        ref_sq = np.sqrt(ref[:, :3]) * np.sqrt(ref[:, :3])
        l_ref, l_sq = FR.luma(ref[:, :3]).astype(np.float64), FR.luma(ref_sq).astype(np.float64)
        tol = float(np.max(np.abs(l_sq - l_ref) / np.maximum(l_ref, 1e-30))) + 2.0 ** -23
    print("squaring exact on", int(exact.sum()), "of", exact.size, "pixels; tolerance elsewhere", tol)
    assert exact.any() and not exact.all() and tol < 1e-6
    assert np.array_equal(u32(err[exact]), u32(want[exact]))
    assert np.all(np.abs(err.astype(np.float64) - want) <= tol * want)


# ------------------------------------------------------------------------------------------ 8. writes nothing
@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "mixed"])
def test_the_call_writes_nothing(scene, mixed):
    a = build(scene, "A", mixed=mixed)

    def answers():
        return [a.resolve(), a.noise(FLOOR, error_map=True)[1], a.resolve_guided(guide=TOL), a.resolve(denoise=True),
                a.resolve_guided(demodulate=DEMOD_FLOOR), *a.features()]

    blob, before = a.snapshot(), answers()
    first = [a.noise_filtered(FLOOR, error_map=True, **kw)[1] for kw in SETTINGS.values()]
    a.noise_filtered(0.2, denoise=dict(iterations=5, sigma=2.0))
    assert a.snapshot() == blob
    for p, q in zip(before, answers()):
        assert np.array_equal(u32(p), u32(q))
    for e, kw in zip(first, SETTINGS.values()):
        assert np.array_equal(u32(e), u32(a.noise_filtered(FLOOR, error_map=True, **kw)[1]))
    a.close()


# ------------------------------------------------------------------------------------------ 9. hrt_accum_noise unchanged
@pytest.mark.gpu
@pytest.mark.parametrize("inp", ["A", "B"])
def test_accum_noise_keeps_its_reduction(states, inp):
    """accum_noise's reduction now lives in a header it shares with the filtered estimate's reduce kernel: its records
    are still the host's tile_reduce of its own error map (hrt_debug_noise), and the restatement's."""
    for mixed in (False, True):
        a = states(inp, "grid", mixed)
        rec, err = a.noise(FLOOR, error_map=True)
        off = 0
        for t, (_, _, tw, th) in enumerate(a.tiles):
            e = err[off:off + tw * th]
            assert np.array_equal(u32([rec[t].mean, rec[t].max]), u32(NF.tile_reduce(e))), (inp, mixed, t)
            off += tw * th
    # the host's arithmetic of one tile: a pass of two chunks onto zero sums gives the tile's errs and its mean / max
    rng = np.random.default_rng(3)
    n = 257
    partial = np.zeros((2, n, 4), F)
    partial[..., :3] = rng.uniform(0.1, 2.0, (2, n, 3))
    dev = hrt.debug_noise(partial, [4, 4], np.zeros((n, 4), F), np.zeros(n, F), 8, 2, FLOOR, on_device=True)
    host = hrt.debug_noise(partial, [4, 4], np.zeros((n, 4), F), np.zeros(n, F), 8, 2, FLOOR, on_device=False)
    for d, hst in zip(dev, host):
        assert np.array_equal(u32(d), u32(hst))
    assert np.array_equal(u32([host[3], host[4]]), u32(NF.tile_reduce(host[2])))


# ------------------------------------------------------------------------------------------ 3. refusals on an accumulator
@pytest.mark.gpu
def test_refusals_change_nothing(scene, states):
    s = scene("random")
    a = states("A")
    no_feat = build(scene, "A", features=False)
    no_fsamples = hrt.Accumulator(s, 64, 36, hrt.tile_grid(64, 36, 16), noise=True, features=True)
    no_noise = hrt.Accumulator(s, 64, 36, hrt.tile_grid(64, 36, 16), features=True)
    empty = hrt.Accumulator(s, 64, 36, hrt.tile_grid(64, 36, 16), noise=True, features=True)
    overlap = hrt.Accumulator(s, 64, 36, [(0, 0, 40, 36), (32, 0, 32, 36)], noise=True)
    for x in (no_fsamples, no_noise, overlap):
        for k in range(3):
            x.add(*setup(s, 64, 36, 42, offset=42 * k))
    no_noise.add_features(*setup(s, 64, 36, 8))
    one = hrt.Accumulator(s, 64, 36, hrt.tile_grid(64, 36, 16), noise=True, features=True)   # one tile short of its second chunk
    chunk = hrt.sample_chunks(s, setup(s, 64, 36, 42)[1])["chunk"]
    one.add(*setup(s, 64, 36, 42))
    few = [r.chunks < 2 for r in one.noise(FLOOR)]
    if not any(few):    # a 42-sample pass is several chunks here: a pass of one chunk's samples holds K = 1
        one.reset()
        one.add(*setup(s, 64, 36, min(chunk, 42)))
        few = [r.chunks < 2 for r in one.noise(FLOOR)]
    one.add_features(*setup(s, 64, 36, 8))
    every = (a, no_feat, no_fsamples, one, overlap)
    before = {x: (x.snapshot(), x.resolve()) for x in every}

    def raises(status, fn):
        with pytest.raises(hrt.HrtError) as e:
            fn()
        assert e.value.status == status, e.value

    raises(hrt.ERR_STATE, lambda: no_feat.noise_filtered(FLOOR, guide=TOL))
    raises(hrt.ERR_STATE, lambda: no_feat.noise_filtered(FLOOR, demodulate=DEMOD_FLOOR))
    raises(hrt.ERR_STATE, lambda: no_fsamples.noise_filtered(FLOOR, guide=dict(normal=0, albedo=0.1, depth=0)))
    raises(hrt.ERR_STATE, lambda: no_noise.noise_filtered(FLOOR))
    raises(hrt.ERR_STATE, lambda: no_noise.noise_filtered(FLOOR, guide=TOL))
    raises(hrt.ERR_STATE, lambda: empty.noise_filtered(FLOOR))
    if any(few):
        raises(hrt.ERR_STATE, lambda: one.noise_filtered(FLOOR))
        raises(hrt.ERR_STATE, lambda: one.noise_filtered(FLOOR, guide=TOL, error_map=True))
    raises(hrt.ERR_UNSUPPORTED, lambda: overlap.noise_filtered(FLOOR))
    raises(hrt.ERR_UNSUPPORTED, lambda: overlap.noise_filtered(FLOOR, error_map=True))
    assert no_fsamples.noise_filtered(FLOOR)[0].samples == 126       # every term off needs no feature samples
    for floor in (0.0, -0.05, float("nan")):
        raises(hrt.ERR_INVALID_ARG, lambda: a.noise_filtered(floor))
        raises(hrt.ERR_INVALID_ARG, lambda: no_noise.noise_filtered(floor))     # argument errors come first
    for it in (0, 6):
        raises(hrt.ERR_INVALID_ARG, lambda: a.noise_filtered(FLOOR, denoise=dict(iterations=it)))
    raises(hrt.ERR_INVALID_ARG, lambda: a.noise_filtered(FLOOR, denoise=dict(sigma=0.0)))
    raises(hrt.ERR_INVALID_ARG, lambda: a.noise_filtered(FLOOR, guide=dict(albedo=-1)))
    for dfloor in (0.0, -0.01, float("nan")):
        raises(hrt.ERR_INVALID_ARG, lambda: a.noise_filtered(FLOOR, demodulate=dfloor))
    L = hrt.load()
    rec = (hrt.TileNoise * len(a.tiles))()
    for r in rec:
        r.mean, r.samples = 7.0, 7

    def call(flags=0, afloor=0.0, reserved=0, g=True, out=rec, acc=a):
        p = hrt.GuidedExParams(3, 4.0, 0.1, 0.1, 0.1, flags, afloor, reserved)
        return L.hrt_accum_noise_filtered(acc.h, ctypes.byref(p) if g else None, FLOOR, None, None,
                                          ctypes.cast(out, ctypes.c_void_p) if out is not None else None)

    for flags in (2, 3, 0x80000001, 0xFFFFFFFE):
        assert call(flags, DEMOD_FLOOR) == hrt.ERR_INVALID_ARG, flags
    for flags in (0, 1):
        assert call(flags, DEMOD_FLOOR, reserved=1) == hrt.ERR_INVALID_ARG
    assert call(g=False) == hrt.ERR_INVALID_ARG and call(out=None) == hrt.ERR_INVALID_ARG
    assert call(acc=no_feat) == hrt.ERR_STATE
    assert all(r.mean == 7.0 and r.samples == 7 for r in rec)
    for x, (blob, px) in before.items():
        assert x.snapshot() == blob and np.array_equal(u32(x.resolve()), u32(px))
    assert call() == hrt.OK and call(1, DEMOD_FLOOR) == hrt.OK and all(r.samples == 126 for r in rec)
    for x in (no_feat, no_fsamples, no_noise, empty, overlap, one):
        x.close()


# ------------------------------------------------------------------------------------------ 10. the refinement loop
PASS, CAP, TILE = 20, 200, 8


def refined(s, policy, target, stop_after=None):
    """A fresh 32x32 `cornell` accumulator in 8-px tiles refined by `policy`; stop_after: on_pass raises after that many
    passes.  Returns (accumulator, passes sent)."""
    a = hrt.Accumulator(s, 32, 32, hrt.tile_grid(32, 32, TILE), noise=True)
    sent = []

    def on_pass(tiles, rec):
        sent.append(list(tiles))
        if stop_after is not None and len(sent) == stop_after:
            raise KeyboardInterrupt

    cam, p = setup(s, 32, 32, PASS)
    try:
        getattr(a, policy)(cam, p, target, PASS, CAP, FLOOR, on_pass=on_pass)
    except KeyboardInterrupt:
        pass
    return a, sent


@pytest.mark.gpu
def test_refine_filtered(scene):
    s = scene("cornell")
    # The target of the strict comparison comes from refine alone: 0.05 (the issue's) if refine stops there after 2 to 9
    # passes, else the first target of the scan 0.05 * 1.1^k at which it does (on this scene refine runs into the cap of 10
    # passes at 0.05: the raw error of a 32x32 cornell is above 0.4 at 200 spp).
    chosen, target = None, 0.05
    while chosen is None and target < 4.0:
        ref, sent = refined(s, "refine", target)
        total = sum(n * TILE * TILE for n in ref.tile_samples)
        ref.close()
        if target == 0.05:
            total_005 = total
        if 2 <= len(sent) <= 9:
            chosen = (target, total)
        target *= 1.1
    assert chosen is not None
    for target, ref_total in {0.05: total_005, chosen[0]: chosen[1]}.items():
        a, sent = refined(s, "refine_filtered", target)
        rec = a.noise_filtered(FLOOR)
        held = a.tile_samples
        total = sum(n * TILE * TILE for n in held)
        print("target", target, "refine", ref_total, "refine_filtered", total, "samples;", len(sent), "passes")
        assert all(r.mean <= target or n >= CAP for r, n in zip(rec, held))
        assert all(n % PASS == 0 and PASS <= n <= CAP for n in held)
        assert total <= ref_total
        if target == chosen[0]:
            assert total < ref_total
        # interrupted after its third pass (or its last but one), snapshotted, restored into a new accumulator and resumed
        stop = min(3, len(sent) - 1)
        assert stop >= 1
        b, part = refined(s, "refine_filtered", target, stop_after=stop)
        blob = b.snapshot()
        b.close()
        c = hrt.Accumulator(s, 32, 32, hrt.tile_grid(32, 32, TILE), noise=True)
        c.restore(blob)
        rest = []
        c.refine_filtered(*setup(s, 32, 32, PASS), target, PASS, CAP, FLOOR, on_pass=lambda t, r: rest.append(list(t)), resume=True)
        assert len(part) == stop and part + rest == sent
        assert c.snapshot() == a.snapshot()
        assert np.array_equal(u32(c.resolve(denoise=True)), u32(a.resolve(denoise=True)))
        c.close()
        a.close()


@pytest.mark.gpu
def test_refine_filtered_needs_feature_samples_first(scene):
    s = scene("cornell")
    a = hrt.Accumulator(s, 32, 32, hrt.tile_grid(32, 32, TILE), noise=True, features=True)
    b = hrt.Accumulator(s, 32, 32, hrt.tile_grid(32, 32, TILE), noise=True)
    for x in (a, b):
        for kw in (dict(guide=True), dict(demodulate=True)):
            with pytest.raises(ValueError):
                x.refine_filtered(*setup(s, 32, 32, PASS), 0.05, PASS, CAP, **kw)
        assert not any(x.tile_samples)
    a.add_features(*setup(s, 32, 32, 8))
    rec = a.refine_filtered(*setup(s, 32, 32, PASS), 0.2, PASS, 2 * PASS, guide=True)
    assert all(r.samples in (PASS, 2 * PASS) for r in rec)
    a.close()
    b.close()
