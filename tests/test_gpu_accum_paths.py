"""Caller-traced paths into the accumulator on the GPU (hrt_accum_add_paths; include/hrt/hrt.h "caller-traced paths into
an accumulator"): the kernel against the host function of csrc/accum_paths.h, and the contract against the render -
Accumulator.add_wavefront and add_paths leave an accumulator where add and add_tiles leave it: sums, noise plane, sample
ranges, chunk counts and identity, so every product downstream is the same bytes.  Every comparison is equality of words."""
import ctypes

import numpy as np
import pytest

import hrt

F = np.float32
SEED = 7
W, H, TILE = 40, 24, 16  # ragged right and bottom tiles: 16, 16, 8 wide and 16, 8 high
TILES = hrt.tile_grid(W, H, TILE)
SCENES = ["random", "cornell", "cornell_smoke", "earth"]
OK, ARG, STATE, UNSUP = hrt.OK, hrt.ERR_INVALID_ARG, hrt.ERR_STATE, hrt.ERR_UNSUPPORTED

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


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def params(s, spp, offset=0, seed=SEED, w=W, h=H):
    return hrt.params(w, h, spp, 50, seed, tuple(s.info.background), sample_offset=offset)


def to_host(tensor):
    import torch

    return tensor.contiguous().view(torch.int32).cpu().numpy().view(hrt.PATH_DTYPE).reshape(-1)


def state(a):
    """Everything downstream of the sums, as bytes (download refuses an accumulator whose tiles hold different passes)."""
    try:
        sums, ranges = a.download()
    except hrt.HrtError as e:
        assert e.status == UNSUP
        sums, ranges = None, None
    noise = [bytes(r) for r in a.noise(0.05)] if a.has_noise and any(a.tile_samples) else None
    return dict(sums=None if sums is None else sums.tobytes(), ranges=ranges, moments=a.moments().tobytes() if a.has_noise else None,
                tile_samples=a.tile_samples, noise=noise, resolve=a.resolve("f32").tobytes() if all(a.tile_samples) else None,
                snapshot=a.snapshot())


def assert_same(a, b):
    sa, sb = state(a), state(b)
    for key in sa:
        assert sa[key] == sb[key], key


# ------------------------------------------------------------------------------------------ 1. the kernel against the host
def synthetic(n_px, spp, seed):
    """Radiance whose sum depends on the order of the adds and stays positive: sample 2j is a_j > 0 over 24 binades,
    sample 2j + 1 is -b_j with b_j <= a_j / 2, or -0.0, or a denormal; one pixel is all positive and holds +inf.  (No NaN
    is made: which payload a sum of two NaNs keeps is the adder's business, not the contract's.)"""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(0.5, 1, (n_px, spp, 3)) * np.exp2(rng.integers(-12, 12, (n_px, spp, 3)))).astype(F)
    rad = a.copy()
    odd = np.arange(1, spp, 2)
    rad[:, odd] = -(a[:, odd - 1] * rng.uniform(0, 0.5, (n_px, len(odd), 3))).astype(F)
    pick = rng.uniform(size=(n_px, len(odd), 3))
    rad[:, odd] = np.where(pick < 0.05, F(-0.0), np.where(pick < 0.1, np.array(0x00000123, np.uint32).view(F), rad[:, odd]))
    if n_px > 2:
        rad[2] = np.abs(rad[2])
        rad[2, spp // 2, 1] = np.inf
    return rad


def batch(n_px, spp, seed):
    rng = np.random.default_rng(seed + 1)
    p = np.zeros(n_px * spp, hrt.PATH_DTYPE)
    p["rng"] = rng.integers(0, 2**32, (n_px * spp, 4), dtype=np.uint64).astype(np.uint32)
    p["throughput"] = rng.uniform(0, 1, (n_px * spp, 3)).astype(F)
    p["radiance"] = synthetic(n_px, spp, seed).reshape(-1, 3)
    p["flags"] = rng.choice([hrt.PATH_DONE, 0, hrt.PATH_DONE | hrt.PATH_INVALID, hrt.PATH_DEPTH], n_px * spp).astype(np.uint32)
    return p


_schedules = {}


def schedule(spp):
    if spp not in _schedules:
        s = hrt.preset("random", 1)
        _schedules[spp] = hrt.sample_chunks(s, hrt.params(W, H, spp))
        s.close()
    return _schedules[spp]


# 2047 samples: the longest row the staging buffer (2048 slots) takes, one pixel per run; 2048 (a row of 2049 slots) and
# 2049: the kernel walks global memory instead
CASES = [(spp, n_px) for spp in (1, 3, 4, 16, 53, 64, 65) for n_px in (1, 63, 65, 4097)] + \
    [(2047, 3), (2048, 3), (2049, 1), (2049, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("spp, n_px", CASES)
def test_kernel_equals_host_function(spp, n_px):
    sch = schedule(spp)
    paths = batch(n_px, spp, 1000 * spp + n_px)
    rng = np.random.default_rng(spp + n_px)
    acc0 = np.zeros((n_px, 4), F)
    acc0[:, :3] = rng.uniform(0, 100, (n_px, 3)).astype(F)
    m0 = rng.uniform(0, 1000, n_px).astype(F)
    total = spp + 11
    not_done = int(((paths["flags"] & hrt.PATH_DONE) == 0).sum())
    for m2, fmt in ((m0, "f32"), (None, "rgba8"), (m0, None), (None, None)):
        want = hrt.debug_accum_paths(paths, spp, sch, acc0, m2, total, fmt, on_device=False)
        got = hrt.debug_accum_paths(paths, spp, sch, acc0, m2, total, fmt, on_device=True)
        assert np.array_equal(bits(got[0]), bits(want[0])), (m2 is not None, fmt)
        assert (m2 is None and got[1] is None) or np.array_equal(bits(got[1]), bits(want[1]))
        assert (fmt is None and got[2] is None) or np.array_equal(got[2].view(np.uint8), want[2].view(np.uint8))
        assert got[3] == want[3] == not_done
    assert not np.array_equal(bits(want[0]), bits(acc0))


# ------------------------------------------------------------------------------------------ 2. the contract against add
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_wavefront_passes_equal_rendered_passes(scene, name):
    s = scene(name)
    cam = hrt.preset_camera(s.info, W, H)
    a = hrt.Accumulator(s, W, H, TILES, noise=True)
    b = hrt.Accumulator(s, W, H, TILES, noise=True)
    try:
        p1, p2 = params(s, 20), params(s, 11, 20)
        rays = a.add_wavefront(cam, p1)
        st = b.add(cam, p1, stats=True)
        assert rays == st.segments
        assert_same(a, b)
        preview, rays = a.add_wavefront(cam, p2, preview="rgba8")
        want, st = b.add(cam, p2, stats=True, preview="rgba8")
        assert rays == st.segments
        assert preview.dtype == np.uint8 and preview.tobytes() == want.tobytes()
        assert_same(a, b)
        assert a.samples == 31 and [r.chunks for r in a.noise(0.05)] == [r.chunks for r in b.noise(0.05)]
        assert a.resolve("f32", denoise=True).tobytes() == b.resolve("f32", denoise=True).tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 3. a subset of the tiles
def raw_sums(a):
    """(n_pixels, 4) raw sums of a HRT_ACCUM_NOISE accumulator whose tiles may hold different passes (download refuses
    those), out of its snapshot: the planes close the blob, sums, then the noise plane padded to 16 bytes, then 8 bytes of
    checksum (include/hrt/hrt.h; tests/test_accum_snapshot.py holds the layout)."""
    blob = np.frombuffer(a.snapshot(), np.uint8)
    n = a.n_pixels
    end = len(blob) - 8 - (4 * n + 15) // 16 * 16
    return blob[end - 16 * n:end].view(F).reshape(n, 4).copy()


@pytest.mark.gpu
def test_subset_equals_add_tiles_and_refines_on(scene):
    s = scene("random")
    cam = hrt.preset_camera(s.info, W, H)
    a = hrt.Accumulator(s, W, H, TILES, noise=True)
    b = hrt.Accumulator(s, W, H, TILES, noise=True)
    try:
        for acc in (a, b):
            acc.add(cam, params(s, 4))
        before, m_before = a.download()[0].copy(), a.moments().copy()
        assert np.array_equal(bits(raw_sums(a)), bits(before))
        sub, p = [4, 1], params(s, 8, 4)
        paths, _ = hrt.trace_paths_fused(s, cam, p, tiles=[TILES[i] for i in sub], device=True)
        assert a.add_paths(paths, cam, p, tiles=sub) is None
        b.add(cam, p, tiles=sub)
        assert a.tile_samples == b.tile_samples == [4, 12, 4, 4, 12, 4]
        assert_same(a, b)
        # the other tiles' bytes are as they were; the two tiles' are not
        off = np.cumsum([0] + [t[2] * t[3] for t in TILES])
        sums, m2 = raw_sums(a), a.moments()
        for t in range(len(TILES)):
            same = np.array_equal(bits(sums[off[t]:off[t + 1]]), bits(before[off[t]:off[t + 1]])) and \
                np.array_equal(bits(m2[off[t]:off[t + 1]]), bits(m_before[off[t]:off[t + 1]]))
            assert same == (t not in sub), t
        # the ledger is right as well as the sums: both go on to the same frame
        ra = a.refine(cam, params(s, 4), target=0.0, pass_spp=4, max_spp=16, resume=True)
        rb = b.refine(cam, params(s, 4), target=0.0, pass_spp=4, max_spp=16, resume=True)
        assert [bytes(r) for r in ra] == [bytes(r) for r in rb]
        assert a.tile_samples == b.tile_samples == [16] * 6
        assert_same(a, b)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 4. unfinished paths
@pytest.mark.gpu
def test_live_count_and_unfinished_paths(scene):
    s = scene("random")
    cam = hrt.preset_camera(s.info, W, H)
    p = params(s, 20)
    rays, paths = hrt.camera_paths(s, cam, p, TILES, device=True)
    s.step(rays, paths, steps=2, seed=p.seed, shutter=(cam.time0, cam.time1), background=tuple(p.background))
    records = to_host(paths)
    not_done = int(((records["flags"] & hrt.PATH_DONE) == 0).sum())
    assert 0 < not_done < len(records)
    a = hrt.Accumulator(s, W, H, TILES, noise=True)
    try:
        none, live = a.add_paths(paths, cam, p, live=True)
        assert none is None and live == not_done
        zero = np.zeros((W * H, 4), F)
        acc, m2, _, count = hrt.debug_accum_paths(records, 20, hrt.sample_chunks(s, p), zero, np.zeros(W * H, F))
        assert count == not_done
        assert np.array_equal(bits(a.download()[0]), bits(acc)) and np.array_equal(bits(a.moments()), bits(m2))
        assert a.samples == 20  # deposited all the same
    finally:
        a.close()


# ------------------------------------------------------------------------------------------ 5. the host variant
@pytest.mark.gpu
def test_host_variant_equals_device_variant(scene):
    s = scene("cornell")
    cam = hrt.preset_camera(s.info, W, H)
    p = params(s, 20)
    paths, _ = hrt.trace_paths_fused(s, cam, p, tiles=TILES, device=True)
    a = hrt.Accumulator(s, W, H, TILES, noise=True)
    b = hrt.Accumulator(s, W, H, TILES, noise=True)
    try:
        a.add_paths(paths, cam, p)
        records = to_host(paths)
        assert b.add_paths(records, cam, p, live=True) == (None, 0)
        assert_same(a, b)
        sub, q = [5, 0], params(s, 3, 20)
        part, _ = hrt.trace_paths_fused(s, cam, q, tiles=[TILES[i] for i in sub], device=True)
        a.add_paths(part, cam, q, tiles=sub)
        b.add_paths(to_host(part), cam, q, tiles=sub)
        assert a.tile_samples == [23, 20, 20, 20, 20, 23]
        assert_same(a, b)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 6. refusals change nothing
class Ctx:
    def __init__(self, s):
        import torch

        self.L = hrt.load()
        self.s = s
        self.cam = hrt.preset_camera(s.info, W, H)
        self.full = hrt.Accumulator(s, W, H, TILES, noise=True)       # holds samples [0, 4) everywhere
        self.full.add(self.cam, params(s, 4))
        self.nonuni = hrt.Accumulator(s, W, H, TILES, noise=True)     # tile 0 alone holds samples [0, 4)
        self.nonuni.add(self.cam, params(s, 4), tiles=[0])
        self.n = W * H * 4
        self.paths = torch.zeros((self.n + 1, 12), dtype=torch.float32, device="cuda")
        self.out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        self.live = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.idx = np.array([4, 1], np.uint32)
        self.host = np.zeros(self.n, hrt.PATH_DTYPE)

    def call(self, a="full", cam=True, p=None, idx=None, n_idx=None, paths=0, n=None, fmt=-1, out=None, live=None):
        a = getattr(self, a).h if a else None
        p = params(self.s, 4, 4) if p is None else p
        ip = None if idx is None else np.array(idx, np.uint32)
        n_idx = (0 if ip is None else ip.size) if n_idx is None else n_idx
        n = (self.n if ip is None else sum(TILES[i][2] * TILES[i][3] for i in idx if i < len(TILES)) * p.samples) if n is None else n
        return self.L.hrt_accum_add_paths(a, ctypes.byref(self.cam) if cam else None, ctypes.byref(p) if p else None,
                                          None if ip is None else ip.ctypes.data, n_idx,
                                          None if paths is None else self.paths.data_ptr() + paths, n, fmt,
                                          None if out is None else self.out.data_ptr(), None if live is None else self.live.data_ptr() + live,
                                          None)

    def close(self):
        self.full.close()
        self.nonuni.close()


@pytest.fixture(scope="module")
def ctx(scene):
    c = Ctx(scene("random"))
    yield c
    c.close()


def other(c, **kw):
    """c's params of the next pass with one field changed."""
    p = params(c.s, 4, 4)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


ROWS = [
    ("null accumulator", lambda c: c.call(a=None), ARG),
    ("null camera", lambda c: c.call(cam=False), ARG),
    ("null paths", lambda c: c.call(paths=None), ARG),
    ("one path short", lambda c: c.call(n=c.n - 1), ARG),
    ("one path more", lambda c: c.call(n=c.n + 1), ARG),
    ("no paths", lambda c: c.call(n=0), ARG),
    ("2^32 paths", lambda c: c.call(n=1 << 32), ARG),
    ("the whole frame's paths for a subset", lambda c: c.call(idx=[4, 1], n=c.n), ARG),
    ("misaligned paths", lambda c: c.call(paths=8), ARG),
    ("misaligned live counter", lambda c: c.call(live=2), ARG),
    ("format 2", lambda c: c.call(fmt=2, out=True), ARG),
    ("format -2", lambda c: c.call(fmt=-2), ARG),
    ("a format without d_out", lambda c: c.call(fmt=0), ARG),
    ("a preview of a subset", lambda c: c.call(idx=[4, 1], fmt=0, out=True), ARG),
    ("a tile index out of range", lambda c: c.call(idx=[4, 6]), ARG),
    ("a tile index given twice", lambda c: c.call(idx=[4, 4]), ARG),
    ("idx without n_idx", lambda c: c.call(idx=[4, 1], n_idx=0), ARG),
    ("another seed", lambda c: c.call(p=other(c, seed=SEED + 1)), ARG),
    ("another depth", lambda c: c.call(p=other(c, max_depth=49)), ARG),
    ("another width", lambda c: c.call(p=other(c, width=W + 8)), ARG),
    ("samples held already", lambda c: c.call(p=other(c, sample_offset=2)), ARG),
    ("samples held already, in the subset", lambda c: c.call(idx=[4, 1], p=other(c, sample_offset=3)), ARG),
    ("no samples", lambda c: c.call(p=other(c, samples=0), n=0), ARG),
    ("unknown render flag", lambda c: c.call(p=other(c, flags=1 << 20)), ARG),
    ("a preview when the tiles hold different passes", lambda c: c.call(a="nonuni", fmt=0, out=True), UNSUP),
]


@pytest.mark.gpu
@pytest.mark.parametrize("what, call, status", ROWS, ids=[r[0] for r in ROWS])
def test_refusal_changes_nothing(ctx, what, call, status):
    before = {n: getattr(ctx, n).snapshot() for n in ("full", "nonuni")}
    got = call(ctx)
    assert got == status, (got, ctx.L.hrt_last_error())
    for n in before:
        assert getattr(ctx, n).snapshot() == before[n], n
    assert int(ctx.live.sum()) == 0 and float(ctx.out.abs().sum()) == 0.0


@pytest.mark.gpu
def test_host_variant_refusals(ctx):
    before = ctx.full.snapshot()
    live = ctypes.c_uint32(5)
    cam, p = ctypes.byref(ctx.cam), params(ctx.s, 4, 4)
    L, buf = ctx.L, ctx.host.ctypes.data
    assert L.hrt_accum_add_paths_host(ctx.full.h, cam, ctypes.byref(p), None, 0, buf, ctx.n - 1, ctypes.byref(live)) == ARG
    assert L.hrt_accum_add_paths_host(ctx.full.h, cam, ctypes.byref(p), None, 0, None, ctx.n, ctypes.byref(live)) == ARG
    assert L.hrt_accum_add_paths_host(ctx.full.h, cam, ctypes.byref(params(ctx.s, 4, 0)), None, 0, buf, ctx.n, ctypes.byref(live)) == ARG
    assert live.value == 5 and ctx.full.snapshot() == before
    # and the calls the table refused go through once they are right
    assert ctx.call(idx=[4, 1], live=0) == OK
    assert ctx.full.tile_samples == [4, 8, 4, 4, 8, 4] and int(ctx.live[0]) == (TILES[4][2] * TILES[4][3] + TILES[1][2] * TILES[1][3]) * 4
