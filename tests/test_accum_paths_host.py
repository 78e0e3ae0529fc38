"""Caller-traced paths into the accumulator, without a GPU: the arithmetic of csrc/accum_paths.h (hrt_debug_accum_paths
with on_device = 0) against a numpy-float32 restatement of the contract in include/hrt/hrt.h ("caller-traced paths into
an accumulator"), against the render (the lane simulator's frame of the same samples, through the host loop of
tests/scatter_sim.py) and against the accumulator's own host arithmetic (hrt.debug_accumulate, hrt.debug_noise) on the
chunk sums; and the refusals that need no device.  Every comparison is equality of words."""
import ctypes

import numpy as np
import pytest

import hrt
import scatter_sim as SS

F = np.float32
NEW = ["hrt_accum_add_paths", "hrt_accum_add_paths_host", "hrt_debug_accum_paths"]
SEED = 3


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------ the restatement
def chunk_ranges(sch, spp):
    """[(s0, s1), ...] of a schedule (hrt.sample_chunks): `head` chunks of `chunk` samples, the first holding `first`,
    then `tail` halving chunks chunk/2, chunk/2, chunk/4, chunk/4, ..."""
    sizes = [sch["first"]] + [sch["chunk"]] * (sch["head"] - 1) + [sch["chunk"] >> (1 + j // 2) for j in range(sch["tail"])]
    ends = np.cumsum(sizes)
    assert ends[-1] == spp and min(sizes) >= 1
    return [(int(e - n), int(e)) for e, n in zip(ends, sizes)]


def restate_chunk_sums(rad, ranges):
    """(n_chunks, n_px, 4): each chunk's sum from +0, its samples' radiance added in sample order, in f32."""
    out = np.zeros((len(ranges), rad.shape[0], 4), F)
    with np.errstate(all="ignore"):
        for c, (s0, s1) in enumerate(ranges):
            s = np.zeros((rad.shape[0], 3), F)
            for k in range(s0, s1):
                s = (s + rad[:, k]).astype(F)
            out[c, :, :3] = s
    return out


def restate_pass(rad, ranges, acc, m2):
    """acc + (chunk sums in chunk order from chunk 0's) and m2 + (chunk terms (Y * Y) * (1 / n_c) likewise), ONE addend each."""
    sums = restate_chunk_sums(rad, ranges)
    with np.errstate(all="ignore"):
        total, moment = sums[0, :, :3], None
        for c, (s0, s1) in enumerate(ranges):
            y = ((sums[c, :, 0] + sums[c, :, 1]).astype(F) + sums[c, :, 2]).astype(F)
            term = ((y * y).astype(F) * (F(1.0) / F(s1 - s0))).astype(F)
            moment = term if c == 0 else (moment + term).astype(F)
            if c:
                total = (total + sums[c, :, :3]).astype(F)
        out = np.zeros((rad.shape[0], 4), F)
        out[:, :3] = (acc[:, :3] + total).astype(F)
        return out, (m2 + moment).astype(F)


def restate_f32(acc, samples):
    scale = F(1.0) / F(samples)
    out = np.ones((len(acc), 4), F)
    with np.errstate(all="ignore"):
        out[:, :3] = np.sqrt((acc[:, :3] * scale).astype(F)).astype(F)
    return out


def restate_rgba8(f32):
    """hrt_image_write's PPM rule per channel: NaN -> 0, clamp to [0, 0.999], (u8)(256 v); alpha 255."""
    v = f32[:, :3].astype(F)
    v = np.where(np.isnan(v), F(0), v)
    v = np.minimum(np.maximum(v, F(0)), F(0.999)).astype(F)
    out = np.full((len(f32), 4), 255, np.uint8)
    out[:, :3] = (F(256) * v).astype(F).astype(np.uint8)
    return out


def paths_of(rad, flags=None):
    """A batch whose radiance is rad (n_px, S, 3); the other words are noise the call must not read into the sums."""
    n = rad.shape[0] * rad.shape[1]
    rng = np.random.default_rng(n)
    p = np.zeros(n, hrt.PATH_DTYPE)
    p["rng"] = rng.integers(0, 2**32, (n, 4), dtype=np.uint64).astype(np.uint32)
    p["throughput"] = rng.uniform(0, 1, (n, 3)).astype(F)
    p["depth_left"] = rng.integers(0, 50, n)
    p["radiance"] = rad.reshape(n, 3)
    p["flags"] = hrt.PATH_DONE if flags is None else flags
    return p


def synthetic(n_px, spp, seed):
    """Radiance whose sum depends on the order of the adds: magnitudes over 24 binades with mixed signs, and among them
    -0.0, denormals, a pixel with a NaN, one with +inf and -inf, one with +inf alone."""
    rng = np.random.default_rng(seed)
    rad = (rng.uniform(-1, 1, (n_px, spp, 3)) * np.exp2(rng.integers(-12, 12, (n_px, spp, 3)))).astype(F)
    rad[rng.uniform(size=rad.shape) < 0.05] = F(-0.0)
    rad[rng.uniform(size=rad.shape) < 0.05] = np.array(0x00000123, np.uint32).view(F)  # a denormal
    rad[rng.uniform(size=rad.shape) < 0.02] = F(3.0e38)
    rad[rng.uniform(size=rad.shape) < 0.02] = F(-3.0e38)  # overflows to an infinity in some orders of the adds only
    if n_px >= 4:  # one NaN payload per pixel: which of two a sum keeps is the adder's business, not the contract's
        rad[1:4] = np.where(np.abs(rad[1:4]) > 1e30, F(1.0), rad[1:4])
        rad[1, spp // 2, 0] = np.nan
        rad[2, 0, 1], rad[2, spp - 1, 1] = np.inf, -np.inf
        rad[3, spp // 3, 2] = np.inf
    return rad


# ------------------------------------------------------------------------------------------ 1. symbols
def test_symbols_are_exported_and_bound():
    L = hrt.load()
    for name in NEW:
        assert name in hrt.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert L.hrt_abi_version() == 6 == hrt.ABI_VERSION
    for name in ("add_paths", "add_wavefront"):
        assert callable(getattr(hrt.Accumulator, name))
    assert callable(hrt.debug_accum_paths)


# ------------------------------------------------------------------------------------------ 2. against the restatement
# (options, spp, the chunk sizes the schedule must have): one chunk; a short first head chunk and a full one; a head and
# halving tail chunks; and the same under chunk_min = 2
SCHEDULES = [({}, 16, [16]), ({}, 20, [4, 16]), ({}, 53, [7, 16, 8, 8, 4, 4, 2, 2, 1, 1]), ({"chunk_min": 2}, 11, None)]


@pytest.fixture(scope="module")
def schedules():
    out = []
    for opts, spp, sizes in SCHEDULES:
        s = hrt.preset("random", 1)  # not committed: the schedule needs no device
        if opts:
            s.set_options(**opts)
        sch = hrt.sample_chunks(s, hrt.params(12, 9, spp))
        ranges = chunk_ranges(sch, spp)
        if sizes is not None:
            assert [b - a for a, b in ranges] == sizes, (spp, sch)
        else:
            assert len(ranges) == 7, (spp, sch)
        out.append((spp, sch, ranges))
        s.close()
    # the three shapes really occur
    assert len(out[0][2]) == 1 and out[1][1]["tail"] == 0 and out[1][1]["first"] < out[1][1]["chunk"] and out[2][1]["tail"] == 8
    return out


@pytest.mark.parametrize("which", range(len(SCHEDULES)))
@pytest.mark.parametrize("n_px", [1, 5, 67])
def test_host_function_matches_restatement(schedules, which, n_px):
    spp, sch, ranges = schedules[which]
    rng = np.random.default_rng(100 * which + n_px)
    rad = synthetic(n_px, spp, 7 * which + n_px)
    flags = rng.choice([hrt.PATH_DONE, 0, hrt.PATH_DONE | hrt.PATH_INVALID, hrt.PATH_DONE | hrt.PATH_MISSED], n_px * spp).astype(np.uint32)
    paths = paths_of(rad, flags)
    acc0 = np.zeros((n_px, 4), F)
    acc0[:, :3] = rng.uniform(0, 100, (n_px, 3)).astype(F)
    m0 = rng.uniform(0, 1000, n_px).astype(F)
    total = spp + 37
    want_acc, want_m2 = restate_pass(rad, ranges, acc0, m0)
    acc, m2, frame, live = hrt.debug_accum_paths(paths, spp, sch, acc0, m0, total, "f32")
    assert np.array_equal(bits(acc), bits(want_acc))
    assert np.array_equal(bits(m2), bits(want_m2))
    assert np.array_equal(bits(frame), bits(restate_f32(want_acc, total)))
    assert live == int(((flags & hrt.PATH_DONE) == 0).sum())
    # without a noise plane and without a preview; and the 8-bit preview
    acc, m2, frame, live = hrt.debug_accum_paths(paths, spp, (sch["chunk"], sch["head"], sch["first"]), acc0)
    assert m2 is None and frame is None and np.array_equal(bits(acc), bits(want_acc))
    acc, m2, rgba, _ = hrt.debug_accum_paths(paths, spp, sch, acc0, m0, total, "rgba8")
    assert rgba.dtype == np.uint8 and np.array_equal(rgba, restate_rgba8(restate_f32(want_acc, total)))
    assert np.array_equal(bits(acc), bits(want_acc)) and np.array_equal(bits(m2), bits(want_m2))


def test_the_order_of_the_adds_matters_on_these_inputs(schedules):
    """The inputs tell the contract's order from another: one flat fold of a pixel's samples gives other words."""
    spp, sch, ranges = schedules[2]
    rad = synthetic(67, spp, 5)
    zero = np.zeros((67, 4), F)
    chunked, _ = restate_pass(rad, ranges, zero, np.zeros(67, F))
    flat, _ = restate_pass(rad, [(0, spp)], zero, np.zeros(67, F))
    assert not np.array_equal(bits(chunked), bits(flat))


def test_a_pass_is_one_addend(schedules):
    """acc + pass_sum, never chunk by chunk or sample by sample: a large acc swallows every addend that is small alone."""
    spp, sch, ranges = schedules[2]
    rad = np.full((3, spp, 3), 0.75, F)
    acc0 = np.zeros((3, 4), F)
    acc0[:, :3] = F(2.0 ** 25)
    acc, _, _, _ = hrt.debug_accum_paths(paths_of(rad), spp, sch, acc0)
    assert (acc[:, :3] == F(2.0 ** 25) + F(0.75 * spp)).all() and (acc[:, :3] != F(2.0 ** 25)).all()


# ------------------------------------------------------------------------------------------ 3. against the render
W, H, SPP = 12, 9, 53


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    return SS.build(tmp_path_factory)


@pytest.fixture(scope="module")
def traced(sims, earth):
    """`random` at 12 x 9 (no multiple of 8 either way), default options: the host loop's finished paths of samples
    [0, 53) as one batch, computed once and never written again."""
    scene = hrt.preset("random", 1, earth)
    blob = hrt.scene_blob(scene)
    cam = hrt.preset_camera(scene.info, W, H)

    def params(spp, offset=0):
        return hrt.params(W, H, spp, 50, SEED, tuple(scene.info.background), sample_offset=offset)

    paths, n_rays, _ = SS.loop(sims, scene, cam, params(SPP), blob=blob)
    assert (paths["flags"] & hrt.PATH_DONE).all()
    paths.flags.writeable = False
    return scene, blob, cam, params, paths, n_rays


def test_one_pass_equals_the_lane_simulators_frame(sims, traced):
    scene, blob, cam, params, paths, n_rays = traced
    sch = hrt.sample_chunks(scene, params(SPP))
    assert sch["head"] + sch["tail"] == 10
    zero = np.zeros((W * H, 4), F)
    acc, m2, frame, live = hrt.debug_accum_paths(paths, SPP, sch, zero, np.zeros(W * H, F), SPP, "f32")
    ref, segments = SS.lane_render(sims, scene, cam, params(SPP), blob=blob, kernel=0)
    assert live == 0 and n_rays == segments
    assert np.array_equal(bits(frame), bits(ref.reshape(-1, 4)))
    # the noise plane is hrt.debug_noise's of the same chunk sums
    rad = paths["radiance"].reshape(W * H, SPP, 3)
    ranges = chunk_ranges(sch, SPP)
    sums = restate_chunk_sums(rad, ranges)
    acc_n, m2_n, _, _, _ = hrt.debug_noise(sums, [b - a for a, b in ranges], zero, np.zeros(W * H, F), SPP, len(ranges))
    assert np.array_equal(bits(acc), bits(acc_n)) and np.array_equal(bits(m2), bits(m2_n))
    assert (m2 > 0).all()


def test_two_passes_of_different_sizes(sims, traced):
    """Samples [0, 20) then [20, 53): each pass alone is the lane simulator's frame of those samples, and the two
    accumulated are what the accumulator's own host arithmetic (hrt.debug_accumulate, hrt.debug_noise) makes of the two
    passes' chunk sums.  (The lane simulator gives frames, not raw sums, so the chunk sums that go through
    debug_accumulate are folded here from the radiance the single-pass comparisons hold to it.)"""
    scene, blob, cam, params, paths, _ = traced
    rad = paths["radiance"].reshape(W * H, SPP, 3)
    both = paths.reshape(W * H, SPP)
    acc, m2 = np.zeros((W * H, 4), F), np.zeros(W * H, F)
    acc_ref, m2_ref = acc.copy(), m2.copy()
    held = chunks = 0
    for s0, n in ((0, 20), (20, 33)):
        p = params(n, s0)
        sch = hrt.sample_chunks(scene, p)
        ranges = chunk_ranges(sch, n)
        batch = np.ascontiguousarray(both[:, s0:s0 + n])
        # alone, into zero sums: the render's frame of the pass
        _, _, alone, _ = hrt.debug_accum_paths(batch, n, sch, np.zeros_like(acc), None, n, "f32")
        ref, _ = SS.lane_render(sims, scene, cam, p, blob=blob, kernel=0)
        assert np.array_equal(bits(alone), bits(ref.reshape(-1, 4)))
        # accumulated
        held, chunks = held + n, chunks + len(ranges)
        acc, m2, frame, _ = hrt.debug_accum_paths(batch, n, sch, acc, m2, held, "f32")
        sums = restate_chunk_sums(rad[:, s0:s0 + n], ranges)
        want_acc, want_frame = hrt.debug_accumulate(sums, acc_ref, held, "f32")
        _, m2_ref, _, _, _ = hrt.debug_noise(sums, [b - a for a, b in ranges], acc_ref, m2_ref, held, chunks)
        acc_ref = want_acc
        assert np.array_equal(bits(acc), bits(acc_ref)) and np.array_equal(bits(m2), bits(m2_ref))
        assert np.array_equal(bits(frame), bits(want_frame))
    assert held == SPP and chunks >= 4


# ------------------------------------------------------------------------------------------ 4. refusals without a device
def test_null_arguments_are_refused():
    L = hrt.load()
    s = hrt.preset("two_spheres", 1)
    cam, p = ctypes.byref(hrt.preset_camera(s.info, 16, 16)), ctypes.byref(hrt.params(16, 16, 2))
    paths = np.zeros(16 * 16 * 2, hrt.PATH_DTYPE)
    buf, live = paths.ctypes.data, ctypes.c_uint32(7)
    n = paths.size
    assert L.hrt_accum_add_paths(None, cam, p, None, 0, buf, n, -1, None, None, None) == hrt.ERR_INVALID_ARG
    assert b"hrt_accum_add_paths" in L.hrt_last_error()
    assert L.hrt_accum_add_paths_host(None, cam, p, None, 0, buf, n, ctypes.byref(live)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_add_paths_host(None, None, None, None, 0, None, 0, None) == hrt.ERR_INVALID_ARG
    assert live.value == 7


def test_debug_entry_refusals():
    L = hrt.load()
    paths = paths_of(np.ones((2, 20, 3), F))
    acc = np.zeros((2, 4), F)
    out = np.zeros((2, 4), F)
    sch = np.array([16, 2, 4], np.uint32)

    def call(paths=paths.ctypes.data, n_px=2, spp=20, sch=sch, acc=acc.ctypes.data, total=20, fmt=-1, out=None):
        return L.hrt_debug_accum_paths(0, paths, n_px, spp, sch.ctypes.data if sch is not None else None, acc, None, total, fmt, out, None)

    assert call() == hrt.OK
    assert call(fmt=0, out=out.ctypes.data) == hrt.OK
    before = acc.copy()
    for kw in (dict(paths=None), dict(sch=None), dict(acc=None), dict(spp=0), dict(fmt=-2), dict(fmt=2, out=out.ctypes.data),
               dict(fmt=0), dict(fmt=0, out=out.ctypes.data, total=0), dict(fmt=1, out=out.ctypes.data, total=(1 << 32) + 1),
               dict(n_px=1 << 31, spp=2),
               # not a schedule of 20 samples: chunks that end past them, no head chunk, an empty first chunk
               dict(sch=np.array([16, 1, 5], np.uint32)), dict(sch=np.array([8, 3, 3], np.uint32)),
               dict(sch=np.array([16, 0, 4], np.uint32)), dict(sch=np.array([16, 2, 0], np.uint32)), dict(spp=21)):
        assert call(**kw) == hrt.ERR_INVALID_ARG, kw
        assert b"hrt_debug_accum_paths" in L.hrt_last_error()
    assert np.array_equal(acc, before)
    assert call(n_px=0) == hrt.OK  # nothing to add
