"""The sample accumulator without a GPU: the arithmetic of csrc/accum.h (hrt_debug_accumulate with on_device = 0)
against a numpy-float32 restatement of the bit contract in include/hrt/hrt.h, and the argument checks of
hrt_accum_create that need no device."""
import ctypes

import numpy as np
import pytest

import hrt


def restate_pass(partial, acc):
    """acc + ((p0 + p1) + p2 ...): the chunk sums in chunk order from chunk 0's, then ONE addition into acc."""
    s = partial[0, :, :3].astype(np.float32)
    for c in range(1, partial.shape[0]):
        s = (s + partial[c, :, :3]).astype(np.float32)
    out = np.zeros((partial.shape[1], 4), np.float32)
    out[:, :3] = (acc[:, :3] + s).astype(np.float32)
    return out


def restate_f32(acc, samples):
    scale = np.float32(1.0) / np.float32(samples)
    out = np.ones((len(acc), 4), np.float32)
    with np.errstate(invalid="ignore"):
        out[:, :3] = np.sqrt((acc[:, :3] * scale).astype(np.float32)).astype(np.float32)
    return out


def restate_rgba8(f32):
    """hrt_image_write's PPM rule per channel: NaN -> 0, clamp to [0, 0.999], (u8)(256 v); alpha 255."""
    v = f32[:, :3].astype(np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(0.999)).astype(np.float32)
    out = np.full((len(f32), 4), 255, np.uint8)
    out[:, :3] = (np.float32(256) * v).astype(np.float32).astype(np.uint8)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n_chunks", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_host_accumulate_matches_restatement(n_chunks, n):
    rng = np.random.default_rng(1000 * n_chunks + n)
    partial = np.zeros((n_chunks, n, 4), np.float32)
    partial[:, :, :3] = rng.uniform(0, 40, (n_chunks, n, 3)).astype(np.float32)
    samples = 37 * n_chunks
    zero = np.zeros((n, 4), np.float32)
    acc, frame = hrt.debug_accumulate(partial, zero, samples, "f32")
    want = restate_pass(partial, zero)
    assert np.array_equal(bits(acc), bits(want))
    assert np.array_equal(bits(frame), bits(restate_f32(want, samples)))
    # a second pass into the sums of the first, without a resolve and with the 8-bit one
    partial2 = np.zeros_like(partial)
    partial2[:, :, :3] = rng.uniform(0, 3, (n_chunks, n, 3)).astype(np.float32)
    acc2, none = hrt.debug_accumulate(partial2, acc)
    assert none is None
    want2 = restate_pass(partial2, want)
    assert np.array_equal(bits(acc2), bits(want2))
    acc3, rgba = hrt.debug_accumulate(partial2, acc, 2 * samples, "rgba8")
    assert np.array_equal(bits(acc3), bits(want2))
    assert rgba.dtype == np.uint8 and np.array_equal(rgba, restate_rgba8(restate_f32(want2, 2 * samples)))


def test_pass_is_one_addend():
    """(acc + ((p0 + p1) + p2)), not ((acc + p0) + p1) + p2: values at which the two differ in f32."""
    acc = np.array([[1.0, 2.0 ** 24, 3.0, 0.0]], np.float32)
    partial = np.zeros((3, 1, 4), np.float32)
    partial[:, 0, 0] = [2.0 ** -24, 2.0 ** -24, 2.0 ** -23]   # each lost against 1.0 alone; their sum 2^-22 is not
    partial[:, 0, 1] = [1.0, 1.0, 1.0]                       # 2^24 + 1 rounds back to 2^24; + 3 does not
    partial[:, 0, 2] = [0.1, 0.2, 0.3]
    got, _ = hrt.debug_accumulate(partial, acc)
    one_addend = restate_pass(partial, acc)
    chunk_by_chunk = acc.copy()
    for c in range(3):
        chunk_by_chunk[:, :3] = (chunk_by_chunk[:, :3] + partial[c, :, :3]).astype(np.float32)
    assert not np.array_equal(bits(one_addend[:, :2]), bits(chunk_by_chunk[:, :2]))  # the vector tells them apart
    assert np.array_equal(bits(got), bits(one_addend))


def test_rgba8_edge_values():
    """The resolved values 0, -0, just below and above k/256, 0.999, 1.0, 4.0, +inf and NaN through the 8-bit rule.
    samples = 1, so the resolved value is sqrt(acc): acc = v * v reaches v only to rounding, so the expected bytes
    come from the restated F32 resolve of the same sums, and the resolved values are checked to hit the edges."""
    edges = []
    for k in (1, 2, 127, 128, 255):
        x = np.float32(k / 256.0)
        edges += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))]
    vals = np.array([0.0, -0.0, 0.999, 1.0, 4.0, np.inf, np.nan, -1.0] + edges, np.float32)
    sq = (vals * vals).astype(np.float32)
    sq[1] = np.float32(-0.0)   # sqrt(-0) = -0
    sq[7] = np.float32(-1.0)   # sqrt(-1) = NaN: a negative sum resolves to NaN, which the rule maps to 0
    n = len(sq)
    partial = np.zeros((1, n, 4), np.float32)
    partial[0, :, 0] = sq
    partial[0, :, 1] = sq[::-1]
    partial[0, :, 2] = np.float32(0.25)
    zero = np.zeros((n, 4), np.float32)
    zero[1, 0] = np.float32(-0.0)   # -0 + -0 = -0 (0 + -0 would be +0)
    acc, f32 = hrt.debug_accumulate(partial, zero, 1, "f32")
    _, rgba = hrt.debug_accumulate(partial, zero, 1, "rgba8")
    assert np.array_equal(bits(f32), bits(restate_f32(acc, 1)))
    assert np.array_equal(rgba, restate_rgba8(f32))
    r = f32[:, 0]
    assert bits(r[0:1])[0] == 0 and bits(r[1:2])[0] == 0x80000000 and r[3] == 1.0 and r[4] == 4.0
    assert np.isinf(r[5]) and np.isnan(r[6]) and np.isnan(r[7])
    assert list(rgba[[0, 1, 3, 4, 5, 6, 7], 0]) == [0, 0, 255, 255, 255, 0, 0]
    assert (rgba[:, 2] == 128).all() and (rgba[:, 3] == 255).all()   # sqrt(0.25) = 0.5 -> 128
    # around k/256 the byte steps from k - 1 to k exactly at the boundary
    got = {float(v): int(b) for v, b in zip(r[8:], rgba[8:, 0])}
    for v, b in got.items():
        assert b == int(np.float32(256) * np.float32(min(v, 0.999))), (v, b)
    assert len(set(rgba[8:, 0])) >= 8


def _create(scene_h, w, h, tiles, out):
    arr = (hrt.Tile * max(1, len(tiles)))(*[hrt.Tile(*t) for t in tiles])
    return hrt.load().hrt_accum_create(scene_h, w, h, ctypes.cast(arr, ctypes.c_void_p), len(tiles), out)


def test_create_argument_and_state_errors():
    L = hrt.load()
    s = hrt.preset("two_spheres", 1)   # not committed
    out = ctypes.c_void_p()
    assert _create(s.h, 16, 16, [(0, 0, 16, 16)], ctypes.byref(out)) == hrt.ERR_STATE
    assert not out.value
    assert _create(None, 16, 16, [(0, 0, 16, 16)], ctypes.byref(out)) == hrt.ERR_INVALID_ARG
    assert _create(s.h, 16, 16, [(0, 0, 16, 16)], None) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_create(s.h, 16, 16, None, 1, ctypes.byref(out)) == hrt.ERR_INVALID_ARG
    assert _create(s.h, 16, 16, [], ctypes.byref(out)) == hrt.ERR_INVALID_ARG              # n_tiles = 0
    assert _create(s.h, 16, 16, [(8, 0, 9, 16)], ctypes.byref(out)) == hrt.ERR_INVALID_ARG  # past the right edge
    assert _create(s.h, 16, 16, [(0, 0, 16, 0)], ctypes.byref(out)) == hrt.ERR_INVALID_ARG  # empty tile
    assert b"tile" in L.hrt_last_error()
    L.hrt_accum_destroy(None)   # a no-op
    with pytest.raises(hrt.HrtError) as e:
        hrt.Accumulator(s, 16, 16)
    assert e.value.status == hrt.ERR_STATE


def test_null_handles_are_invalid_arguments():
    L = hrt.load()
    n = ctypes.c_uint64()
    assert L.hrt_accum_samples(None, ctypes.byref(n)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_reset(None, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_resolve_host(None, 0, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_merge(None, None, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_accumulate(0, None, 1, 1, None, 1, -1, None) == hrt.ERR_INVALID_ARG


def test_every_entry_point_refuses_a_null_accumulator():
    """The accumulator entry points test_null_handles_are_invalid_arguments leaves out: a null accumulator (or scene, or
    blob) is refused before any device call, whatever else is passed."""
    L = hrt.load()
    s = hrt.preset("two_spheres", 1)
    cam, p = ctypes.byref(hrt.preset_camera(s.info, 16, 16)), ctypes.byref(hrt.params(16, 16, 2))
    f, g, x = ctypes.byref(hrt.filter_params()), ctypes.byref(hrt.guided_params()), ctypes.byref(hrt.guided_ex_params())
    arr = np.zeros(16 * 16 * 4, np.float32)
    buf = arr.ctypes.data
    n64, n32, out = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_void_p()
    tile = ctypes.cast((hrt.Tile * 1)(hrt.Tile(0, 0, 16, 16)), ctypes.c_void_p)
    calls = {
        "create_ex": lambda: L.hrt_accum_create_ex(None, 16, 16, tile, 1, 0, ctypes.byref(out)),
        "add": lambda: L.hrt_accum_add(None, cam, p, None, None),
        "add_resolve": lambda: L.hrt_accum_add_resolve(None, cam, p, 0, buf, None, None),
        "add_tiles": lambda: L.hrt_accum_add_tiles(None, cam, p, buf, 1, None, None),
        "tile_samples": lambda: L.hrt_accum_tile_samples(None, buf),
        "noise": lambda: L.hrt_accum_noise(None, 0.05, None, None, buf),
        "debug_accum_moments": lambda: L.hrt_debug_accum_moments(None, buf),
        "resolve": lambda: L.hrt_accum_resolve(None, 0, buf, None),
        "resolve_filtered": lambda: L.hrt_accum_resolve_filtered(None, f, 0, buf, None),
        "resolve_filtered_host": lambda: L.hrt_accum_resolve_filtered_host(None, f, 0, buf),
        "add_features": lambda: L.hrt_accum_add_features(None, cam, p, None),
        "feature_samples": lambda: L.hrt_accum_feature_samples(None, ctypes.byref(n64)),
        "features": lambda: L.hrt_accum_features(None, buf, buf, None),
        "features_host": lambda: L.hrt_accum_features_host(None, buf, buf),
        "debug_accum_features": lambda: L.hrt_debug_accum_features(None, buf, buf),
        "resolve_guided": lambda: L.hrt_accum_resolve_guided(None, g, 0, buf, None),
        "resolve_guided_host": lambda: L.hrt_accum_resolve_guided_host(None, g, 0, buf),
        "resolve_guided_ex": lambda: L.hrt_accum_resolve_guided_ex(None, x, 0, buf, None),
        "resolve_guided_ex_host": lambda: L.hrt_accum_resolve_guided_ex_host(None, x, 0, buf),
        "noise_filtered": lambda: L.hrt_accum_noise_filtered(None, x, 0.05, None, None, buf),
        "merge_tiles": lambda: L.hrt_accum_merge_tiles(None, None, None),
        "download": lambda: L.hrt_accum_download(None, None, None, 0, ctypes.byref(n32)),
        "upload": lambda: L.hrt_accum_upload(None, cam, p, buf, None, 0),
        "snapshot": lambda: L.hrt_accum_snapshot(None, None, 0, ctypes.byref(n64)),
        "restore": lambda: L.hrt_accum_restore(None, buf, 16),
        "snapshot_info": lambda: L.hrt_accum_snapshot_info(None, 0, ctypes.byref(hrt.SnapshotInfo()), None, 0),
    }
    for name, call in calls.items():
        assert call() == hrt.ERR_INVALID_ARG, name
    assert not out.value
    s.close()
