"""Scatter queries on the GPU: scatter.hip and query.hip's camera paths through Scene.scatter, hrt.camera_paths and
hrt.trace_paths, the bit contract of include/hrt/hrt.h.  The device's rays and paths are held to
tests/native/scatter_sim.hip round by round (the same per-lane code on the host, which tests/test_scatter_host.py holds to
the lane simulator's render and to the oracle), the whole loop to hrt.render and to hrt.trace_path."""
import ctypes

import numpy as np
import pytest

import hrt
import query_sim as QS
import scatter_sim as SS

F = np.float32
SEED = 7
# name: (width, height, samples)
SCENES = {"random": (64, 36, 2), "cornell": (32, 32, 1), "cornell_smoke": (32, 32, 1), "features": (32, 32, 1), "earth": (32, 32, 1)}
PIXELS = [(0, 0), (3, 7), (9, 2), (13, 13), (20, 5), (31, 17), (16, 9), (7, 15), (25, 11), (30, 0), (1, 16), (18, 3)]  # inside 32 x 18

_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    def get(name):
        if name not in _scenes:
            s = hrt.preset(name, 1, earth)
            s.commit()
            _scenes[name] = (s, hrt.scene_blob(s))
        return _scenes[name]

    yield get
    for s, _ in _scenes.values():
        s.close()
    _scenes.clear()


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    return SS.build(tmp_path_factory, lane=False)


def to_device(records):
    import torch

    return torch.from_numpy(QS.words(records).view(np.int32).copy()).cuda()


def to_host(tensor):
    import torch

    return tensor.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 12)


def frame_of(radiance, w, h):
    return np.sqrt(radiance.astype(F) * F(1.0)).reshape(h, w, 3)


# ------------------------------------------------------------------------------------------ 1. device against simulator
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_device_loop_equals_the_simulator_round_by_round(scene, sims, name):
    """Device and host run the same per-lane code under -ffp-contract=off: after every round all 48 bytes of every ray
    and every path are EQUAL, from the camera paths to the last path's end."""
    s, blob = scene(name)
    w, h, spp = SCENES[name]
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, spp, 50, SEED, tuple(s.info.background))
    n_mats = s.scene_info().materials
    d_rays, d_paths = hrt.camera_paths(s, cam, p, device=True)
    want_r, want_p = SS.camera_paths(sims, cam, p)
    assert np.array_equal(to_host(d_rays), SS.words(want_r)) and np.array_equal(to_host(d_paths), SS.words(want_p))
    assert np.array_equal(to_host(hrt.camera_rays(s, cam, p, device=True)), SS.words(want_r))  # hrt_camera_rays' word for word
    rounds = []

    def on_round(i, rays, hits, paths):
        d_hits = s.intersect(d_rays, seed=SEED, shutter=(cam.time0, cam.time1))
        assert np.array_equal(to_host(d_hits), SS.words(hits)), (name, i)
        out_r, out_p = s.scatter(d_rays, d_hits, d_paths, tuple(p.background))
        assert out_r is d_rays and out_p is d_paths  # in place
        got_r, got_p = to_host(d_rays), to_host(d_paths)
        assert np.array_equal(got_r, SS.words(rays)), (name, i, np.flatnonzero((got_r != SS.words(rays)).any(axis=1))[:8])
        assert np.array_equal(got_p, SS.words(paths)), (name, i, np.flatnonzero((got_p != SS.words(paths)).any(axis=1))[:8])
        rounds.append(i)

    paths, n_rays, scattered = SS.loop(sims, s, cam, p, blob=blob, on_round=on_round, n_mats=n_mats)
    assert (paths["flags"] & hrt.PATH_DONE).all() and not (paths["flags"] & hrt.PATH_INVALID).any()
    assert len(rounds) >= 2 and n_rays > w * h * spp and scattered.sum() > 0
    if name == "cornell_smoke":
        assert scattered[4] > 0  # the isotropic medium
    # the host variants give the device variants' records
    h_rays, h_paths = hrt.camera_paths(s, cam, p)
    assert np.array_equal(SS.words(h_rays), SS.words(want_r)) and np.array_equal(SS.words(h_paths), SS.words(want_p))
    h_hits = s.intersect(h_rays, seed=SEED, shutter=(cam.time0, cam.time1))
    r1, p1 = s.scatter(h_rays, h_hits, h_paths, tuple(p.background))
    sim_r, sim_p = SS.scatter(sims, blob, h_rays, h_hits, h_paths, tuple(p.background), n_mats)
    assert r1 is not h_rays and np.array_equal(SS.words(h_paths), SS.words(want_p))  # new arrays come back
    assert np.array_equal(SS.words(r1), SS.words(sim_r)) and np.array_equal(SS.words(p1), SS.words(sim_p))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "0"])
def test_perlin_tables_in_lds_and_in_global_memory_give_the_same_records(scene, sims, monkeypatch, knob):
    """A noise-textured scene runs scatter_staged_kernel (the Perlin tables in LDS, a resident grid striding over the
    batch) and, under HRT_SCATTER_PERLIN_LDS=0, scatter_kernel: the simulator's rays and paths after every round, on a
    batch that is no multiple of the workgroup."""
    s, blob = scene("two_perlin_spheres")
    w, h = 50, 37
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 2, 50, SEED, tuple(s.info.background))
    d_rays, d_paths = hrt.camera_paths(s, cam, p, device=True)
    if knob is not None:
        monkeypatch.setenv("HRT_SCATTER_PERLIN_LDS", knob)
    hrt.render(s, cam, hrt.params(w, h, 1, 1, SEED))  # another kernel's launch record
    rounds = []

    def on_round(i, rays, hits, paths):
        s.scatter(d_rays, to_device(hits), d_paths, tuple(p.background))
        assert np.array_equal(to_host(d_rays), SS.words(rays)) and np.array_equal(to_host(d_paths), SS.words(paths)), i
        rounds.append(i)

    paths, _, scattered = SS.loop(sims, s, cam, p, blob=blob, on_round=on_round, n_mats=s.scene_info().materials)
    info = hrt.last_launch()
    assert ("scatter_staged_kernel" in info["kernel"]) == (knob is None)
    assert knob is not None or (info["block"] == 256 and info["lds_bytes"] >= 12288)
    assert len(rounds) >= 2 and scattered[0] > 1000 and (paths["flags"] & hrt.PATH_DONE).all()


# ------------------------------------------------------------------------------------------ 2. tails
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_tails_and_guard_records(scene, sims, n):
    """n records of a larger batch: records [0, n) are the simulator's, the guard records behind them are untouched."""
    import torch

    s, blob = scene("cornell_smoke")
    w = h = 72  # 5184 paths: room behind 4097
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 1, 50, SEED, tuple(s.info.background))
    rays, paths = SS.camera_paths(sims, cam, p)
    hits = QS.intersect(sims.Q, s, rays, seed=SEED, shutter=(cam.time0, cam.time1), blob=blob)
    want_r, want_p = SS.scatter(sims, blob, rays[:n], hits[:n], paths[:n], tuple(p.background), s.scene_info().materials)
    d_rays, d_hits, d_paths = to_device(rays), to_device(hits), to_device(paths)
    sp = hrt.scatter_params(tuple(p.background))
    assert hrt.load().hrt_scene_scatter(s.h, ctypes.byref(sp), d_rays.data_ptr(), d_hits.data_ptr(), d_paths.data_ptr(), n, None) == hrt.OK
    torch.cuda.synchronize()
    got_r, got_p = to_host(d_rays), to_host(d_paths)
    assert np.array_equal(got_r[:n], SS.words(want_r)) and np.array_equal(got_p[:n], SS.words(want_p))
    assert np.array_equal(got_r[n:], SS.words(rays)[n:]) and np.array_equal(got_p[n:], SS.words(paths)[n:])
    assert np.array_equal(to_host(d_hits), SS.words(hits))  # hits are read only
    assert (got_p[:n] != SS.words(paths)[:n]).any()


# ------------------------------------------------------------------------------------------ 3. the loop against the render
@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,ks", [("random", 64, 36, (0, 1, 2, 3)), ("cornell_smoke", 32, 32, (0, 1))])
@pytest.mark.parametrize("depth", [0, 1, 3, 50])
def test_trace_paths_equals_the_render(scene, name, w, h, ks, depth):
    s, _ = scene(name)
    cam = hrt.preset_camera(s.info, w, h)
    for k in ks:
        p = hrt.params(w, h, 1, depth, SEED, tuple(s.info.background), sample_offset=k)
        radiance, n_rays = hrt.trace_paths(s, cam, p)
        frame, st = hrt.render(s, cam, p, stats=True)
        assert np.array_equal(frame_of(radiance, w, h).view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32)), (name, k, depth)
        assert n_rays == int(st.segments), (name, k, depth)
        assert (n_rays == 0) == (depth == 0) and (depth == 0 or radiance.any())


# ------------------------------------------------------------------------------------------ 4. single paths
@pytest.mark.gpu
def test_single_paths_equal_trace_path(scene):
    s, _ = scene("random")
    w, h, spp = 32, 18, 4
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, spp, 50, SEED, tuple(s.info.background))
    radiance, _ = hrt.trace_paths(s, cam, p)
    radiance = radiance.reshape(h, w, spp, 3)
    for i, (x, y) in enumerate(PIXELS):
        k = i % spp
        _, rad = hrt.trace_path(s, cam, p, x, y, k)
        assert np.array_equal(radiance[y, x, k].view(np.uint32), rad.view(np.uint32)), (x, y, k)
    tile = (5, 3, 9, 7)  # ... and a tile's paths are the frame's
    sub, _ = hrt.trace_paths(s, cam, p, tiles=[tile])
    assert np.array_equal(sub.reshape(7, 9, spp, 3).view(np.uint32), radiance[3:10, 5:14].view(np.uint32))


# ------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.gpu
def test_refusals_change_nothing(scene, sims):
    import torch

    L = hrt.load()
    s, blob = scene("random")
    w, h = 16, 9
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 1, 50, SEED, tuple(s.info.background))
    rays, paths = SS.camera_paths(sims, cam, p)
    hits = QS.intersect(sims.Q, s, rays, seed=SEED, shutter=(cam.time0, cam.time1), blob=blob)
    n = len(rays)
    d_rays, d_hits, d_paths = to_device(rays), to_device(hits), to_device(paths)
    r, hh, q = d_rays.data_ptr(), d_hits.data_ptr(), d_paths.data_ptr()
    sp = hrt.scatter_params(tuple(p.background))
    bg = hrt._F3(0.5, 0.5, 0.5)
    never = hrt.preset("two_spheres", 1)  # not committed
    cases = [((None, ctypes.byref(sp), r, hh, q, n), hrt.ERR_INVALID_ARG, b"null"),
             ((s.h, None, r, hh, q, n), hrt.ERR_INVALID_ARG, b"null"),
             ((s.h, ctypes.byref(sp), None, hh, q, n), hrt.ERR_INVALID_ARG, b"null buffer"),
             ((s.h, ctypes.byref(sp), r, None, q, n), hrt.ERR_INVALID_ARG, b"null buffer"),
             ((s.h, ctypes.byref(sp), r, hh, None, n), hrt.ERR_INVALID_ARG, b"null buffer"),
             ((s.h, ctypes.byref(sp), r + 4, hh, q, n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             ((s.h, ctypes.byref(sp), r, hh + 8, q, n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             ((s.h, ctypes.byref(sp), r, hh, q + 12, n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             ((s.h, ctypes.byref(hrt.ScatterParams(1, 0, bg, 0)), r, hh, q, n), hrt.ERR_INVALID_ARG, b"scatter params"),
             ((s.h, ctypes.byref(hrt.ScatterParams(0, 7, bg, 0)), r, hh, q, n), hrt.ERR_INVALID_ARG, b"scatter params"),
             ((s.h, ctypes.byref(hrt.ScatterParams(0, 0, bg, 7)), r, hh, q, n), hrt.ERR_INVALID_ARG, b"scatter params"),
             ((s.h, ctypes.byref(hrt.scatter_params((0.5, float("nan"), 0.5))), r, hh, q, n), hrt.ERR_INVALID_ARG, b"scatter params"),
             ((s.h, ctypes.byref(hrt.scatter_params((float("inf"), 0.5, 0.5))), r, hh, q, n), hrt.ERR_INVALID_ARG, b"scatter params"),
             ((s.h, ctypes.byref(sp), r, hh, q, 1 << 32), hrt.ERR_INVALID_ARG, b"2^32"),
             ((never.h, ctypes.byref(sp), r, hh, q, n), hrt.ERR_STATE, b"not committed")]
    for args, status, text in cases:
        assert L.hrt_scene_scatter(*args, None) == status, text
        assert text in L.hrt_last_error(), (text, L.hrt_last_error())
    assert L.hrt_scene_scatter(s.h, ctypes.byref(sp), None, None, None, 0, None) == hrt.OK  # n == 0 launches nothing
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, w, h))
    a = (s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, r, q)
    for i in (0, 1, 2, 3, 5, 6):
        assert L.hrt_camera_paths(*a[:i], None, *a[i + 1:], None) == hrt.ERR_INVALID_ARG
    assert L.hrt_camera_paths(*a[:4], 0, *a[5:], None) == hrt.ERR_INVALID_ARG
    assert L.hrt_camera_paths(*a[:5], r + 4, q, None) == hrt.ERR_INVALID_ARG and b"16-byte aligned" in L.hrt_last_error()
    assert L.hrt_camera_paths(*a[:5], r, q + 4, None) == hrt.ERR_INVALID_ARG and b"16-byte aligned" in L.hrt_last_error()
    outside = (hrt.Tile * 1)(hrt.Tile(8, 0, 9, 9))
    assert L.hrt_camera_paths(*a[:3], outside, 1, r, q, None) == hrt.ERR_INVALID_ARG and b"tile outside" in L.hrt_last_error()
    huge = hrt.params(65535, 65535, 2, 50, SEED)  # 2^32 rays or more
    whole = (hrt.Tile * 1)(hrt.Tile(0, 0, 65535, 65535))
    big_cam = hrt.preset_camera(s.info, 65535, 65535)
    assert L.hrt_camera_paths(s.h, ctypes.byref(big_cam), ctypes.byref(huge), whole, 1, r, q, None) == hrt.ERR_INVALID_ARG
    assert b"2^32" in L.hrt_last_error()
    assert L.hrt_camera_paths(never.h, *a[1:], None) == hrt.ERR_STATE
    torch.cuda.synchronize()
    assert np.array_equal(to_host(d_rays), SS.words(rays)) and np.array_equal(to_host(d_paths), SS.words(paths))
    assert np.array_equal(to_host(d_hits), SS.words(hits))
    never.close()
