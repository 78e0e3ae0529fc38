"""Ray queries on the GPU: query.hip through Scene.intersect and hrt.camera_rays, the bit contract of include/hrt/hrt.h.
The device's hits are held to tests/native/query_sim.hip (the same per-lane code on the host, which
tests/test_query_host.py holds to the oracle's primitives and to the feature pass), to the segments hrt.trace_path
reports, and to the feature planes."""
import ctypes

import numpy as np
import pytest

import hrt
import query_sim as QS
import scenes_oracle as SO

F = np.float32
SEED = 7
N_RANDOM = 4096
VARIANTS = (0, hrt.QUERY_NO_LDS, hrt.QUERY_REFERENCE_CULL)
# name: (width, height, samples)
SCENES = {"random": (64, 36, 2), "cornell": (32, 32, 1), "cornell_smoke": (32, 32, 1), "features": (32, 32, 1), "motion": (32, 18, 1),
          "earth": (32, 32, 1)}
PIXELS = [(0, 0), (3, 7), (9, 2), (13, 13), (20, 5), (31, 17), (16, 9), (7, 15), (25, 11), (30, 0), (1, 16), (18, 3)]  # inside 32 x 18

_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    def get(name):
        if name not in _scenes:
            s = SO.bvh_intervals().to_hrt() if name == "bvh_intervals" else hrt.preset(name, 1, earth)
            s.commit()
            _scenes[name] = (s, hrt.scene_blob(s))
        return _scenes[name]

    yield get
    for s, _ in _scenes.values():
        s.close()
    _scenes.clear()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return QS.build(tmp_path_factory)


def to_device(records):
    import torch

    return torch.from_numpy(QS.words(records).view(np.int32).copy()).cuda()


def to_host(tensor):
    import torch

    return tensor.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 12)


def device_hits(s, rays, **kw):
    return to_host(s.intersect(to_device(rays), **kw))


def setup(s, name):
    w, h, spp = SCENES[name]
    return hrt.preset_camera(s.info, w, h), hrt.params(w, h, spp, 50, SEED, tuple(s.info.background))


def random_rays(s, shutter, n=N_RANDOM, seed=11):
    """Origins in the scene's bounding box grown by a tenth (the huge ground spheres clipped to 20 units), random
    directions of random lengths, times over the shutter, a fifth of them with a finite t_max."""
    rng = np.random.default_rng(seed)
    mn, mx = (np.clip(np.array(v, np.float64), -20.0, 600.0) for v in s.bounding_box(s.info.root))
    grow = 0.1 * (mx - mn)
    o = rng.uniform(mn - grow, mx + grow, (n, 3))
    d = rng.normal(size=(n, 3)) * rng.uniform(0.2, 3.0, (n, 1))
    t_max = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.5, 0.5 * np.linalg.norm(mx - mn), n), np.inf)
    return QS.make_rays(o, d, time=rng.uniform(shutter[0], shutter[1], n), t_min=0.001, t_max=t_max,
                        pixel=rng.integers(0, 1 << 20, n), sample=rng.integers(0, 64, n), segment=rng.integers(0, 8, n))


# ------------------------------------------------------------------------------------------ 1. device against simulator
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_device_hits_equal_the_simulator(scene, sim, name):
    """Device and host run the same per-lane code under -ffp-contract=off: all 48 bytes of every hit are EQUAL, for the
    frame's camera rays and for incoherent rays, with the scene in LDS, in global memory and under the reference test."""
    s, blob = scene(name)
    cam, p = setup(s, name)
    shutter = (cam.time0, cam.time1)
    cam_rays = QS.camera_rays(sim, cam, p)
    rays = np.concatenate([cam_rays, random_rays(s, shutter)])
    want = QS.words(QS.intersect(sim, s, rays, seed=SEED, shutter=shutter, blob=blob))
    hit = (want[:, 3] & hrt.HIT_HIT) != 0
    assert 0.05 < hit[len(cam_rays):].mean() < 1.0 and hit[:len(cam_rays)].any()
    if name in ("cornell_smoke", "features"):
        assert ((want[:, 3] & hrt.HIT_MEDIUM) != 0).sum() > (20 if name == "cornell_smoke" else 0)
    for flags in VARIANTS:
        got = device_hits(s, rays, flags=flags, seed=SEED, shutter=shutter)
        assert np.array_equal(got, want), (name, flags, np.flatnonzero((got != want).any(axis=1))[:8])
    info = hrt.last_launch()
    assert "launch_one" in info["kernel"] and "CULL = 0" in info["kernel"] and info["block"] == 512 and info["lds_bytes"] > 0


# ------------------------------------------------------------------------------------------ 2. camera rays
@pytest.mark.gpu
def test_camera_rays_equal_the_simulator_and_the_path_trace(scene, sim):
    s, _ = scene("random")
    w, h, spp = 32, 18, 3
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, spp, 50, SEED, tuple(s.info.background), sample_offset=5)
    want = QS.camera_rays(sim, cam, p)
    got = to_host(hrt.camera_rays(s, cam, p, device=True))
    assert np.array_equal(got, QS.words(want))
    assert np.array_equal(QS.words(hrt.camera_rays(s, cam, p)), QS.words(want))  # the host variant
    # tiles: packed back to back, a ragged split
    tiles = [(0, 0, 19, 18), (19, 0, 13, 5), (19, 5, 13, 13)]
    packed = np.concatenate([want.reshape(h, w, spp)[y:y + th, x:x + tw].reshape(-1) for x, y, tw, th in tiles])
    assert np.array_equal(to_host(hrt.camera_rays(s, cam, p, tiles=tiles, device=True)), QS.words(packed))
    # segment 0 of the path of that (pixel, absolute sample)
    frame = want.reshape(h, w, spp)
    for x, y in PIXELS:
        segs, _ = hrt.trace_path(s, cam, hrt.params(w, h, 16, 50, SEED, tuple(s.info.background)), x, y, 6)
        r = frame[y, x, 1]
        assert r["sample"] == 6 and r["pixel"] == y * w + x
        assert np.array_equal(r["origin"], segs[0][0]) and np.array_equal(r["direction"], segs[0][1]) and r["time"] == F(segs[0][2])


# ------------------------------------------------------------------------------------------ 3. whole paths
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "cornell_smoke"])
def test_every_segment_of_a_path_is_a_query(scene, name):
    """A query with a path's seed, pixel, sample and segment number repeats that segment: t and the winner, bit for bit."""
    s, (buf, info) = scene(name)
    w, h = 32, 18
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 4, 50, SEED, tuple(s.info.background))
    sphere_plan = (info.feature_mask & ~0x641) == 0 and not info.walk_general  # layout.h F_BASIC
    nodes = np.frombuffer(buf, np.uint32, count=info.n_nodes * 8, offset=info.off_nodes).reshape(-1, 8)
    rays, want_t, want_prim = [], [], []
    for k, (x, y) in enumerate(PIXELS):
        sample = k % 4
        segs, _ = hrt.trace_path(s, cam, p, x, y, sample, max_segments=64)
        assert 1 <= len(segs) < 64
        for i, (o, d, time, t, winner) in enumerate(segs):
            rays.append(QS.make_rays(o, d, time=time, t_min=p.t_min, t_max=np.inf, pixel=y * w + x, sample=sample, segment=i))
            want_t.append(F(t))
            want_prim.append(QS.MISS if winner == QS.MISS else (winner if sphere_plan else int(nodes[winner, 7] & 0xFFFFFF)))
    rays = np.concatenate(rays)
    hits = device_hits(s, rays, seed=SEED, shutter=(cam.time0, cam.time1)).view(hrt.HIT_DTYPE).reshape(-1)
    assert len(rays) > 30
    assert np.array_equal(hits["prim"], np.array(want_prim, np.uint32))
    hit = (hits["flags"] & hrt.HIT_HIT) != 0
    assert np.array_equal(hit, np.array(want_prim, np.uint32) != QS.MISS) and hit.any() and not hit.all()
    assert np.array_equal(hits["t"][hit].view(np.uint32), np.array(want_t, F)[hit].view(np.uint32))
    if name == "cornell_smoke":
        assert ((hits["flags"] & hrt.HIT_MEDIUM) != 0).any()


# ------------------------------------------------------------------------------------------ 4. the feature plane
@pytest.mark.gpu
def test_one_sample_feature_plane_equals_the_query(scene):
    s, _ = scene("random")
    w, h = 64, 36
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 1, 50, SEED, tuple(s.info.background))
    a = hrt.Accumulator(s, w, h, [(0, 0, w, h)], features=True)
    a.add_features(cam, p)
    fa, fn = a.debug_features()
    a.close()
    rays = hrt.camera_rays(s, cam, p, device=True)
    hits = to_host(s.intersect(rays, seed=SEED, shutter=(cam.time0, cam.time1))).view(hrt.HIT_DTYPE).reshape(-1)
    r = to_host(rays).view(hrt.RAY_DTYPE).reshape(-1)
    hit = (hits["flags"] & hrt.HIT_HIT) != 0
    assert np.array_equal(fa[:, 3], hit.astype(F)) and 0.7 < hit.mean() < 0.9
    assert np.array_equal(fn[:, :3].view(np.uint32), hits["normal"].view(np.uint32))
    d = r["direction"]
    depth = np.where(hit, hits["t"] * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=F), F(0)).astype(F)
    assert np.array_equal(fn[:, 3].view(np.uint32), depth.view(np.uint32))


# ------------------------------------------------------------------------------------------ 5. tails
@pytest.mark.gpu
def test_tails_and_untouched_output(scene):
    import torch

    s, _ = scene("random")
    rays = to_device(random_rays(s, (0.0, 1.0)))
    full = to_host(s.intersect(rays))
    for n in (1, 63, 64, 65, 257, 1000):
        out = torch.full((N_RANDOM, 12), -12345, dtype=torch.int32, device="cuda")
        s.intersect(rays[:n], out=out[:n])
        got = out.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint32), full[:n]), n
        assert (got[n:] == -12345).all(), n
    q = hrt.query_params()
    assert hrt.load().hrt_scene_intersect(s.h, ctypes.byref(q), None, 0, None, None) == hrt.OK
    assert hrt.load().hrt_scene_intersect_host(s.h, ctypes.byref(q), None, 0, None) == hrt.OK


@pytest.mark.gpu
def test_claims_of_several_blocks(scene, sim, monkeypatch):
    """A batch of 2 x 16384 blocks of 64 rays and more takes two blocks per atomicAdd (query.hip claim_blocks): the
    smallest size at which the kernel's inner loop runs twice, here with a ragged last block and a last claim cut short.
    HRT_QUERY_CLAIM forces 3 and 64 blocks per claim on a small batch: more blocks per claim than the batch has."""
    s, blob = scene("cornell")
    n = 2 * 16384 * 64 + 64 + 13
    rays = random_rays(s, (0.0, 1.0), n=n, seed=12)
    want = QS.words(QS.intersect(sim, s, rays, blob=blob))
    d = to_device(rays)
    assert np.array_equal(to_host(s.intersect(d)), want)
    for claim, m, flags in (("3", 64 * 7 + 5, 0), ("64", 64 * 9, hrt.QUERY_NO_LDS), ("2", 1, 0)):
        monkeypatch.setenv("HRT_QUERY_CLAIM", claim)
        assert np.array_equal(to_host(s.intersect(d[:m], flags=flags)), want[:m]), claim
        assert "HRT_QUERY_CLAIM=" + claim in hrt.last_launch()["knobs"]


# ------------------------------------------------------------------------------------------ 6. variants and errors
@pytest.mark.gpu
def test_host_variant_interval_outside_the_bvhs_and_errors(scene, sim):
    s, blob = scene("bvh_intervals")
    assert (blob[1].box_t0, blob[1].box_t1) == (0.25, 0.75)
    mn, mx = (-5.0, -1.0, -5.0), (5.0, 3.0, 5.0)
    rng = np.random.default_rng(3)
    rays = QS.make_rays(rng.uniform(mn, mx, (N_RANDOM, 3)), rng.normal(size=(N_RANDOM, 3)), time=rng.uniform(0, 1, N_RANDOM))
    for shutter in ((0.0, 1.0), (0.25, 0.75)):  # outside the boxes' interval: the reference test; inside: exact
        want = QS.intersect(sim, s, rays, shutter=shutter, blob=blob)
        assert ((want["flags"] & hrt.HIT_INVALID) != 0).any() == (shutter != (0.0, 1.0))
        assert ((want["flags"] & hrt.HIT_HIT) != 0).mean() > 0.2
        assert np.array_equal(device_hits(s, rays, shutter=shutter), QS.words(want))
        assert np.array_equal(QS.words(s.intersect(rays, shutter=shutter)), QS.words(want))  # numpy: the host variant
    q = hrt.query_params(flags=8)
    d = to_device(rays)
    L = hrt.load()
    assert L.hrt_scene_intersect(s.h, ctypes.byref(q), d.data_ptr(), 4, d.data_ptr() + 48 * 8, None) == hrt.ERR_INVALID_ARG
    with pytest.raises(hrt.HrtError) as e:
        s.intersect(rays, flags=16)
    assert e.value.status == hrt.ERR_INVALID_ARG
