"""Ray queries on the host (tests/native/query_sim.hip over csrc/query.h), without a GPU: the C layout and the argument
errors of the entry points, hit records against the oracle's primitives, first hits against the feature pass, the
medium's keyed draws, the interval rule, invalid rays and batch independence (the contract: include/hrt/hrt.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import feature_sim as FS
import hrt
import query_sim as QS
from conftest import ROOT, tool_env
from oracle import oracle as O

F = np.float32
INF = QS.INF
NEW = ["hrt_scene_intersect", "hrt_scene_intersect_host", "hrt_camera_rays", "hrt_camera_rays_host"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return QS.build(tmp_path_factory)


@pytest.fixture(scope="module")
def fsim(tmp_path_factory):
    return FS.build(tmp_path_factory)


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. layout and ABI
def test_struct_layouts(tmp_path):
    structs = {"hrt_ray": ["origin", "t_min", "direction", "t_max", "time", "pixel", "sample", "segment"],
               "hrt_hit": ["t", "prim", "material", "flags", "point", "u", "normal", "v"],
               "hrt_query_params": ["flags", "reserved", "time0", "time1", "seed"]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hrt/hrt.h"', "int main(void) {",
             '  printf("%d %d %d %d %d", (int)HRT_ABI_VERSION, HRT_HIT_HIT, HRT_HIT_FRONT, HRT_HIT_MEDIUM, HRT_HIT_INVALID);',
             '  printf(" %d %d %d", HRT_QUERY_SKIP_MEDIA, HRT_QUERY_NO_LDS, HRT_QUERY_REFERENCE_CULL);']
    for name, fields in structs.items():
        lines.append(f'  printf(" %zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          env=tool_env())
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert v[:8] == [6, 1, 2, 4, 8, 1, 2, 4]
    assert v[8:17] == [48, 0, 12, 16, 28, 32, 36, 40, 44]
    assert v[17:26] == [48, 0, 4, 8, 12, 16, 28, 32, 44]
    assert v[26:] == [24, 0, 4, 8, 12, 16]
    assert hrt.RAY_DTYPE.itemsize == 48 and [hrt.RAY_DTYPE.fields[f][1] for f in structs["hrt_ray"]] == v[9:17]
    assert hrt.HIT_DTYPE.itemsize == 48 and [hrt.HIT_DTYPE.fields[f][1] for f in structs["hrt_hit"]] == v[18:26]
    assert ctypes.sizeof(hrt.QueryParams) == 24 and [getattr(hrt.QueryParams, f).offset for f in structs["hrt_query_params"]] == v[27:]
    assert (hrt.HIT_HIT, hrt.HIT_FRONT, hrt.HIT_MEDIUM, hrt.HIT_INVALID) == (1, 2, 4, 8)
    assert (hrt.QUERY_SKIP_MEDIA, hrt.QUERY_NO_LDS, hrt.QUERY_REFERENCE_CULL) == (1, 2, 4)


def test_symbols_are_exported_and_bound():
    L = hrt.load()
    for name in NEW:
        assert hasattr(L, name) and name in hrt.EXPORTS and getattr(L, name).argtypes is not None
    assert L.hrt_abi_version() == 6 == hrt.ABI_VERSION
    assert callable(hrt.Scene.intersect) and callable(hrt.camera_rays) and callable(hrt.query_params)


def test_argument_errors_without_a_device():
    L = hrt.load()
    s = hrt.preset("two_spheres", 1)  # never committed
    rays, hits = QS.aligned(4, hrt.RAY_DTYPE), QS.aligned(4, hrt.HIT_DTYPE)
    r, h = rays.ctypes.data, hits.ctypes.data
    q = hrt.query_params()
    for fn, tail in ((L.hrt_scene_intersect, (None,)), (L.hrt_scene_intersect_host, ())):
        assert fn(None, ctypes.byref(q), r, 4, h, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, None, r, 4, h, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(q), None, 4, h, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(q), r, 4, None, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(q), r, 1 << 32, h, *tail) == hrt.ERR_INVALID_ARG
        for bad in (hrt.QueryParams(8, 0, 0.0, 1.0, 0), hrt.QueryParams(0, 1, 0.0, 1.0, 0), hrt.QueryParams(0, 0, 1.0, 0.5, 0),
                    hrt.QueryParams(0, 0, float("nan"), 1.0, 0), hrt.QueryParams(0, 0, 0.0, float("inf"), 0)):
            assert fn(s.h, ctypes.byref(bad), r, 4, h, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(q), r, 4, h, *tail) == hrt.ERR_STATE  # good arguments: the scene is not committed
        assert fn(s.h, ctypes.byref(hrt.QueryParams(0, 0, 0.5, 0.5, 0)), r, 4, h, *tail) == hrt.ERR_STATE  # time0 == time1 is an interval
    assert L.hrt_scene_intersect(s.h, ctypes.byref(q), r + 4, 1, h, None) == hrt.ERR_INVALID_ARG  # misaligned records
    assert (hits.view(np.uint8) == 0).all()
    cam, p = hrt.preset_camera(s.info, 8, 8), hrt.params(8, 8, 1)
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, 8, 8))
    big = QS.aligned(64, hrt.RAY_DTYPE)
    for fn, tail in ((L.hrt_camera_rays, (None,)), (L.hrt_camera_rays_host, ())):
        assert fn(None, ctypes.byref(cam), ctypes.byref(p), tile, 1, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, None, ctypes.byref(p), tile, 1, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(cam), None, tile, 1, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(cam), ctypes.byref(p), None, 1, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 0, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, None, *tail) == hrt.ERR_INVALID_ARG
        zero = hrt.params(8, 8, 0)
        assert fn(s.h, ctypes.byref(cam), ctypes.byref(zero), tile, 1, big.ctypes.data, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, big.ctypes.data, *tail) == hrt.ERR_STATE
    with pytest.raises(hrt.HrtError) as e:
        s.intersect(np.zeros(2, hrt.RAY_DTYPE))
    assert e.value.status == hrt.ERR_STATE


# ------------------------------------------------------------------------------------------ 2. records against the oracle
CLOUD_SEED = 5


def cloud():
    """30 spheres, 8 moving spheres with their own shutters and 6 rects (two per plane) under one bvh, built through the
    constructors, every primitive with a material of its own.  Returns (scene, [(oracle kind, oracle params, p0 of the
    flattened record)] in list order)."""
    rng = np.random.default_rng(CLOUD_SEED)
    s = hrt.Scene()
    prims, nodes = [], []

    def mat():
        return s.lambertian(s.solid(*rng.uniform(0.1, 0.9, 3)))

    for _ in range(30):
        c, r = F(rng.uniform(-4, 4, 3)), F(rng.uniform(0.3, 0.9))
        nodes.append(s.sphere(c, r, mat()))
        prims.append((0, np.array([*c, r], F), np.array([*c, r], F)))
    shutters = [(0.0, 1.0), (0.25, 0.75), (-0.5, 0.5), (1.5, 2.5), (0.0, 0.5), (0.5, 1.0), (0.1, 0.9), (-1.0, 2.0)]
    for t0, t1 in shutters:
        c0, r = F(rng.uniform(-4, 4, 3)), F(rng.uniform(0.3, 0.7))
        c1 = F(c0 + F(rng.uniform(-0.8, 0.8, 3)))
        nodes.append(s.moving_sphere(c0, c1, t0, t1, r, mat()))
        prims.append((1, np.array([*c0, *c1, t0, t1, r], F), np.array([*c0, r], F)))
    for plane in (hrt.PLANE_XY, hrt.PLANE_YZ, hrt.PLANE_ZX):
        for k in (F(-2.5), F(3.0)):
            a0, b0 = F(rng.uniform(-4, 0, 2))
            a1, b1 = F(a0 + F(rng.uniform(2, 4))), F(b0 + F(rng.uniform(2, 4)))
            if plane == hrt.PLANE_ZX:  # rect.rs:97-102 boxes a ZX rect with its two extents transposed, and BvhNode::hit then
                b0, b1 = a0, a1        # culls real hits, which no brute force over primitives does: equal extents have a true box
            nodes.append(s.rect(plane, a0, a1, b0, b1, k + F(plane) * F(0.25), mat()))
            prims.append((2, np.array([plane, a0, a1, b0, b1, k + F(plane) * F(0.25)], F), np.array([a0, a1, b0, b1], F)))
    s.set_root(s.bvh(nodes, 0.0, 1.0))
    return s, prims


def cloud_rays(n=2000):
    """Half from a point outside towards the cloud, half from origins inside its bounds with random directions."""
    rng = np.random.default_rng(CLOUD_SEED + 1)
    o = np.empty((n, 3), F)
    d = np.empty((n, 3), F)
    o[:n // 2] = (14.0, 3.0, 9.0)
    d[:n // 2] = rng.uniform(-7, 7, (n // 2, 3)) - o[:n // 2]  # not normalised, about 18 long
    o[n // 2:] = rng.uniform(-4, 4, (n - n // 2, 3))
    d[n // 2:] = rng.normal(size=(n - n // 2, 3))
    return QS.make_rays(o, d, time=rng.uniform(0, 1, n), t_min=0.001, t_max=np.inf)


def brute_force(prims, rays):
    """Per ray (winner or -1, the oracle's 10-float record, how many primitives hit at the winning t)."""
    L = O.load()
    out = []
    for r in rays:
        ray = np.array([*r["origin"], *r["direction"], r["time"]], F)
        tmax, win, rec, ts = float(r["t_max"]), -1, None, []
        for i, (kind, p, _) in enumerate(prims):
            o10 = np.zeros(10, F)
            if L.oracle_prim_hit(kind, p.ctypes.data, ray.ctypes.data, float(r["t_min"]), tmax, o10.ctypes.data):
                tmax, win, rec = float(o10[0]), i, o10
            full = np.zeros(10, F)  # the hit against the whole interval, for the uniqueness of the winning t
            if L.oracle_prim_hit(kind, p.ctypes.data, ray.ctypes.data, float(r["t_min"]), float(r["t_max"]), full.ctypes.data):
                ts.append(full[0])
        out.append((win, rec, 0 if win < 0 else sum(1 for t in ts if t == rec[0])))
    return out


def test_records_equal_the_oracles_primitives(sim):
    """Measured on the CPU with CLOUD_SEED = 5: 0 of the 2 000 rays disagree with the brute force in t (the bound: at most
    1, the reference box test's ~1e-7 of grazing hits); 679 hit, each at a t no other primitive shares, and 1 321 miss."""
    s, prims = cloud()
    rays = cloud_rays()
    blob = hrt.scene_blob(s)
    hits = QS.intersect(sim, s, rays, blob=blob)
    want = brute_force(prims, rays)
    n_hit = sum(1 for w, _, _ in want if w >= 0)
    print("hits", n_hit, "misses", len(rays) - n_hit)
    assert n_hit >= len(rays) // 4 and len(rays) - n_hit >= len(rays) // 4
    t_differs, compared = 0, 0
    for h, r, (win, rec, same_t) in zip(hits, rays, want):
        if win < 0:
            t_differs += int(h["flags"] != 0)
            if h["flags"] == 0:
                assert h["t"] == r["t_max"] and h["prim"] == h["material"] == QS.MISS
                assert (QS.words(h)[0, 4:] == 0).all()
            continue
        if not (h["flags"] & hrt.HIT_HIT) or u32(h["t"]) != u32(rec[0]):
            t_differs += 1
            continue
        if same_t != 1:
            continue
        compared += 1
        got = np.array([h["t"], *h["point"], *h["normal"], h["u"], h["v"]], F)
        assert np.array_equal(u32(got), u32(rec[:9])), (win, got, rec)
        assert bool(h["flags"] & hrt.HIT_FRONT) == bool(rec[9]) and not h["flags"] & (hrt.HIT_MEDIUM | hrt.HIT_INVALID)
        record = hrt.prim_record(s, int(h["prim"]))
        assert np.array_equal(u32(record[:4]), u32(prims[win][2])), win  # reference pre-order: the flattened record
        assert h["material"] == record[11:12].view(np.uint32)[0] >> 4 == win  # the material made for primitive `win`
    print("t differs", t_differs, "compared", compared)
    assert t_differs == 0  # the issue allows 1; this seed has none
    assert compared >= n_hit - 5
    # the same hits under the reference test alone and from the other instantiation's walk
    assert np.array_equal(QS.words(QS.intersect(sim, s, rays, flags=hrt.QUERY_REFERENCE_CULL, blob=blob)), QS.words(hits))


# ------------------------------------------------------------------------------------------ 3. first hits against the feature pass
def first_hits(sim, s, cam, p, **kw):
    rays = QS.camera_rays(sim, cam, p)
    hits = QS.intersect(sim, s, rays, seed=p.seed, shutter=(cam.time0, cam.time1), **kw)
    return rays, hits


def depth_of(rays, hits):
    d = rays["direction"]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.where(hits["flags"] & hrt.HIT_HIT, hits["t"] * np.sqrt(dd, dtype=F), F(0)).astype(F)


@pytest.mark.parametrize("name,w,h,spp", [("random", 32, 18, 3), ("cornell_smoke", 16, 16, 2)])
def test_first_hits_equal_the_feature_pass(sim, fsim, name, w, h, spp):
    s = hrt.preset(name, 1)
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, spp, 50, 7, tuple(s.info.background))
    rays, hits = first_hits(sim, s, cam, p)
    a, kinds, _ = FS.run(fsim, s, cam, p)
    a, kinds = a.reshape(-1, 8), kinds.reshape(-1)
    hit = (hits["flags"] & hrt.HIT_HIT) != 0
    assert np.array_equal(hit, a[:, 3] == 1.0) and hit.sum() > len(hit) // 2
    assert np.array_equal(u32(hits["normal"]), u32(a[:, 4:7]))
    assert np.array_equal(u32(depth_of(rays, hits)), u32(a[:, 7]))
    medium = (hits["flags"] & hrt.HIT_MEDIUM) != 0
    assert np.array_equal(medium, kinds == FS.M_ISOTROPIC)
    assert (hits["normal"][medium] == 0).all() and not (hits["flags"][medium] & hrt.HIT_FRONT).any()
    assert (medium.sum() > 20) == (name == "cornell_smoke")
    # the keys and the interval hrt_camera_rays writes
    px = np.repeat(np.arange(w * h, dtype=np.uint32), spp)
    assert np.array_equal(rays["pixel"], px) and np.array_equal(rays["sample"], np.tile(np.arange(spp, dtype=np.uint32), w * h))
    assert (rays["segment"] == 0).all() and (rays["t_min"] == p.t_min).all() and np.isposinf(rays["t_max"]).all()
    # a later pass's rays are those of that sample index
    later = QS.camera_rays(sim, cam, hrt.params(w, h, 1, 50, 7, tuple(s.info.background), sample_offset=spp - 1))
    assert np.array_equal(QS.words(later), QS.words(rays[spp - 1::spp]))


# ------------------------------------------------------------------------------------------ 4. media
def test_media_flag_and_segment_key(sim):
    s = hrt.preset("cornell_smoke", 1)
    w = h = 16
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 2, 50, 7, tuple(s.info.background))
    rays, hits = first_hits(sim, s, cam, p)
    _, clear = first_hits(sim, s, cam, p, flags=hrt.QUERY_SKIP_MEDIA)
    assert ((hits["flags"] & hrt.HIT_MEDIUM) != 0).sum() > 20
    assert not (clear["flags"] & hrt.HIT_MEDIUM).any()
    assert (clear["t"] >= hits["t"]).all() and (clear["t"] > hits["t"]).any()
    moved = rays.copy()
    moved["segment"] = 1
    other = QS.intersect(sim, s, moved, seed=p.seed, shutter=(cam.time0, cam.time1))
    medium = ((hits["flags"] | other["flags"]) & hrt.HIT_MEDIUM) != 0
    assert (QS.words(other)[medium] != QS.words(hits)[medium]).any()
    assert np.array_equal(QS.words(other)[~medium], QS.words(hits)[~medium])  # surfaces draw nothing
    # medium ids: the two boxes' media, each with its phase function's material
    ids = set(zip(hits["prim"][(hits["flags"] & hrt.HIT_MEDIUM) != 0].tolist(), hits["material"][(hits["flags"] & hrt.HIT_MEDIUM) != 0].tolist()))
    assert len(ids) == 2 and {i for i, _ in ids} == {0, 1}


# ------------------------------------------------------------------------------------------ 5. intervals and invalid rays
def one_sphere():
    s = hrt.Scene()
    s.set_root(s.bvh([s.sphere((0, 0, 0), 1.0, s.lambertian(s.solid(0.5, 0.5, 0.5)))], 0.0, 1.0))
    return s


def test_interval_ends(sim):
    s = one_sphere()
    base = dict(origin=(0.3, 0.2, 5), direction=(0, 0, -2.0), time=0.5)
    h0 = QS.intersect(sim, s, QS.make_rays(**base))[0]
    assert h0["flags"] == hrt.HIT_HIT | hrt.HIT_FRONT and 1.9 < h0["t"] < 2.1
    t = F(h0["t"])
    below, above = np.nextafter(t, F(0)), np.nextafter(t, INF)
    rays = np.concatenate([QS.make_rays(t_max=below, **base), QS.make_rays(t_max=t, **base), QS.make_rays(t_min=t, **base),
                           QS.make_rays(t_min=above, **base)])
    miss, at_max, at_min, exit_ = QS.intersect(sim, s, rays)
    assert miss["flags"] == 0 and miss["t"] == below and miss["prim"] == QS.MISS
    assert np.array_equal(QS.words(at_max), QS.words(h0)) and np.array_equal(QS.words(at_min), QS.words(h0))  # both ends are accepted
    assert exit_["flags"] == hrt.HIT_HIT and exit_["t"] > 2.9 and exit_["normal"][2] > 0  # the exit: front clear, the normal turned to face the ray
    assert exit_["prim"] == 0 and exit_["material"] == 0


def test_invalid_rays(sim):
    s = one_sphere()
    good = dict(origin=(0, 0, 5), direction=(0, 0, -1), time=0.5, t_min=0.001, t_max=np.inf)
    nan, inf = float("nan"), float("inf")
    cases = [dict(origin=(nan, 0, 5)), dict(origin=(0, inf, 5)), dict(direction=(0, nan, -1)), dict(direction=(0, 0, -inf)),
             dict(time=nan), dict(time=inf), dict(t_min=nan), dict(t_min=-inf), dict(t_max=nan), dict(direction=(0, 0, 0)),
             dict(t_min=2.0, t_max=2.0), dict(t_min=3.0, t_max=1.0), dict(time=-0.25), dict(time=1.5)]
    rays = np.concatenate([QS.make_rays(**good)] + [QS.make_rays(**{**good, **c}) for c in cases] + [QS.make_rays(**{**good, "direction": (0, 0, -0.0)})])
    hits = QS.intersect(sim, s, rays)
    assert hits[0]["flags"] == hrt.HIT_HIT | hrt.HIT_FRONT
    want = np.zeros(12, np.uint32)
    want[1] = want[2] = QS.MISS
    want[3] = hrt.HIT_INVALID
    for k in range(1, len(rays)):
        assert np.array_equal(QS.words(hits[k:k + 1])[0], want), k
    # the declared interval is the params': the same ray is valid under a shutter that holds its time
    assert QS.intersect(sim, s, QS.make_rays(**{**good, "time": 1.5}), shutter=(1.0, 2.0))[0]["flags"] & hrt.HIT_HIT
    assert QS.intersect(sim, s, QS.make_rays(**{**good, "t_max": inf, "t_min": -5.0}))[0]["flags"] & hrt.HIT_HIT  # -5 < t_min is finite


# ------------------------------------------------------------------------------------------ 6. batch independence
def test_batch_independence(sim):
    s = hrt.preset("cornell_smoke", 1)
    cam = hrt.preset_camera(s.info, 16, 16)
    p = hrt.params(16, 16, 1, 50, 7, tuple(s.info.background))
    rays = QS.camera_rays(sim, cam, p)
    kw = dict(seed=p.seed, shutter=(cam.time0, cam.time1), blob=hrt.scene_blob(s))
    hits = QS.words(QS.intersect(sim, s, rays, **kw))
    assert np.array_equal(QS.words(QS.intersect(sim, s, rays[::-1].copy(), **kw))[::-1], hits)
    parts = [QS.words(QS.intersect(sim, s, rays[a:b].copy(), **kw)) for a, b in ((0, 1), (1, 64), (64, 129), (129, 256))]
    assert np.array_equal(np.concatenate(parts), hits)
    for n in (1, 63, 65):
        assert np.array_equal(QS.words(QS.intersect(sim, s, rays[:n].copy(), **kw)), hits[:n])
