"""Scatter queries on the host (tests/native/scatter_sim.hip over csrc/scatter.h), without a GPU: the C layout and the
argument errors of the entry points; the loop camera paths -> (intersect -> scatter) until done against the lane
simulator's render bit for bit and against the oracle; depth caps; the conditions that keep those comparisons from hiding
anything; malformed records; batch independence (the contract: include/hrt/hrt.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hrt
import query_sim as QS
import scatter_sim as SS
from conftest import ROOT, tool_env
from oracle import oracle as O

F = np.float32
TOL = 1e-3
NEW = ["hrt_scene_scatter", "hrt_scene_scatter_host", "hrt_camera_paths", "hrt_camera_paths_host"]
SPHERE_SCENES = {"random", "motion", "earth", "two_perlin_spheres"}  # the sphere kernel's lane (lane_sim kernel 0)
# (preset, width, height, sample indices), all at depth 50
INPUTS = [("random", 32, 18, (0, 1, 2, 3)), ("cornell", 16, 16, (0, 1)), ("cornell_smoke", 16, 16, (0, 1)), ("earth", 16, 16, (0,)),
          ("two_perlin_spheres", 16, 16, (0,)), ("motion", 32, 18, (0,))]
SEED = 3
M_LAMBERTIAN, M_METAL, M_DIELECTRIC, M_DIFFUSE_LIGHT, M_ISOTROPIC = range(5)


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    return SS.build(tmp_path_factory)


class Setup:
    def __init__(self, name, w, h, earth):
        self.name, self.w, self.h = name, w, h
        self.scene = hrt.preset(name, 1, earth)
        self.cam = hrt.preset_camera(self.scene.info, w, h)
        self.blob = hrt.scene_blob(self.scene)

    def params(self, k, depth=50):
        return hrt.params(self.w, self.h, 1, depth, SEED, tuple(self.scene.info.background), sample_offset=k)


_loops = {}


def run_loop(sims, earth, name, w, h, k, depth=50):
    """The loop's result for one input, computed once per module: (setup, paths, n_rays, scattered)."""
    key = (name, w, h, k, depth)
    if key not in _loops:
        if (name, w, h) not in _loops:
            _loops[(name, w, h)] = Setup(name, w, h, earth)
        st = _loops[(name, w, h)]
        paths, n_rays, scattered = SS.loop(sims, st.scene, st.cam, st.params(k, depth), blob=st.blob)
        paths.flags.writeable = False
        _loops[key] = (st, paths, n_rays, scattered)
    return _loops[key]


CASES = [(n, w, h, k) for n, w, h, ks in INPUTS for k in ks]


# ------------------------------------------------------------------------------------------ 1. layout and ABI
def test_struct_layouts(tmp_path):
    structs = {"hrt_path": ["rng", "throughput", "depth_left", "radiance", "flags"],
               "hrt_scatter_params": ["flags", "reserved", "background", "reserved2"]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hrt/hrt.h"', "int main(void) {",
             '  printf("%d %d %d %d %d %d", (int)HRT_ABI_VERSION, HRT_PATH_DONE, HRT_PATH_MISSED, HRT_PATH_ABSORBED, HRT_PATH_DEPTH,'
             ' HRT_PATH_INVALID);', '  printf(" %zu %zu", sizeof(hrt_ray), sizeof(hrt_hit));']
    for name, fields in structs.items():
        lines.append(f'  printf(" %zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          env=tool_env())
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert v[:6] == [6, 1, 2, 4, 8, 16]
    assert v[6:8] == [48, 48]
    assert v[8:14] == [48, 0, 16, 28, 32, 44]
    assert v[14:] == [24, 0, 4, 8, 20]
    assert hrt.PATH_DTYPE.itemsize == 48 and [hrt.PATH_DTYPE.fields[f][1] for f in structs["hrt_path"]] == v[9:14]
    assert ctypes.sizeof(hrt.ScatterParams) == 24
    assert [getattr(hrt.ScatterParams, f).offset for f in structs["hrt_scatter_params"]] == v[15:]
    assert (hrt.PATH_DONE, hrt.PATH_MISSED, hrt.PATH_ABSORBED, hrt.PATH_DEPTH, hrt.PATH_INVALID) == (1, 2, 4, 8, 16)


def test_symbols_are_exported_and_bound():
    L = hrt.load()
    for name in NEW:
        assert hasattr(L, name) and name in hrt.EXPORTS and getattr(L, name).argtypes is not None
    assert L.hrt_abi_version() == 6 == hrt.ABI_VERSION
    assert callable(hrt.Scene.scatter) and callable(hrt.camera_paths) and callable(hrt.scatter_params) and callable(hrt.trace_paths)


def test_argument_errors_without_a_device():
    L = hrt.load()
    s = hrt.preset("two_spheres", 1)  # never committed
    rays, hits, paths = QS.aligned(4, hrt.RAY_DTYPE), QS.aligned(4, hrt.HIT_DTYPE), QS.aligned(4, hrt.PATH_DTYPE)
    r, h, q = rays.ctypes.data, hits.ctypes.data, paths.ctypes.data
    sp = hrt.scatter_params((0.7, 0.8, 1.0))
    for fn, tail in ((L.hrt_scene_scatter, (None,)), (L.hrt_scene_scatter_host, ())):
        assert fn(None, ctypes.byref(sp), r, h, q, 4, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, None, r, h, q, 4, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(sp), None, h, q, 4, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(sp), r, None, q, 4, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(sp), r, h, None, 4, *tail) == hrt.ERR_INVALID_ARG
        assert fn(s.h, ctypes.byref(sp), r, h, q, 1 << 32, *tail) == hrt.ERR_INVALID_ARG
        bg = hrt._F3(0.5, 0.5, 0.5)
        for bad in (hrt.ScatterParams(1, 0, bg, 0), hrt.ScatterParams(0, 1, bg, 0), hrt.ScatterParams(0, 0, bg, 1),
                    hrt.scatter_params((float("nan"), 0, 0)), hrt.scatter_params((0, float("inf"), 0)),
                    hrt.scatter_params((0, 0, -float("inf")))):
            assert fn(s.h, ctypes.byref(bad), r, h, q, 4, *tail) == hrt.ERR_INVALID_ARG
            assert b"scatter params" in L.hrt_last_error()
        assert fn(s.h, ctypes.byref(sp), r, h, q, 4, *tail) == hrt.ERR_STATE  # good arguments: the scene is not committed
    for k in range(3):  # misaligned records, each buffer in turn
        ptrs = [r, h, q]
        ptrs[k] += 4
        assert L.hrt_scene_scatter(s.h, ctypes.byref(sp), *ptrs, 1, None) == hrt.ERR_INVALID_ARG
    assert (rays.view(np.uint8) == 0).all() and (paths.view(np.uint8) == 0).all()
    cam, p = hrt.preset_camera(s.info, 8, 8), hrt.params(8, 8, 1)
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, 8, 8))
    br, bp = QS.aligned(64, hrt.RAY_DTYPE), QS.aligned(64, hrt.PATH_DTYPE)
    for fn, tail in ((L.hrt_camera_paths, (None,)), (L.hrt_camera_paths_host, ())):
        a = (s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, br.ctypes.data, bp.ctypes.data)
        for i in (0, 1, 2, 3, 5, 6):
            assert fn(*a[:i], None, *a[i + 1:], *tail) == hrt.ERR_INVALID_ARG
        assert fn(*a[:4], 0, *a[5:], *tail) == hrt.ERR_INVALID_ARG
        zero = hrt.params(8, 8, 0)
        assert fn(*a[:2], ctypes.byref(zero), *a[3:], *tail) == hrt.ERR_INVALID_ARG
        assert fn(*a, *tail) == hrt.ERR_STATE
    assert L.hrt_camera_paths(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, br.ctypes.data, bp.ctypes.data + 4, None) == \
        hrt.ERR_INVALID_ARG
    with pytest.raises(hrt.HrtError) as e:
        s.scatter(np.zeros(2, hrt.RAY_DTYPE), np.zeros(2, hrt.HIT_DTYPE), np.zeros(2, hrt.PATH_DTYPE), (0, 0, 0))
    assert e.value.status == hrt.ERR_STATE


# ------------------------------------------------------------------------------------------ 2. the camera paths
def test_camera_paths_are_the_camera_rays_and_start_samples_state(sims, earth):
    st = Setup("random", 32, 18, earth)
    p = hrt.params(32, 18, 3, 50, SEED, sample_offset=5)
    rays, paths = SS.camera_paths(sims, st.cam, p)
    assert np.array_equal(SS.words(rays), SS.words(QS.camera_rays(sims.Q, st.cam, p)))
    assert (paths["throughput"] == 1).all() and (SS.words(paths)[:, 8:] == 0).all() and (paths["depth_left"] == 50).all()
    assert (paths["rng"] != 0).any(axis=1).all() and len(np.unique(paths["rng"], axis=0)) == len(paths)
    region = (5, 3, 9, 7)
    rr, pr = SS.camera_paths(sims, st.cam, p, region)
    full = SS.words(paths).reshape(18, 32, 3, 12)[3:10, 5:14].reshape(-1, 12)
    assert np.array_equal(SS.words(pr), full)
    # a depth cap of 0: every path starts finished and its ray invalid
    p0 = hrt.params(32, 18, 1, 0, SEED)
    r0, q0 = SS.camera_paths(sims, st.cam, p0)
    assert (q0["flags"] == hrt.PATH_DONE | hrt.PATH_DEPTH).all() and (r0["t_max"] == r0["t_min"]).all()
    assert (QS.intersect(sims.Q, st.scene, r0, blob=st.blob)["flags"] == hrt.HIT_INVALID).all()


# ------------------------------------------------------------------------------------------ 3. the loop against the render
@pytest.mark.parametrize("name,w,h,k", CASES)
def test_loop_equals_the_lane_simulators_render(sims, earth, name, w, h, k):
    st, paths, n_rays, _ = run_loop(sims, earth, name, w, h, k)
    ref, segments = SS.lane_render(sims, st.scene, st.cam, st.params(k), blob=st.blob, kernel=0 if name in SPHERE_SCENES else 1)
    assert (paths["flags"] & hrt.PATH_DONE).all()
    assert np.array_equal(SS.frame(paths, w, h).view(np.uint32), ref[..., :3].view(np.uint32))
    assert n_rays == segments


@pytest.mark.parametrize("name,w,h,k", CASES)
def test_loop_against_the_oracle(sims, earth, name, w, h, k):
    st, paths, n_rays, _ = run_loop(sims, earth, name, w, h, k)
    ref, cnt = O.OracleScene(hrt.PRESETS[name], 1, earth).render(w, h, 1, 50, seed=SEED, threads=8, sample_offset=k)
    assert n_rays == cnt["segments"]
    err = float(np.abs(SS.frame(paths, w, h) - ref[..., :3]).max())
    print(f"{name} {w}x{h} k={k}: L-inf {err:.3g}, {n_rays} rays")
    assert err <= TOL


@pytest.mark.parametrize("name,w,h", [("random", 32, 18), ("cornell", 16, 16)])
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_depth_caps(sims, earth, name, w, h, depth):
    st, paths, n_rays, _ = run_loop(sims, earth, name, w, h, 0, depth)
    ref, segments = SS.lane_render(sims, st.scene, st.cam, st.params(0, depth), blob=st.blob, kernel=0 if name in SPHERE_SCENES else 1)
    assert (paths["flags"] & hrt.PATH_DONE).all() and n_rays == segments
    assert np.array_equal(SS.frame(paths, w, h).view(np.uint32), ref[..., :3].view(np.uint32))
    oref, cnt = O.OracleScene(hrt.PRESETS[name], 1, earth).render(w, h, 1, depth, seed=SEED, threads=8)
    assert n_rays == cnt["segments"] and np.abs(SS.frame(paths, w, h) - oref[..., :3]).max() <= TOL
    if depth == 0:
        assert n_rays == 0 and (paths["radiance"] == 0).all()
    else:
        assert (paths["flags"] & hrt.PATH_DEPTH).any() and (paths["depth_left"][(paths["flags"] & hrt.PATH_DEPTH) != 0] == 0).all()


def test_the_inputs_exercise_every_outcome_and_material(sims, earth):
    """What keeps the comparisons above from hiding anything: no path ends INVALID, every other way to end occurs, and
    every material kind of the presets is scattered from."""
    ends, scattered = np.zeros(32, np.int64), np.zeros(8, np.int64)
    per_scene = {}
    for name, w, h, k in CASES:
        _, paths, _, sc = run_loop(sims, earth, name, w, h, k)
        ends += np.bincount(paths["flags"], minlength=32)[:32]
        scattered += sc
        per_scene[name] = per_scene.get(name, 0) + sc
    print("ends by flags:", {int(f): int(c) for f, c in enumerate(ends) if c}, "scatter steps by kind:", scattered[:5].tolist())
    assert ends[[f for f in range(32) if f & hrt.PATH_INVALID]].sum() == 0
    for why in (hrt.PATH_MISSED, hrt.PATH_ABSORBED, hrt.PATH_DEPTH):
        assert ends[hrt.PATH_DONE | why] > 0
    assert ends.sum() == ends[[hrt.PATH_DONE | w for w in (hrt.PATH_MISSED, hrt.PATH_ABSORBED, hrt.PATH_DEPTH)]].sum()
    assert (scattered[:5] > 0).all() and (scattered[5:] == 0).all()
    assert per_scene["cornell_smoke"][M_ISOTROPIC] > 0 and per_scene["cornell"][M_DIFFUSE_LIGHT] > 0
    assert per_scene["random"][M_METAL] > 0 and per_scene["random"][M_DIELECTRIC] > 0


# ------------------------------------------------------------------------------------------ 4. malformed records
def three_material_scene():
    """Two spheres and a light through the constructors: exactly three materials (ids 0, 1, 2)."""
    s = hrt.Scene()
    ground = s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))
    metal = s.metal((0.8, 0.6, 0.2), 0.3)
    light = s.diffuse_light(s.solid(4, 4, 4))
    s.set_root(s.bvh([s.sphere((0, -100.5, -1), 100, ground), s.sphere((0, 0, -1), 0.5, metal), s.sphere((0, 2, -1), 0.5, light)]))
    return s, (ground, metal, light)


def test_robustness_of_a_mixed_batch(sims):
    s, mats = three_material_scene()
    assert sorted(mats) == [0, 1, 2]
    blob = hrt.scene_blob(s)
    cam = hrt.camera((0, 0.5, 2), (0, 0, -1), 60, 0.0, 3.0, 0.0, 1.0, 16, 16)
    p = hrt.params(16, 16, 1, 50, SEED)
    rays, paths = SS.camera_paths(sims, cam, p)
    hits = QS.intersect(sims.Q, s, rays, seed=SEED, blob=blob)
    n = len(rays)
    is_hit = (hits["flags"] & hrt.HIT_HIT) != 0
    assert is_hit.sum() > 40 and (~is_hit).sum() > 40
    good_r, good_p = SS.scatter(sims, blob, rays, hits, paths, (0.7, 0.8, 1.0), n_mats=3)
    assert (good_p["flags"] & hrt.PATH_INVALID == 0).all()
    hit_at = np.flatnonzero(is_hit)
    rays, hits, paths = rays.copy(), hits.copy(), paths.copy()
    done = np.arange(0, n, 7)  # finished paths of every kind, with contents no step would leave
    paths["flags"][done] = hrt.PATH_DONE | np.array([0, 2, 4, 8, 16])[np.arange(len(done)) % 5]
    bad_mat, bad_mat2, inv, unknown, no_hit_bits, zero_rng, no_depth = (hit_at[i::7][:5] for i in range(7))
    hits["material"][bad_mat] = 3            # the first id out of range
    hits["material"][bad_mat2] = 0xFFFFFFFF
    hits["flags"][inv] |= hrt.HIT_INVALID
    hits["flags"][unknown] |= np.array([16, 32, 1 << 20, 1 << 31, 64], np.uint32)
    hits["flags"][no_hit_bits] = np.array([2, 4, 6, 2, 4], np.uint32)  # bits without HIT_HIT
    paths["rng"][zero_rng] = 0
    paths["depth_left"][no_depth] = 0
    out_r, out_p = SS.scatter(sims, blob, rays, hits, paths, (0.7, 0.8, 1.0), n_mats=3)
    live = np.ones(n, bool)
    live[done] = False
    # DONE on entry: not one byte of the ray or the path is written
    assert np.array_equal(SS.words(out_r)[done], SS.words(rays)[done]) and np.array_equal(SS.words(out_p)[done], SS.words(paths)[done])
    refused = np.concatenate([bad_mat, bad_mat2, inv, unknown, no_hit_bits, zero_rng])
    refused = refused[live[refused]]
    assert len(refused) > 15
    # a refused record: INVALID | DONE, nothing else of the path, and of the ray only t_max
    want_p = paths[refused].copy()
    want_p["flags"] |= hrt.PATH_INVALID | hrt.PATH_DONE
    assert np.array_equal(SS.words(out_p)[refused], SS.words(want_p))
    want_r = rays[refused].copy()
    want_r["t_max"] = want_r["t_min"]
    assert np.array_equal(SS.words(out_r)[refused], SS.words(want_r))
    capped = no_depth[live[no_depth]]
    want_p = paths[capped].copy()
    want_p["flags"] |= hrt.PATH_DEPTH | hrt.PATH_DONE
    assert len(capped) and np.array_equal(SS.words(out_p)[capped], SS.words(want_p))
    # every other record is what the untouched batch gave
    rest = live.copy()
    rest[refused] = rest[capped] = False
    assert np.array_equal(SS.words(out_r)[rest], SS.words(good_r)[rest]) and np.array_equal(SS.words(out_p)[rest], SS.words(good_p)[rest])
    # id 2 is in range, id 3 is not: the bound is the scene's material count
    assert (good_p["flags"][hit_at[hits["material"][hit_at] == 2]] & hrt.PATH_INVALID == 0).all()
    # the rays of finished paths are invalid to the intersect
    finished = (out_p["flags"] & hrt.PATH_DONE) != 0
    finished[done] = False  # (made up above: their rays were never finished by a scatter)
    again = QS.intersect(sims.Q, s, out_r, seed=SEED, blob=blob)
    assert finished.sum() > 60 and (again["flags"][finished] == hrt.HIT_INVALID).all()
    assert (again["flags"][~finished & live] != hrt.HIT_INVALID).all()


def test_batch_independence(sims, earth):
    st = Setup("cornell_smoke", 16, 16, earth)
    p = st.params(0)
    rays, paths = SS.camera_paths(sims, st.cam, p)
    rng = np.random.default_rng(11)
    for _ in range(3):  # three rounds deep, so that lights, media and finished paths are all in the batch
        hits = QS.intersect(sims.Q, st.scene, rays, seed=SEED, shutter=(st.cam.time0, st.cam.time1), blob=st.blob)
        r1, p1 = SS.scatter(sims, st.blob, rays, hits, paths, tuple(p.background))
        perm = rng.permutation(len(rays))
        r2, p2 = SS.scatter(sims, st.blob, rays[perm], hits[perm], paths[perm], tuple(p.background))
        assert np.array_equal(SS.words(r2), SS.words(r1)[perm]) and np.array_equal(SS.words(p2), SS.words(p1)[perm])
        sub = perm[:37]  # ... and of n
        r3, p3 = SS.scatter(sims, st.blob, rays[sub], hits[sub], paths[sub], tuple(p.background))
        assert np.array_equal(SS.words(r3), SS.words(r1)[sub]) and np.array_equal(SS.words(p3), SS.words(p1)[sub])
        rays, paths = r1, p1
    assert 0 < ((paths["flags"] & hrt.PATH_DONE) != 0).sum() < len(paths)
