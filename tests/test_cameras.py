"""Cameras and shutters the presets never use (tests/cameras.py), on the host: the kernels' per-lane code
(tests/native/lane_sim.hip over csrc/lane.h) against the oracle rendering from the same camera, and the per-cell
leaf lists (csrc/primary_list.h) against the walk they replace.  tests/test_gpu_cameras.py runs the same table on
the GPU.

Lanes: every (scene, camera) at 40x24x8 (sphere scenes), 24x24x8 (cornell, cornell_smoke), 24x24x2 (final), seed 3,
depth 50, under EXACT culling: the oracle's segment count, finite pixels, L-inf <= 1e-3, and the same bits as the
lanes under the verbatim reference box test.

Shutters: inside [0, 1] the EXACT lanes equal the oracle.  For an interval that reaches outside [0, 1] (the interval
the BVH boxes are built for) only the reference box test is faithful, which is what render.hip plan() falls back
to: the REFERENCE lanes equal the oracle, and on `random` (-0.5, 1.5) the EXACT lanes' segment count differs from
the oracle's (21294 against 21232 when this was written), so the GPU shutter cases fail without plan()'s guard.

Lists: tests/test_primary_lists.py's check (missing == mismatch == hull_out == 0) at every sphere camera on
`random`, `motion` and `two_spheres`; on the first two at the list-friendly cameras the lists must really be walked (list_steps > 0, overflow share
<= 0.25 at 1920x1080; the builder measured <= 0.133).  `far` overflows every cell and `opp_octant_bigap` most:
their share is printed.  The shim built without the hull's pads fails the check at the new cameras too.
"""
import ctypes

import numpy as np
import pytest

import cameras as C
import hrt
from oracle import oracle as O
from test_lane_sim import BASIC_SCENES, CULL_EXACT, CULL_REFERENCE, TOL, _build_sim
from test_primary_lists import CAP, _build, _cells, _check

SEED = 3


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build_sim(tmp_path_factory)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _build(tmp_path_factory)


@pytest.fixture(scope="module")
def lib_no_pad(tmp_path_factory):
    return _build(tmp_path_factory, ("-DHRT_PL_NO_PAD",))


@pytest.fixture(scope="module")
def oracles(earth):
    """One oracle scene per preset (their renders do not change them)."""
    out = {}

    def get(name):
        if name not in out:
            out[name] = O.OracleScene(hrt.PRESETS[name], 1, earth)
        return out[name]

    return get


def _lanes(L, earth, name, sp, cull, w, h, spp, t_min=0.001):
    """lane_sim_render of preset `name` from the camera spec `sp`: kernel 0 (sphere scenes) or 1 (general)."""
    s = hrt.preset(name, 1, earth)
    cam = C.hrt_camera(sp, w, h)
    blob, info = hrt.scene_blob(s)
    p = hrt.params(w, h, spp, 50, SEED, tuple(s.info.background), t_min=t_min)
    out = np.zeros((h, w, 4), np.float32)
    cnt = np.zeros(8, np.uint64)
    kernel = 0 if name in BASIC_SCENES else 1
    rc = L.lane_sim_render(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), kernel, cull, 0, 0, w, h,
                           out.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out, int(cnt[0]), s


def _info(name, earth):
    return hrt.preset(name, 1, earth).info


def test_oracle_camera_argument_of_the_presets_own_values_is_the_default_render(earth, oracles):
    """camera= set to the preset's own values returns the same bytes and counters as no argument (render and
    render_rows go through the same Camera constructor and the same render())."""
    for name in ("random", "final"):
        o = oracles(name)
        own = (o.look_from, o.look_at, o.fov, o.aperture, o.focus_dist, o.time0, o.time1)
        mine = C.spec(name, None, _info(name, earth))  # the library's preset camera holds the same values
        assert np.array_equal(np.hstack([np.ravel(v) for v in own]).astype(np.float32),
                              np.hstack([np.ravel(v) for v in mine]).astype(np.float32))
        a, ca = o.render(24, 16, 2, seed=SEED)
        b, cb = o.render(24, 16, 2, seed=SEED, camera=own)
        assert a.tobytes() == b.tobytes() and ca == cb
        a, ca = o.render_rows(24, 16, 2, [3, 11], seed=SEED, x0=2, w=19, task_w=7)
        b, cb = o.render_rows(24, 16, 2, [3, 11], seed=SEED, x0=2, w=19, task_w=7, camera=own)
        assert a.tobytes() == b.tobytes() and ca == cb
        c, _ = o.render(24, 16, 2, seed=SEED, camera=(*own[:2], o.fov * 0.5, *own[3:]))
        assert c.tobytes() != a.tobytes()  # the argument is used


@pytest.mark.parametrize("name,cam", C.scene_cameras())
def test_lanes_match_oracle_at_camera(sim, earth, oracles, name, cam):
    w, h, spp = C.ORACLE_SIZE[name]
    sp = C.spec(name, cam)
    img, seg, _ = _lanes(sim, earth, name, sp, CULL_EXACT, w, h, spp)
    ref, cnt = oracles(name).render(w, h, spp, 50, seed=SEED, camera=sp)
    linf = float(np.abs(img - ref).max())
    print(f"{name} {cam}: segments {seg} (oracle {cnt['segments']}), L-inf {linf:.3g}")
    assert seg == cnt["segments"]
    assert np.isfinite(img).all()
    assert linf <= TOL
    b, seg_b, _ = _lanes(sim, earth, name, sp, CULL_REFERENCE, w, h, spp)
    assert seg_b == seg
    assert np.array_equal(img.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", C.SPHERE_SCENES + C.GENERAL_SCENES)
def test_shutter_inside_the_boxes_interval_exact_lanes_match_oracle(sim, earth, oracles, name):
    w, h, spp = C.ORACLE_SIZE[name]
    sp = C.spec(name, None, _info(name, earth), C.SHUTTER_INSIDE)
    img, seg, s = _lanes(sim, earth, name, sp, CULL_EXACT, w, h, spp)
    _, info = hrt.scene_blob(s)
    assert info.box_t0 <= C.SHUTTER_INSIDE[0] and C.SHUTTER_INSIDE[1] <= info.box_t1  # plan() keeps EXACT here
    ref, cnt = oracles(name).render(w, h, spp, 50, seed=SEED, camera=sp)
    assert seg == cnt["segments"]
    assert np.isfinite(img).all()
    assert np.abs(img - ref).max() <= TOL


@pytest.mark.parametrize("shutter", C.SHUTTERS_OUTSIDE)
@pytest.mark.parametrize("name", C.SHUTTER_SCENES)
def test_shutter_outside_the_boxes_interval_reference_lanes_match_oracle(sim, earth, oracles, name, shutter):
    w, h, spp = C.ORACLE_SIZE[name]
    sp = C.spec(name, None, _info(name, earth), shutter)
    img, seg, s = _lanes(sim, earth, name, sp, CULL_REFERENCE, w, h, spp)
    _, info = hrt.scene_blob(s)
    assert shutter[0] < info.box_t0 or shutter[1] > info.box_t1  # plan() leaves EXACT for this shutter
    ref, cnt = oracles(name).render(w, h, spp, 50, seed=SEED, camera=sp)
    assert seg == cnt["segments"]
    assert np.isfinite(img).all()
    assert np.abs(img - ref).max() <= TOL


def test_exact_culling_is_wrong_outside_the_boxes_interval(sim, earth, oracles):
    """What plan()'s shutter guard is for: `random` with the shutter (-0.5, 1.5) under forced EXACT culling traces
    other paths than the oracle, so the GPU parity case of this shutter fails if the guard goes."""
    w, h, spp = C.ORACLE_SIZE["random"]
    sp = C.spec("random", None, _info("random", earth), (-0.5, 1.5))
    img, seg, _ = _lanes(sim, earth, "random", sp, CULL_EXACT, w, h, spp)
    ref, cnt = oracles("random").render(w, h, spp, 50, seed=SEED, camera=sp)
    print(f"EXACT lanes {seg} segments, oracle {cnt['segments']}, L-inf {float(np.abs(img - ref).max()):.3g}")
    assert seg != cnt["segments"]


LIST_FRAMES = [(1920, 1080, 60), (40, 24, None), (37, 23, None)]


@pytest.mark.parametrize("W,H,n", LIST_FRAMES)
@pytest.mark.parametrize("cam", list(C.SPHERE_CAMERAS))
@pytest.mark.parametrize("name", C.PARITY_SPHERE_SCENES)
def test_list_holds_every_leaf_the_walk_tests_at_camera(lib, earth, name, cam, W, H, n):
    cells = _cells(W, H, n)
    tot, counts = _check(lib, earth, name, W, H, cells, camera=C.spec(name, cam))
    overflow = float((counts > CAP).mean())
    print(f"{name} {cam} {W}x{H}: {len(cells)} cells, {tot['rays']} rays, list length median {np.median(counts):.0f} "
          f"max {counts.max()}, overflow share {overflow:.4f}, list steps {tot['list_steps']}")
    assert tot["rays"] >= len(cells) * 36
    assert tot["missing"] == 0
    assert tot["mismatch"] == 0
    assert tot["hull_out"] == 0
    if W == 1920 and cam in C.LIST_FRIENDLY and name in C.SPHERE_SCENES:
        assert tot["list_steps"] > 0  # lists were walked
        assert overflow <= 0.25, overflow


@pytest.mark.parametrize("cam", C.LIST_FRIENDLY)
@pytest.mark.parametrize("name", C.SPHERE_SCENES)
def test_gpu_list_tiles_hold_listed_cells(lib, earth, name, cam):
    """The tiles test_gpu_cameras.py renders with and without lists (cameras.LIST_TILES): the host builder's leaf
    counts of their cells include lists usable at capacity 8 and 3, and lists that overflow capacity 3 alone."""
    W, H = 1920, 1080
    cells = sorted({(cx, cy) for x, y, w, h in C.LIST_TILES[cam]
                    for cx in range(x // 8, (x + w - 1) // 8 + 1) for cy in range(y // 8, (y + h - 1) // 8 + 1)})
    s = hrt.preset(name, 1, earth)
    c = C.hrt_camera(C.spec(name, cam), W, H)
    blob, info = hrt.scene_blob(s)
    p = hrt.params(W, H, 8, 50, 3, tuple(s.info.background))
    arr = np.array(cells, np.uint32)
    rec = np.zeros((len(arr), 8), np.uint16)
    cnt = np.zeros(len(arr), np.uint32)
    assert lib.pl_build(blob, ctypes.byref(info), ctypes.byref(c), ctypes.byref(p), CAP, arr.ctypes.data_as(ctypes.c_void_p),
                        len(arr), rec.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)) == 0
    print(name, cam, sorted(cnt.tolist()))
    assert ((cnt >= 1) & (cnt <= 3)).any() and ((cnt >= 4) & (cnt <= CAP)).any()


@pytest.mark.parametrize("cam", ["opp_octant_bigap", "near_ground"])
def test_check_fails_without_the_hulls_pads_at_camera(lib_no_pad, earth, cam):
    tot, _ = _check(lib_no_pad, earth, "random", 1920, 1080, _cells(1920, 1080, 60), camera=C.spec("random", cam))
    assert tot["hull_out"] > 0
