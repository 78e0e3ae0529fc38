"""The cameras and shutters of tests/cameras.py on the GPU (tests/test_cameras.py holds the host lanes and the host
list check to the same table).

- Parity: the default path against the oracle rendering from the same camera, at the oracle sizes of cameras.py:
  equal segment counts, finite pixels, L-inf <= 1e-3.  The shutters that reach outside [0, 1] (random, motion,
  final) are the test of render.hip plan()'s guard: under exact culling the paths differ from the oracle's
  (test_cameras.py::test_exact_culling_is_wrong_outside_the_boxes_interval), so the guard must pick the reference
  box test, which the launch record's kernel name shows.
- Exact culling against HRT_RENDER_REFERENCE_CULL, bit for bit, at 160x90x8 (200x200x4 for `final`): frames with
  far more grazing rays than the oracle-sized ones.
- Lists on / off at the list-friendly cameras: tiles of the 1920x1080 frame (cameras.LIST_TILES) at capacity 8 and
  3, identical bits and stats, fewer node visits with the lists.
- One committed scene across launches that change the camera and the frame (the list buffer grows with the cell
  count and is rebuilt per launch), set_view with another camera than the render's, and t_min other than 0.001.
"""
import re

import numpy as np
import pytest

import cameras as C
import hrt
from oracle import oracle as O
from test_gpu_primary_lists import _both, _render, _same

TOL = 1e-3
SEED = 3
CULL_REFERENCE, CULL_EXACT = 0, 2  # csrc/layout.h


@pytest.fixture(scope="module")
def scenes(earth):
    out = {}

    def get(name):
        if name not in out:
            s = hrt.preset(name, 1, earth)
            s.commit()
            out[name] = s
        return out[name]

    return get


@pytest.fixture(scope="module")
def oracles(earth):
    out = {}

    def get(name):
        if name not in out:
            out[name] = O.OracleScene(hrt.PRESETS[name], 1, earth)
        return out[name]

    return get


def _launch_cull():
    """The culling mode of the calling thread's last launch, from the launcher's template arguments in its name."""
    k = hrt.last_launch()["kernel"]
    if k.startswith("launch_g["):  # render_gwalk_kernel: plan() sends general scenes there under exact culling alone
        return CULL_EXACT
    m = re.search(r"CULL = (\d+)", k)
    assert m, k
    return int(m.group(1))


def _parity(s, o, name, sp, label, t_min=0.001, size=None, seed=SEED):
    w, h, spp = size or C.ORACLE_SIZE[name]
    p = hrt.params(w, h, spp, 50, seed, tuple(s.info.background), t_min=t_min)
    img, st = hrt.render(s, C.hrt_camera(sp, w, h), p, stats=True)
    cull = _launch_cull()
    ref, cnt = o.render(w, h, spp, 50, seed=seed, t_min=t_min, camera=sp)
    linf = float(np.abs(img - ref).max())
    print(f"{name} {label}: segments {st.segments} (oracle {cnt['segments']}), L-inf {linf:.3g}, cull {cull}")
    assert st.pixels == w * h and st.samples == w * h * spp
    assert st.segments == cnt["segments"], (st.segments, cnt["segments"])
    assert np.isfinite(img).all()
    assert linf <= TOL, linf
    return cull


@pytest.mark.gpu
@pytest.mark.parametrize("name,cam", C.scene_cameras())
def test_camera_parity(scenes, oracles, name, cam):
    assert _parity(scenes(name), oracles(name), name, C.spec(name, cam), cam) == CULL_EXACT


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.SPHERE_SCENES + C.GENERAL_SCENES)
def test_shutter_inside_parity(scenes, oracles, name):
    s = scenes(name)
    sp = C.spec(name, None, s.info, C.SHUTTER_INSIDE)
    assert _parity(s, oracles(name), name, sp, f"shutter {C.SHUTTER_INSIDE}") == CULL_EXACT


@pytest.mark.gpu
@pytest.mark.parametrize("shutter", C.SHUTTERS_OUTSIDE)
@pytest.mark.parametrize("name", C.SHUTTER_SCENES)
def test_shutter_outside_parity(scenes, oracles, name, shutter):
    """plan()'s guard: ray times outside the interval the BVH boxes hold for take the reference box test."""
    s = scenes(name)
    sp = C.spec(name, None, s.info, shutter)
    assert _parity(s, oracles(name), name, sp, f"shutter {shutter}") == CULL_REFERENCE


@pytest.mark.gpu
@pytest.mark.parametrize("name,cam", C.scene_cameras())
def test_exact_equals_reference_cull_at_camera(scenes, name, cam):
    w, h, spp = (200, 200, 4) if name == "final" else (160, 90, 8)
    s = scenes(name)
    c = C.hrt_camera(C.spec(name, cam), w, h)
    out = []
    for flags, cull in ((0, CULL_EXACT), (hrt.RENDER_REFERENCE_CULL, CULL_REFERENCE)):
        img, st = hrt.render(s, c, hrt.params(w, h, spp, 50, 5, tuple(s.info.background), flags=flags), stats=True)
        assert _launch_cull() == cull
        out.append((img.view(np.uint32), st))
    (a, sa), (b, sb) = out
    assert (sa.segments, sa.samples, sa.pixels) == (sb.segments, sb.samples, sb.pixels)
    assert np.isfinite(out[0][0].view(np.float32)).all()
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("lists", [None, 3])
@pytest.mark.parametrize("cam", C.LIST_FRIENDLY)
@pytest.mark.parametrize("name", C.SPHERE_SCENES)
def test_lists_on_off_at_camera(monkeypatch, scenes, name, cam, lists):
    off, st_off, on, st_on = _both(monkeypatch, scenes(name), 1920, 1080, 8, tiles=C.LIST_TILES[cam], lists=lists,
                                   flags=hrt.RENDER_COUNT_WORK, camera=C.spec(name, cam))
    _same(off, st_off, on, st_on)
    assert 0 < st_on.node_visits < st_off.node_visits, (st_on.node_visits, st_off.node_visits)


@pytest.mark.gpu
def test_one_scene_across_cameras_and_frame_sizes(earth):
    """A at 64x36 (40 cells), B on tiles of 1920x1080 (32400 cells: the list buffer grows), A again, and on through
    more launches than the scene has scratch slots: every A frame and every B frame equals a fresh scene's."""
    def fresh():
        s = hrt.preset("random", 1, earth)
        s.commit()
        return s

    a_args = dict(W=64, H=36, spp=8, camera=None)
    b_args = dict(W=1920, H=1080, spp=8, tiles=C.LIST_TILES["inside_glass"], camera=C.spec("random", "inside_glass"))
    c_args = dict(W=37, H=23, spp=8, camera=C.spec("random", "opp_octant_bigap"))
    want = {k: _render(fresh(), **a) for k, a in (("a", a_args), ("b", b_args), ("c", c_args))}
    s = fresh()
    for k in "abacabca":
        img, st = _render(s, **{"a": a_args, "b": b_args, "c": c_args}[k])
        assert np.array_equal(img, want[k][0]), k
        assert (st.segments, st.samples, st.pixels) == (want[k][1].segments, want[k][1].samples, want[k][1].pixels), k


@pytest.mark.gpu
@pytest.mark.parametrize("cam", ["opp_octant_bigap", "inside_glass"])
def test_set_view_of_another_camera(earth, cam):
    """random_10k stages the node parts its view hint reaches first; a render from another camera is the frame of a
    scene committed with no view, bit for bit."""
    w, h, spp = 48, 27, 4
    plain = hrt.preset("random_10k", 1, earth)
    hinted = hrt.preset("random_10k", 1, earth)
    hinted.set_view(hrt.preset_camera(hinted.info, w, h))
    plain.commit()
    hinted.commit()
    sp = C.SPHERE_CAMERAS[cam] + (0.0, 1.0)
    a, sa = _render(plain, w, h, spp, camera=sp)
    b, sb = _render(hinted, w, h, spp, camera=sp)
    assert sa.segments == sb.segments > 0
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("t_min", [0.01, 0.0])
@pytest.mark.parametrize("name", ["random", "cornell_smoke"])
def test_t_min_parity(scenes, oracles, name, t_min):
    s = scenes(name)
    _parity(s, oracles(name), name, C.spec(name, None, s.info), f"t_min {t_min}", t_min=t_min, size=(32, 18, 4), seed=11)
