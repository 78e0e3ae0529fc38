"""The sphere kernel's pass order (render_sphere.hip: retire, claim / start / lists, ONE shading block, ray setup,
walk) on the GPU, at the smallest frames on which that order can go wrong.

A path that is over (a miss, the untraced segment of a max_depth 0 path, a hit whose shading ended the path) retires
at the start of a pass, ahead of the claim; the shading block then serves the walked and the listed hits together.
Per-lane work is what it was, so every frame is held to the CPU oracle (equal segment counts, L-inf <= 1e-3, exact
sample and pixel counts) and to the kernel's other instantiations bit for bit.

- mixed frame: sky rows, ground, listed cells and overflow cells, head + tail chunks;
- 1 spp: every retire is a chunk's end, written straight out, blocks partial on both axes;
- max_depth 0 / 1 / 2: untraced segments, and paths that end inside shading by the cap;
- a camera that sees only sky: consecutive retires across chunk ends with no walk at all;
- Metal scatters below the surface (fuzz 0.999 and 1.5): terminations only shading can find.
"""
import os

import numpy as np
import pytest

import hrt
import scenes_oracle as S
from oracle import oracle as O

TOL = 1e-3  # the project's bar (tests/test_gpu_parity.py)
SEED = 5
# from (13, 2, 3) up towards (0, 40, 0): the lens (radius 0.05) stays above y = 1.95 and every ray rises, and no
# sphere near x = 13 reaches that height, so each sample is one ray that misses
SKY_CAMERA = ((13, 2, 3), (0, 40, 0), 20.0, 0.1, 10.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def scene(earth):
    s = hrt.preset("random", 1, earth)
    s.commit()
    return s


@pytest.fixture(scope="module")
def oracle(earth):
    return O.OracleScene(hrt.PRESETS["random"], 1, earth)


def _frame(s, W, H, spp, depth, flags=0, camera=None):
    cam = hrt.preset_camera(s.info, W, H) if camera is None else hrt.camera(*camera, W, H)
    p = hrt.params(W, H, spp, depth, SEED, tuple(s.info.background), flags=flags)
    img, st = hrt.render(s, cam, p, stats=True)
    assert "launch_basic" in hrt.last_launch()["kernel"]  # the sphere kernel's launcher
    return img, st


def _holds_to_oracle(img, st, ref, cnt, W, H, spp, label):
    linf = float(np.abs(img - ref).max())
    print(f"{label}: segments {st.segments} (oracle {cnt['segments']}), samples {st.samples}, L-inf {linf:.3g}")
    assert st.samples == W * H * spp and st.pixels == W * H, (st.samples, st.pixels)
    assert st.segments == cnt["segments"], (st.segments, cnt["segments"])
    assert (img[..., 3] == 1.0).all()
    assert linf <= TOL, linf


@pytest.fixture(scope="module")
def mixed(scene):
    """The mixed frame under the default plan (no HRT_PRIMARY_LISTS in the environment: the launch builds and reads
    the leaf lists), shared and left unchanged."""
    saved = os.environ.pop("HRT_PRIMARY_LISTS", None)
    try:
        return _frame(scene, 64, 36, 40, 8)
    finally:
        if saved is not None:
            os.environ["HRT_PRIMARY_LISTS"] = saved


@pytest.mark.gpu
def test_mixed_frame_matches_oracle(mixed, oracle):
    """64x36, 40 spp (chunks 16 / 16 / 8), depth 8: sky rows, ground, cells with 1..16 leaves and overflow cells."""
    W, H, spp = 64, 36, 40
    img, st = mixed
    ref, cnt = oracle.render(W, H, spp, 8, seed=SEED)
    _holds_to_oracle(img, st, ref, cnt, W, H, spp, "mixed")


@pytest.mark.gpu
def test_mixed_frame_reads_lists(monkeypatch, scene, mixed):
    """The default launch of the mixed frame takes the lists path: the COUNT build of the same instantiation renders
    the same bits with fewer node visits and walk steps than with HRT_PRIMARY_LISTS=0 (the list rounds replace the
    camera rays' inner nodes in the 24 cells that do not overflow)."""
    img, st = mixed
    monkeypatch.delenv("HRT_PRIMARY_LISTS", raising=False)
    on, st_on = _frame(scene, 64, 36, 40, 8, flags=hrt.RENDER_COUNT_WORK)
    name_on = hrt.last_launch()["kernel"]
    monkeypatch.setenv("HRT_PRIMARY_LISTS", "0")
    off, st_off = _frame(scene, 64, 36, 40, 8, flags=hrt.RENDER_COUNT_WORK)
    assert hrt.last_launch()["kernel"] == name_on and "COUNT = true" in name_on, name_on
    for b, sb in ((on, st_on), (off, st_off)):
        assert (st.segments, st.samples, st.pixels) == (sb.segments, sb.samples, sb.pixels)
        assert np.array_equal(img.view(np.uint32), b.view(np.uint32))
    print(f"node visits {st_on.node_visits} with lists, {st_off.node_visits} without; walk steps {st_on.walk_steps} / {st_off.walk_steps}")
    assert 0 < st_on.node_visits < st_off.node_visits, (st_on.node_visits, st_off.node_visits)
    assert 0 < st_on.walk_steps < st_off.walk_steps, (st_on.walk_steps, st_off.walk_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["no lists", "reference cull", "no LDS"])
def test_mixed_frame_bit_equal_to_its_variants(monkeypatch, scene, mixed, variant):
    """Every ray walking the stream (HRT_PRIMARY_LISTS=0), a non-walk-stream instantiation, and the stream read from
    global memory: the same bits and the same counts."""
    img, st = mixed
    flags = 0
    monkeypatch.delenv("HRT_PRIMARY_LISTS", raising=False)
    if variant == "no lists":
        monkeypatch.setenv("HRT_PRIMARY_LISTS", "0")
    elif variant == "reference cull":
        flags = hrt.RENDER_REFERENCE_CULL
    else:
        flags = hrt.RENDER_NO_LDS
    b, sb = _frame(scene, 64, 36, 40, 8, flags=flags)
    kernel = hrt.last_launch()["kernel"]
    if variant == "reference cull":
        assert "CULL = 0" in kernel, kernel
    assert (st.segments, st.samples, st.pixels) == (sb.segments, sb.samples, sb.pixels), variant
    assert np.array_equal(img.view(np.uint32), b.view(np.uint32)), variant


@pytest.mark.gpu
def test_one_sample_per_item(scene, oracle):
    """37x19 at 1 spp: every retire ends its chunk and writes the pixel straight out; partial blocks on both axes."""
    W, H, spp = 37, 19, 1
    img, st = _frame(scene, W, H, spp, 8)
    ref, cnt = oracle.render(W, H, spp, 8, seed=SEED)
    _holds_to_oracle(img, st, ref, cnt, W, H, spp, "1 spp")


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_depth_caps(scene, oracle, depth):
    """max_depth 0: untraced segments retire, zero rays.  1 and 2: every path that hits ends inside shading by the
    cap, and retires at the start of the next pass."""
    W, H, spp = 40, 24, 8
    img, st = _frame(scene, W, H, spp, depth)
    ref, cnt = oracle.render(W, H, spp, depth, seed=SEED)
    _holds_to_oracle(img, st, ref, cnt, W, H, spp, f"depth {depth}")
    if depth == 0:
        assert st.segments == 0 and (img[..., :3] == 0.0).all()  # black, no world.hit
    if depth == 1:
        assert st.segments == W * H * spp  # the camera ray alone


@pytest.mark.gpu
def test_all_miss_view(scene, oracle):
    """40x24, 33 spp (chunks 16 / 16 / 1), a camera that sees only sky: one ray per sample, retire after retire
    across chunk ends with no walk."""
    W, H, spp = 40, 24, 33
    ref, cnt = oracle.render(W, H, spp, 8, seed=SEED, camera=SKY_CAMERA)
    assert cnt["segments"] == W * H * spp, cnt  # the premise: every sample of this camera is one ray
    img, st = _frame(scene, W, H, spp, 8, camera=SKY_CAMERA)
    _holds_to_oracle(img, st, ref, cnt, W, H, spp, "all miss")
    assert st.segments == st.samples == W * H * spp


@pytest.mark.gpu
def test_terminations_only_shading_finds():
    """materials_spheres (Metal fuzz 0.999 and 1.5: scatters below the surface end paths at a hit), built through
    the constructors and replayed by the oracle, at 48x27x8."""
    d = S.TABLE["materials_spheres"][0]()
    s = d.to_hrt()
    s.commit()
    try:
        w, h, spp = 48, 27, 8
        img, st = hrt.render(s, d.hrt_camera(w, h, None), d.params(w, h, spp, S.SEED), stats=True)
        assert "launch_basic" in hrt.last_launch()["kernel"]
        ref, cnt = d.to_oracle().render(w, h, spp, 50, seed=S.SEED, camera=d.spec(None))
        assert np.isfinite(img).all()
        _holds_to_oracle(img, st, ref, cnt, w, h, spp, "materials_spheres")
    finally:
        s.close()
