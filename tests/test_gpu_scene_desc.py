"""The constructor-built scenes of tests/scenes_oracle.py on the GPU, at the sizes tests/test_scene_desc.py runs on
the host lanes: each description is built by the library through the C ABI and by the oracle (oracle.cpp
build_desc), and the frame the default plan renders is held to the oracle's.

- Default plan against the oracle: equal segment counts, finite pixels, L-inf <= 1e-3; the launch record names the
  kernel plan() chose (the sphere kernel, the general walk kernel, or the segment kernel for a nested medium).
- Bit equality of the default frame with HRT_RENDER_REFERENCE_CULL, HRT_KERNEL=segment / persistent,
  HRT_RENDER_NO_LDS, and HRT_SPHERE_PACKET=0 / 1 on the two small sphere scenes.
- bvh_intervals: EXACT culling for shutters inside [0.25, 0.75], REFERENCE for (0, 1), each equal to the oracle.
- Chunked accumulation on the new branches, and one Accumulator pass on media_nested.
"""
import numpy as np
import pytest

import hrt
import scenes_oracle as S
from test_gpu_cameras import CULL_EXACT, CULL_REFERENCE, _launch_cull

TOL = 1e-3  # the project's bar (tests/test_gpu_parity.py)


def _family(kernel):
    """The kernel family of a launch record's name (render.hip launch_any)."""
    for prefix, fam in (("launch_basic[", "sphere"), ("launch_g[", "general walk"), ("launch_full[", "persistent"),
                        ("launch[", "segment")):
        if kernel.startswith(prefix):
            return fam
    raise AssertionError(kernel)


def _expected_family(info):
    """render.hip plan() under the default flags and exact culling."""
    if info.media_nested:
        return "segment"
    return "general walk" if info.walk_general else "sphere"


@pytest.fixture(scope="module")
def built():
    """name -> (Desc, committed hrt.Scene, OracleScene)"""
    out = {}

    def get(name):
        if name not in out:
            d = S.TABLE[name][0]()
            s = d.to_hrt()
            s.commit()
            out[name] = (d, s, d.to_oracle())
        return out[name]

    yield get
    for _, s, _ in out.values():
        s.close()


def _render(d, s, size, shutter=None, flags=0, seed=S.SEED):
    w, h, spp = size
    img, st = hrt.render(s, d.hrt_camera(w, h, shutter), d.params(w, h, spp, seed, flags=flags), stats=True)
    assert st.pixels == w * h and st.samples == w * h * spp
    return img, st


def _parity(d, s, o, size, label, shutter=None):
    w, h, spp = size
    img, st = _render(d, s, size, shutter)
    kernel = hrt.last_launch()["kernel"]
    cull = _launch_cull()
    ref, cnt = o.render(w, h, spp, 50, seed=S.SEED, camera=d.spec(shutter))
    linf = float(np.abs(img - ref).max())
    print(f"{label}: segments {st.segments} (oracle {cnt['segments']}), L-inf {linf:.3g}, {_family(kernel)} kernel, cull {cull}")
    assert st.segments == cnt["segments"], (st.segments, cnt["segments"])
    assert np.isfinite(img).all()
    assert linf <= TOL, linf
    return img, st, kernel, cull


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.TABLE))
def test_default_plan_matches_oracle(built, name):
    d, s, o = built(name)
    _, _, kernel, cull = _parity(d, s, o, S.TABLE[name][1], name)
    assert cull == CULL_EXACT
    _, info = hrt.scene_blob(s)
    assert _family(kernel) == _expected_family(info), kernel
    if name == "lit_spheres":  # sphere geometry with a light: never the sphere kernel (shade_walk gathers at a miss only)
        si = s.scene_info()
        assert si.feature_mask & (1 << 7) and si.feature_mask & (1 << 8)  # layout.h F_LIGHT, F_ISOTROPIC
        assert _family(kernel) == "general walk"
    if name in ("tex_sizes", "big_textured"):
        assert "HEAVY = true" in kernel, kernel
    if name in ("materials_spheres", "nested_checker"):
        assert "HEAVY = false" in kernel, kernel


def _same(a, sa, b, sb, what):
    assert (sa.segments, sa.samples, sa.pixels) == (sb.segments, sb.samples, sb.pixels), what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.TABLE))
def test_default_plan_bit_equal_to_its_variants(built, monkeypatch, name):
    """The verbatim reference box test, the scene in global memory, and the segment / persistent kernels (plan()
    keeps a nested medium on the segment kernel and a BASIC sphere scene on the sphere kernel whatever HRT_KERNEL
    says) render the default frame bit for bit."""
    d, s, _ = built(name)
    size = S.TABLE[name][1]
    a, sa = _render(d, s, size)
    assert np.isfinite(a).all()
    b, sb = _render(d, s, size, flags=hrt.RENDER_REFERENCE_CULL)
    assert _launch_cull() == CULL_REFERENCE
    _same(a, sa, b, sb, "reference cull")
    b, sb = _render(d, s, size, flags=hrt.RENDER_NO_LDS)
    _same(a, sa, b, sb, "no LDS")
    _, info = hrt.scene_blob(s)
    for k in ("segment", "persistent"):
        monkeypatch.setenv("HRT_KERNEL", k)
        b, sb = _render(d, s, size)
        fam = _family(hrt.last_launch()["kernel"])
        monkeypatch.delenv("HRT_KERNEL")
        _same(a, sa, b, sb, k)
        if info.media_nested:
            assert fam == "segment", (k, fam)
        elif info.walk_general:
            assert fam == k, (k, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["materials_spheres", "nested_checker"])
def test_sphere_packet_knob_bit_equal(built, monkeypatch, name):
    """HRT_SPHERE_PACKET (read at commit and at launch) 0 and 1: the per-lane walk and the packet walk."""
    d, s, _ = built(name)
    size = S.TABLE[name][1]
    a, sa = _render(d, s, size)
    for v in ("0", "1"):
        monkeypatch.setenv("HRT_SPHERE_PACKET", v)
        s2 = d.to_hrt()
        s2.commit()
        b, sb = _render(d, s2, size)
        kernel = hrt.last_launch()["kernel"]
        s2.close()
        monkeypatch.delenv("HRT_SPHERE_PACKET")
        assert ("PACKET = true" in kernel) == (v == "1"), kernel
        _same(a, sa, b, sb, v)


@pytest.mark.gpu
@pytest.mark.parametrize("shutter", S.BVH_SHUTTERS)
def test_bvh_intervals_shutters(built, shutter):
    """scene.cpp build_bvh intersects the nested BvhNodes' intervals into [0.25, 0.75]; plan()'s shutter guard reads
    it: exact culling inside, the reference box test for (0, 1), and the oracle's frame either way."""
    d, s, o = built("bvh_intervals")
    _, info = hrt.scene_blob(s)
    assert (info.box_t0, info.box_t1) == (0.25, 0.75)
    _, _, _, cull = _parity(d, s, o, S.SPHERE_SIZE, f"bvh_intervals shutter {shutter}", shutter=shutter)
    assert cull == (CULL_REFERENCE if shutter == (0.0, 1.0) else CULL_EXACT)


# one chunked case per kernel class (lane.h sample_chunk: more than 32 samples on a sphere scene, 64 on a general one)
CHUNKED = [("materials_spheres", (24, 16, 40)), ("instances", (16, 16, 70)), ("media_nested", (16, 16, 70))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", CHUNKED)
def test_chunked_accumulation_matches_oracle(built, name, size):
    d, s, o = built(name)
    w, h, spp = size
    ch = hrt.sample_chunks(s, d.params(w, h, spp, S.SEED))
    print(name, ch)
    assert ch["head"] + ch["tail"] > 1  # several chunk sums per pixel
    _parity(d, s, o, size, f"{name} {spp} spp")


@pytest.mark.gpu
def test_accumulator_pass_on_nested_media(built):
    """include/hrt/hrt.h: one hrt_accum pass resolves to hrt_render's frame bit for bit, here on the segment kernel
    a nested medium runs."""
    d, s, _ = built("media_nested")
    w, h, spp = S.GENERAL_SIZE
    cam, p = d.hrt_camera(w, h), d.params(w, h, spp, S.SEED)
    ref, st_ref = hrt.render(s, cam, p, stats=True)
    a = hrt.Accumulator(s, w, h)
    st = a.add(cam, p, stats=True)
    img = a.resolve()
    assert a.samples == spp and st.segments == st_ref.segments
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    a.close()
