"""Scenes built through the constructors, held to the oracle on the host (tests/scenes_oracle.py; the GPU runs the
same table in tests/test_gpu_scene_desc.py).

Before this file every oracle comparison rendered a preset: the constructor-built scenes of tests/scenes.py were
compared with the library's own reference traversal, which shares lane.h's shading, material, texture, primitive,
instance and medium code with the path under test.  Here one description (tests/scene_desc.py Desc) is built twice,
by the library through the C ABI and by the oracle from its reference-shaped types (oracle.cpp build_desc), and the
kernels' per-lane code (tests/native/lane_sim.hip over csrc/lane.h) must trace the oracle's paths.

- The description path is the preset path: four presets written by hand as descriptions render the same bytes as
  OracleScene(preset) / hrt.preset, which the known-answer fixtures of tests/golden pin.
- Lanes against the oracle, for every table scene and every lane kernel that accepts it under exact culling: the
  oracle's segment count, finite pixels, L-inf <= 1e-3 (test_lane_sim.TOL), and the bits of the reference-culling
  lanes.
- Each scene reaches the branch it exists for (blob info, leaf payloads, oracle counters), and each off-preset
  parameter changes the oracle's frame and segment count at the test's size.
"""
import ctypes

import numpy as np
import pytest

import hrt
import scenes_oracle as S
from oracle import oracle as O
from scene_desc import MAGIC, OPS
from test_lane_sim import CULL_EXACT, CULL_REFERENCE, TOL, _build_sim

F = {n: 1 << k for k, n in enumerate(("MOVING", "RECT", "INSTANCE", "MEDIUM", "NOISE", "IMAGE", "CHECKER", "LIGHT", "ISOTROPIC",
                                      "METAL", "DIELECTRIC"))}  # csrc/layout.h F_*
F_BASIC = F["MOVING"] | F["CHECKER"] | F["METAL"] | F["DIELECTRIC"]
F_HEAVY_TEX = F["NOISE"] | F["IMAGE"]
WT_SOLID, WT_CHECKER, WT_GLOBAL = 0, 1, 2
WALK_PEND = 1 << 31


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build_sim(tmp_path_factory)


@pytest.fixture(scope="module")
def built():
    """name -> (Desc, hrt.Scene, blob, blob info, OracleScene), built once (renders change none of them)."""
    out = {}

    def get(name):
        if name not in out:
            d = S.TABLE[name][0]()
            s = d.to_hrt()
            blob, info = hrt.scene_blob(s)
            out[name] = (d, s, blob, info, d.to_oracle())
        return out[name]

    return get


def lanes(L, d, blob, info, w, h, spp, kernel, cull, seed=S.SEED, shutter=None):
    cam = d.hrt_camera(w, h, shutter)
    p = d.params(w, h, spp, seed)
    out = np.zeros((h, w, 4), np.float32)
    cnt = np.zeros(8, np.uint64)
    rc = L.lane_sim_render(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), kernel, cull, 0, 0, w, h,
                           out.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
    return rc, out, int(cnt[0])


def lane_kernels(info):
    """(accepted, refused) lane kernels of a scene under exact culling: the sphere lane (0) needs a sphere stream,
    the general walk lane (3) a general one; the full (1) and segment (2) lanes walk the reference stream."""
    sphere = info.walk_bytes > 0 and not info.walk_general and (info.feature_mask & ~(F_BASIC | F_HEAVY_TEX)) == 0
    general = info.walk_bytes > 0 and bool(info.walk_general)
    ok = ([0] if sphere else []) + [1, 2] + ([3] if general else [])
    return ok, [k for k in (0, 3) if k not in ok]


def sphere_leaf_words(blob, info):
    """The material word mw of every leaf payload of a sphere walk stream (layout.h): M_* | WT_* << 4 | mat << 8."""
    assert info.walk_bytes > 0 and not info.walk_general and not info.walk_c16 and info.walk_half == 16
    u = np.frombuffer(bytes(blob)[info.off_walk:info.off_walk + info.walk_bytes], np.uint32)
    out, stack = [], [0]
    while stack:
        off = stack.pop()
        pas = int(u[off // 4 + 7])
        if pas & WALK_PEND:
            out.append(int(u[(pas - WALK_PEND) // 4 + 23]))
        else:
            stack += [int(u[pas // 4 + 3]), pas]
    return out


# ---------------------------------------------------------------- the entry point itself
def _words(*records, root=0):
    hdr = [MAGIC, root] + [0] * 14
    return np.array(hdr + [w for r in records for w in r], np.uint32)


def _fbits(*v):
    return np.array(v, np.float32).view(np.uint32).tolist()


def test_description_errors_are_reported():
    """A bad id, a node used twice, a missing box where bvh_node.rs panics, and a malformed description raise with
    oracle_last_error's text instead of building something."""
    solid = [OPS["solid"], *_fbits(0.5, 0.5, 0.5)]
    lam = [OPS["lambertian"], 0]
    sph = [OPS["sphere"], *_fbits(0, 0, 0, 1), 0]
    ok = O.OracleScene.from_description(_words(solid, lam, sph))
    assert ok.count() == 1
    cases = {
        "bad texture id": _words(solid, [OPS["lambertian"], 1], sph),
        "bad material id": _words(solid, lam, [OPS["sphere"], *_fbits(0, 0, 0, 1), 3]),
        "bad node id": _words(solid, lam, sph, root=1),
        "node already owned": _words(solid, lam, sph, [OPS["list"], 1, 0], [OPS["list"], 1, 0], root=1),
        "no bounding box": _words(solid, lam, sph, [OPS["list"], 0], [OPS["bvh"], *_fbits(0, 1), 2, 0, 1], root=2),
        "no elements in scene": _words(solid, lam, [OPS["bvh"], *_fbits(0, 1), 0]),
        "truncated": _words(solid, lam, sph[:-2]),
        "unknown record": _words(solid, lam, sph, [99]),
        "header": np.array([0] * 16, np.uint32),
    }
    # consumed by a parent, then named as the root
    cases["node already owned by"] = _words(solid, lam, sph, [OPS["translate"], 0, *_fbits(1, 0, 0)], root=0)
    for text, words in cases.items():
        with pytest.raises(RuntimeError, match=text):
            O.OracleScene.from_description(words)
    with pytest.raises(RuntimeError, match="image outside the blob"):
        O.OracleScene.from_description(_words([OPS["image"], 2, 2, 3, 0]), np.zeros(11, np.uint8))


def test_desc_returns_the_librarys_ids():
    """Desc counts node ids as the library does (a Cuboid pushes its six sides first, a BvhNode of n objects
    2n - 1 nodes): to_hrt asserts every id, here on scenes with cuboids and nested BvhNodes."""
    for name in ("instances", "media_nested", "sphere_lists"):
        S.TABLE[name][0]().to_hrt()


# ---------------------------------------------------------------- the new builder is the old one
def _hand_presets():
    rv = np.zeros(768, np.float32)
    pm = np.zeros(768, np.uint32)
    O.load().oracle_perlin_tables(1, rv.ctypes.data, pm.ctypes.data)
    return {"two_spheres": S.preset_two_spheres(), "cornell": S.preset_cornell(), "cornell_smoke": S.preset_cornell_smoke(),
            "simple_light": S.preset_simple_light(rv, pm)}


@pytest.mark.parametrize("name", ["two_spheres", "cornell", "cornell_smoke", "simple_light"])
def test_described_preset_is_the_preset(sim, earth, name):
    d = _hand_presets()[name]
    w, h, spp = 24, 24, 4
    a, ca = d.to_oracle().render(w, h, spp, seed=S.SEED)
    op = O.OracleScene(hrt.PRESETS[name], 1, earth)
    b, cb = op.render(w, h, spp, seed=S.SEED)
    assert ca == cb and a.tobytes() == b.tobytes()
    assert ca["segments"] > w * h * spp
    mine = d.to_oracle()
    own = (op.look_from, op.look_at, op.fov, op.aperture, op.focus_dist, op.time0, op.time1)
    assert np.array_equal(np.hstack([np.ravel(v) for v in own]).astype(np.float32),
                          np.hstack([np.ravel(v) for v in d.camera]).astype(np.float32))
    assert np.array_equal(mine.background, op.background) and mine.n_media == op.n_media
    c, cc = mine.render(w, h, spp, seed=S.SEED, camera=d.spec())  # with camera= as well
    assert cc == ca and c.tobytes() == a.tobytes()
    # the library: the description through the constructors against hrt_preset_build, on the host lanes
    sp = hrt.preset(name, 1, earth)
    blob_p, info_p = hrt.scene_blob(sp)
    blob_d, info_d = hrt.scene_blob(d.to_hrt())
    assert np.array_equal(np.array(sp.info.background, np.float32), np.array(d.background, np.float32))
    for kernel in (1, 3) if name != "two_spheres" else (0, 1):
        rc, x, sx = lanes(sim, d, blob_p, info_p, w, h, spp, kernel, CULL_EXACT)
        assert rc == 0
        rc, y, sy = lanes(sim, d, blob_d, info_d, w, h, spp, kernel, CULL_EXACT)
        assert rc == 0
        assert sx == sy == ca["segments"] and x.tobytes() == y.tobytes()


# ---------------------------------------------------------------- lanes against the oracle
def _lanes_match(sim, d, blob, info, o, size, shutter=None, exact_ok=True):
    w, h, spp = size
    ref, cnt = o.render(w, h, spp, 50, seed=S.SEED, camera=d.spec(shutter))
    ok, refused = lane_kernels(info)
    for k in refused:
        rc, _, _ = lanes(sim, d, blob, info, 8, 8, 1, k, CULL_EXACT, shutter=shutter)
        assert rc == 1, k
    rc, base, seg_r = lanes(sim, d, blob, info, w, h, spp, 2, CULL_REFERENCE, shutter=shutter)
    assert rc == 0
    linf = float(np.abs(base - ref).max())
    print(f"reference lanes: segments {seg_r} (oracle {cnt['segments']}), L-inf {linf:.3g}")
    assert seg_r == cnt["segments"] and np.isfinite(base).all() and linf <= TOL
    if not exact_ok:
        return cnt
    for k in ok:
        rc, img, seg = lanes(sim, d, blob, info, w, h, spp, k, CULL_EXACT, shutter=shutter)
        assert rc == 0, k
        linf = float(np.abs(img - ref).max())
        print(f"kernel {k}: segments {seg} (oracle {cnt['segments']}), L-inf {linf:.3g}")
        assert seg == cnt["segments"], k
        assert np.isfinite(img).all(), k
        assert linf <= TOL, (k, linf)
        # the general walk lane has no reference mode, and the sphere lane's walks the reference stream with the
        # BASIC shading alone (no noise / image textures: plan() sends those frames to the segment kernel)
        basic = (info.feature_mask & ~F_BASIC) == 0
        cull_k = k if k in (1, 2) or (k == 0 and basic) else 2
        rc, b, seg_b = lanes(sim, d, blob, info, w, h, spp, cull_k, CULL_REFERENCE, shutter=shutter)
        assert rc == 0 and seg_b == seg, k
        assert np.array_equal(img.view(np.uint32), b.view(np.uint32)), k
    return cnt


@pytest.mark.parametrize("name", list(S.TABLE))
def test_lanes_match_oracle(sim, built, name):
    d, _, blob, info, o = built(name)
    if name == "bvh_intervals":
        assert (info.box_t0, info.box_t1) == (0.25, 0.75)
    cnt = _lanes_match(sim, d, blob, info, o, S.TABLE[name][1])
    assert cnt["segments"] > cnt["samples"]  # paths bounce: the scene is in the frame


# one chunked case per kernel class (lane.h sample_chunk), the frames tests/test_gpu_scene_desc.py renders
CHUNKED = [("materials_spheres", (24, 16, 40)), ("instances", (16, 16, 70)), ("media_nested", (16, 16, 70))]


@pytest.mark.parametrize("name,size", CHUNKED)
def test_chunked_lanes_match_oracle(sim, built, name, size):
    d, _, blob, info, o = built(name)
    _lanes_match(sim, d, blob, info, o, size)


@pytest.mark.parametrize("shutter", S.BVH_SHUTTERS)
def test_bvh_intervals_shutters(sim, built, shutter):
    """Inside [box_t0, box_t1] = [0.25, 0.75] the exact lanes equal the oracle; under (0, 1) plan() falls back to the
    reference box test, which alone is held to the oracle here."""
    d, _, blob, info, o = built("bvh_intervals")
    inside = info.box_t0 <= shutter[0] and shutter[1] <= info.box_t1
    assert inside == (shutter != (0.0, 1.0))
    cnt = _lanes_match(sim, d, blob, info, o, S.SPHERE_SIZE, shutter=shutter, exact_ok=inside)
    assert cnt["moving"] > 0


# ---------------------------------------------------------------- each scene reaches its branch
def test_scenes_reach_their_branches(built):
    d, _, blob, info, _ = built("materials_spheres")
    assert info.feature_mask == F_BASIC and info.walk_general == 0 and info.media_nested == 0
    wts = [(w >> 4) & 15 for w in sphere_leaf_words(blob, info)]
    assert WT_GLOBAL not in wts and WT_CHECKER in wts and WT_SOLID in wts
    d, _, blob, info, _ = built("nested_checker")
    assert info.feature_mask & ~F_BASIC == 0 and info.walk_general == 0
    wts = [(w >> 4) & 15 for w in sphere_leaf_words(blob, info)]
    assert wts.count(WT_GLOBAL) == 2 and WT_CHECKER in wts  # the ground and one sphere; a plain checker besides
    _, _, blob, info, _ = built("lit_spheres")
    assert info.feature_mask & F["LIGHT"] and info.feature_mask & F["ISOTROPIC"]
    assert info.feature_mask & (F["RECT"] | F["INSTANCE"] | F["MEDIUM"] | F["MOVING"]) == 0
    assert info.walk_general == 1 and info.walk_bytes > 0  # off the sphere stream
    _, _, blob, info, _ = built("tex_sizes")
    assert info.feature_mask & F_HEAVY_TEX == F_HEAVY_TEX and info.feature_mask & ~(F_BASIC | F_HEAVY_TEX) == 0
    assert info.walk_general == 0 and WT_GLOBAL in [(w >> 4) & 15 for w in sphere_leaf_words(blob, info)]
    _, _, _, info, _ = built("instances")
    assert info.feature_mask & F["INSTANCE"] and info.feature_mask & F["IMAGE"] and not info.feature_mask & F["MEDIUM"]
    assert info.walk_general == 1 and info.media_nested == 0
    _, _, _, info, _ = built("media_nested")
    assert info.media_nested == 1 and info.walk_general == 0 and info.walk_bytes == 0  # build_gwalk returned early
    assert info.feature_mask & F["MEDIUM"] and info.feature_mask & F["NOISE"]
    _, _, _, info, _ = built("foggy")
    assert info.media_nested == 0 and info.walk_general == 1 and info.feature_mask & F["MEDIUM"]
    assert not info.feature_mask & (F["INSTANCE"] | F_HEAVY_TEX)  # media without instances or heavy textures
    _, _, _, info, _ = built("sphere_lists")
    assert info.walk_general == 1 and info.feature_mask & ~F_BASIC == 0
    _, _, _, info, _ = built("big_textured")
    assert info.walk_general == 0 and info.walk_hot > 0
    for k in S.ROOT_KINDS:
        _, _, _, info, _ = built(f"roots_{k}")
        assert info.n_nodes > 0 and info.main_end > 0
    _, _, _, info, _ = built("roots_translate_bvh")
    assert info.feature_mask & F["INSTANCE"]


COUNTERS = {
    "materials_spheres": ("moving", "tex_checker"), "nested_checker": ("tex_checker",), "lit_spheres": ("tex_checker",),
    "tex_sizes": ("tex_image", "tex_noise", "tex_checker"), "instances": ("rect", "moving", "tex_image"),
    "media_nested": ("medium", "rect", "moving", "tex_noise", "tex_checker"), "bvh_intervals": ("moving",),
    "foggy": ("medium", "rect", "moving"), "big_textured": ("tex_image", "tex_noise"), "sphere_lists": ("tex_checker",),
}


@pytest.mark.parametrize("name", list(COUNTERS))
def test_oracle_counters_show_the_scenes_features(built, name):
    d, _, _, _, o = built(name)
    w, h, spp = S.TABLE[name][1]
    _, cnt = o.render(w, h, spp, 50, seed=S.SEED)
    print(name, cnt)
    for c in COUNTERS[name]:
        assert cnt[c] > 0, c
    if name == "nested_checker":  # the nested checkers are evaluated: more checker values than Lambertian hits of one
        _, flat = S.nested_checker(nested=False).to_oracle().render(w, h, spp, 50, seed=S.SEED)
        assert cnt["tex_checker"] > flat["tex_checker"]


# ---------------------------------------------------------------- the parameter is visible in the frame
# label: (scene, the builder's argument put back to the presets' value, does it change the paths)
MUTATIONS = {
    "ior 2.4 -> 1.5": ("materials_spheres", dict(ior=1.5), True),
    "fuzz 1.5 -> 1.0": ("materials_spheres", dict(fuzz=1.0), True),
    "angle 33.3 -> 30": ("instances", dict(angle=30.0), True),
    "nested medium un-nested": ("media_nested", dict(nested=False), True),
    "nested checker flattened": ("nested_checker", dict(nested=False), False),
    "image 3x2 -> 1x1": ("tex_sizes", dict(small=True), False),
}


@pytest.mark.parametrize("label", list(MUTATIONS))
def test_parameter_is_visible(built, label):
    """The scene with one off-preset value put back to the presets' renders another oracle image at the test's size
    and camera, so a kernel that ignored the parameter could not pass.  A parameter of the geometry or of a
    scatter direction also changes the segment count.  (Un-nesting a medium gives the same scene in real arithmetic:
    media_nested keeps one medium in a far object frame, where the two forms round the scatter point differently
    enough to part the paths.)  An albedo cannot: ray_color (application.rs:477-495) ends a path at a miss, a light,
    a Metal that scatters into its surface or the depth cap, none of which reads the attenuation, so for the two
    texture mutations the segment counts must be EQUAL while the frames differ."""
    name, kw, paths = MUTATIONS[label]
    make, (w, h, spp) = S.TABLE[name]
    _, _, _, _, o = built(name)
    a, ca = o.render(w, h, spp, 50, seed=S.SEED)
    b, cb = make(**kw).to_oracle().render(w, h, spp, 50, seed=S.SEED)
    diff = int((a != b).any(axis=2).sum())
    print(f"{label}: {diff} of {w * h} pixels differ, segments {ca['segments']} -> {cb['segments']}")
    assert diff > 0
    assert (ca["segments"] != cb["segments"]) == paths
