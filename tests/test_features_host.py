"""The first-hit feature pass on the host (tests/native/feature_sim.hip over csrc/feature_pass.h), without a GPU: against
the independent restatement of the path (tests/test_path_restated.py), against the oracle's miss counts, the pass
schedule's place in the bit contract (include/hrt/hrt.h), and the other scene classes."""
import numpy as np
import pytest

import feature_sim as FS
import hrt
import test_path_restated as T
from oracle import oracle as O

K, SB, f = T.K, T.SB, np.float32
KIND = {"lambertian": FS.M_LAMBERTIAN, "lambertian_checker": FS.M_LAMBERTIAN, "metal": FS.M_METAL,
        "dielectric": FS.M_DIELECTRIC, "light": FS.M_DIFFUSE_LIGHT}
RANDOM_PIXELS = [(20, 10), (45, 22), (5, 30), (33, 17), (60, 2), (31, 12)]  # tests/test_path_restated.py's
# Cornell at 32 x 32: the light, the tall box's rotated front, the side wall, and a pixel on the silhouette between the
# two boxes (its 16 samples see both boxes' fronts)
CORNELL_PIXELS = [(14, 26), (12, 12), (3, 20), (15, 8)]
W, H = 64, 36


def u32(a):
    return np.ascontiguousarray(a, f).view(np.uint32)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return FS.build(tmp_path_factory)


def restated_first_hits(world, cam, bg, w, h, x, y, n, seed, t0, t1, v_first=False):
    """(kind, albedo, normal, depth) of the first hit of samples 0 .. n - 1 of a pixel: render_pixel's draws
    (tests/test_path_restated.py), then world.hit alone.  v_first: the teeth case, v's jitter drawn before u's."""
    out = []
    for s in range(n):
        rng = K.Rng(K.path_key(seed, y * w + x, s))
        if v_first:
            v = (f(y) + rng.gen_f32()) / (f(h) - f(1))
            u = (f(x) + rng.gen_f32()) / (f(w) - f(1))
        else:
            u = (f(x) + rng.gen_f32()) / (f(w) - f(1))
            v = (f(y) + rng.gen_f32()) / (f(h) - f(1))
        r = K.camera_ray(cam, u, v, T.random_in_unit_disk(rng), rng.gen_range(t0, t1))
        o, d = tuple(r[0:3]), tuple(r[3:6])
        hit = world.hit(o, d, r[6], f(0.001), T.INF)
        if hit is None:
            out.append((FS.MISS, bg, (f(0), f(0), f(0)), f(0)))
            continue
        rec, mat = hit
        if mat[0] == "lambertian_checker":  # checker_texture.rs:22-29: the choice at the restated hit point
            albedo = mat[1] if K.checker(tuple(rec[1:4])) == K.F3((0.2, 0.3, 0.1)) else mat[2]
        elif mat[0] == "dielectric":
            albedo = (f(1), f(1), f(1))
        else:
            albedo = mat[1]
        out.append((KIND[mat[0]], albedo, tuple(rec[4:7]), f(rec[0]) * np.sqrt(K.dot(d, d))))
    return out


def compare(sim, name, world, w, h, pixels, v_first=False):
    """The number of (sample, value) disagreements between feature_sim and the restatement over the pixels."""
    s = hrt.preset(name, 1)
    info = s.info
    cam = K.camera(K.F3(info.look_from), K.F3(info.look_at), f(info.fov), f(info.aperture), f(info.focus_dist), w, h)
    p = hrt.params(w, h, 16, 50, 3, tuple(info.background))
    bad, kinds = 0, set()
    for x, y in pixels:
        a, k, _ = FS.run(sim, s, hrt.preset_camera(info, w, h), p, region=(x, y, 1, 1))
        want = restated_first_hits(world, cam, K.F3(info.background), w, h, x, y, 16, 3, float(info.time0), float(info.time1), v_first)
        for i, (kind, albedo, normal, depth) in enumerate(want):
            got = a[0, 0, i]
            kinds.add(kind)
            bad += int(k[0, 0, i] != kind) + int(got[3] != (0.0 if kind == FS.MISS else 1.0))
            bad += int(not np.array_equal(u32(albedo), u32(got[:3])))
            # normal and depth: measured on the CPU, the library's values EQUAL the restatement's at all 160 samples
            # (largest deviation 0 for both, so ten times that is equality, inside the 1e-3 parity bar)
            bad += int(not np.array_equal(np.array(normal, f), got[4:7])) + int(f(depth) != got[7])
    return bad, kinds


def test_random_first_hits_equal_the_restatement(sim):
    bad, kinds = compare(sim, "random", T.Bvh(SB.random_scene(K.scene_rng(1))), W, H, RANDOM_PIXELS)
    assert bad == 0 and {FS.M_LAMBERTIAN, FS.M_METAL, FS.MISS} <= kinds


def test_cornell_first_hits_equal_the_restatement(sim):
    bad, kinds = compare(sim, "cornell", T.cornell_world(), 32, 32, CORNELL_PIXELS)
    assert bad == 0 and kinds == {FS.M_LAMBERTIAN, FS.M_DIFFUSE_LIGHT}


def test_restatement_has_teeth(sim):
    """v's jitter drawn before u's gives other camera rays: the comparison above is not one that anything passes."""
    bad, _ = compare(sim, "random", T.Bvh(SB.random_scene(K.scene_rng(1))), W, H, RANDOM_PIXELS[:2], v_first=True)
    assert bad > 0


def input_a():
    s = hrt.preset("random", 1)
    return s, hrt.preset_camera(s.info, W, H), lambda n, off: hrt.params(W, H, n, 50, 7, tuple(s.info.background), sample_offset=off)


def oracle_miss_counts(n=16):
    """The oracle at depth 1 returns sqrt(misses * background / n) on `random` (a hit's scattered ray is cut to black),
    so rint(z^2 n / bg) is the miss count: every channel within 3e-6 of an integer, the three channels agreeing."""
    s = hrt.preset("random", 1)
    ref, _ = O.OracleScene(hrt.PRESETS["random"], 1).render(W, H, n, 1, seed=7, threads=8)
    m = (ref[..., :3].astype(np.float64) ** 2) * n / np.array(s.info.background, np.float64)
    assert np.abs(m - np.rint(m)).max() <= 3e-6 and (np.rint(m) == np.rint(m[..., :1])).all()
    return np.rint(m[..., 0])


def test_hit_counts_equal_the_oracles_over_the_whole_frame(sim):
    s, cam, mk = input_a()
    _, _, sums = FS.run(sim, s, cam, mk(16, 0), per_sample=False)
    miss = oracle_miss_counts()
    assert 0.75 < (miss == 0).mean() < 0.85 and 0.12 < (miss == 16).mean() < 0.22 and ((miss > 0) & (miss < 16)).sum() > 50
    assert np.array_equal(16 - sums[..., 3], miss)


def test_the_pass_schedule_is_part_of_the_contract(sim):
    s, cam, mk = input_a()
    smp, _, one = FS.run(sim, s, cam, mk(16, 0))
    two = FS.planes(sim, s, cam, mk, [(0, 5), (5, 16)])
    head, tail = np.zeros((H, W, 8), f), np.zeros((H, W, 8), f)
    for k in range(5):
        head = head + smp[:, :, k]
    for k in range(5, 16):
        tail = tail + smp[:, :, k]
    assert np.array_equal(u32((np.zeros((H, W, 8), f) + head) + tail), u32(two))
    assert np.array_equal(u32(FS.planes(sim, s, cam, mk, [(0, 16)])), u32(one))
    assert (u32(one) != u32(two)).any()
    # the samples of a later pass are those of that index: offsets select, they do not reseed
    later, _, _ = FS.run(sim, s, cam, mk(11, 5))
    assert np.array_equal(u32(later), u32(smp[:, :, 5:]))


def test_every_instantiation_gives_the_same_bits_on_a_sphere_scene(sim):
    s, cam, mk = input_a()
    _, _, want = FS.run(sim, s, cam, mk(4, 0), per_sample=False)
    for cull in (FS.CULL_REFERENCE, FS.CULL_EXACT):
        for full in (0, 1):
            assert np.array_equal(u32(FS.run(sim, s, cam, mk(4, 0), cull=cull, full=full, per_sample=False)[2]), u32(want))


@pytest.mark.parametrize("name", ["cornell_smoke", "earth", "features"])
def test_other_scene_classes(sim, earth, name):
    """Media (zero normal, the medium's sub-stream), an image texture through (u, v), rotations and nested instances."""
    s = hrt.preset(name, 1, earth)
    p = hrt.params(32, 32, 4, 50, 7, tuple(s.info.background))
    a, k, sums = FS.run(sim, s, hrt.preset_camera(s.info, 32, 32), p)
    assert np.isfinite(a).all() and np.isfinite(sums).all()
    assert np.isin(a[..., 3], (0.0, 1.0)).all() and ((a[..., 3] == 0) == (k == FS.MISS)).all()
    hit = a[..., 3] == 1
    assert (a[..., 7][hit] > 0).all() and (a[..., 7][~hit] == 0).all() and (a[..., 4:7][~hit] == 0).all()
    surface = hit & (k != FS.M_ISOTROPIC)
    assert np.allclose(np.linalg.norm(a[..., 4:7][surface].astype(np.float64), axis=-1), 1.0, atol=1e-3)  # (p - c) / r in f32, then the instance rotations
    if name == "earth":
        assert len(np.unique(a[..., :3][hit], axis=0)) > 100  # the image's texels, not one colour
    if name != "cornell_smoke":
        return
    medium = k == FS.M_ISOTROPIC
    assert medium.sum() > 100 and (a[..., 4:7][medium] == 0).all() and (a[..., 7][medium] > 0).all()
    # a medium hit lies inside its box: behind the box's front face, which is the same sample's first hit in `cornell`
    # (whose boxes are the media's boundaries), by less than the tall box's diagonal
    solid = hrt.preset("cornell", 1, earth)
    b, kb, _ = FS.run(sim, solid, hrt.preset_camera(solid.info, 32, 32), p)
    front, depth = b[..., 7][medium], a[..., 7][medium]
    assert (kb[medium] == FS.M_LAMBERTIAN).all() and (depth > front).all()
    assert (depth < front + np.sqrt(165.0 ** 2 + 330.0 ** 2 + 165.0 ** 2)).all()
    # ... and in front of what the same ray hits when the medium lets it through: the far wall, at least 555 away
    wall = a[..., 7][hit & ~medium]
    assert depth.max() < wall.max()
    again = FS.run(sim, s, hrt.preset_camera(s.info, 32, 32), p)[0]
    assert np.array_equal(u32(again), u32(a))  # the keyed sub-stream: a rerun draws the same scatter distances
