"""Scenes built through the constructors that the oracle builds too (tests/scene_desc.py): each exists for one
branch of scene.cpp / render.hip plan() / lane.h that no preset reaches, named in its docstring.  Test
infrastructure; seeds are fixed and parameters literal.  tests/test_scene_desc.py runs the table on the host lanes,
tests/test_gpu_scene_desc.py on the GPU, both against the oracle's render of the same description.

Every builder returns a Desc that carries its camera and background.  A keyword argument of a builder is an
off-preset parameter; the value the presets use for it gives the mutated copy that
test_scene_desc.py::test_parameter_is_visible renders to show the parameter reaches the frame.
"""
import numpy as np

import hrt
import scenes
from scene_desc import Desc

X, Y, Z = hrt.AXIS_X, hrt.AXIS_Y, hrt.AXIS_Z
SPHERE_SIZE = (48, 27, 8)   # (width, height, spp) of the oracle comparisons: sphere geometry
GENERAL_SIZE = (32, 32, 8)  # rects, instances, media
BIG_SIZE = (32, 18, 4)      # big_textured


def _ground_checker(s):
    return s.lambertian(s.checker(s.solid(0.2, 0.3, 0.1), s.solid(0.9, 0.9, 0.9)))


def _small_lambertians(s, rng, n, y=0.25, r=0.25, span=4.0):
    out = []
    for _ in range(n):
        c = (float(rng.uniform(-span, span)), y, float(rng.uniform(-span, span)))
        out.append(s.sphere(c, r, s.lambertian(s.solid(*rng.uniform(0.1, 0.9, 3)))))
    return out


def materials_spheres(ior=2.4, fuzz=1.5):
    """F_BASIC sphere kernel, lane.h scatter's ior / fuzz word of the leaf payload (layout.h: f): Dielectric 2.4,
    1 / 1.5 and 1.0 (the presets: 1.5 everywhere), Metal fuzz 0, 0.999 and 1.5 (the presets: at most 1.0), and
    MovingSpheres with their own intervals, one of them outside [0, 1] (moving_sphere.rs:53-58 extrapolates)."""
    rng = np.random.default_rng(21)
    s = Desc(camera=((13, 2, 3), (0, 0.5, 0), 22.0, 0.1, 10.0, 0.0, 1.0))
    o = [s.sphere((0, -1000, 0), 1000, _ground_checker(s))]
    o.append(s.sphere((0, 1, 0), 1.0, s.dielectric(ior)))
    o.append(s.sphere((2.5, 0.6, 1.8), 0.6, s.dielectric(1.0 / 1.5)))
    o.append(s.sphere((2.5, 0.6, -1.6), 0.6, s.dielectric(1.0)))
    o.append(s.sphere((-3, 1, -1.8), 1.0, s.metal((0.7, 0.6, 0.5), 0.0)))
    o.append(s.sphere((4.5, 0.5, 0.2), 0.5, s.metal((0.9, 0.8, 0.6), 0.999)))
    o.append(s.sphere((-2, 0.8, 2.4), 0.8, s.metal((0.8, 0.8, 0.9), fuzz)))
    o += _small_lambertians(s, rng, 8)
    red = s.lambertian(s.solid(0.8, 0.2, 0.2))
    for k, (t0, t1) in enumerate(((0.0, 1.0), (0.25, 0.75), (-0.5, 0.5), (1.5, 2.5))):
        c0 = (1.0 + 1.2 * k, 0.3, 3.0 - 1.5 * k)
        o.append(s.moving_sphere(c0, (c0[0], c0[1] + 0.4, c0[2] + 0.2), t0, t1, 0.3, red if k % 2 else s.dielectric(ior)))
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def nested_checker(nested=True):
    """A WT_GLOBAL leaf in the non-HEAVY sphere kernel (scene.cpp's WT_CHECKER packing takes a checker of two
    SolidColors only; shade_walk<HEAVY = false> falls through to tex_value<false> from P.mats): the ground is
    checker(checker(solid, solid), solid), one sphere checker(solid, checker(solid, solid)).  nested=False: both
    flattened to checkers of two solids (WT_CHECKER leaves, the presets' form)."""
    rng = np.random.default_rng(22)
    s = Desc(camera=((13, 2, 3), (0, 0.5, 0), 22.0, 0.1, 10.0, 0.0, 1.0))
    inner = s.checker(s.solid(0.9, 0.1, 0.1), s.solid(0.1, 0.1, 0.9)) if nested else s.solid(0.9, 0.1, 0.1)
    ground = s.checker(inner, s.solid(0.9, 0.9, 0.9))
    o = [s.sphere((0, -1000, 0), 1000, s.lambertian(ground))]
    inner2 = s.checker(s.solid(0.1, 0.8, 0.1), s.solid(0.9, 0.9, 0.1)) if nested else s.solid(0.1, 0.8, 0.1)
    o.append(s.sphere((0, 1, 0), 1.0, s.lambertian(s.checker(s.solid(0.2, 0.2, 0.2), inner2))))
    o.append(s.sphere((3, 0.7, 1.8), 0.7, s.metal((0.7, 0.6, 0.5), 0.1)))
    o.append(s.sphere((-3, 1, -1.5), 1.0, s.dielectric(1.5)))
    o.append(s.sphere((3, 0.6, -1.6), 0.6, _ground_checker(s)))
    o += _small_lambertians(s, rng, 8)
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def lit_spheres():
    """Sphere geometry that leaves F_BASIC through F_LIGHT and F_ISOTROPIC alone, with no rect, instance or medium
    (shade_walk gathers radiance at a miss only, so plan() must not give this scene to the sphere kernel): a
    DiffuseLight sphere (emit 4), another whose emission is a checker of two colours, and a sphere with
    hrt_mat_isotropic as its SURFACE material; black background."""
    rng = np.random.default_rng(23)
    s = Desc(background=(0, 0, 0), camera=((13, 2, 3), (0, 0.8, 0), 24.0, 0.05, 10.0, 0.0, 1.0))
    o = [s.sphere((0, -1000, 0), 1000, s.lambertian(s.solid(0.6, 0.6, 0.6)))]
    o.append(s.sphere((0, 2.4, 0), 0.7, s.diffuse_light(s.solid(4, 4, 4))))
    o.append(s.sphere((2.5, 0.8, 2.0), 0.5, s.diffuse_light(s.checker(s.solid(3, 0.5, 0.5), s.solid(0.5, 0.5, 3)))))
    o.append(s.sphere((0, 0.8, 0), 0.8, s.isotropic(s.solid(0.8, 0.7, 0.3))))
    o.append(s.sphere((-2.5, 0.9, -1.2), 0.9, s.metal((0.8, 0.8, 0.8), 0.05)))
    o.append(s.sphere((2.5, 0.6, -1.4), 0.6, s.dielectric(1.5)))
    o += _small_lambertians(s, rng, 6)
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def _image(rng, h, w, c):
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def tex_sizes(small=False):
    """The sphere kernel's HEAVY instantiation: tex_value<true>, sphere_uv and image addressing at the edges
    (image_texture.rs:41-62) on images of 1x1, 3x2, 5x7 with 4 components and no data (magenta), noise scales 0.1
    and 37 over two different table sets, and checker(image, noise).  small=True: the 3x2 image becomes 1x1."""
    rng = np.random.default_rng(24)
    s = Desc(camera=((13, 2, 3), (0, 0.8, 0), 24.0, 0.05, 10.0, 0.0, 1.0))
    rv_a, pm_a = scenes.perlin_tables(31)
    rv_b, pm_b = scenes.perlin_tables(32)
    o = [s.sphere((0, -1000, 0), 1000, s.lambertian(s.noise(0.1, rv_a, pm_a)))]
    i32 = _image(rng, 2, 3, 3)
    o.append(s.sphere((0, 1, 0), 1.0, s.lambertian(s.image(i32[:1, :1] if small else i32))))
    o.append(s.sphere((2.6, 0.7, 2.0), 0.7, s.lambertian(s.image(_image(rng, 1, 1, 3)))))
    o.append(s.sphere((2.6, 0.7, -1.6), 0.7, s.lambertian(s.image(_image(rng, 7, 5, 4)))))
    o.append(s.sphere((-3, 1, -1.8), 1.0, s.lambertian(s.image(None))))
    o.append(s.sphere((-2, 0.8, 2.4), 0.8, s.lambertian(s.noise(37.0, rv_b, pm_b))))
    mixed = s.checker(s.image(_image(rng, 3, 4, 3)), s.noise(5.0, rv_b, pm_b))
    o.append(s.sphere((4.6, 0.5, 0.3), 0.5, s.lambertian(mixed)))
    o.append(s.sphere((0.5, 0.4, 3.0), 0.4, s.metal((0.8, 0.8, 0.8), 0.0)))
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


ANGLES = (0.0, 90.0, 180.0, -270.0, 405.0, 33.3)


def instances(angle=33.3):
    """Instance chains the presets never build, G::Inst's IF_INV / IF_DD and the TRIM_MEDIA instantiation with heavy
    textures present: a bare Rotation at 0, 90, 180, -270, 405 and 33.3 degrees about each axis over cuboids and
    rects (rotation.rs:38-99: sin / cos exact, or of a wrapped angle), Rotation of Rotation about another axis,
    Translation of Translation, Translation(Rotation(List[rect, sphere, moving sphere])), Rotation(BvhNode), an
    image-textured rect under an instance, a light; no medium.  angle: the 33.3 of the three bare rotations
    (the presets' nearest: 30)."""
    rng = np.random.default_rng(25)
    s = Desc(background=(0.25, 0.3, 0.4), camera=((9, 7, 11), (0, 0, 0), 50.0, 0.0, 10.0, 0.0, 1.0))
    white = s.lambertian(s.solid(0.73, 0.73, 0.73))
    cols = [s.lambertian(s.solid(*c)) for c in ((0.65, 0.05, 0.05), (0.12, 0.45, 0.15), (0.2, 0.2, 0.8))]
    o = []
    for ax in (X, Y, Z):  # objects strung along the axis they turn about, 0.9 off it
        for k, a in enumerate(ANGLES):
            t = -4.2 + 1.5 * k
            p0 = [0.9, 0.5, 0.0]
            p0.insert(ax, t)
            p0 = p0[:3]  # coordinate `ax` = t, the other two 0.9 and 0.5
            if k % 2 == 0:
                obj = s.cuboid(p0, [c + d for c, d in zip(p0, (0.9, 0.6, 0.7))], cols[ax])
            else:  # a rect in the plane that holds the axis: XY for X, YZ for Y, ZX for Z
                lo = p0[ax]
                obj = s.rect((hrt.PLANE_XY, hrt.PLANE_YZ, hrt.PLANE_ZX)[ax], lo, lo + 1.0, 0.3, 1.2, 0.8, white)
            o.append(s.rotate(ax, obj, angle if a == 33.3 else a))
    o.append(s.rotate(Z, s.rotate(X, s.cuboid((1.5, 1.5, 1.5), (2.5, 2.2, 2.4), white), 25.0), -40.0))
    o.append(s.translate(s.translate(s.sphere((0, 0, 0), 0.6, s.metal((0.8, 0.7, 0.5), 0.2)), (1.0, 2.0, 0.5)), (-3.0, 0.5, 2.5)))
    member = s.list([s.rect(hrt.PLANE_XY, -0.8, 0.8, -0.5, 0.5, 0.0, cols[0]), s.sphere((0, 0.9, 0), 0.4, s.dielectric(1.5)),
                     s.moving_sphere((0.9, 0, 0), (0.9, 0.4, 0.2), 0.0, 1.0, 0.3, cols[1])])
    o.append(s.translate(s.rotate(Y, member, 62.0), (3.0, 2.5, -2.5)))
    cloud = [s.sphere(tuple(rng.uniform(0, 1.5, 3)), 0.2, s.lambertian(s.solid(*rng.uniform(0.1, 0.9, 3)))) for _ in range(10)]
    o.append(s.rotate(X, s.bvh(cloud, 0.0, 1.0), 120.0))
    pic = s.lambertian(s.image(_image(rng, 5, 6, 3)))
    o.append(s.translate(s.rotate(Y, s.rect(hrt.PLANE_XY, -1.5, 1.5, -1.0, 1.0, 0.0, pic), -35.0), (-2.5, 2.0, -3.0)))
    o.append(s.rect(hrt.PLANE_ZX, -3, 3, -3, 3, 7.0, s.diffuse_light(s.solid(5, 5, 5))))
    o.append(s.rect(hrt.PLANE_ZX, -8, 8, -8, 8, -5.0, white))
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def media_nested(nested=True):
    """media_nested == 1 (a ConstantMedium inside a Translation / Rotation: plan() takes the scene off the general
    walk kernel onto the segment kernel, build_gwalk returns early): Translation(Rotation(medium(cuboid))),
    Rotation(medium(sphere)) and Translation(medium(moving sphere)) next to the presets'
    medium(Translation(Rotation(cuboid))); phase textures solid, checker and noise; a light.  nested=False: the
    first three un-nested into the presets' form, the instance inside the medium."""
    rng = np.random.default_rng(26)
    s = Desc(background=(0.05, 0.06, 0.1), camera=((0, 3, 12), (0, 1.2, 0), 38.0, 0.0, 10.0, 0.0, 1.0))
    white = s.lambertian(s.solid(0.73, 0.73, 0.73))
    glass = s.dielectric(1.5)
    rv, pm = scenes.perlin_tables(33)
    o = [s.rect(hrt.PLANE_ZX, -8, 8, -8, 8, 0.0, white)]
    o.append(s.rect(hrt.PLANE_ZX, -2, 2, -2, 2, 6.0, s.diffuse_light(s.solid(7, 7, 7))))

    def put(boundary, density, tex, wrap):
        """medium(boundary) inside the instances of `wrap` (innermost first), or, un-nested, around them."""
        node = s.constant_medium(boundary, density, tex) if nested else boundary
        for kind, *a in wrap:
            node = s.rotate(a[0], node, a[1]) if kind == "r" else s.translate(node, a[0])
        return node if nested else s.constant_medium(node, density, tex)

    o.append(put(s.cuboid((0, 0, 0), (1.5, 2.0, 1.5), white), 0.9, s.solid(0.1, 0.1, 0.1),
                 [("r", Y, 28.0), ("t", (-3.5, 0.0, -1.0))]))
    o.append(put(s.sphere((2.0, 1.0, 0.5), 0.9, glass), 1.5, s.checker(s.solid(0.9, 0.2, 0.2), s.solid(0.2, 0.9, 0.2)),
                 [("r", Y, -33.0)]))
    # a far object frame: the nested form scatters at moved.at(t) + displacement (translation.rs:29-30, ulp 2e-3
    # at 3e4), the un-nested form at ray.at(t) in the world frame, so the two forms trace visibly different paths
    o.append(put(s.moving_sphere((-30000, 0.8, 0), (-29999.7, 1.0, 0), 0.0, 1.0, 0.7, glass), 1.2, s.noise(3.0, rv, pm),
                 [("t", (29999.2, 0.1, 2.5))]))
    box = s.translate(s.rotate(Y, s.cuboid((0, 0, 0), (1.2, 1.2, 1.2), white), 45.0), (2.5, 0.0, 2.0))
    o.append(s.constant_medium(box, 0.8, s.solid(0.2, 0.4, 0.9)))
    o += _small_lambertians(s, rng, 5, y=0.3, r=0.3, span=3.0)
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def _root_spheres(s):
    return [s.sphere((0, 1, 0), 1.0, s.lambertian(s.solid(0.4, 0.2, 0.1))), s.sphere((3, 0.7, 1.5), 0.7, s.dielectric(1.5)),
            s.sphere((0, -1000, 0), 1000, _ground_checker(s)), s.sphere((-3, 1, -1.5), 1.0, s.metal((0.7, 0.6, 0.5), 0.0))]


def roots(kind):
    """emit / flatten at the root and the stream builders on degenerate hierarchies: the root is a List
    ("list"), one sphere ("sphere"), a BvhNode of one sphere ("bvh1"), or a Translation of a BvhNode
    ("translate_bvh"); every preset's root is a BvhNode of several objects."""
    s = Desc(camera=((13, 2, 3), (0, 0.5, 0), 22.0, 0.1, 10.0, 0.0, 1.0))
    if kind == "list":
        s.set_root(s.list(_root_spheres(s)))
    elif kind == "sphere":
        s.set_root(s.sphere((0, 0.5, 0), 1.5, _ground_checker(s)))
    elif kind == "bvh1":
        s.set_root(s.bvh([s.sphere((0, 0.5, 0), 1.5, _ground_checker(s))], 0.0, 1.0))
    else:
        s.set_root(s.translate(s.bvh(_root_spheres(s), 0.0, 1.0), (0.5, 0.25, -0.5)))
    return s


ROOT_KINDS = ("list", "sphere", "bvh1", "translate_bvh")
BVH_SHUTTERS = ((0.25, 0.75), (0.0, 1.0), (0.3, 0.6))


def bvh_intervals():
    """box_t0 / box_t1 (scene.cpp build_bvh intersects the intervals of every BvhNode built) and plan()'s
    REFERENCE fallback on a constructor-built scene: moving spheres under bvh(..., 0.25, 0.75) nested in
    bvh(..., 0.0, 1.0), so the boxes hold for ray times in [0.25, 0.75] only; rendered with the shutters
    BVH_SHUTTERS.  Under (0, 1) a sphere can be outside its box, which the reference then misses
    (bvh_node.rs:104-127 tests the box first): only the verbatim box test reproduces that."""
    rng = np.random.default_rng(27)
    s = Desc(camera=((13, 2, 3), (0, 0.5, 0), 22.0, 0.1, 10.0, 0.25, 0.75))
    movers = []
    for k in range(10):
        c0 = (float(rng.uniform(-3, 3)), 0.3, float(rng.uniform(-3, 3)))
        c1 = (c0[0] + float(rng.uniform(-1, 1)), 0.3 + float(rng.uniform(0, 1.5)), c0[2] + float(rng.uniform(-1, 1)))
        mat = s.lambertian(s.solid(*rng.uniform(0.1, 0.9, 3))) if k % 3 else s.metal((0.8, 0.7, 0.6), 0.1)
        movers.append(s.moving_sphere(c0, c1, 0.0, 1.0, 0.3, mat))
    inner = s.bvh(movers, 0.25, 0.75)
    o = [inner, s.sphere((0, -1000, 0), 1000, _ground_checker(s)), s.sphere((0, 1, 0), 1.0, s.dielectric(1.5)),
         s.moving_sphere((3, 0.5, 0), (3, 1.5, 0.5), 0.0, 1.0, 0.5, s.lambertian(s.solid(0.8, 0.3, 0.1)))]
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def _recorded(make, **kw):
    s = Desc()
    make(s=s, **kw)
    return s


# name: (builder, (width, height, spp)).  The last three are tests/scenes.py's, recorded.
TABLE = {
    "materials_spheres": (materials_spheres, SPHERE_SIZE),
    "nested_checker": (nested_checker, SPHERE_SIZE),
    "lit_spheres": (lit_spheres, SPHERE_SIZE),
    "tex_sizes": (tex_sizes, SPHERE_SIZE),
    "instances": (instances, GENERAL_SIZE),
    "media_nested": (media_nested, GENERAL_SIZE),
    **{f"roots_{k}": ((lambda k=k: roots(k)), SPHERE_SIZE) for k in ROOT_KINDS},
    "bvh_intervals": (bvh_intervals, SPHERE_SIZE),
    "sphere_lists": ((lambda: _recorded(scenes.sphere_lists)), SPHERE_SIZE),
    "big_textured": ((lambda: _recorded(scenes.big_textured)), BIG_SIZE),
    "foggy": ((lambda: _recorded(scenes.foggy)), GENERAL_SIZE),
}
SEED = 3


# ---------------------------------------------------------------- four presets written by hand
def preset_two_spheres():
    """application.rs:567-587"""
    s = Desc(camera=((13, 2, 3), (0, 0, 0), 20.0, 0.0, 10.0, 0.0, 1.0))
    checker = _ground_checker(s)
    s.set_root(s.bvh([s.sphere((0, -10, 0), 10, checker), s.sphere((0, 10, 0), 10, checker)], 0.0, 1.0))
    return s


def _cornell(smoke):
    """application.rs:639-815"""
    s = Desc(background=(0, 0, 0), camera=((278, 278, -800), (278, 278, 0), 40.0, 0.0, 10.0, 0.0, 1.0))
    red = s.lambertian(s.solid(0.65, 0.05, 0.05))
    white = s.lambertian(s.solid(0.73, 0.73, 0.73))
    green = s.lambertian(s.solid(0.12, 0.45, 0.15))
    light = s.diffuse_light(s.solid(15, 15, 15))
    o = [s.rect(hrt.PLANE_YZ, 0, 555, 0, 555, 555, green), s.rect(hrt.PLANE_YZ, 0, 555, 0, 555, 0, red),
         s.rect(hrt.PLANE_ZX, 213, 343, 227, 332, 554, light), s.rect(hrt.PLANE_ZX, 0, 555, 0, 555, 0, white),
         s.rect(hrt.PLANE_ZX, 0, 555, 0, 555, 555, white), s.rect(hrt.PLANE_XY, 0, 555, 0, 555, 555, white)]
    c1 = s.translate(s.rotate(Y, s.cuboid((0, 0, 0), (165, 330, 165), white), 15.0), (265, 0, 295))
    o.append(s.constant_medium(c1, 0.01, s.solid(0, 0, 0)) if smoke else c1)
    c2 = s.translate(s.rotate(Y, s.cuboid((0, 0, 0), (165, 165, 165), white), -18.0), (130, 0, 65))
    o.append(s.constant_medium(c2, 0.01, s.solid(1, 1, 1)) if smoke else c2)
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s


def preset_cornell():
    return _cornell(False)


def preset_cornell_smoke():
    return _cornell(True)


def preset_simple_light(ranvec, perm):
    """application.rs:614-637; the Perlin tables are the first draws of the preset's builder stream."""
    s = Desc(background=(0, 0, 0), camera=((26, 3, 6), (0, 2, 0), 20.0, 0.0, 10.0, 0.0, 1.0))
    noise = s.lambertian(s.noise(4.0, ranvec, perm))
    o = [s.sphere((0, -1000, 0), 1000, noise), s.sphere((0, 2, 0), 2, noise),
         s.rect(hrt.PLANE_XY, 3, 5, 1, 3, -2, s.diffuse_light(s.solid(4, 4, 4)))]
    s.set_root(s.bvh(o, 0.0, 1.0))
    return s
