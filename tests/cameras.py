"""Named cameras and shutters the presets never use, shared by tests/test_cameras.py (host lanes and the host
list check) and tests/test_gpu_cameras.py.  Test infrastructure, like tests/scenes.py.

Every oracle comparison elsewhere in the suite renders a preset from its own camera with the shutter [0, 1]; the
three list scenes share (13,2,3) -> (0,0,0), fov 20.  The cameras here reach what that one viewpoint leaves out
of the camera-dependent code: the per-cell leaf lists' hull pads, focus-plane split and inflation
(csrc/primary_list.h), the exact-culling error budget in |o|, |C - o| and the direction (lane.h box_ce, set_dir's
NaN mode), and plan()'s shutter guard (render.hip).

A camera is (look_from, look_at, fov, aperture, focus_dist); `spec` adds the shutter and gives the tuple
OracleScene.render(camera=) takes, `hrt_camera` the library's camera of the same values.
"""
import hrt

# name: (look_from, look_at, fov, aperture, focus_dist)
SPHERE_CAMERAS = {
    # origin inside a leaf's box and inside the dielectric sphere (0,1,0) r 1 of random / motion
    "inside_glass": ((0, 1, 0), (4, 1, 0), 60.0, 0.05, 4.0),
    # view nearly parallel to vup: u and v come from a cross product of nearly parallel vectors
    "topdown": ((0.001, 30, 0.001), (0, 0, 0), 30.0, 0.5, 30.0),
    # the direction signs opposite to the presets'; a lens (radius 1) wider than the small spheres
    "opp_octant_bigap": ((-13, 2, -3), (0, 0, 0), 20.0, 2.0, 10.0),
    # axis-aligned basis: zero components in horizontal and vertical, rays with zero direction components
    "axis": ((0, 1, 20), (0, 1, 0), 20.0, 0.1, 20.0),
    # a wide view: a cell's beam spans many leaves, directions far from the axis
    "wide": ((13, 2, 3), (0, 0, 0), 150.0, 0.1, 10.0),
    # origin 1.5e-3 above the radius-1000 ground sphere: |C - o| ~ r, grazing rays along the ground
    "near_ground": ((2, 0.0015, 2), (0, 0.2, 0), 40.0, 0.02, 2.8),
    # large |o| and a narrow beam: the pads that scale with |O| + |llc|; every cell overflows (culling only)
    "far": ((1300, 200, 300), (0, 0, 0), 0.2, 0.1, 1340.0),
    # looks upward from among the small spheres: sky behind them, the third sign pattern
    "low_up": ((3, 0.5, 3), (0, 1, 0), 40.0, 0.1, 4.0),
}

# cameras at which most 8x8 cells of the 1920x1080 frame keep a usable list (overflow share <= 0.25 at capacity 8)
LIST_FRIENDLY = ("inside_glass", "topdown", "wide", "axis", "near_ground")

# Three tiles of the 1920x1080 frame per list-friendly camera, chosen from the host builder's per-cell leaf counts
# (tests/native/primary_list.hip pl_build) so that on `random` and on `motion` each set holds cells of 1..3 leaves
# (listed at capacity 8 and 3) and cells of 4..8 leaves (listed at capacity 8, overflow at 3); the second and third
# tile start off the 8-px cell grid.  tests/test_cameras.py checks the counts.
LIST_TILES = {
    "inside_glass": [(1480, 184, 64, 16), (924, 312, 40, 24), (429, 485, 24, 8)],
    "topdown": [(712, 424, 64, 16), (916, 424, 40, 24), (933, 645, 24, 8)],
    "wide": [(888, 552, 64, 16), (300, 376, 40, 24), (645, 421, 24, 8)],
    "axis": [(984, 312, 64, 16), (588, 328, 40, 24), (613, 509, 24, 8)],
    "near_ground": [(416, 408, 64, 16), (964, 400, 40, 24), (1837, 421, 24, 8)],
}

GENERAL_CAMERAS = {
    # origin inside the Cornell box (and inside `final`'s volume of boxes and spheres)
    "inside_box": ((278, 278, 100), (400, 100, 400), 90.0, 0.0, 10.0),
    # looks up at the light, slightly off the vup axis
    "up_at_light": ((278, 50, 278), (278.5, 554, 279), 60.0, 0.0, 10.0),
    # a large lens (radius 10) from outside the box
    "lens": ((100, 400, -300), (278, 278, 200), 50.0, 20.0, 600.0),
}

SPHERE_SCENES = ("random", "motion")  # scenes whose launches build leaf lists
# two_spheres (two radius-10 spheres, 2 leaves; the sphere kernel's packet walk on the GPU) has no lens of its own:
# the cameras above give it one
PARITY_SPHERE_SCENES = SPHERE_SCENES + ("two_spheres",)
GENERAL_SCENES = ("cornell", "cornell_smoke", "final")

# (width, height, spp) of the oracle comparisons
ORACLE_SIZE = {"random": (40, 24, 8), "motion": (40, 24, 8), "two_spheres": (40, 24, 8), "cornell": (24, 24, 8),
               "cornell_smoke": (24, 24, 8), "final": (24, 24, 2)}

# shutters, the camera otherwise the preset's.  The BVH boxes of every preset are built for ray times in [0, 1]
# (hrt_blob_info box_t0 / box_t1): inside it the exact culling holds; a ray time outside it can put a moving sphere
# outside its box, and plan() falls back to the reference box test.
SHUTTER_INSIDE = (0.25, 0.75)
SHUTTERS_OUTSIDE = ((-0.5, 1.5), (0.5, 1.5), (3.0, 4.0))
SHUTTER_SCENES = ("random", "motion", "final")  # scenes with moving spheres


def cameras_of(name):
    return SPHERE_CAMERAS if name in PARITY_SPHERE_SCENES else GENERAL_CAMERAS


def scene_cameras():
    """Every (scene, camera name) pair of the two tables."""
    return [(s, c) for s in PARITY_SPHERE_SCENES for c in SPHERE_CAMERAS] + [(s, c) for s in GENERAL_SCENES for c in GENERAL_CAMERAS]


def spec(name, cam, info=None, shutter=None):
    """(look_from, look_at, fov, aperture, focus_dist, time0, time1): the named camera of scene `name` (cam None:
    the preset's own, from its hrt PresetInfo `info`) with the preset's shutter or `shutter`."""
    if cam is None:
        c = (tuple(info.look_from), tuple(info.look_at), info.fov, info.aperture, info.focus_dist)
    else:
        c = cameras_of(name)[cam]
    t0, t1 = shutter if shutter is not None else ((info.time0, info.time1) if info is not None else (0.0, 1.0))
    return (*c, float(t0), float(t1))


def hrt_camera(sp, width, height):
    return hrt.camera(*sp, width, height)
