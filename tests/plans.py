"""The kernel plans of render.hip plan() / launch_any(), render_sphere.hip launch_sphere() and render_general.hip
launch_gwalk(): a hand-written checklist of the instantiations the dispatch can reach, and a table with at least one
row per entry.  Test infrastructure, like tests/cameras.py and tests/scenes_oracle.py.

tests/test_plans.py (CPU) holds the checklist to the dispatch's source and to the table, and qualifies the inputs of
the approximate rows on the host lanes and in the oracle; tests/test_gpu_plans.py renders every row on the GPU.

CHECKLIST
  key -> Entry(launcher, args, where, unreached).  `args` are the template arguments that name the instantiation in
  a launch record (hrt_last_launch: "launch_basic[CULL = 2, COUNT = false, LDS = true, ...]"), COUNT left out: every
  entry exists with COUNT = false and COUNT = true, and every row is rendered with both.  `where` cites the dispatch.
  `unreached`: None, or why no row reaches the entry.

ROWS
  Row(id, entries, scene, size, seed, flags, commit, launch, kind, shutter, extra, unambiguous)
  - scene: a key of SCENES (a preset name, or a builder of tests/scenes_oracle.py / tests/scenes.py);
  - size (width, height, spp); at most 64 x 36 x 8, random_10k and final at most 48 x 27 x 4;
  - flags: hrt.RENDER_*; commit / launch: the knobs set while the scene is committed / while it is rendered;
  - kind: "exact" (every cull but slab: oracle segment counts, L-inf <= 1e-3, the default plan's bits), "slab"
    (HRT_RENDER_FAST_CULL: the default plan's bits and segments on inputs the CPU test qualified), "sah"
    (HRT_RENDER_FAST_CULL | HRT_RENDER_SAH on the octant streams: the slab frame's bits on the unambiguous pixels,
    L-inf <= 1e-3 against the oracle);
  - extra: further substrings the launch record must hold ("!x": must not hold);
  - unambiguous: "sah" rows, the number of pixels whose bits the oracle renders alike under the scene's BvhNode
    root and under a plain List of the same spheres (tests/test_plans.py checks the number and that it is >= 99%).
"""
from collections import namedtuple

import hrt
import scenes
import scenes_oracle as S

CULL_REFERENCE, CULL_SLAB, CULL_EXACT = 0, 1, 2  # csrc/layout.h
WM_LDS, WM_BUF, WM_HYB = 0, 1, 3                 # csrc/lane.h
TRIM_MEDIA, TRIM_HEAVY_TEX, TRIM_PROGRAMS = 1, 2, 4

Entry = namedtuple("Entry", "launcher args where unreached")
Row = namedtuple("Row", "id entries scene size seed flags commit launch kind shutter extra unambiguous")


def _b(v):
    return "true" if v else "false"


# ------------------------------------------------------------------------------------------------ the checklist
CHECKLIST = {}


def _sphere(key, cull, lds, hyb, heavy, split, c16, packet, where, unreached=None):
    CHECKLIST["sphere/" + key] = Entry("launch_basic", (("CULL", str(cull)), ("LDS", _b(lds)), ("HYB", _b(hyb)),
                                                        ("HEAVY", _b(heavy)), ("SPLIT", _b(split)), ("C16", _b(c16)),
                                                        ("PACKET", _b(packet))), where, unreached)


# render_sphere.hip launch_sphere(): 18 tuples (CULL, LDS, HYB, HEAVY, SPLIT, C16, PACKET)
E = CULL_EXACT
_sphere("packet", E, 1, 0, 0, 0, 0, 1, "launch_sphere: packet && lds && exact && walk_hot == 0, !heavy")
_sphere("packet_heavy", E, 1, 0, 1, 0, 0, 1, "launch_sphere: packet ..., heavy")
_sphere("heavy_hyb", E, 1, 1, 1, 0, 0, 0, "launch_sphere: heavy, lds && walk_hot > 0")
_sphere("heavy_lds", E, 1, 0, 1, 0, 0, 0, "launch_sphere: heavy, lds")
_sphere("heavy_nolds", E, 0, 0, 1, 0, 0, 0, "launch_sphere: heavy, !lds")
_sphere("c16_hyb", E, 1, 1, 0, 0, 1, 0, "launch_sphere: exact && walk_c16, lds")
_sphere("c16_nolds", E, 0, 0, 0, 0, 1, 0, "launch_sphere: exact && walk_c16, !lds")
_sphere("hyb_split", E, 1, 1, 0, 1, 0, 0, "launch_sphere: walk_half == WALK_SPLIT_HALF_HYB, lds && walk_hot > 0")
_sphere("hyb_split_nolds", E, 0, 1, 0, 1, 0, 0, "launch_sphere: walk_half == WALK_SPLIT_HALF_HYB, nothing staged")
_sphere("hyb", E, 1, 1, 0, 0, 0, 0, "launch_sphere: exact && lds && walk_hot > 0")
_sphere("split_lds", E, 1, 0, 0, 1, 0, 0, "launch_sphere: exact && walk_half != 16, lds")
_sphere("split_nolds", E, 0, 0, 0, 1, 0, 0, "launch_sphere: exact && walk_half != 16, !lds")
_sphere("exact_lds", E, 1, 0, 0, 0, 0, 0, "launch_sphere: exact, lds")
_sphere("exact_nolds", E, 0, 0, 0, 0, 0, 0, "launch_sphere: exact, !lds")
_sphere("slab_lds", CULL_SLAB, 1, 0, 0, 0, 0, 0, "launch_sphere: slab, lds")
_sphere("slab_nolds", CULL_SLAB, 0, 0, 0, 0, 0, 0, "launch_sphere: slab, !lds")
_sphere("ref_lds", CULL_REFERENCE, 1, 0, 0, 0, 0, 0, "launch_sphere: reference, lds")
_sphere("ref_nolds", CULL_REFERENCE, 0, 0, 0, 0, 0, 0, "launch_sphere: reference, !lds")
SPHERE_EXACT = [k for k, e in CHECKLIST.items() if e.launcher == "launch_basic" and e.args[0][1] == str(E)]


def _segment(key, cull, full, lds, fast, gw, trim, where, unreached=None):
    CHECKLIST["segment/" + key] = Entry("launch", (("CULL", str(cull)), ("FULL", _b(full)), ("LDS", _b(lds)),
                                                   ("FAST", _b(fast)), ("GW", str(gw)), ("TRIM", str(trim))), where,
                                        unreached)


# render.hip launch_any(): the segment kernel render_kernel<CULL, FULL, COUNT, LDS, FAST, GW, TRIM>
for _lds, _n in ((1, "lds"), (0, "nolds")):
    _segment("fast_" + _n, CULL_SLAB, 0, _lds, 1, 0, 0, "launch_any: pl.fast")
    _segment("trim_both_" + _n, E, 1, _lds, 0, 4, TRIM_MEDIA | TRIM_HEAVY_TEX,
             "launch_any: pl.general && pl.full, exact, gen_waves 4, trim MEDIA | HEAVY_TEX")
    _segment("trim_tex_" + _n, E, 1, _lds, 0, 4, TRIM_HEAVY_TEX, "launch_any: ... gen_waves 4, trim HEAVY_TEX")
    _segment("full_exact4_" + _n, E, 1, _lds, 0, 4, 0, "launch_any: ... exact, gen_waves 4, trim 0")
    _segment("full_exact3_" + _n, E, 1, _lds, 0, 0, 0, "launch_any: ... exact, gen_waves 3 (F_NOISE in LDS)")
    _segment("full_slab_" + _n, CULL_SLAB, 1, _lds, 0, 0, 0, "launch_any: pl.general && pl.full, slab")
    _segment("full_ref_" + _n, CULL_REFERENCE, 1, _lds, 0, 0, 0, "launch_any: pl.general && pl.full, reference")
    # sphere scenes on the segment kernel (the diagnostic HRT_KERNEL=general)
    _segment("basic_exact_" + _n, E, 0, _lds, 0, 0, 0, "launch_any: pl.general && !pl.full, exact")
    _segment("basic_slab_" + _n, CULL_SLAB, 0, _lds, 0, 0, 0, "launch_any: pl.general && !pl.full, slab")
    _segment("basic_ref_" + _n, CULL_REFERENCE, 0, _lds, 0, 0, 0, "launch_any: pl.general && !pl.full, reference")

# render.hip launch_any(): render_full_kernel<CULL, COUNT, LDS> (HRT_KERNEL=persistent)
for _c, _cn in ((E, "exact"), (CULL_SLAB, "slab"), (CULL_REFERENCE, "ref")):
    for _lds, _n in ((1, "lds"), (0, "nolds")):
        CHECKLIST[f"persistent/{_cn}_{_n}"] = Entry("launch_full", (("CULL", str(_c)), ("LDS", _b(_lds))),
                                                    f"launch_any: !pl.general && pl.full, {_cn}", None)


def _gwalk(key, args, where, unreached=None):
    CHECKLIST["gwalk/" + key] = Entry("launch_g", args, where, unreached)


# render_general.hip launch_g_mem(): the shapes (WMEM, LREF, BIG, ONE, PACKET) ...
def _shape(wmem, lref, big, one, packet):
    return (("WMEM", str(wmem)), ("LREF", _b(lref)), ("BIG", _b(big)), ("ONE", _b(one)), ("PACKET", _b(packet)))


_gwalk("packet", _shape(WM_LDS, 1, 0, 0, 1), "launch_g_mem: wmem == WM_LDS && lref && packet (no TRIM_PROGRAMS)")
_gwalk("lds_lref", _shape(WM_LDS, 1, 0, 0, 0), "launch_g_mem: WM_LDS, lref")
_gwalk("lds", _shape(WM_LDS, 0, 0, 0, 0), "launch_g_mem: WM_LDS, !lref")
_gwalk("hyb_big_one", _shape(WM_HYB, 0, 1, 1, 0), "launch_g_mem: WM_HYB && smem > LDS_SCENE_MAX_BYTES, one")
_gwalk("hyb_big", _shape(WM_HYB, 0, 1, 0, 0), "launch_g_mem: WM_HYB && smem > LDS_SCENE_MAX_BYTES, !one")
_gwalk("hyb", _shape(WM_HYB, 0, 0, 0, 0), "launch_g_mem: WM_HYB")
_gwalk("buf", _shape(WM_BUF, 0, 0, 0, 0), "launch_g_mem: WM_BUF")
# ... times the six trims launch_gwalk() instantiates; the table reaches each trim and each shape, not their product
GWALK_TRIMS = (0, TRIM_MEDIA, TRIM_HEAVY_TEX, TRIM_MEDIA | TRIM_HEAVY_TEX, TRIM_PROGRAMS,
               TRIM_MEDIA | TRIM_HEAVY_TEX | TRIM_PROGRAMS)
for _t in GWALK_TRIMS:
    _gwalk(f"trim{_t}", (("TRIM", str(_t)),), f"launch_gwalk: trim == {_t}")


def expected(row):
    """The substrings (and "!substring"s) the launch record of `row` must hold."""
    out = []
    for key in row.entries:
        e = CHECKLIST[key]
        out.append(e.launcher + "[")
        out += [f"{n} = {v}" for n, v in e.args]
    return out + list(row.extra)


# ------------------------------------------------------------------------------------------------ the scenes
PRESETS = ("random", "random_10k", "two_spheres", "two_perlin_spheres", "simple_light", "cornell", "cornell_smoke", "final")
# layout.h: a sphere stream is 32 B (WALK_NODE_BYTES) per node part and 96 B per leaf payload, 2 n - 1 node parts for
# n leaves, so 160 n - 32 B; it exceeds LDS_SCENE_MAX_BYTES (77 KiB = 78848 B) from n = 494 leaves.  big_textured has
# grid^2 + 3 spheres: grid 22 gives 487 leaves (77888 B, staged whole), grid 23 gives 532 (85088 B), the smallest hybrid one.
BUILDERS = {
    "materials_spheres": S.materials_spheres,
    "nested_checker": S.nested_checker,
    "tex_sizes": S.tex_sizes,
    "instances": S.instances,
    "media_nested": S.media_nested,
    "textured_19": lambda: S._recorded(scenes.big_textured, grid=4),     # HEAVY, 37 node parts: beyond the packet walk
    "textured_532": lambda: S._recorded(scenes.big_textured, grid=23),   # HEAVY and hybrid
}
SCENES = PRESETS + tuple(BUILDERS)
SPHERE_ONLY_DESC = ("materials_spheres", "nested_checker")  # F_BASIC scenes built through Desc: the SAH rows' scenes


class Source:
    """One scene of SCENES for the library and for the oracle."""

    def __init__(self, name, earth):
        self.name, self.earth = name, earth
        self.desc = BUILDERS[name]() if name in BUILDERS else None
        self._oracle = None

    def build(self):
        """An uncommitted hrt.Scene (the caller sets the commit knobs)."""
        return self.desc.to_hrt() if self.desc else hrt.preset(self.name, 1, self.earth)

    def oracle(self):
        if self._oracle is None:
            from oracle import oracle as O

            self._oracle = self.desc.to_oracle() if self.desc else O.OracleScene(hrt.PRESETS[self.name], 1, self.earth)
        return self._oracle

    def spec(self, scene, shutter=None):
        if self.desc:
            return self.desc.spec(shutter)
        i = scene.info
        t = shutter if shutter is not None else (i.time0, i.time1)
        return (tuple(i.look_from), tuple(i.look_at), i.fov, i.aperture, i.focus_dist, float(t[0]), float(t[1]))

    def background(self, scene):
        return self.desc.background if self.desc else tuple(scene.info.background)


def list_root(desc):
    """`desc` with its root BvhNode replaced by a plain List of the same children in the same order (for the
    oracle alone: the brute-force frame, no hierarchy)."""
    d = desc.copy()
    name, args, rid = d.calls.pop()
    assert name == "bvh" and rid == d.root
    d._n["node"] -= max(1, 2 * len(args[0]) - 1)
    d.set_root(d.list(args[0]))
    return d


# ------------------------------------------------------------------------------------------------ the table
NO_LDS, COUNT_WORK = hrt.RENDER_NO_LDS, hrt.RENDER_COUNT_WORK
REF, FASTC, SAH = hrt.RENDER_REFERENCE_CULL, hrt.RENDER_FAST_CULL, hrt.RENDER_FAST_CULL | hrt.RENDER_SAH
SIZES = {"random": (40, 24, 8), "random_10k": (48, 27, 4), "final": (32, 24, 4), "two_spheres": (48, 27, 8),
         "two_perlin_spheres": (48, 27, 8), "simple_light": (32, 24, 8), "cornell": (24, 24, 8), "cornell_smoke": (24, 24, 8),
         "materials_spheres": S.SPHERE_SIZE, "nested_checker": S.SPHERE_SIZE, "tex_sizes": S.SPHERE_SIZE,
         "instances": S.GENERAL_SIZE, "media_nested": S.GENERAL_SIZE, "textured_19": S.SPHERE_SIZE, "textured_532": S.BIG_SIZE}
SEED = 3
SHUTTER_OUTSIDE = (-0.5, 1.5)
ROWS = []


def _row(rid, entries, scene, flags=0, commit=(), launch=(), kind="exact", shutter=None, extra=(), unambiguous=None,
         seed=SEED):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)
    ROWS.append(Row(rid, entries, scene, SIZES[scene], seed, flags, tuple(commit), tuple(launch), kind, shutter,
                    tuple(extra), unambiguous))


SPLIT, C16 = ("HRT_WALK_SPLIT", "1"), ("HRT_WALK_C16", "1")
# --- the sphere kernel
_row("packet", "sphere/packet", "two_spheres")
_row("packet_heavy", "sphere/packet_heavy", "two_perlin_spheres")
_row("packet_heavy_images", "sphere/packet_heavy", "tex_sizes")  # 15 node parts: SPHERE_PACKET_NODES exactly
_row("heavy_hyb", "sphere/heavy_hyb", "textured_532")
_row("heavy_hyb_nolds", "sphere/heavy_nolds", "textured_532", NO_LDS)  # a hybrid layout read from global memory
_row("heavy_lds", "sphere/heavy_lds", "textured_19")
_row("heavy_nolds", "sphere/heavy_nolds", "textured_19", NO_LDS)
_row("c16_hyb", "sphere/c16_hyb", "random_10k", commit=[C16])
_row("c16_nolds", "sphere/c16_nolds", "random_10k", NO_LDS, commit=[C16])
_row("hyb", "sphere/hyb", "random_10k")
_row("hyb_nolds", "sphere/exact_nolds", "random_10k", NO_LDS)
_row("hyb_split", "sphere/hyb_split", "random_10k", commit=[SPLIT])
_row("hyb_split_nolds", "sphere/hyb_split_nolds", "random_10k", NO_LDS, commit=[SPLIT])
_row("split_lds", "sphere/split_lds", "random", commit=[SPLIT])
_row("split_nolds", "sphere/split_nolds", "random", NO_LDS, commit=[SPLIT])
_row("exact_lds", "sphere/exact_lds", "random")
_row("exact_nolds", "sphere/exact_nolds", "random", NO_LDS)
_row("slab_lds", "sphere/slab_lds", "random", FASTC, kind="slab")
_row("slab_nolds", "sphere/slab_nolds", "random", FASTC | NO_LDS, kind="slab")
_row("ref_lds", "sphere/ref_lds", "random", REF)
_row("ref_nolds", "sphere/ref_nolds", "random", REF | NO_LDS)
for _s in SPHERE_ONLY_DESC:
    _row(f"{_s}_exact", "sphere/exact_lds", _s)
    _row(f"{_s}_slab", "sphere/slab_lds", _s, FASTC, kind="slab")
# HRT_PRIMARY_LISTS=0: one row per exact sphere entry (render.hip primary_list_cap builds lists for exact_lds alone)
NO_LISTS = ("HRT_PRIMARY_LISTS", "0")
for _e, _scene, _flags, _commit in (
        ("packet", "two_spheres", 0, ()), ("packet_heavy", "two_perlin_spheres", 0, ()),
        ("heavy_hyb", "textured_532", 0, ()), ("heavy_lds", "textured_19", 0, ()), ("heavy_nolds", "textured_19", NO_LDS, ()),
        ("c16_hyb", "random_10k", 0, (C16,)), ("c16_nolds", "random_10k", NO_LDS, (C16,)), ("hyb", "random_10k", 0, ()),
        ("hyb_split", "random_10k", 0, (SPLIT,)), ("hyb_split_nolds", "random_10k", NO_LDS, (SPLIT,)),
        ("split_lds", "random", 0, (SPLIT,)), ("split_nolds", "random", NO_LDS, (SPLIT,)),
        ("exact_lds", "random", 0, ()), ("exact_nolds", "random", NO_LDS, ())):
    _row(f"nolists_{_e}", "sphere/" + _e, _scene, _flags, commit=_commit, launch=[NO_LISTS])
assert sorted(r.entries[0] for r in ROWS if r.id.startswith("nolists_")) == sorted(SPHERE_EXACT)

# --- the SAH octant streams (segment kernel, FAST) and the fall-backs
_row("sah_materials", "segment/fast_lds", "materials_spheres", SAH, kind="sah", unambiguous=1296)
_row("sah_materials_nolds", "segment/fast_nolds", "materials_spheres", SAH | NO_LDS, kind="sah", unambiguous=1296)
_row("sah_nested_checker", "segment/fast_lds", "nested_checker", SAH, kind="sah", unambiguous=1296)
# a shutter outside [0, 1]: plan() takes the reference box test and no octant stream
_row("sah_shutter_outside", "sphere/ref_lds", "materials_spheres", SAH, shutter=SHUTTER_OUTSIDE, extra=["!FAST = true"])
# a general scene: the segment kernel over the reference stream under slab culling
_row("sah_general", "segment/full_slab_lds", "simple_light", SAH, kind="slab")

# --- the segment kernel on general scenes
SEGMENT, GENERAL, PERSISTENT = ("HRT_KERNEL", "segment"), ("HRT_KERNEL", "general"), ("HRT_KERNEL", "persistent")
_row("seg_nested_w3", "segment/full_exact3_lds", "media_nested")  # a nested medium: the segment kernel by default
_row("seg_nested_w4_nolds", "segment/full_exact4_nolds", "media_nested", NO_LDS)
_row("seg_nested_w3_nolds", "segment/full_exact3_nolds", "media_nested", NO_LDS, launch=[("HRT_GEN_WAVES_RT", "3")])
_row("seg_instances_w4", "segment/full_exact4_lds", "instances", launch=[SEGMENT])  # image texture, no noise: trim 0
_row("seg_cornell_trim3", "segment/trim_both_lds", "cornell", launch=[SEGMENT])
_row("seg_cornell_trim3_nolds", "segment/trim_both_nolds", "cornell", NO_LDS, launch=[SEGMENT])
_row("seg_smoke_trim2", "segment/trim_tex_lds", "cornell_smoke", launch=[SEGMENT])
_row("seg_smoke_trim2_nolds", "segment/trim_tex_nolds", "cornell_smoke", NO_LDS, launch=[SEGMENT])
# slab culling needs boxes that hold their geometry (scene.cpp box_ok: every preset with a ZX light rect of
# a0..a1 != b0..b1 fails, and plan() then ignores HRT_RENDER_FAST_CULL): simple_light and media_nested pass
_row("seg_light_slab", "segment/full_slab_lds", "simple_light", FASTC, kind="slab")
_row("seg_light_slab_nolds", "segment/full_slab_nolds", "simple_light", FASTC | NO_LDS, kind="slab")
_row("seg_nested_slab", "segment/full_slab_lds", "media_nested", FASTC, kind="slab")
_row("cornell_ignores_fast_cull", ("gwalk/lds_lref", "gwalk/trim7"), "cornell", FASTC)
_row("seg_cornell_ref", "segment/full_ref_lds", "cornell", REF)
_row("seg_cornell_ref_nolds", "segment/full_ref_nolds", "cornell", REF | NO_LDS)
# --- the segment kernel on a sphere scene (HRT_KERNEL=general)
_row("seg_random_exact", "segment/basic_exact_lds", "random", launch=[GENERAL])
_row("seg_random_exact_nolds", "segment/basic_exact_nolds", "random", NO_LDS, launch=[GENERAL])
_row("seg_random10k_exact", "segment/basic_exact_nolds", "random_10k", launch=[GENERAL])  # 640 KB of nodes: never LDS
_row("seg_random_slab", "segment/basic_slab_lds", "random", FASTC, launch=[GENERAL], kind="slab")
_row("seg_random_slab_nolds", "segment/basic_slab_nolds", "random", FASTC | NO_LDS, launch=[GENERAL], kind="slab")
_row("seg_random_ref", "segment/basic_ref_lds", "random", REF, launch=[GENERAL])
_row("seg_random_ref_nolds", "segment/basic_ref_nolds", "random", REF | NO_LDS, launch=[GENERAL])

# --- render_full_kernel
_row("pers_exact", "persistent/exact_lds", "cornell", launch=[PERSISTENT])
_row("pers_exact_nolds", "persistent/exact_nolds", "cornell", NO_LDS, launch=[PERSISTENT])
_row("pers_slab", "persistent/slab_lds", "simple_light", FASTC, launch=[PERSISTENT], kind="slab")
_row("pers_slab_nolds", "persistent/slab_nolds", "simple_light", FASTC | NO_LDS, launch=[PERSISTENT], kind="slab")
_row("pers_ref", "persistent/ref_lds", "cornell", REF, launch=[PERSISTENT])
_row("pers_ref_nolds", "persistent/ref_nolds", "cornell", REF | NO_LDS, launch=[PERSISTENT])

# --- the general walk kernel
_row("gwalk_cornell", ("gwalk/lds_lref", "gwalk/trim7"), "cornell")
_row("gwalk_cornell_lds", ("gwalk/lds", "gwalk/trim7"), "cornell", launch=[("HRT_GWALK_LREF", "0")])
_row("gwalk_cornell_buf", ("gwalk/buf", "gwalk/trim7"), "cornell", NO_LDS)
_row("gwalk_cornell_trim3", ("gwalk/lds_lref", "gwalk/trim3"), "cornell", launch=[("HRT_GWALK_TRIMP", "0")])
_row("gwalk_smoke_packet", ("gwalk/packet", "gwalk/trim2"), "cornell_smoke")
_row("gwalk_light_trim1", ("gwalk/lds_lref", "gwalk/trim1"), "simple_light")
_row("gwalk_instances_trim1", "gwalk/trim1", "instances")
_row("gwalk_final_one", ("gwalk/hyb_big_one", "gwalk/trim4"), "final")
_row("gwalk_final_big", ("gwalk/hyb_big", "gwalk/trim4"), "final", launch=[("HRT_GWALK_ONE", "0")])
_row("gwalk_final_hyb", ("gwalk/hyb", "gwalk/trim4"), "final", commit=[("HRT_GWALK_BIG", "0")])
_row("gwalk_final_buf", ("gwalk/buf", "gwalk/trim4"), "final", NO_LDS)
_row("gwalk_final_trim0", ("gwalk/hyb_big_one", "gwalk/trim0"), "final", launch=[("HRT_GWALK_TRIMP", "0")])

FAMILIES = ("sphere", "segment", "persistent", "gwalk")


def family(row):
    return row.entries[0].split("/")[0]


def lane_kernel(row):
    """tests/native/lane_sim.hip's lane of a "slab" row: 0 the sphere kernel's, 1 render_full_kernel's, 2 the segment
    kernel's (general scenes under the default plan: HRT_RENDER_FAST_CULL routes them to render_kernel)."""
    return {"sphere": 0, "persistent": 1, "segment": 2}[family(row)]
