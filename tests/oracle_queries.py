"""What hrt_scene_intersect, hrt_scene_scatter and hrt_scene_step must answer, computed by the oracle alone
(oracle/oracle.cpp oracle_scene_hit and oracle_scatter: the recursive world->hit and Material::scatter) and hrt.h's
rules restated in Python.  Shared by tests/test_query_oracle.py, tests/test_scatter_oracle.py (the host simulators) and
tests/test_gpu_query_oracle.py, tests/test_gpu_scatter_oracle.py (the device).  Nothing here reads the library's blob:
scenes come from descriptions (tests/scenes_oracle.py), which both sides build from the same words, so ids compare.
Test infrastructure."""
import numpy as np

import hrt
import ray_families as RF
import scenes_oracle as SO
from oracle import oracle as O
from scene_desc import Desc

F = np.float32
U = np.uint32
SEED = 9            # the key of the media's draws
NONE = 0xFFFFFFFF
INF = F(np.inf)
FAMILIES = "ABCDEFG"


# ---------------------------------------------------------------- scenes
# name: (description builder, or None for the `motion` preset, which has no description form; the query's shutter)
SCENES = {"materials_spheres": (SO.materials_spheres, (0.0, 1.0)), "lit_spheres": (SO.lit_spheres, (0.0, 1.0)),
          **{"instances_%g" % a: ((lambda a=a: SO.instances(a)), (0.0, 1.0)) for a in SO.ANGLES},
          "media_nested": ((lambda: SO.media_nested(True)), (0.0, 1.0)), "media_flat": ((lambda: SO.media_nested(False)), (0.0, 1.0)),
          **{"roots_" + k: ((lambda k=k: SO.roots(k)), (0.0, 1.0)) for k in SO.ROOT_KINDS},
          **{"bvh_intervals_%g_%g" % sh: (SO.bvh_intervals, sh) for sh in SO.BVH_SHUTTERS},
          "cornell": (SO.preset_cornell, (0.0, 1.0)), "cornell_smoke": (SO.preset_cornell_smoke, (0.0, 1.0)),
          "motion": (None, (0.0, 1.0))}
MEDIA_SCENES = ("media_nested", "media_flat", "cornell_smoke")
MOTION_PRESET = 12  # oracle.cpp build_preset; hrt.preset("motion")


def _simple_light():
    rv, pm = np.zeros(768, F), np.zeros(768, U)
    O.load().oracle_perlin_tables(1, rv.ctypes.data, pm.ctypes.data)
    return SO.preset_simple_light(rv, pm)


# the scatter tests' scenes: together every material and texture kind, Isotropic included
SCATTER_SCENES = {"materials_spheres": SO.materials_spheres, "lit_spheres": SO.lit_spheres, "tex_sizes": (lambda: SO.tex_sizes(small=True)),
                  "nested_checker": SO.nested_checker, "cornell_smoke": SO.preset_cornell_smoke, "simple_light": _simple_light}


def without_media(desc):
    """The description with every ConstantMedium removed (and with it an instance or a list left without a child): the
    scene HRT_QUERY_SKIP_MEDIA traces.  Boundaries stay as unowned nodes, which neither builder reaches."""
    out = Desc(desc.background, desc.camera)
    dead, new_id = set(), {}
    for name, a, rid in desc.calls:
        if name not in ("sphere", "moving_sphere", "rect", "cuboid", "translate", "rotate", "constant_medium", "list", "bvh"):
            getattr(out, name)(*a)
            continue
        if name == "constant_medium":
            dead.add(rid)
        elif name == "translate":
            if a[0] in dead:
                dead.add(rid)
            else:
                new_id[rid] = out.translate(new_id[a[0]], a[1])
        elif name == "rotate":
            if a[1] in dead:
                dead.add(rid)
            else:
                new_id[rid] = out.rotate(a[0], new_id[a[1]], a[2])
        elif name in ("list", "bvh"):
            kids = [new_id[c] for c in a[0] if c not in dead]
            if not kids:
                dead.add(rid)
            else:
                new_id[rid] = out.list(kids) if name == "list" else out.bvh(kids, a[1], a[2])
        else:
            new_id[rid] = getattr(out, name)(*a)
    out.set_root(new_id[desc.root])
    return out


class Case:
    """One scene on the oracle's side: the description, the oracle's scene, its bounding box and its numbering."""

    def __init__(self, name, desc, shutter, preset=None):
        self.name, self.desc, self.shutter = name, desc, shutter
        self.oracle = desc.to_oracle() if desc is not None else O.OracleScene(preset, 1)
        self.bbox = self.oracle.bbox()
        self.prims = self.oracle.prims()
        self.media = self.oracle.media()
        self.has_ids = desc is not None
        self.n_mats = desc._n["mat"] + len(self.media) if desc is not None else None
        self.prim_of = contract_prim_index(self.prims)
        self.medium_rank = np.zeros(int(self.media.max()) + 1 if len(self.media) else 0, U)  # medium_id -> pre-order rank
        self.medium_rank[self.media] = np.arange(len(self.media), dtype=U)
        self.background = desc.background if desc is not None else tuple(float(c) for c in self.oracle.background)
        self._families = None
        self._clear = None

    def to_hrt(self, earth=None):
        return self.desc.to_hrt() if self.desc is not None else hrt.preset("motion", 1, earth)

    def clear(self):
        """The same description with its media removed, for HRT_QUERY_SKIP_MEDIA: (oracle scene, its prim -> this
        scene's prim), matched by the primitives' own parameters, which must be unique among those outside media."""
        if self._clear is None:
            osc = without_media(self.desc).to_oracle()
            key = lambda p: (int(p["kind"]), p["p"].tobytes())
            mine = {}
            for i, p in enumerate(self.prims):
                if p["boundary_of"] == NONE:
                    assert key(p) not in mine, "two primitives with the same parameters"
                    mine[key(p)] = self.prim_of[i]
            self._clear = (osc, np.array([mine[key(p)] for p in osc.prims()], U))
        return self._clear

    def families(self):
        """{letter: rays} and what the conditions need, computed once: `hits` {letter: the oracle's records}."""
        if self._families is None:
            self._families = make_families(self)
        return self._families


def contract_prim_index(prims):
    """hrt.h's `prim` from the oracle's pre-order index: the primitives outside every medium boundary keep their
    pre-order among themselves; the boundaries' primitives follow, boundary by boundary in the media's pre-order (a
    record never names one of them: a medium's record carries the medium)."""
    outside = np.flatnonzero(prims["boundary_of"] == NONE)
    inside = np.flatnonzero(prims["boundary_of"] != NONE)
    out = np.zeros(len(prims), U)
    out[outside] = np.arange(len(outside), dtype=U)
    out[inside] = len(outside) + np.arange(len(inside), dtype=U)
    return out


_cases = {}


def case(name):
    if name not in _cases:
        make, shutter = SCENES[name]
        _cases[name] = Case(name, make() if make is not None else None, shutter, MOTION_PRESET)
    return _cases[name]


def scatter_case(name):
    key = "scatter:" + name
    if key not in _cases:
        _cases[key] = Case(name, SCATTER_SCENES[name](), (0.0, 1.0))
    return _cases[key]


# ---------------------------------------------------------------- records
def to_oracle_rays(rays):
    r = np.zeros(len(rays), O.RAY)
    for f in ("origin", "direction", "time", "t_min", "t_max", "pixel", "sample", "segment"):
        r[f] = rays[f]
    return r


def to_oracle_hits(hits):
    h = np.zeros(len(hits), O.HIT)
    for f in ("t", "point", "normal", "u", "v", "material"):
        h[f] = hits[f]
    h["hit"] = (hits["flags"] & hrt.HIT_HIT) != 0
    h["front_face"] = (hits["flags"] & hrt.HIT_FRONT) != 0
    return h


def valid(rays, shutter):
    """hrt.h "Invalid ray", restated."""
    fin = np.isfinite(rays["origin"]).all(axis=1) & np.isfinite(rays["direction"]).all(axis=1) & np.isfinite(rays["time"]) & \
        np.isfinite(rays["t_min"])
    with np.errstate(invalid="ignore"):
        ok = fin & ~np.isnan(rays["t_max"]) & (rays["direction"] != 0).any(axis=1) & (rays["t_min"] < rays["t_max"])
        return ok & (rays["time"] >= F(shutter[0])) & (rays["time"] <= F(shutter[1]))


def oracle_hits(c, rays, seed=SEED, clear=False):
    """world.hit of every ray by the oracle (no validity rule), in the scene with its media removed if clear."""
    osc = c.clear()[0] if clear else c.oracle
    return osc.hit(to_oracle_rays(rays), seed)


def expected_hits(c, rays, seed=SEED, clear=False, raw=None):
    """The HIT_DTYPE records hrt.h's contract names for `rays`, from the oracle: an invalid ray's record, a miss's, or the
    oracle's hit with the ids.  Returns (records, nan) with nan (n, 12) bool: the float words that are NaN in the oracle's
    record, which the library must answer with a NaN of any sign and payload."""
    raw = oracle_hits(c, rays, seed, clear) if raw is None else raw
    n = len(rays)
    want = np.zeros(n, hrt.HIT_DTYPE)
    ok = valid(rays, c.shutter)
    hit = ok & (raw["hit"] != 0)
    miss = ok & ~hit
    want["prim"] = want["material"] = NONE
    want["flags"][~ok] = hrt.HIT_INVALID
    want["t"][miss] = rays["t_max"][miss]
    for f in ("t", "point", "normal", "u", "v"):
        want[f][hit] = raw[f][hit]
    medium = hit & (raw["medium"] != 0)
    want["flags"][hit] = hrt.HIT_HIT | np.where(raw["front_face"][hit] != 0, hrt.HIT_FRONT, 0) | np.where(medium[hit], hrt.HIT_MEDIUM, 0)
    prim_of = c.clear()[1] if clear else c.prim_of
    surface = hit & ~medium
    want["prim"][surface] = prim_of[raw["prim"][surface]]
    want["prim"][medium] = c.medium_rank[raw["medium_id"][medium]]  # the medium's place in the flattened scene
    want["material"][hit] = raw["material"][hit]
    w = words(want)
    nan = np.zeros((n, 12), bool)
    for col in (0, 4, 5, 6, 7, 8, 9, 10, 11):
        nan[:, col] = np.isnan(w[:, col].view(F))
    return want, nan


def words(a):
    return np.ascontiguousarray(a).view(U).reshape(-1, 12)


def differing(got, want, nan, ids=True):
    """Indices of the records whose 12 words are not the expected ones.  A word that is NaN in the oracle's record must be
    NaN in the library's; every other word must be equal.  ids=False (a preset, which has no description): the material
    word is left out."""
    got, want = words(got), words(want)
    same = got == want
    same |= nan & np.isnan(got.view(F))
    if not ids:
        same[:, 2] = True
    return np.flatnonzero(~same.all(axis=1))


def nan_equal(got, want):
    """Indices of the ray or path records that differ from `want`, a float word that is NaN in `want` being any NaN in
    `got` (the host's and the device's 0 / 0 differ in sign)."""
    g, w = words(got), words(want)
    same = (g == w) | (np.isnan(w.view(F)) & np.isnan(g.view(F)))
    return np.flatnonzero(~same.all(axis=1))


def report(c, rays, got, want, nan, what, ids=True, limit=6):
    bad = differing(got, want, nan, ids)
    if len(bad) == 0:
        return
    lines = ["%s: %d of %d records differ" % (what, len(bad), len(rays))]
    g, w = np.ascontiguousarray(got).view(hrt.HIT_DTYPE).reshape(-1), want
    for i in bad[:limit]:
        lines.append("  ray %d %r\n    got  %r\n    want %r" % (i, rays[i], g[i], w[i]))
    raise AssertionError("\n".join(lines))


# ---------------------------------------------------------------- the families of a scene
def make_families(c):
    sh, bbox = c.shutter, c.bbox
    seed = 1000 + sum(ord(ch) for ch in c.name)
    fam, hits = {}, {}
    ground = RF.ground_level(c.desc) if c.desc is not None else 0.0
    fam["A"] = RF.family_a(bbox, sh, seed, ground)
    hits["A"] = oracle_hits(c, fam["A"])
    fam["B"] = RF.family_b(bbox, sh, seed + 1, RF.snap_coords(c.desc) if c.desc is not None else None)
    fam["C"] = RF.family_c(bbox, sh, seed + 2)
    a_ok = valid(fam["A"], sh) & (hits["A"]["hit"] != 0)
    inside = RF.interior_points(c.desc) if c.desc is not None else None
    fam["D"] = RF.family_d(bbox, sh, seed + 3, hits["A"]["point"][a_ok], inside)
    fam["E"] = RF.family_e(bbox, sh, seed + 4)
    fam["F"], f_src = RF.family_f(fam["A"], a_ok, hits["A"]["t"])
    fam["G"], g_bad = RF.family_g(bbox, sh, seed + 6)
    for k in "BCDEFG":
        hits[k] = oracle_hits(c, fam[k])
    return {"rays": fam, "hits": hits, "f_src": f_src, "g_bad": g_bad}


def batch(c):
    """Every family of the scene in one array, and (letter, start, stop) of each."""
    f = c.families()["rays"]
    parts, at = [], 0
    for k in FAMILIES:
        parts.append((k, at, at + len(f[k])))
        at += len(f[k])
    return np.concatenate([f[k] for k in FAMILIES]), parts


def raw_batch(c):
    return np.concatenate([c.families()["hits"][k] for k in FAMILIES])


# ---------------------------------------------------------------- scatter: hrt.h rules 1 to 5 around Material::scatter
DONE, MISSED, ABSORBED, DEPTH, INVALID = hrt.PATH_DONE, hrt.PATH_MISSED, hrt.PATH_ABSORBED, hrt.PATH_DEPTH, hrt.PATH_INVALID
KNOWN_HIT = hrt.HIT_HIT | hrt.HIT_FRONT | hrt.HIT_MEDIUM | hrt.HIT_INVALID


def expected_scatter(c, rays, hits, paths, background):
    """(rays, paths) after hrt_scene_scatter, from OracleScene.scatter and the rules of hrt.h, one f32 rounding per
    operation in lane.h shade()'s order."""
    rays, paths = rays.copy(), paths.copy()
    bg = np.array(background, F)
    flags = hits["flags"]
    is_hit = (flags & hrt.HIT_HIT) != 0
    live = (paths["flags"] & DONE) == 0
    bad = ((flags & hrt.HIT_INVALID) != 0) | ((flags & ~U(KNOWN_HIT)) != 0) | np.where(is_hit, hits["material"] >= c.n_mats, flags != 0)
    bad |= (paths["rng"] == 0).all(axis=1)
    refuse = live & bad
    capped = live & ~bad & (paths["depth_left"] == 0)
    miss = live & ~bad & ~capped & ~is_hit
    step = live & ~bad & ~capped & is_hit
    paths["flags"][refuse] |= INVALID | DONE
    paths["flags"][capped] |= DEPTH | DONE
    paths["radiance"][miss] = paths["radiance"][miss] + paths["throughput"][miss] * bg
    paths["flags"][miss] |= MISSED | DONE
    idx = np.flatnonzero(step)
    sc = c.oracle.scatter(hits["material"][idx], to_oracle_rays(rays[idx]), to_oracle_hits(hits[idx]), paths["rng"][idx])
    paths["radiance"][idx] = paths["radiance"][idx] + paths["throughput"][idx] * sc["emitted"]
    paths["rng"][idx] = sc["rng"]
    on = sc["scattered"] != 0
    paths["flags"][idx[~on]] |= ABSORBED | DONE
    go = idx[on]
    paths["throughput"][go] = paths["throughput"][go] * sc["attenuation"][on]
    paths["depth_left"][go] -= 1
    rays["origin"][go], rays["direction"][go] = sc["origin"][on], sc["direction"][on]
    assert np.array_equal(sc["time"][on].view(U), rays["time"][go].view(U))  # the scattered ray keeps the time
    rays["segment"][go] += 1
    rays["t_max"][go] = INF
    paths["flags"][go[paths["depth_left"][go] == 0]] |= DEPTH | DONE
    ended = live & ((paths["flags"] & DONE) != 0)
    rays["t_max"][ended] = rays["t_min"][ended]
    return rays, paths


def random_paths(rng, n):
    """Paths with a random non-zero rng, a throughput in (0, 1]^3, a random radiance and depth_left from {1, 2, 50}."""
    p = np.zeros(n, hrt.PATH_DTYPE)
    p["rng"] = rng.integers(1, 1 << 32, (n, 4), dtype=np.uint64).astype(U)
    p["throughput"] = (1.0 - rng.uniform(0, 1, (n, 3))).astype(F)
    p["radiance"] = rng.uniform(0, 2, (n, 3)).astype(F)
    p["depth_left"] = np.choose(rng.integers(0, 3, n), [1, 2, 50])
    return p


def scatter_batch(c, seed=5):
    """The scatter tests' input on a scene: the oracle's hits of families A and D without the NaN records (hrt.h excludes
    them), misses among them as they fell, and the rule-2 refusals put over every 16th record."""
    f = c.families()
    rays = np.concatenate([f["rays"]["A"], f["rays"]["D"]])
    raw = np.concatenate([f["hits"]["A"], f["hits"]["D"]])
    hits, nan = expected_hits(c, rays, raw=raw)
    keep = ~nan.any(axis=1)
    rays, hits = rays[keep], hits[keep]
    n = len(rays)
    rng = np.random.default_rng(seed)
    paths = random_paths(rng, n)
    refusals = [("hit", "flags", hrt.HIT_INVALID), ("hit", "flags", hrt.HIT_HIT | 32), ("hit", "material", c.n_mats),
                ("hit", "material", 0xFFFFFF00), ("hit", "flags", hrt.HIT_FRONT), ("path", "rng", 0), ("path", "depth_left", 0),
                ("path", "flags", DONE | MISSED)]
    for k, i in enumerate(range(7, n, 16)):
        what, field, v = refusals[k % len(refusals)]
        if what == "hit":
            if field == "material":
                hits["flags"][i] |= hrt.HIT_HIT
            hits[field][i] = v
        else:
            paths[field][i] = v
    return rays, hits, paths


def chained(c, steps=2, seed=6):
    """`steps` rounds of oracle hit and oracle scatter on family A: (start rays, start paths, final rays, final paths,
    the hit of each path's last intersect and which paths had one, the valid rays walked)."""
    rays0 = c.families()["rays"]["A"]
    paths0 = random_paths(np.random.default_rng(seed), len(rays0))
    rays, paths = rays0.copy(), paths0.copy()
    last = np.zeros(len(rays), hrt.HIT_DTYPE)
    last_nan = np.zeros((len(rays), 12), bool)
    walked = 0
    for _ in range(steps):
        live = (paths["flags"] & DONE) == 0
        hits, nan = expected_hits(c, rays)
        walked += int((live & ((hits["flags"] & hrt.HIT_INVALID) == 0)).sum())
        last[live], last_nan[live] = hits[live], nan[live]
        rays, paths = expected_scatter(c, rays, hits, paths, c.background)
    stepped = (paths0["flags"] & DONE) == 0
    return rays0, paths0, rays, paths, last, last_nan, stepped, walked
