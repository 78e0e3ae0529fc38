"""Ray families for the query tests that hold hrt_scene_intersect to the oracle (tests/test_query_oracle.py and
tests/test_gpu_query_oracle.py): the rays a render never produces.  Plain numpy, seeded.  Test infrastructure.

Each family is a function of a scene's ORACLE bounding box (OracleScene.bbox()), a shutter (time0, time1) and a seed, and
returns hrt.RAY_DTYPE records with random pixel, sample and segment.  Scene coordinates come from the scene DESCRIPTION
(tests/scene_desc.py Desc), never from the library's flattened blob: `snap_coords` for family B, `interior_points` for
family D.  A scene without a description (a preset) passes none.

The box is clipped to [CLIP_LO, CLIP_HI] per coordinate, as tests/test_gpu_query.py random_rays clips it: the ground
spheres of radius 1000 and media_nested's far object frame would otherwise put every origin inside or far off the scene.
"""
import numpy as np

import hrt

F = np.float32
N = 1000
CLIP_LO, CLIP_HI = -20.0, 600.0
INF = np.inf
T_MINS = (0.001, 0.0, -1.0, None)  # None: 0.5 / the direction's length
# Family E: its distances in scene diagonals and their cumulative shares.  The issue names 1e3, 1e4 and 1e6 diagonals.
# Measured on the oracle alone, rays from there cannot meet its own conditions: the reference's sphere roots cancel
# (half_b^2 - a c at |oc| ~ 1e4) so a small sphere's (at(root) - center) / radius is far from unit length and sphere.rs's
# acos gives a NaN v on about nine hits in ten (instances: 349 of 388 at 1e3 diagonals), and a rect's 0.0002-thick box is
# thinner than an ulp of t there, so aabb.rs culls every wall (cornell_smoke: no surface hit from 1e4 diagonals on).  So
# most of the family starts 10, 30 and 100 diagonals away, where the records are clean, and the three named distances
# keep four rays in a thousand each: their records are compared like any other (a NaN must be a NaN, every other word
# equal) but stay within the 2% of NaN records a family may hold.
SNAP_EVERY = 8  # family B
FAR_DISTANCES = (10.0, 30.0, 100.0, 1e3, 1e4, 1e6)
FAR_SHARES = (0.45, 0.90, 0.988, 0.992, 0.996)


def _box(bbox):
    b = np.asarray(bbox, np.float64)
    mn, mx = np.clip(b[:3], CLIP_LO, CLIP_HI), np.clip(b[3:], CLIP_LO, CLIP_HI)
    return mn, mx, float(np.linalg.norm(mx - mn))


def _records(rng, o, d, time, t_min, t_max):
    n = len(o)
    r = np.zeros(n, hrt.RAY_DTYPE)
    r["origin"], r["direction"] = np.asarray(o, F), np.asarray(d, F)
    r["time"], r["t_min"], r["t_max"] = np.asarray(time, F), np.asarray(t_min, F), np.asarray(t_max, F)
    r["pixel"], r["sample"], r["segment"] = rng.integers(0, 1 << 20, n), rng.integers(0, 64, n), rng.integers(0, 8, n)
    return r


def _times(rng, shutter, n):
    """Across the shutter, a tenth each exactly time0 and time1."""
    t = rng.uniform(shutter[0], shutter[1], n)
    pick = rng.uniform(size=n)
    return np.where(pick < 0.1, shutter[0], np.where(pick < 0.2, shutter[1], t))


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _origins(rng, mn, mx, n):
    grow = 0.1 * (mx - mn)
    return rng.uniform(mn - grow, mx + grow, (n, 3))


def family_a(bbox, shutter, seed, ground=None, n=2 * N):
    """Incoherent: origins in the box grown by a tenth, normal directions with lengths log-uniform in [1e-3, 1e3], t_min
    from {0.001, 0, -1, 0.5 / length}, a fifth with a finite t_max inside the scene's extent (in units of the direction's
    length), times across the shutter with exactly time0 and time1 among them.  ground: the y below which a scene's
    ground sphere lies (the description's), or None; two thirds of the origins are then lifted above it, since a ray
    that starts inside a sphere of radius 1000 can only hit it.  Twice the other families' size: with 1000 rays
    media_nested's small media scatter 19 and 15 of them, under the 20 the tests ask for."""
    rng = np.random.default_rng(seed)
    mn, mx, diag = _box(bbox)
    o = _origins(rng, mn, mx, n)
    if ground is not None:
        lift = rng.uniform(size=n) < 2.0 / 3.0
        o[lift, 1] = ground + np.abs(o[lift, 1] - ground)
    length = 10.0 ** rng.uniform(-3, 3, n)
    d = _unit(rng, n) * length[:, None]
    pick = rng.integers(0, len(T_MINS), n)
    t_min = np.choose(pick, [0.001, 0.0, -1.0, 0.5 / length])
    t_max = np.where(rng.uniform(size=n) < 0.2, t_min + rng.uniform(0.05, 0.5, n) * diag / length, INF)
    return _records(rng, o, d, _times(rng, shutter, n), t_min, t_max)


def family_b(bbox, shutter, seed, coords=None, n=N):
    """Axis-parallel: one or two direction components exactly +0 or -0.  One origin in SNAP_EVERY has the coordinate of
    each zero component snapped to a coordinate of the scene's primitives (coords: three arrays, one per axis, from
    snap_coords), so aabb.rs's 0 * inf arises and rays lie in a rect's plane; the others are random.  (With every second
    origin snapped, as first planned, 74 of cornell's 1000 records are NaN: more than the 2% a family may hold.)"""
    rng = np.random.default_rng(seed)
    mn, mx, _ = _box(bbox)
    o = _origins(rng, mn, mx, n).astype(F)
    d = (_unit(rng, n) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    for i in range(n):
        axes = rng.permutation(3)[:rng.integers(1, 3)]
        for a in axes:
            d[i, a] = F(0.0) if rng.uniform() < 0.5 else F(-0.0)
        if i % SNAP_EVERY == 1 and coords is not None:
            for a in axes:
                if len(coords[a]):
                    o[i, a] = coords[a][rng.integers(0, len(coords[a]))]
    return _records(rng, o, d, _times(rng, shutter, n), np.full(n, 0.001), np.full(n, INF))


def family_c(bbox, shutter, seed, n=N):
    """Extreme components: one component denormal (+-1e-42) beside ordinary ones, or the whole direction of length 1e-18,
    or of length 1e15, one in twenty of those 1e18.  (At 1e18 sphere.rs's half_b^2 - a c is inf - inf against a ground
    sphere 1000 units away: where no box culls it first - roots("list") - every such ray is a NaN hit, 347 records of
    1000 with a third of the family at 1e18.  1e15 is the largest power of 1000 that stays finite there.)"""
    rng = np.random.default_rng(seed)
    mn, mx, _ = _box(bbox)
    o = _origins(rng, mn, mx, n)
    d = _unit(rng, n).astype(F)
    kind = rng.integers(0, 3, n)
    for i in range(n):
        if kind[i] == 0:
            d[i, rng.integers(0, 3)] = F(1e-42) if rng.uniform() < 0.5 else F(-1e-42)
        else:
            d[i] = d[i] * (F(1e-18) if kind[i] == 1 else (F(1e18) if rng.integers(0, 20) == 0 else F(1e15)))
    return _records(rng, o, d, _times(rng, shutter, n), np.full(n, 0.001), np.full(n, INF))


def family_d(bbox, shutter, seed, points, inside=None, n=N):
    """From surfaces and insides: half the origins are `points` (family A's oracle hit points), half `inside` (sphere
    centres, points inside and on the faces of every box and medium boundary: interior_points; a preset has none and
    takes `points` alone), drawn at random; directions over the whole sphere, of ordinary lengths; t_min from {0, 0.001}."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(points, F).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)]
    o = pts[rng.integers(0, len(pts), n)] if len(pts) else _origins(rng, *_box(bbox)[:2], n).astype(F)
    if inside is not None and len(inside):
        ins = np.asarray(inside, F).reshape(-1, 3)
        half = rng.uniform(size=n) < 0.5
        o[half] = ins[rng.integers(0, len(ins), int(half.sum()))]
    d = _unit(rng, n) * rng.uniform(0.5, 2.0, (n, 1))
    t_min = np.where(rng.uniform(size=n) < 0.5, 0.0, 0.001)
    return _records(rng, o, d, _times(rng, shutter, n), t_min, np.full(n, INF))


def family_e(bbox, shutter, seed, n=N):
    """Far: origins FAR_DISTANCES scene diagonals away (up to 1e3, 1e4 and 1e6), aimed at points inside the box and, for a
    third, at points outside it (a thousandth of its size to its whole size beyond a face, log-uniform); directions of
    length 1 or of the whole distance."""
    rng = np.random.default_rng(seed)
    mn, mx, diag = _box(bbox)
    size = mx - mn
    target = rng.uniform(mn, mx, (n, 3))
    out = rng.uniform(size=n) < 1.0 / 3.0
    axis = rng.integers(0, 3, n)
    side = rng.integers(0, 2, n)
    for i in np.flatnonzero(out):
        a = axis[i]
        off = 10.0 ** rng.uniform(-3, 0) * size[a]
        target[i, a] = (mx[a] + off) if side[i] else (mn[a] - off)
    dist = np.array(FAR_DISTANCES)[np.searchsorted(FAR_SHARES, rng.uniform(size=n))] * diag
    o = (target - _unit(rng, n) * dist[:, None]).astype(F)
    d = target - o.astype(np.float64)
    unit = rng.uniform(size=n) < 0.5
    d[unit] /= np.linalg.norm(d[unit], axis=1, keepdims=True)
    return _records(rng, o, d, _times(rng, shutter, n), np.full(n, 0.001), np.full(n, INF))


def family_f(rays_a, hit_a, t_a):
    """Interval ends: for each oracle hit of family A (hit_a: bool, t_a: the oracle's t) with a finite t above the ray's
    t_min, four copies of the ray, in this order: t_max = t, t_max = the float just below t (nextafter(t, 0) for a positive
    t; t_min = -1 gives negative ones too), t_min = t, t_min = nextafter(t, inf).  Only where the two neighbours of t
    still lie inside (t_min, t_max): otherwise a copy would be an invalid ray, which family G covers."""
    t = np.asarray(t_a, F)
    below = np.nextafter(t, F(-INF))
    ok = np.asarray(hit_a, bool) & np.isfinite(t) & (rays_a["t_min"] < below) & (np.nextafter(t, F(INF)) < rays_a["t_max"])
    idx = np.flatnonzero(ok)
    out = np.repeat(rays_a[idx], 4)
    out["t_max"][0::4] = t[idx]
    out["t_max"][1::4] = below[idx]
    out["t_min"][2::4] = t[idx]
    out["t_min"][3::4] = np.nextafter(t[idx], F(INF))
    return out, idx


def invalid_table():
    """tests/test_query_host.py test_invalid_rays' cases: the field changes that make a ray invalid under shutter (0, 1)
    shifted to the family's own."""
    nan, inf = float("nan"), float("inf")
    return [dict(origin=(nan, 0, 5)), dict(origin=(0, inf, 5)), dict(direction=(0, nan, -1)), dict(direction=(0, 0, -inf)),
            dict(time=nan), dict(time=inf), dict(t_min=nan), dict(t_min=-inf), dict(t_max=nan), dict(direction=(0, 0, 0)),
            dict(t_min=2.0, t_max=2.0), dict(t_min=3.0, t_max=1.0), dict(time="before"), dict(time="after"),
            dict(direction=(0, 0, -0.0))]


def family_g(bbox, shutter, seed, n=N):
    """Invalid rays scattered among valid ones: every third ray of a family-A batch takes one case of invalid_table, so a
    64-lane wave holds both kinds."""
    rng = np.random.default_rng(seed)
    rays = family_a(bbox, shutter, seed + 1, None, n)
    rays["t_max"] = INF
    rays["t_min"] = 0.001
    table = invalid_table()
    span = shutter[1] - shutter[0] + 1.0
    for k, i in enumerate(range(0, n, 3)):
        for field, v in table[k % len(table)].items():
            if v == "before":
                v = shutter[0] - 0.25 * span
            elif v == "after":
                v = shutter[1] + 0.5 * span
            rays[field][i] = v
    return rays, np.arange(0, n, 3)


# ---------------------------------------------------------------- coordinates of a description
def _rot(axis, p, deg):
    """rotation.rs's object-to-world turn of a point (f64: these are only origins)."""
    a, b = ((1, 2), (2, 0), (0, 1))[axis]
    th = np.radians(deg)
    q = np.array(p, np.float64)
    q[a] = np.cos(th) * p[a] - np.sin(th) * p[b]
    q[b] = np.sin(th) * p[a] + np.cos(th) * p[b]
    return q


def _parents(desc):
    """node id -> (call name, args) of the node that owns it."""
    up = {}
    for name, a, rid in desc.calls:
        if name in ("translate", "constant_medium"):
            up[a[0]] = (name, a, rid)
        elif name == "rotate":
            up[a[1]] = (name, a, rid)
        elif name in ("list", "bvh"):
            for c in a[0]:
                up[c] = (name, a, rid)
    return up


def _to_world(desc, up, rid, p):
    p = np.array(p, np.float64)
    while rid in up:
        name, a, parent = up[rid]
        if name == "translate":
            p = p + np.array(a[1], np.float64)
        elif name == "rotate":
            p = _rot(a[0], p, a[2])
        rid = parent
    return p


def interior_points(desc):
    """World-space points of a description: every sphere's centre (a moving sphere's at its start), and for every cuboid
    (box or medium boundary) its centre, a point near a corner inside it and the centre of each face."""
    up = _parents(desc)
    pts = []
    for name, a, rid in desc.calls:
        if name == "sphere":
            pts.append(_to_world(desc, up, rid, a[0]))
        elif name == "moving_sphere":
            pts.append(_to_world(desc, up, rid, a[0]))
        elif name == "cuboid":
            p0, p1 = np.array(a[0], np.float64), np.array(a[1], np.float64)
            mid = 0.5 * (p0 + p1)
            local = [mid, p0 + 0.05 * (p1 - p0)]
            for ax in range(3):
                for v in (p0[ax], p1[ax]):
                    q = mid.copy()
                    q[ax] = v
                    local.append(q)
            pts += [_to_world(desc, up, rid, q) for q in local]
    return np.array(pts, F).reshape(-1, 3)


def snap_coords(desc):
    """Per axis, the f32 coordinates of a description's primitives in their own frames: sphere centres and the faces of
    their boxes (c -+ r), rect planes k, the faces of a rect's box (k -+ 0.0001, rect.rs) and its extents, cuboid
    corners."""
    c = [[], [], []]
    for name, a, _ in desc.calls:
        if name in ("sphere", "moving_sphere"):
            r = F(a[1] if name == "sphere" else a[4])
            for ctr in ([a[0]] if name == "sphere" else [a[0], a[1]]):
                for ax in range(3):
                    x = F(ctr[ax])
                    c[ax] += [x, F(x - r), F(x + r)]
        elif name == "rect":
            plane, a0, a1, b0, b1, k = a[0], *[F(v) for v in a[1:6]]
            k_ax, a_ax, b_ax = ((2, 0, 1), (0, 1, 2), (1, 2, 0))[plane]
            c[k_ax] += [k, F(k - F(0.0001)), F(k + F(0.0001))]
            c[a_ax] += [a0, a1]
            c[b_ax] += [b0, b1]
        elif name == "cuboid":
            for ax in range(3):
                c[ax] += [F(a[0][ax]), F(a[1][ax])]
    return [np.unique(np.array(v, F)) for v in c]


def ground_level(desc):
    """The top of a description's ground sphere (radius >= 100), or None."""
    for name, a, _ in desc.calls:
        if name == "sphere" and a[1] >= 100.0:
            return float(a[0][1] + a[1])
    return None
