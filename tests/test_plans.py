"""tests/plans.py on the CPU: the checklist against the dispatch's source and against the table, and the inputs of the
approximate rows qualified on the host lanes and in the oracle (tests/test_gpu_plans.py renders the rows).

- The checklist is hand-written; the launchers' instantiations are read back from launch_sphere(), launch_any(),
  launch_g_mem() and launch_gwalk() and must be the checklist's, in both COUNT variants: an instantiation added to
  or taken out of the dispatch without its checklist entry (and so without a row) fails here.
- Every reachable entry has a row, every row names entries, sizes stay within the limits.
- Slab rows: the host lane of the row's kernel renders the row's inputs under CULL_SLAB and under CULL_EXACT; both
  equal the oracle (segments, L-inf <= 1e-3) and each other bit for bit, which is what lets the GPU test hold the
  slab frame to the default plan's bits.  The slab lane visits no more nodes than the verbatim reference test.
  (Mutants of lane.h box_hit<CULL_SLAB> tried on a scratch copy: one that rejects a box whose centre the ray
  passes fails the segment counts and the bits here; one that accepts every box fails the node-visit bound.)
- SAH rows: the oracle renders the scene under its BvhNode root and under a plain List of the same spheres; the
  pixels with equal bits are the unambiguous ones, at least 99% of the frame, their number the table's.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import hrt
import plans as P
from test_lane_sim import _build_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc")
TOL = 1e-3


# ------------------------------------------------------------------------------------ the dispatch, read back
def _body(path, signature):
    """The text of the function whose definition starts with `signature`, up to its closing brace at column 0."""
    src = open(os.path.join(CSRC, path)).read()
    a = src.index(signature)
    return src[a:src.index("\n}\n", a)]


_NAMES = {"G::CULL_EXACT": P.CULL_EXACT, "G::CULL_SLAB": P.CULL_SLAB, "G::CULL_REFERENCE": P.CULL_REFERENCE,
          "WM_LDS": P.WM_LDS, "WM_BUF": P.WM_BUF, "WM_HYB": P.WM_HYB, "TRIM_MEDIA": P.TRIM_MEDIA,
          "TRIM_HEAVY_TEX": P.TRIM_HEAVY_TEX, "TRIM_PROGRAMS": P.TRIM_PROGRAMS, "true": True, "false": False}


def _val(text):
    """A template argument: a number, a name of _NAMES or names joined with |; other names (COUNT, TRIM) stay text."""
    text = text.strip()
    if re.fullmatch(r"\d+", text):
        return int(text)
    parts = [t.strip() for t in text.split("|")]
    if not all(t in _NAMES for t in parts):
        return text
    if len(parts) == 1:
        return _NAMES[parts[0]]
    v = 0
    for t in parts:
        v |= _NAMES[t]
    return v


_ARITY = {"launch_basic": 8, "launch": 7, "launch_full": 3, "launch_g": 7, "launch_g_mem": 2}


def _calls(body, name, defaults):
    """The template argument lists of every `name<...>` in `body`, completed with the trailing `defaults`."""
    out = []
    for m in re.finditer(r"(?<![A-Za-z_])" + name + r"<([^<>]*)>", body):
        args = [_val(a) for a in m.group(1).split(",")]
        missing = _ARITY[name] - len(args)
        assert 0 <= missing <= len(defaults), m.group(0)
        out.append(tuple(args + list(defaults[len(defaults) - missing:])))
    assert out, name
    return out


def _txt(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    return str(v)


def _checklist_args(launcher, names):
    return {tuple(dict(e.args)[n] for n in names) for e in P.CHECKLIST.values()
            if e.launcher == launcher and set(dict(e.args)) == set(names)}


def _by_count(calls, count_at):
    """{COUNT value: the set of the other arguments as launch-record text}"""
    out = {}
    for c in calls:
        rest = tuple(_txt(v) for k, v in enumerate(c) if k != count_at)
        out.setdefault(c[count_at], set()).add(rest)
    return out


def test_sphere_dispatch_is_the_checklist():
    calls = _calls(_body("render_sphere.hip", "void launch_sphere("), "launch_basic", [False] * 5)
    got = _by_count(calls, 1)
    want = _checklist_args("launch_basic", ("CULL", "LDS", "HYB", "HEAVY", "SPLIT", "C16", "PACKET"))
    assert len(want) == 18
    assert got == {True: want, False: want}


def test_segment_and_persistent_dispatch_is_the_checklist():
    body = _body("render.hip", "void launch_any(")
    seg = _by_count(_calls(body, "launch", [0, 0]), 2)
    assert seg == {"COUNT": _checklist_args("launch", ("CULL", "FULL", "LDS", "FAST", "GW", "TRIM"))}
    full = _by_count(_calls(body, "launch_full", []), 1)
    assert full == {"COUNT": _checklist_args("launch_full", ("CULL", "LDS"))}


def test_gwalk_dispatch_is_the_checklist():
    shapes = _by_count(_calls(_body("render_general.hip", "void launch_g_mem("), "launch_g", [False] * 3), 0)
    # (WMEM, LREF, TRIM, BIG, ONE, PACKET) with TRIM the enclosing template's: the shapes, TRIM dropped
    got = {(a[0], a[1], a[3], a[4], a[5]) for a in shapes["COUNT"]}
    assert set(shapes) == {"COUNT"} and all(a[2] == "TRIM" for a in shapes["COUNT"])
    assert got == _checklist_args("launch_g", ("WMEM", "LREF", "BIG", "ONE", "PACKET"))
    trims = _by_count(_calls(_body("render_general.hip", "void launch_gwalk("), "launch_g_mem", []), 0)
    want = {(str(t),) for t in P.GWALK_TRIMS}
    assert trims == {True: want, False: want}
    assert _checklist_args("launch_g", ("TRIM",)) == want


# ------------------------------------------------------------------------------------ the table
def test_rows_and_checklist_agree():
    ids = [r.id for r in P.ROWS]
    assert len(ids) == len(set(ids))
    reached = set()
    for r in P.ROWS:
        assert r.entries and all(k in P.CHECKLIST for k in r.entries), r.id
        assert all(P.CHECKLIST[k].unreached is None for k in r.entries), r.id
        assert len({P.CHECKLIST[k].launcher for k in r.entries}) == 1, r.id
        reached.update(r.entries)
        assert r.scene in P.SCENES and r.kind in ("exact", "slab", "sah")
        w, h, spp = r.size
        cap = (48, 27, 4) if r.scene in ("random_10k", "final") else (64, 36, 8)
        assert w * h <= cap[0] * cap[1] and w <= 64 and h <= 36 and spp <= cap[2], r.id
        assert (r.kind == "slab") <= bool(r.flags & hrt.RENDER_FAST_CULL), r.id
        assert (r.kind == "sah") == (r.unambiguous is not None), r.id
        if r.kind == "sah":
            assert r.flags & P.SAH == P.SAH and r.scene in P.SPHERE_ONLY_DESC, r.id
        assert not r.flags & hrt.RENDER_COUNT_WORK  # the GPU test adds it to every row
    unreached = {k for k, e in P.CHECKLIST.items() if e.unreached is not None}
    assert reached == set(P.CHECKLIST) - unreached, sorted(set(P.CHECKLIST) - unreached - reached)
    # every exact sphere entry once more without the camera segment's leaf lists
    no_lists = {r.entries[0] for r in P.ROWS if P.NO_LISTS in r.launch}
    assert no_lists == set(P.SPHERE_EXACT)
    # a "sah" row is held to the slab frame of its scene: that scene has a "slab" row of its own
    for r in P.ROWS:
        if r.kind == "sah":
            assert any(q.kind == "slab" and (q.scene, q.size, q.seed) == (r.scene, r.size, r.seed) for q in P.ROWS), r.id
    print({f: sum(P.family(r) == f for r in P.ROWS) for f in P.FAMILIES}, len(P.ROWS), "rows,", len(P.CHECKLIST), "entries,",
          len(unreached), "unreached")


# ------------------------------------------------------------------------------------ host slab lanes
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build_sim(tmp_path_factory)


@pytest.fixture(scope="module")
def sources(earth):
    out = {}

    def get(name):
        if name not in out:
            out[name] = P.Source(name, earth)
        return out[name]

    return get


def _lane(L, src, size, seed, kernel, cull, shutter=None):
    w, h, spp = size
    s = src.build()
    cam = hrt.camera(*src.spec(s, shutter), w, h)
    blob, info = hrt.scene_blob(s)
    p = hrt.params(w, h, spp, 50, seed, src.background(s))
    out = np.zeros((h, w, 4), np.float32)
    cnt = np.zeros(8, np.uint64)
    rc = L.lane_sim_render(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), kernel, cull, 0, 0, w, h,
                           out.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out, int(cnt[0]), int(cnt[2])  # the frame, segments, node visits


SLAB_INPUTS = sorted({(r.scene, r.size, r.seed, P.lane_kernel(r)) for r in P.ROWS if r.kind == "slab"})


@pytest.mark.parametrize("scene,size,seed,kernel", SLAB_INPUTS)
def test_slab_lane_equals_exact_lane_on_the_rows_inputs(sim, sources, scene, size, seed, kernel):
    src = sources(scene)
    w, h, spp = size
    slab, n_slab, v_slab = _lane(sim, src, size, seed, kernel, P.CULL_SLAB)
    exact, n_exact, _ = _lane(sim, src, size, seed, kernel, P.CULL_EXACT)
    verbatim, n_ref, v_ref = _lane(sim, src, size, seed, kernel, P.CULL_REFERENCE)
    ref, cnt = src.oracle().render(w, h, spp, 50, seed=seed, camera=src.spec(src.build()))
    for name, img, n in (("slab", slab, n_slab), ("exact", exact, n_exact)):
        assert n == cnt["segments"], (name, n, cnt["segments"])
        assert np.isfinite(img).all()
        assert float(np.abs(img - ref).max()) <= TOL, name
    assert n_slab == n_exact == n_ref
    assert np.array_equal(slab.view(np.uint32), exact.view(np.uint32))
    assert np.array_equal(slab.view(np.uint32), verbatim.view(np.uint32))
    # The slab interval is the intersection of the per-axis intervals the reference tests one by one against
    # [t_min, t_max], so every box the reference test culls the slab test culls too, over the same node stream: the
    # slab lane never visits more nodes, and on a scene of many small boxes (a ray passes each axis of a box it
    # misses) it visits fewer.
    print(scene, kernel, "node visits: slab", v_slab, "reference", v_ref)
    assert v_slab <= v_ref
    if scene in ("random", "materials_spheres", "nested_checker"):
        assert v_slab < v_ref


# ------------------------------------------------------------------------------------ brute force for SAH
def unambiguous_mask(src, size, seed):
    """Pixels the oracle renders to the same bits under the scene's BvhNode root and under a List of its spheres."""
    w, h, spp = size
    r, _ = src.oracle().render(w, h, spp, 50, seed=seed, camera=src.desc.spec())
    b, _ = P.list_root(src.desc).to_oracle().render(w, h, spp, 50, seed=seed, camera=src.desc.spec())
    return np.all(r.view(np.uint32) == b.view(np.uint32), axis=2)


SAH_INPUTS = sorted({(r.scene, r.size, r.seed, r.unambiguous) for r in P.ROWS if r.kind == "sah"})


@pytest.mark.parametrize("scene,size,seed,count", SAH_INPUTS)
def test_sah_rows_inputs_are_unambiguous(sources, scene, size, seed, count):
    src = sources(scene)
    assert [c[0] for c in src.desc.calls].count("bvh") == 1  # spheres under one BvhNode root
    mask = unambiguous_mask(src, size, seed)
    print(scene, int(mask.sum()), "of", mask.size)
    assert int(mask.sum()) == count
    assert mask.sum() >= 0.99 * mask.size


def test_a_sah_scene_has_moving_spheres(sources):
    names = {r.scene for r in P.ROWS if r.kind == "sah"}
    assert any("moving_sphere" in [c[0] for c in sources(n).desc.calls] for n in names)


# ------------------------------------------------------------------------------------ the rows' scenes on the host
def _blob_info(make, commit=()):
    old = {k: os.environ.get(k) for k, _ in commit}
    os.environ.update(dict(commit))
    try:
        return hrt.scene_blob(make())[1]
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def test_streams_have_the_layouts_the_rows_name(sources):
    """What the exact sphere rows rely on, from the blob (no GPU): the placement a commit knob asks for, the node
    counts on either side of the packet walk's limit, and the smallest textured scene beyond the LDS budget."""
    import scenes
    import scenes_oracle as S

    info = {r.id: _blob_info(sources(r.scene).build, r.commit) for r in P.ROWS
            if P.family(r) == "sphere" and P.NO_LISTS not in r.launch}
    for rid, i in info.items():
        e = dict(P.CHECKLIST[next(r for r in P.ROWS if r.id == rid).entries[0]].args)
        if e["CULL"] != str(P.CULL_EXACT):
            continue
        assert (i.walk_c16 == 1) == (e["C16"] == "true"), rid
        assert (i.walk_half != 16) == (e["SPLIT"] == "true"), rid
        assert (i.walk_nodes <= 15) == (e["PACKET"] == "true"), rid  # layout.h SPHERE_PACKET_NODES
        if e["HYB"] == "true":
            assert i.walk_hot > 0 and i.walk_bytes > 77 * 1024, rid      # layout.h LDS_SCENE_MAX_BYTES
            assert i.walk_half == (8192 if e["SPLIT"] == "true" else 16), rid  # layout.h WALK_SPLIT_HALF_HYB
        elif e["LDS"] == "true":
            assert i.walk_hot == 0 and i.walk_bytes <= 77 * 1024, rid
    assert info["packet_heavy_images"].walk_nodes == 15
    below = _blob_info(lambda: S._recorded(scenes.big_textured, grid=22).to_hrt())
    assert below.walk_hot == 0 and below.walk_bytes == 160 * 487 - 32
    assert info["heavy_hyb"].walk_bytes == 160 * 532 - 32
