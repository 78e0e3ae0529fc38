"""The host builders of the walk hierarchy (scene.cpp walk_regroup, walk_regroup_dp) against
their restatement in tests/hierarchy.py, through hrt_debug_walk_regroup, which runs the code commit runs on bare
leaf boxes.  tests/test_gpu_hierarchy.py holds the device build to the same table.

- Builder 0 (greedy) on every row of the input table: a valid tree (check_tree), and the restated cuts node for
  node (leaf, end, depth, box bits).  The inputs that are there for a reason are checked to do what they are for:
  the steep chains reach depth n - 1, the nested cubes a quarter of it, the identical boxes with integer corners cut at (n - 1) // 2 everywhere, the
  two clusters cut 3 | n - 3 first.
- Builders 1 and 2 (the DP over 2 x half area / half area x leaves) at n = 2, 3, 4, 5, 17, 64, 96 of every family:
  valid, the restated DP node for node, and a total cost not above the greedy tree's under the same objective.
- Builder 3 (greedy, the DP below dp_sub) with dp_sub = 0, 2, 16, 256 at n = 257 and 1000: valid, the restated
  greedy_sub; dp_sub = 0 is builder 0 and dp_sub >= n is builder 1.
- The entry's error cases write nothing.
- `random` under HRT_WALK_DP = 0, 1, 2, 3 and `random_10k` under 0 and 3 on the host lanes: the oracle's segment
  count, L-inf <= 1e-3, the same frame bits whatever the mode, and for `random` three different streams.
"""
import hashlib

import numpy as np
import pytest

import hierarchy as Hy
import hrt
from oracle import oracle as O
from test_lane_sim import CULL_EXACT, TOL, _build_sim, sim_render

GREEDY, DP_AREA, DP_LEAVES, GREEDY_SUB = hrt.WALK_GREEDY, hrt.WALK_DP_AREA, hrt.WALK_DP_LEAVES, hrt.WALK_GREEDY_SUB


def _left_counts(nodes):
    """(leaves, leaves of the left child) of every inner node."""
    leaf, end, _, _ = nodes
    inner = np.flatnonzero(leaf < 0)
    m = (end[inner].astype(np.int64) - inner + 1) // 2
    left = (end[inner + 1].astype(np.int64) - (inner + 1) + 1) // 2
    return m, left


@pytest.mark.parametrize("name,n", Hy.ROWS)
def test_greedy_builder_equals_restatement(name, n):
    boxes = Hy.boxes_of(name, n)
    t = hrt.walk_regroup(boxes, GREEDY)
    Hy.check_tree(boxes, t)
    ref = Hy.greedy_of(name, n)
    Hy.check_tree(boxes, ref)
    assert Hy.same_tree(t, ref)
    m, left = _left_counts(ref)
    if name == "steep_chain":
        assert Hy.max_depth(ref) == n - 1 and (left == 1).all()          # cut k = 0 at every level
    if name == "steep_chain_reversed":
        assert Hy.max_depth(ref) == n - 1 and (left == m - 1).all()      # cut k = n - 2 at every level
    if name == "nested_chain":
        assert (left <= 4).all() and 4 * Hy.max_depth(ref) >= n - 1
    if name == "nested_chain_reversed":
        assert (m - left <= 4).all() and 4 * Hy.max_depth(ref) >= n - 1
    if name in ("identical_exact", "points_equal"):
        assert (left == (m - 1) // 2 + 1).all()                          # every cost equal: the middle cut
    if name == "two_clusters" and n >= 5:
        assert left[0] == 3


def test_input_table_holds_the_ties_it_is_there_for():
    """lattice: at some range the least cost is reached by several cuts, two of them at the same distance from the
    middle (the third key decides) and the chosen one not at the middle; identical_generic: the costs of a range
    are not all equal (rounding separates them), so the cut depends on how they are rounded."""
    third = off_middle = 0
    for n in (255, 512, 1000):
        b = Hy.boxes_of("lattice", n)
        leaf, end, _, _ = Hy.greedy_of("lattice", n)
        for i in np.flatnonzero(leaf < 0):
            lo = int((leaf[:i] >= 0).sum())
            m = (int(end[i]) - int(i) + 1) // 2
            if m < 3:
                continue
            mn, mx = b[lo:lo + m, :3], b[lo:lo + m, 3:]
            pre = Hy.half_area(np.minimum.accumulate(mn, axis=0), np.maximum.accumulate(mx, axis=0))
            suf = Hy.half_area(np.minimum.accumulate(mn[::-1], axis=0)[::-1], np.maximum.accumulate(mx[::-1], axis=0)[::-1])
            k = np.arange(m - 1)
            c = pre[:-1] * (k + 1) + suf[1:] * (m - 1 - k)
            cand = np.flatnonzero(c == c.min())
            d = np.abs(cand - (m - 1) // 2)
            third += int((d == d.min()).sum() > 1)
            off_middle += int(d.min() >= 1 and len(cand) > 1)
    print(f"lattice: {third} ranges decided by the third key, {off_middle} tied ranges cut away from the middle")
    assert third > 0 and off_middle > 0
    b = Hy.boxes_of("identical_generic", 1000)
    a = Hy.half_area(b[0, :3], b[0, 3:])
    k = np.arange(999)
    c = a * (k + 1).astype(np.float64) + a * (999 - k).astype(np.float64)
    assert len(np.unique(c)) > 1


@pytest.mark.parametrize("mode", [DP_AREA, DP_LEAVES])
@pytest.mark.parametrize("name,n", Hy.DP_ROWS)
def test_dp_builders_equal_restatement(name, n, mode):
    boxes = Hy.boxes_of(name, n)
    t = hrt.walk_regroup(boxes, mode)
    Hy.check_tree(boxes, t)
    assert Hy.same_tree(t, Hy.dp(boxes, mode))
    g = hrt.walk_regroup(boxes, GREEDY)
    # the DP minimises the objective as it sums it in f64; an exactly rounded sum of the same <= n - 1 terms
    # differs from either tree's by at most n roundings of 2^-53 relative each
    assert Hy.tree_cost(t, mode) <= Hy.tree_cost(g, mode) * (1.0 + 2 * n * 2.0 ** -53)


SUB_ROWS = [(name, n) for name in Hy.FAMILIES for n in (Hy.FAMILIES[name][1][-2:] if "chain" in name else (257, 1000))]


@pytest.mark.parametrize("dp_sub", [0, 2, 16, 256])
@pytest.mark.parametrize("name,n", SUB_ROWS)
def test_greedy_with_dp_below_a_range_size_equals_restatement(name, n, dp_sub):
    boxes = Hy.boxes_of(name, n)
    t = hrt.walk_regroup(boxes, GREEDY_SUB, dp_sub)
    Hy.check_tree(boxes, t)
    assert Hy.same_tree(t, Hy.greedy_sub(boxes, dp_sub))
    if dp_sub == 0:
        assert Hy.same_tree(t, hrt.walk_regroup(boxes, GREEDY))
    if dp_sub >= n:
        assert Hy.same_tree(t, hrt.walk_regroup(boxes, DP_AREA))


@pytest.mark.parametrize("name,n", SUB_ROWS)
def test_dp_sub_of_at_least_n_is_the_dp(name, n):
    boxes = Hy.boxes_of(name, n)
    whole = hrt.walk_regroup(boxes, DP_AREA)
    for dp_sub in ((n, 2048, 0xFFFFFFFF) if n <= 257 else (n,)):  # (each DP over 1000 leaves takes most of a second)
        assert Hy.same_tree(hrt.walk_regroup(boxes, GREEDY_SUB, dp_sub), whole)
    if n <= 257:
        assert Hy.same_tree(whole, Hy.dp(boxes, 1))


def _pattern(n):
    m = 2 * max(n, 1) - 1 + 4
    return (np.full(m, -77, np.int32), np.full(m, 0xA5A5A5A5, np.uint32), np.full(m, 0x5A5A5A5A, np.uint32),
            np.full((m, 6), np.float32(-123.25), np.float32))


BAD = {
    "empty": (lambda: np.zeros((0, 6), np.float32), GREEDY),
    "nan": (lambda: _poke(Hy.boxes_of("scattered", 5), 2, 4, np.nan), GREEDY),
    "nan_min": (lambda: _poke(Hy.boxes_of("scattered", 5), 4, 0, np.nan), DP_AREA),
    "min_above_max": (lambda: _poke(Hy.boxes_of("lattice", 5), 3, 1, 9.0), GREEDY),
    "inf": (lambda: _poke(Hy.boxes_of("scattered", 5), 0, 5, np.inf), GREEDY_SUB),
    "minus_inf": (lambda: _poke(Hy.boxes_of("scattered", 5), 1, 2, -np.inf), DP_LEAVES),
    "dp_2049": (lambda: Hy.lattice(2049), DP_AREA),
    "dp_leaves_2049": (lambda: Hy.lattice(2049), DP_LEAVES),
    "builder_5": (lambda: Hy.boxes_of("lattice", 5), 5),
    "builder_negative": (lambda: Hy.boxes_of("lattice", 5), -1),
}


def _poke(b, i, j, v):
    b = b.copy()
    b[i, j] = v
    return b


@pytest.mark.parametrize("case", list(BAD))
def test_entry_rejects_bad_input_and_writes_nothing(case):
    make, builder = BAD[case]
    boxes = make()
    out = _pattern(len(boxes))
    with pytest.raises(hrt.HrtError) as e:
        hrt.walk_regroup(boxes, builder, 16, out=out)
    assert e.value.status == hrt.ERR_INVALID_ARG
    for got, want in zip(out, _pattern(len(boxes))):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    L = hrt.load()
    b = Hy.boxes_of("lattice", 5)
    assert L.hrt_debug_walk_regroup(0, None, 5, 0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                    out[3].ctypes.data) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_walk_regroup(0, b.ctypes.data, 5, 0, None, None, None, None) == hrt.ERR_INVALID_ARG


def test_entry_accepts_2048_leaves_for_the_dp_and_more_for_the_greedy_builders():
    b = Hy.lattice(2049)
    for builder in (GREEDY, GREEDY_SUB):
        Hy.check_tree(b, hrt.walk_regroup(b, builder, 16))
    b = Hy.identical_exact(2048)
    t = hrt.walk_regroup(b, DP_LEAVES)
    Hy.check_tree(b, t)


# ------------------------------------------------------------------------------------------------ rendered
RENDER = {"random": (40, 24, 8, ("0", "1", "2", "3")), "random_10k": (32, 18, 2, ("0", "3"))}
SEED = 3


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build_sim(tmp_path_factory)


@pytest.fixture(scope="module")
def lanes(sim, earth):
    """(scene, HRT_WALK_DP) -> (frame, counters, sha256 of the walk stream) on the sphere kernel's host lanes, and
    (scene, "oracle") -> the oracle's (frame, counters); each rendered once."""
    cache = {}

    def get(name, mode):
        w, h, spp, _ = RENDER[name]
        if (name, mode) in cache:
            return cache[(name, mode)]
        if mode == "oracle":
            out = O.OracleScene(hrt.PRESETS[name], 1, earth).render(w, h, spp, 50, seed=SEED, threads=8)
        else:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("HRT_WALK_DP", mode)
                mp.setenv("HRT_WALK_DP_SUB", "16")
                img, st = sim_render(sim, name, w, h, spp, 50, SEED, earth, kernel=0, cull=CULL_EXACT)
                buf, info = hrt.scene_blob(hrt.preset(name, 1, earth))
            assert info.walk_regrouped == 1 and info.walk_general == 0
            out = (img, st, hashlib.sha256(buf.raw[info.off_walk:info.off_walk + info.walk_bytes]).hexdigest())
        cache[(name, mode)] = out
        return out

    return get


@pytest.mark.parametrize("name,mode", [(name, m) for name, (_, _, _, modes) in RENDER.items() for m in modes])
def test_every_host_builders_stream_renders_the_oracles_frame(lanes, name, mode):
    """Any hierarchy over the reference leaf order renders the same image: each mode's stream on the host lanes has
    the oracle's segment count and L-inf <= 1e-3, and the frame is the one the scene's first mode renders, bit for
    bit."""
    ref, cnt = lanes(name, "oracle")
    img, st, stream = lanes(name, mode)
    linf = float(np.abs(img - ref).max())
    print(f"{name} HRT_WALK_DP={mode}: segments {st['segments']} (oracle {cnt['segments']}), L-inf {linf:.3g}, "
          f"node visits {st['nodes']}, stream {stream[:12]}")
    assert st["segments"] == cnt["segments"]
    assert np.isfinite(img).all()
    assert linf <= TOL
    first = lanes(name, RENDER[name][3][0])
    assert np.array_equal(img.view(np.uint32), first[0].view(np.uint32))
    assert st["segments"] == first[1]["segments"] and st["prims"] == first[1]["prims"]


def test_walk_dp_modes_select_different_streams(lanes):
    """`random` under HRT_WALK_DP = 0, 1, 2: three streams, or the knob selected nothing."""
    assert len({lanes("random", m)[2] for m in ("0", "1", "2")}) == 3
    assert lanes("random_10k", "0")[2] != lanes("random_10k", "3")[2]
