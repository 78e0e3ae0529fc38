"""The walk hierarchy's builders restated, and the inputs they are held to.  Test infrastructure, like
tests/scenes.py; plain numpy, nothing of the library is imported.

The sphere kernel walks a hierarchy this project builds over the reference's leaf sequence:
scene.cpp walk_regroup / walk_regroup_dp on the host, build_walk.hip split_level on the device.  This file states
their rules a second time, from those comments, so that tests/test_hierarchy.py (host) and
tests/test_gpu_hierarchy.py (device) compare every builder, through hrt_debug_walk_regroup, with something that
shares no code with it.

A tree is the tuple hrt.walk_regroup returns: (leaf int32, end uint32, depth uint32, boxes (2n - 1, 6) float32)
over the 2n - 1 nodes in pre-order; leaf = -1 marks an inner node; a box is min xyz, max xyz.

  check_tree   the structure every builder must produce, whatever its cuts
  greedy       walk_regroup's cut rule (builder 0, and the device build)
  dp           walk_regroup_dp without a view, modes 1 and 2 (builders 1 and 2)
  greedy_sub   greedy down to ranges of at most dp_sub leaves, dp(., 1) on each (builder 3)
  tree_cost    the objective of a dp mode summed over a tree
  FAMILIES     the inputs: name -> (function of n giving (n, 6) float32 boxes, the sizes it is used at); ROWS and
               DP_ROWS list the (name, n) cases, boxes_of / greedy_of build each once for both test files
"""
import functools
import math

import numpy as np

F64 = np.float64


# ------------------------------------------------------------------------------------------------ validator
def check_tree(boxes, nodes):
    """Node 0 spans all leaves; a leaf node ends at self + 1 and holds its input box; an inner node over m leaves
    ends at self + 2m - 1, its children sit at self + 1 and self + 2 n_left one level down, and its box is the
    min / max union of its leaves' boxes bit for bit; the leaves appear once each, in order 0..n-1."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    leaf, end, depth, nb = nodes
    n = len(boxes)
    assert n >= 1 and len(leaf) == len(end) == len(depth) == len(nb) == 2 * n - 1
    assert np.array_equal(leaf[leaf >= 0], np.arange(n)), "leaves out of order"
    assert int((leaf < 0).sum()) == n - 1 and (leaf >= -1).all()
    bits, nbits = boxes.view(np.uint32), np.ascontiguousarray(nb, np.float32).view(np.uint32)
    todo = [(0, 0, n, 0)]  # node, first leaf, one past its last leaf, depth
    seen = 0
    while todo:
        self, lo, hi, d = todo.pop()
        seen += 1
        m = hi - lo
        assert int(depth[self]) == d, (self, int(depth[self]), d)
        assert int(end[self]) == self + 2 * m - 1, (self, int(end[self]), m)
        if m == 1:
            assert int(leaf[self]) == lo, (self, int(leaf[self]), lo)
            assert np.array_equal(nbits[self], bits[lo]), ("leaf box", self)
            continue
        assert int(leaf[self]) == -1, self
        union = np.concatenate([boxes[lo:hi, :3].min(axis=0), boxes[lo:hi, 3:].max(axis=0)])
        assert np.array_equal(nbits[self], union.view(np.uint32)), ("inner box", self, nb[self], union)
        left = self + 1
        span = int(end[left]) - left  # 2 n_left - 1
        assert span >= 1 and span % 2 == 1 and span < 2 * m - 1, (self, span)
        n_left = (span + 1) // 2
        todo.append((self + 2 * n_left, lo + n_left, hi, d + 1))
        todo.append((left, lo, lo + n_left, d + 1))
    assert seen == 2 * n - 1


# ------------------------------------------------------------------------------------------------ restatements
def half_area(mn, mx):
    """x y + y z + z x of the f64 extents; every product and sum is an f64 operation of its own, in this order."""
    e = np.asarray(mx, np.float32).astype(F64) - np.asarray(mn, np.float32).astype(F64)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    xy = x * y
    yz = y * z
    zx = z * x
    s = xy + yz
    return s + zx


def _pick(cost, dist):
    """The least index under the order (cost, dist, index)."""
    cand = np.flatnonzero(cost == cost.min())
    return int(cand[np.argmin(dist[cand])])  # argmin: the first of equal distances, the smaller index


def greedy_cut(boxes, lo, hi):
    """walk_regroup: the cut k (left = leaves lo..lo+k, right = the rest) of least
    half_area(prefix_k) (k + 1) + half_area(suffix_k+1) (n - 1 - k), ties to the cut nearest (n - 1) // 2, then to
    the smaller cut."""
    n = hi - lo
    mn, mx = boxes[lo:hi, :3], boxes[lo:hi, 3:]
    pre = half_area(np.minimum.accumulate(mn, axis=0), np.maximum.accumulate(mx, axis=0))
    suf = half_area(np.minimum.accumulate(mn[::-1], axis=0)[::-1], np.maximum.accumulate(mx[::-1], axis=0)[::-1])
    k = np.arange(n - 1)
    left = pre[:-1] * (k + 1).astype(F64)
    right = suf[1:] * (n - 1 - k).astype(F64)
    return _pick(left + right, np.abs(k - (n - 1) // 2))


class _Tree:
    def __init__(self, boxes):
        self.boxes = boxes
        self.leaf, self.end, self.depth, self.nb = [], [], [], []

    def push_leaf(self, i, depth):
        self.leaf.append(i)
        self.end.append(len(self.end) + 1)
        self.depth.append(depth)
        self.nb.append(self.boxes[i])

    def push_inner(self, lo, hi, depth):
        self.leaf.append(-1)
        self.end.append(len(self.end) + 2 * (hi - lo) - 1)
        self.depth.append(depth)
        self.nb.append(np.concatenate([self.boxes[lo:hi, :3].min(axis=0), self.boxes[lo:hi, 3:].max(axis=0)]))

    def done(self):
        return (np.array(self.leaf, np.int32), np.array(self.end, np.uint32), np.array(self.depth, np.uint32),
                np.array(self.nb, np.float32).reshape(-1, 6))


def _dp_cuts(boxes, lo, hi, mode):
    """walk_regroup_dp without a view over the leaves lo..hi-1: K[i][j], the first leaf of the right child of the
    range [i, j) (indices relative to lo).  cost(i, j) = min_k (cost(i, k) + cost(k, j)) + w(i, j), leaves cost 0,
    w = 2.0 x half area (mode 1) or half area x leaves (mode 2); ranges by increasing length; a tie goes to the k
    nearest i + len // 2, then to the smaller k.  All ranges of one length are evaluated together: the distance of
    the t-th candidate to the middle is the same in each."""
    n = hi - lo
    mn, mx = boxes[lo:hi, :3], boxes[lo:hi, 3:]
    A = np.zeros((n + 1, n + 1), F64)
    for i in range(n):
        A[i, i + 1:] = half_area(np.minimum.accumulate(mn[i:], axis=0), np.maximum.accumulate(mx[i:], axis=0))
    C = np.zeros((n + 1, n + 1), F64)
    K = np.zeros((n + 1, n + 1), np.int64)
    for ln in range(2, n + 1):
        i = np.arange(n - ln + 1)[:, None]
        t = np.arange(ln - 1)[None, :]            # candidate k = i + 1 + t
        c = C[i, i + 1 + t] + C[i + 1 + t, i + ln]
        best = c.min(axis=1)
        dist = np.abs(t + 1 - ln // 2)
        key = np.where(c == best[:, None], dist * ln + t, 2 * ln * ln)  # (distance, k) among the least costs
        tb = key.argmin(axis=1)
        ii = i[:, 0]
        a = A[ii, ii + ln]
        w = 2.0 * a if mode == 1 else a * F64(ln)
        C[ii, ii + ln] = best + w
        K[ii, ii + ln] = ii + 1 + tb
    return K


def _emit_dp(T, K, lo, n, depth0):
    todo = [(0, n, depth0)]
    while todo:
        a, b, d = todo.pop()
        if b - a == 1:
            T.push_leaf(lo + a, d)
            continue
        T.push_inner(lo + a, lo + b, d)
        k = int(K[a, b])
        todo.append((k, b, d + 1))
        todo.append((a, k, d + 1))


def dp(boxes, mode):
    """Builders 1 and 2 (meant for n <= 96; the work grows with n^3)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    assert mode in (1, 2)
    return greedy_sub(boxes, len(boxes), mode)


def greedy_sub(boxes, dp_sub, mode=1):
    """Builder 3: the greedy cuts down to ranges of at most dp_sub leaves (and at most 2048, the DP's limit), the
    DP of `mode` on each of those.  dp_sub = 0 is the greedy build."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    T = _Tree(boxes)
    todo = [(0, len(boxes), 0)]
    while todo:
        lo, hi, d = todo.pop()
        n = hi - lo
        if n == 1:
            T.push_leaf(lo, d)
            continue
        if n <= dp_sub and n <= 2048:
            _emit_dp(T, _dp_cuts(boxes, lo, hi, mode), lo, n, d)
            continue
        T.push_inner(lo, hi, d)
        k = 0 if n == 2 else greedy_cut(boxes, lo, hi)
        todo.append((lo + k + 1, hi, d + 1))  # right after left
        todo.append((lo, lo + k + 1, d + 1))
    return T.done()


def greedy(boxes):
    """Builders 0 and 4."""
    return greedy_sub(boxes, 0)


def tree_cost(nodes, mode):
    """The DP's objective summed over a tree's inner nodes (exactly rounded sum): mode 1: 2 x half area, mode 2:
    half area x leaves."""
    leaf, end, _, nb = nodes
    inner = np.flatnonzero(leaf < 0)
    a = half_area(nb[inner, :3], nb[inner, 3:])
    m = (end[inner].astype(np.int64) - inner + 1) // 2
    return math.fsum((2.0 * a if mode == 1 else a * m.astype(F64)).tolist())


def same_tree(a, b):
    """Node for node: leaf, end, depth, and the boxes' bits."""
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and \
        np.array_equal(np.ascontiguousarray(a[3], np.float32).view(np.uint32),
                       np.ascontiguousarray(b[3], np.float32).view(np.uint32))


def max_depth(nodes):
    return int(nodes[2].max())


# ------------------------------------------------------------------------------------------------ inputs
def _spheres(c, r):
    c = np.asarray(c, np.float32).reshape(-1, 3)
    r = np.asarray(r, np.float32).reshape(-1, 1)
    return np.hstack([c - r, c + r]).astype(np.float32) + np.float32(0.0)  # (+ 0: no negative zero)


def scattered(n, seed=5):
    """Spheres scattered over a square, as tests/test_gpu_build.py _big_scene places them: generic positions."""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(n)) * 1.2
    xs, zs = rng.uniform(-side / 2, side / 2, n), rng.uniform(-side / 2, side / 2, n)
    rs = rng.uniform(0.1, 0.4, n)
    return _spheres(np.stack([xs, rs, zs], axis=1), rs)


def identical_generic(n):
    """n copies of one box with edges 0.3, 0.7, 1.1 (f32): the costs A (k + 1) + A (n - 1 - k) differ by f64
    rounding only, so a re-associated or contracted sum on the device moves the cut."""
    mn = np.array([0.1, 0.2, 0.3], np.float32)
    mx = mn + np.array([0.3, 0.7, 1.1], np.float32)
    return np.tile(np.concatenate([mn, mx]), (n, 1))


def identical_exact(n):
    """n copies of a box with small integer corners: every cost is exactly equal; the cut is (n - 1) // 2."""
    return np.tile(np.array([1, 2, 3, 3, 5, 7], np.float32), (n, 1))


def lattice(n):
    """Unit boxes on an integer lattice in raster order: exact ties away from the middle."""
    s = max(1, math.ceil(round(n ** (1 / 3), 9)))
    i = np.arange(n)
    mn = np.stack([i % s, (i // s) % s, i // (s * s)], axis=1).astype(np.float32)
    return np.hstack([mn, mn + np.float32(1.0)])


def points_equal(n):
    """Zero-extent boxes, all the same point: every cost is 0."""
    p = np.array([0.5, 0.25, -1.5], np.float32)
    return np.tile(np.concatenate([p, p]), (n, 1))


def points_scattered(n, seed=11):
    """Zero-extent boxes at scattered points: the leaves have no area, the inner boxes little."""
    p = np.random.default_rng(seed).normal(0.0, 1.0, (n, 3)).astype(np.float32) + np.float32(0.0)
    return np.hstack([p, p])


def _cubes(half_edges):
    h = np.asarray(half_edges, np.float32)[:, None] * np.ones((1, 3), np.float32)
    return np.hstack([-h, h])


def nested_chain(n):
    """Cube i has edge 2^-i, centred at the origin, largest first (n <= 100: every edge a normal f32).  Every
    prefix box is cube 0 and the cost of cut k over m leaves is 3 ((k + 1) + (m - 1 - k) / 4^(k + 1)): it grows
    with k once 4^(k + 2) >= 3 m, so for m <= 100 the cut is k <= 3, the left child holds at most 4 leaves, and
    the tree is at least (n - 1) / 4 deep.  (Not a chain: the leaf count in the cost outweighs a quarter of the
    area from m = 6 up.  steep_chain is the chain.)"""
    assert n <= 100
    return _cubes(np.ldexp(np.float32(0.5), -np.arange(n)))


def nested_chain_reversed(n):
    """nested_chain, smallest first: the mirrored costs, the right child holds at most 4 leaves."""
    return nested_chain(n)[::-1].copy()


def steep_chain(n):
    """Cube i has edge 2^(91 - 3 i), centred at the origin, largest first (n <= 64: every edge a normal f32).  The
    area falls 64-fold per cube: over m <= 64 leaves cut 0 costs A (1 + (m - 1) / 64) < 2 A, every other cut at
    least (k + 1) A >= 2 A.  The cut is k = 0 at every level and the tree is a chain of depth n - 1: the device
    build runs n levels, and the pre-order numbering node + 2 (cut + 1) is used at each."""
    assert n <= 64
    return _cubes(np.ldexp(np.float32(1.0), 90 - 3 * np.arange(n)))


def steep_chain_reversed(n):
    """steep_chain, smallest first: every suffix box is the last cube, the cut is k = n - 2 at every level."""
    return steep_chain(n)[::-1].copy()


def line_sorted(n):
    """Equal spheres along x in increasing order."""
    c = np.zeros((n, 3), np.float32)
    c[:, 0] = np.arange(n, dtype=np.float32) * np.float32(1.25)
    return _spheres(c, np.full(n, 0.5, np.float32))


def two_clusters(n, seed=7):
    """A cluster of 3 leaves and one of n - 3 far away: a very unbalanced first cut (k = 2); the second range's
    length is n - 3."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (n, 3))
    c[3:, 0] += 1000.0
    return _spheres(c, np.full(n, 0.1))


SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 258, 511, 512, 513, 1000)
CHAIN_SIZES = (2, 3, 64, 100)
STEEP_SIZES = (2, 3, 33, 64)
DP_SIZES = (2, 3, 4, 5, 17, 64, 96)
BIG = 33000  # just above the size from which commit builds on the device by default (32768 leaves)

FAMILIES = {
    "scattered": (scattered, SIZES + (BIG,)),
    "identical_generic": (identical_generic, SIZES),
    "identical_exact": (identical_exact, SIZES),
    "lattice": (lattice, SIZES),
    "points_equal": (points_equal, SIZES),
    "points_scattered": (points_scattered, SIZES),
    "nested_chain": (nested_chain, CHAIN_SIZES),
    "nested_chain_reversed": (nested_chain_reversed, CHAIN_SIZES),
    "steep_chain": (steep_chain, STEEP_SIZES),
    "steep_chain_reversed": (steep_chain_reversed, STEEP_SIZES),
    "line_sorted": (line_sorted, SIZES),
    "two_clusters": (two_clusters, SIZES + (259, 260)),  # n - 3 = 256, 257: the second range at a chunk edge
}

ROWS = [(name, n) for name, (_, sizes) in FAMILIES.items() for n in sizes]
DP_ROWS = [(name, n) for name in FAMILIES for n in DP_SIZES if n <= max(FAMILIES[name][1])]


@functools.lru_cache(maxsize=None)
def boxes_of(name, n):
    b = np.ascontiguousarray(FAMILIES[name][0](n), np.float32)
    assert b.shape == (n, 6) and np.isfinite(b).all() and (b[:, :3] <= b[:, 3:]).all()
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def greedy_of(name, n):
    """greedy(boxes_of(name, n)), computed once for the host and the device tests."""
    t = greedy(boxes_of(name, n))
    for a in t:
        a.setflags(write=False)
    return t
