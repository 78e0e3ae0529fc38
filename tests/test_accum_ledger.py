"""The sample accumulator's bookkeeping (csrc/accum_ledger.h AccumLedger) against a model, on the host.

The ledger says which samples, in how many chunks, every tile of an accumulator holds: one shared record while the
tiles hold the same passes, a record per tile once a pass over a subset (hrt_accum_add_tiles) made them differ, and
the shared record again as soon as every tile holds the same ranges and the same chunk count.  tests/native/
accum_ledger.cpp puts its member functions behind a C interface.  The model keeps a set of sample indices and a chunk
count per tile and knows nothing of ranges or representations; after every operation, a refused one included, every
query of the ledger must equal the model's answer:
- uniform() is "all tiles hold the same set and the same chunk count";
- samples(t) and chunks(t) per tile, empty();
- while uniform, the shared range list is the set's maximal runs, sorted (adjacent ranges coalesce); while not, the
  ledger says so: uniform() is false and there is no shared list.
"""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADDABLE, BAD_RANGE, OVERLAP = 0, 1, 2
TOP = 1 << 32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ledger") / "libledger.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared",
                    "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", "accum_ledger.cpp"), "-o", so], check=True, env=tool_env())
    L = ctypes.CDLL(so)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    for name, res, args in [("ledger_new", vp, [u32]), ("ledger_free", None, [vp]), ("ledger_uniform", ctypes.c_int, [vp]),
                            ("ledger_empty", ctypes.c_int, [vp]), ("ledger_samples", u64, [vp, u32]),
                            ("ledger_chunks", u64, [vp, u32]), ("ledger_ranges", ctypes.c_int32, [vp, vp, u32]),
                            ("ledger_may_add", ctypes.c_int, [vp, u64, u64, vp, u32]),
                            ("ledger_record", None, [vp, u64, u64, u64, vp, u32]), ("ledger_merge", None, [vp, vp]),
                            ("ledger_clear", None, [vp])]:
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


def _idx(tiles):
    if tiles is None:
        return None, 0
    return (ctypes.c_uint32 * len(tiles))(*tiles), len(tiles)


def _runs(samples):
    """A set of integers as its maximal runs [begin, end), sorted."""
    out = []
    for s in sorted(samples):
        if out and out[-1][1] == s:
            out[-1][1] = s + 1
        else:
            out.append([s, s + 1])
    return [tuple(r) for r in out]


class Pair:
    """A ledger and its model, driven together; check() after every operation."""

    def __init__(self, lib, n_tiles):
        self.lib, self.nt = lib, n_tiles
        self.h = lib.ledger_new(n_tiles)
        self.sets = [set() for _ in range(n_tiles)]
        self.k = [0] * n_tiles
        self.refusals = set()
        self.check()

    def close(self):
        self.lib.ledger_free(self.h)

    def ranges(self):
        buf = (ctypes.c_uint64 * 256)()
        n = self.lib.ledger_ranges(self.h, buf, 128)
        return None if n < 0 else [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    def model_uniform(self):
        return all(s == self.sets[0] and k == self.k[0] for s, k in zip(self.sets, self.k))

    def check(self):
        got_uniform = bool(self.lib.ledger_uniform(self.h))
        assert got_uniform == self.model_uniform(), (self.sets, self.k)
        assert bool(self.lib.ledger_empty(self.h)) == (not any(self.sets))
        for t in range(self.nt):
            assert self.lib.ledger_samples(self.h, t) == len(self.sets[t]), t
            assert self.lib.ledger_chunks(self.h, t) == self.k[t], t
        assert self.ranges() == (_runs(self.sets[0]) if got_uniform else None)

    def add(self, begin, end, k, tiles=None):
        """A pass of k chunks over [begin, end) on `tiles` (None: all), if the ledger allows it.  Returns its answer."""
        on = range(self.nt) if tiles is None else tiles
        new = set(range(begin, end))
        want = BAD_RANGE if begin >= end or end > TOP else OVERLAP if any(self.sets[t] & new for t in on) else ADDABLE
        idx, n = _idx(tiles)
        got = self.lib.ledger_may_add(self.h, begin, end, idx, n)
        assert got == want, (begin, end, tiles)
        if got == ADDABLE:
            self.lib.ledger_record(self.h, begin, end, k, idx, n)
            for t in on:
                self.sets[t] |= new
                self.k[t] += k
        else:
            self.refusals.add(got)
        self.check()  # a refusal changed nothing
        return got

    def merge(self, src):
        """hrt_accum_merge's use: every range of src checked against this ledger first, then all of them taken."""
        assert self.model_uniform() and src.model_uniform()
        new = src.sets[0]
        idx, n = _idx(None)
        answers = [self.lib.ledger_may_add(self.h, b, e, idx, n) for b, e in src.ranges()]
        assert all(a in (ADDABLE, OVERLAP) for a in answers)
        assert any(a == OVERLAP for a in answers) == bool(self.sets[0] & new)
        if all(a == ADDABLE for a in answers):
            self.lib.ledger_merge(self.h, src.h)
            for t in range(self.nt):
                self.sets[t] |= new
                self.k[t] += src.k[0]
        else:
            self.refusals.add(OVERLAP)
        self.check()
        src.check()

    def clear(self):
        self.lib.ledger_clear(self.h)
        self.sets = [set() for _ in range(self.nt)]
        self.k = [0] * self.nt
        self.check()


@pytest.fixture
def pair(lib):
    made = []

    def make(n_tiles):
        made.append(Pair(lib, n_tiles))
        return made[-1]
    yield make
    for p in made:
        p.close()


def test_adjacent_ranges_coalesce_and_overlaps_are_refused(pair):
    p = pair(3)
    assert p.add(8, 16, 2) == ADDABLE
    assert p.add(16, 20, 1) == ADDABLE and p.ranges() == [(8, 20)]      # adjacent above
    assert p.add(4, 8, 1) == ADDABLE and p.ranges() == [(4, 20)]        # adjacent below
    assert p.add(24, 28, 1) == ADDABLE and p.ranges() == [(4, 20), (24, 28)]
    for begin, end in [(10, 12), (4, 20), (24, 28),   # inside, equal
                       (2, 6), (18, 22), (0, 30),     # straddling an end, a whole range
                       (19, 21), (3, 5), (23, 25), (27, 29)]:  # by one sample
        assert p.add(begin, end, 1) == OVERLAP, (begin, end)
    assert p.add(20, 24, 3) == ADDABLE and p.ranges() == [(4, 28)]      # the gap: three ranges become one
    assert [p.lib.ledger_chunks(p.h, t) for t in range(3)] == [8, 8, 8]
    # the same on a per-tile record
    assert p.add(28, 30, 1, [1]) == ADDABLE
    assert p.add(29, 31, 1, [0, 1]) == OVERLAP and p.add(29, 31, 1, [0, 2]) == ADDABLE
    assert p.add(30, 31, 1) == OVERLAP and p.add(31, 32, 1) == ADDABLE
    assert p.refusals == {OVERLAP}


def test_range_bounds(pair):
    """Up to 2^32 is a sample range, past it is not, and neither is an empty one.  The model here compares bounds."""
    p = pair(2)
    h, L = p.h, p.lib
    for begin, end in [(5, 5), (6, 5), (TOP, TOP), (TOP - 4, TOP + 1), (0, TOP + 1), (TOP, TOP + 1)]:
        assert L.ledger_may_add(h, begin, end, None, 0) == BAD_RANGE, (begin, end)
    assert L.ledger_may_add(h, TOP - 4, TOP, None, 0) == ADDABLE
    L.ledger_record(h, TOP - 4, TOP, 1, None, 0)
    assert L.ledger_may_add(h, TOP - 5, TOP - 3, None, 0) == OVERLAP
    assert L.ledger_may_add(h, TOP - 1, TOP, None, 0) == OVERLAP
    assert L.ledger_may_add(h, TOP - 4, TOP + 1, None, 0) == BAD_RANGE  # the bounds are looked at first
    assert L.ledger_may_add(h, TOP - 6, TOP - 4, (ctypes.c_uint32 * 1)(1), 1) == ADDABLE
    L.ledger_record(h, TOP - 6, TOP - 4, 1, (ctypes.c_uint32 * 1)(1), 1)
    assert not L.ledger_uniform(h)
    assert [L.ledger_samples(h, t) for t in range(2)] == [4, 6] and [L.ledger_chunks(h, t) for t in range(2)] == [1, 2]
    L.ledger_record(h, TOP - 6, TOP - 4, 1, (ctypes.c_uint32 * 1)(0), 1)
    assert L.ledger_uniform(h) and p.ranges() == [(TOP - 6, TOP)]
    assert L.ledger_may_add(h, 0, TOP - 6, None, 0) == ADDABLE
    L.ledger_record(h, 0, TOP - 6, 1, None, 0)
    assert p.ranges() == [(0, TOP)] and L.ledger_samples(h, 1) == TOP and L.ledger_chunks(h, 0) == 3


def test_subset_passes_split_and_rejoin(pair):
    p = pair(4)
    p.add(0, 8, 3)
    p.add(8, 12, 2, [1, 3])
    assert not p.model_uniform() and p.ranges() is None  # check() held uniform() to the model
    p.add(8, 12, 2)                                        # tiles 1 and 3 hold it: refused for the frame
    p.add(12, 16, 1)                                       # a whole-frame pass on per-tile records
    assert not p.model_uniform()
    p.add(8, 12, 2, [2])
    assert not p.model_uniform()
    p.add(8, 12, 2, [0])                                   # the last tile catches up: same ranges, same chunks
    assert p.model_uniform() and p.ranges() == [(0, 16)]
    assert p.lib.ledger_chunks(p.h, 3) == 6
    p.add(16, 20, 1)                                       # and the shared record goes on from there
    assert p.ranges() == [(0, 20)] and p.refusals == {OVERLAP}


def test_same_ranges_with_other_chunk_counts_stay_apart(pair):
    p = pair(2)
    p.add(0, 4, 1, [0])
    p.add(0, 4, 2, [1])                                    # the same samples in two chunks, not one
    assert p.sets[0] == p.sets[1] and not p.model_uniform()
    assert not p.lib.ledger_uniform(p.h)
    p.add(4, 6, 2, [0])
    p.add(4, 6, 1, [1])                                    # 3 chunks each, [0, 6) each
    assert p.lib.ledger_uniform(p.h) and p.ranges() == [(0, 6)]
    # the same sample count from different ranges is not the same passes either
    p.add(10, 12, 1, [0])
    p.add(20, 22, 1, [1])
    assert not p.lib.ledger_uniform(p.h)


@pytest.mark.parametrize("n_tiles", [1, 5, 12])
def test_subset_pass_over_every_tile_of_a_fresh_ledger(pair, n_tiles):
    p = pair(n_tiles)
    tiles = list(range(n_tiles))
    random.Random(n_tiles).shuffle(tiles)
    p.add(3, 9, 2, tiles)
    assert p.lib.ledger_uniform(p.h) and p.ranges() == [(3, 9)]
    p.add(0, 3, 1, tiles)
    assert p.ranges() == [(0, 9)]


def test_clear_from_both_representations(pair):
    p = pair(3)
    p.add(0, 4, 1)
    p.clear()
    p.add(2, 6, 1)                                         # what was held is gone: no overlap
    p.add(6, 8, 1, [2])
    assert not p.lib.ledger_uniform(p.h)
    p.clear()
    assert p.lib.ledger_uniform(p.h) and p.lib.ledger_empty(p.h)
    p.add(0, 8, 1, [1])
    assert p.refusals == set()


def test_merge_takes_ranges_and_chunks(pair):
    dst, src, other = pair(3), pair(3), pair(3)
    dst.add(0, 4, 2)
    src.add(4, 8, 1)
    src.add(10, 12, 2)
    dst.merge(src)
    assert dst.ranges() == [(0, 8), (10, 12)] and dst.lib.ledger_chunks(dst.h, 2) == 5
    other.add(11, 13, 1)
    dst.merge(other)                                       # overlaps by one sample: nothing changes
    assert dst.ranges() == [(0, 8), (10, 12)] and dst.refusals == {OVERLAP}
    dst.merge(pair(3))                                     # an empty one
    empty = pair(3)
    empty.merge(dst)
    assert empty.ranges() == dst.ranges() and empty.k == dst.k


@pytest.mark.parametrize("seed", range(12))
def test_random_sequences(pair, seed):
    rng = random.Random(seed)
    nt = seed + 1
    p = pair(nt)

    def some_range():
        begin = rng.randrange(0, 64)
        return begin, min(64, begin + rng.choice([0, 1, 1, 2, 3, 5, 8]))

    for _ in range(150):
        op = rng.random()
        begin, end = some_range()
        k = rng.randrange(1, 4)
        if op < 0.30:
            p.add(begin, end, k)
        elif op < 0.60:
            p.add(begin, end, k, rng.sample(range(nt), rng.randrange(1, nt + 1)))
        elif op < 0.80:  # the same pass to some tiles, then to the others: as uniform after it as before
            tiles = rng.sample(range(nt), rng.randrange(1, nt + 1))
            rest = [t for t in range(nt) if t not in tiles]
            if p.add(begin, end, k, tiles) == ADDABLE and rest:
                p.add(begin, end, k, rest)
        elif op < 0.92:
            if p.model_uniform():
                src = pair(nt)
                for _ in range(rng.randrange(0, 4)):
                    src.add(*some_range(), rng.randrange(1, 4))
                p.merge(src)
        else:
            p.clear()
    assert p.refusals == {BAD_RANGE, OVERLAP}
