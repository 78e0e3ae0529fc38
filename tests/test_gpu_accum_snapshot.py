"""Snapshots and per-tile merges of the sample accumulator on the GPU (hrt_accum_snapshot / _restore / _snapshot_info,
hrt_accum_merge_tiles, Accumulator.refine(resume=True)): the restore contract and the merge contract of
include/hrt/hrt.h, bit for bit.

Inputs are tests/test_gpu_accum_noise.py's: A = `random` (scene seed 1, render seed 7) at 64x36 in 16-px tiles (12 tiles,
the top row 4 px high: 64-px tiles below one block); B = `cornell` at 32x32 in 16-px tiles (4 tiles)."""
import ctypes
import struct

import numpy as np
import pytest

import hrt

SEED = 7
FLOOR = 0.05
F = np.float32
INPUTS = {"A": ("random", 64, 36), "B": ("cornell", 32, 32)}
SUBSET = {"A": [0, 5, 11], "B": [0, 3]}   # the tiles of the state's subset pass


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits(x):
    """A float's f32 bit pattern."""
    return int(u32(F(x))[0])


_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    def get(name):
        if name not in _scenes:
            s = hrt.preset(name, 1, earth)
            s.commit()
            _scenes[name] = s
        return _scenes[name]

    yield get
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def setup(s, w, h, spp, offset=0, seed=SEED):
    cam = hrt.preset_camera(s.info, w, h)
    return cam, hrt.params(w, h, spp, 50, seed, tuple(s.info.background), sample_offset=offset)


def fresh(s, w, h, noise=True, features=False, tile=16):
    return hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, tile), noise=noise, features=features)


def add(a, s, begin, end, tiles=None, seed=SEED):
    a.add(*setup(s, a.width, a.height, end - begin, offset=begin, seed=seed), tiles=tiles)


def tile_spans(a):
    out, off = [], 0
    for _, _, tw, th in a.tiles:
        out.append((off, tw * th))
        off += tw * th
    return out


def state(s, inp, noise, features):
    """Passes (0, 40), (40, 80), then (80, 120) on a subset of the tiles, and 8 feature samples."""
    _, w, h = INPUTS[inp]
    a = fresh(s, w, h, noise, features)
    add(a, s, 0, 40)
    add(a, s, 40, 80)
    add(a, s, 80, 120, tiles=SUBSET[inp])
    if features:
        a.add_features(*setup(s, w, h, 8))
    return a


def answers(a):
    """Everything an accumulator answers, as name -> uint32 array (or a list of integers)."""
    out = {"tile_samples": a.tile_samples, "f32": u32(a.resolve()), "rgba8": a.resolve("rgba8").copy()}
    if a.has_noise:
        rec, err = a.noise(FLOOR, error_map=True)
        out["m2"] = u32(a.moments())
        out["records"] = [(bits(r.mean), bits(r.max), r.samples, r.chunks) for r in rec]
        out["error_map"] = u32(err)
        out["filtered"] = u32(a.resolve(denoise=True))
    if a.has_features:
        fa, fn = a.debug_features()
        out["fa"], out["fn"], out["feature_samples"] = u32(fa), u32(fn), [a.feature_samples]
        if a.feature_samples:
            al, no = a.features()
            out["albedo"], out["normal"] = u32(al), u32(no)
            if a.has_noise:
                out["guided"] = u32(a.resolve_guided())
    return out


def same(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


def raises(status, fn):
    with pytest.raises(hrt.HrtError) as e:
        fn()
    assert e.value.status == status, e.value


# the blob's layout, from include/hrt/hrt.h
P, MASK = 0x100000001B3, (1 << 64) - 1


def checksum(data: bytes) -> int:
    h = [(0xCBF29CE484222325 + i) & MASK for i in range(4)]
    for j, (w,) in enumerate(struct.iter_unpack("<Q", data)):
        h[j & 3] = ((h[j & 3] ^ w) * P) & MASK
    r = h[0]
    for i in (1, 2, 3):
        r = ((r * P) & MASK) ^ h[i]
    r = ((r ^ (len(data) // 8)) * P) & MASK
    return r ^ (r >> 32)


def planes(blob):
    """{"sums": (offset, uint32 words), "m2": ...} of a blob."""
    flags, _, _, n_tiles = struct.unpack_from("<4I", blob, 16)
    (n_px,) = struct.unpack_from("<Q", blob, 32)
    _, n_records, n_f, _ = struct.unpack_from("<4I", blob, 40)
    at = 184 + 16 * n_tiles
    for _ in range(n_records):
        at += 16 + 16 * struct.unpack_from("<2Q", blob, at)[1]
    at = (at + 16 * n_f + 15) & ~15
    out = {"sums": (at, 4 * n_px)}
    at += 16 * n_px
    if flags & hrt.ACCUM_NOISE:
        out["m2"] = (at, n_px)
        at += (4 * n_px + 15) & ~15
    if flags & hrt.ACCUM_FEATURES:
        out["fa"], out["fn"] = (at, 4 * n_px), (at + 16 * n_px, 4 * n_px)
        at += 32 * n_px
    assert at + 8 == len(blob) == struct.unpack_from("<Q", blob, 8)[0]
    return out


def plane(blob, name):
    off, words = planes(blob)[name]
    return np.frombuffer(blob, np.uint32, words, off)


def resealed(blob: bytearray) -> bytes:
    blob[-8:] = struct.pack("<Q", checksum(bytes(blob[:-8])))
    return bytes(blob)


# ------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.gpu
@pytest.mark.parametrize("inp,noise,features", [("A", True, True), ("B", True, True), ("A", False, False), ("A", True, False),
                                                ("A", False, True)])
def test_round_trip(scene, inp, noise, features):
    name, w, h = INPUTS[inp]
    s = scene(name)
    a = state(s, inp, noise, features)
    blob = a.snapshot()
    assert len(blob) == a.snapshot_size() and checksum(blob[:-8]) == struct.unpack_from("<Q", blob, len(blob) - 8)[0]
    info, tiles = hrt.snapshot_info(blob)
    assert (info.width, info.height, info.n_tiles, info.uniform, info.n_pixels) == (w, h, len(a.tiles), 0, a.n_pixels)
    assert info.flags == (hrt.ACCUM_NOISE if noise else 0) | (hrt.ACCUM_FEATURES if features else 0) and tiles == a.tiles
    if noise:
        assert np.array_equal(plane(blob, "m2"), u32(a.moments()))
    if features:
        assert np.array_equal(plane(blob, "fa"), u32(a.debug_features()[0]).reshape(-1))
        assert np.array_equal(plane(blob, "fn"), u32(a.debug_features()[1]).reshape(-1))
    b = fresh(s, w, h, noise, features)
    b.restore(blob)
    want = answers(a)
    same(answers(b), want)
    assert b.snapshot() == blob                     # and a snapshot of the restored one is the same bytes
    raises(hrt.ERR_STATE, lambda: b.samples)        # the tiles differ, as on the original
    # a reset accumulator takes it as a fresh one does
    a.reset()
    a.restore(blob)
    same(answers(a), want)
    # both go on alike: the subset pass to the other tiles makes them ordinary accumulators again
    rest = [t for t in range(len(a.tiles)) if t not in SUBSET[inp]]
    for x in (a, b):
        add(x, s, 80, 120, tiles=rest)
    assert a.samples == b.samples == 120
    same(answers(a), answers(b))
    assert np.array_equal(u32(a.download()[0]), u32(b.download()[0])) and a.download()[1] == b.download()[1] == [(0, 120)]
    a.close()
    b.close()


@pytest.mark.gpu
def test_plain_snapshot_holds_the_downloaded_sums(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    a = fresh(s, w, h, noise=False)
    add(a, s, 0, 40)
    add(a, s, 60, 100)
    sums, ranges = a.download()
    blob = a.snapshot()
    assert hrt.snapshot_info(blob)[0].uniform == 1 and sorted(planes(blob)) == ["sums"]
    assert np.array_equal(plane(blob, "sums"), u32(sums).reshape(-1))
    b = fresh(s, w, h, noise=False)
    b.restore(blob)
    assert b.samples == 80 and b.download()[1] == ranges == [(0, 40), (60, 100)]
    assert np.array_equal(u32(b.download()[0]), u32(sums))
    # an empty accumulator round-trips too
    e = fresh(s, w, h, noise=False)
    empty = e.snapshot()
    e.restore(empty)
    assert e.samples == 0 and e.snapshot() == empty
    for x in (a, b, e):
        x.close()


# ------------------------------------------------------------------------------------------ 2. resume
class Stop(Exception):
    pass


@pytest.mark.gpu
def test_resumed_refine_equals_the_uninterrupted_one(scene, tmp_path):
    name, w, h = INPUTS["A"]
    s = scene(name)
    cam, p = setup(s, w, h, 1)
    kw = dict(target=0.05, pass_spp=40, max_spp=400, floor=FLOOR)
    whole, log = fresh(s, w, h), []
    rec = whole.refine(cam, p, on_pass=lambda t, r: log.append(list(t)), **kw)
    print(f"\nrefine: {len(log)} passes over {[len(t) for t in log]} tiles, samples per tile {whole.tile_samples}")
    assert len(log) >= 4                             # the precondition: the run goes on past the interruption
    assert len(set(whole.tile_samples)) > 1

    part, seen = fresh(s, w, h), []

    def stop_after_two(t, r):
        seen.append(list(t))
        if len(seen) == 2:
            raise Stop

    with pytest.raises(Stop):
        part.refine(cam, p, on_pass=stop_after_two, **kw)
    assert seen == log[:2]
    path = tmp_path / "refine.hrts"
    part.save(path)
    part.close()
    back, log2 = hrt.Accumulator.load(s, path), []
    assert back.tiles == whole.tiles and back.has_noise and not back.has_features
    with pytest.raises(ValueError):
        back.refine(cam, p, **kw)                    # without the keyword refine is unchanged
    rec2 = back.refine(cam, p, resume=True, on_pass=lambda t, r: log2.append(list(t)), **kw)
    assert log2 == log[2:]
    assert [(r.samples, r.chunks) for r in rec2] == [(r.samples, r.chunks) for r in rec]
    same(answers(back), answers(whole))
    # resuming a finished run sends nothing
    back.refine(cam, p, resume=True, on_pass=lambda t, r: log2.append("more"), **kw)
    assert "more" not in log2
    whole.close()
    back.close()


# ------------------------------------------------------------------------------------------ 3. refusals survive a restore
@pytest.mark.gpu
def test_restored_accumulator_refuses_what_the_original_refused(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    a = state(s, "A", True, True)
    b = fresh(s, w, h, True, True)
    b.restore(a.snapshot())
    want = answers(a)
    for x in (a, b):
        raises(hrt.ERR_INVALID_ARG, lambda: add(x, s, 100, 140))                    # overlaps tiles 0, 5, 11 alone
        raises(hrt.ERR_INVALID_ARG, lambda: add(x, s, 119, 121, tiles=[5]))         # by one sample
        raises(hrt.ERR_INVALID_ARG, lambda: x.add_features(*setup(s, w, h, 4, offset=6)))   # [6, 10) overlaps [0, 8)
        raises(hrt.ERR_INVALID_ARG, lambda: add(x, s, 200, 240, seed=SEED + 1))     # another identity
        raises(hrt.ERR_INVALID_ARG, lambda: x.add_features(*setup(s, w, h, 4, offset=8, seed=SEED + 1)))
        raises(hrt.ERR_UNSUPPORTED, lambda: x.download())                           # the old calls keep their refusals
        same(answers(x), want)
    for x in (a, b):                                                                # and both accept what is free
        add(x, s, 80, 120, tiles=[1])
        x.add_features(*setup(s, w, h, 4, offset=8))
    same(answers(a), answers(b))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------ 4. errors change nothing
@pytest.mark.gpu
def test_restore_and_snapshot_errors_change_nothing(scene):
    name, w, h = INPUTS["A"]
    s = scene(name)
    a = state(s, "A", True, True)
    blob = a.snapshot()
    want = answers(a)
    raises(hrt.ERR_STATE, lambda: a.restore(blob))                                  # holds samples
    same(answers(a), want)
    only_features = fresh(s, w, h, True, True)
    only_features.add_features(*setup(s, w, h, 4))
    raises(hrt.ERR_STATE, lambda: only_features.restore(blob))                      # feature samples are samples
    assert only_features.feature_samples == 4 and only_features.tile_samples == [0] * 12
    only_features.close()
    L = hrt.load()
    for target in (fresh(s, w, h, True, True, tile=32), fresh(s, w, h, True, False), fresh(s, w, h, False, True), fresh(s, w, h, False, False),
                   hrt.Accumulator(s, 32, 36, hrt.tile_grid(32, 36, 16), noise=True, features=True),
                   hrt.Accumulator(s, w, h, list(reversed(hrt.tile_grid(w, h, 16))), noise=True, features=True)):
        raises(hrt.ERR_INVALID_ARG, lambda: target.restore(blob))
        assert target.tile_samples == [0] * len(target.tiles) and target.samples == 0
        add(target, s, 0, 40)                                                        # still an empty accumulator: any first pass
        assert target.samples == 40
        target.close()
    t = fresh(s, w, h, True, True)
    before = t.snapshot()
    flipped = bytearray(blob)
    flipped[planes(blob)["m2"][0] + 5] ^= 0x10
    header = bytearray(blob)
    header[20] ^= 1                                                                  # the width, behind a good checksum
    for bad in (blob[:-1], blob[:len(blob) // 2], blob[:100], b"", bytes(flipped), resealed(header), blob + bytes(8)):
        assert L.hrt_accum_restore(t.h, bad, len(bad)) == hrt.ERR_INVALID_ARG, len(bad)
        assert t.snapshot() == before and t.tile_samples == [0] * 12 and t.feature_samples == 0
    t.restore(blob)                                                                  # and the good blob still goes in
    same(answers(t), want)
    # a buffer that is too small is not written, whatever cap says
    size = a.snapshot_size()
    buf = np.full(size, 0xA5, np.uint8)
    n = ctypes.c_uint64()
    for cap in (0, 1, 184, size - 1):
        assert L.hrt_accum_snapshot(a.h, buf.ctypes.data, cap, ctypes.byref(n)) == hrt.ERR_INVALID_ARG
        assert n.value == size and (buf == 0xA5).all()
    assert a.snapshot_into(buf) == size and buf.tobytes() == blob
    same(answers(a), want)
    a.close()
    t.close()


# ------------------------------------------------------------------------------------------ 5. merge_tiles
def merge_case(scene, inp, noise=True):
    """dst: (0, 40) everywhere plus (40, 80) on two tiles; src: (100, 140) on two tiles alone, one of them common."""
    name, w, h = INPUTS[inp]
    s = scene(name)
    nt = len(hrt.tile_grid(w, h, 16))
    extra, theirs = ([1, 2], [2, 7]) if nt > 4 else ([1, 2], [2, 3])
    dst, src = fresh(s, w, h, noise), fresh(s, w, h, noise)
    add(dst, s, 0, 40)
    add(dst, s, 40, 80, tiles=extra)
    add(src, s, 100, 140, tiles=theirs)
    return s, dst, src, extra, theirs


@pytest.mark.gpu
@pytest.mark.parametrize("inp,noise", [("A", True), ("B", True), ("A", False)])
def test_merge_tiles(scene, inp, noise):
    s, dst, src, extra, theirs = merge_case(scene, inp, noise)
    w, h, nt = dst.width, dst.height, len(dst.tiles)
    spans = tile_spans(dst)
    assert src.tile_samples == [40 if t in theirs else 0 for t in range(nt)]
    # poke -0.0 (and a NaN) into a dst tile src holds nothing for, through a hand-edited snapshot
    quiet = next(t for t in range(nt) if t not in theirs and t not in extra)
    edited = bytearray(dst.snapshot())
    off = planes(edited)["sums"][0] + 16 * spans[quiet][0]
    edited[off:off + 8] = struct.pack("<2I", 0x80000000, 0x7FC00001)
    edited = resealed(edited)
    dst.reset()
    dst.restore(edited)
    d0, s0 = dst.snapshot(), src.snapshot()
    assert d0 == edited and plane(d0, "sums")[4 * spans[quiet][0]] == 0x80000000
    k_before = [r.chunks for r in dst.noise(FLOOR)] if noise else None
    k_src = [r.chunks for r in src.noise(FLOOR)] if noise else None   # a 40-spp pass: 3 chunks on A, 2 on B; 0 where src is empty
    held = dst.tile_samples
    dst.merge_tiles(src)
    d1 = dst.snapshot()
    assert src.snapshot() == s0                                                      # src is read only
    assert dst.tile_samples == [n + (40 if t in theirs else 0) for t, n in enumerate(held)]
    for name_, words in (("sums", 4), ("m2", 1)) if noise else (("sums", 4),):
        before, other, after = plane(d0, name_), plane(s0, name_), plane(d1, name_)
        for t, (off, cnt) in enumerate(spans):
            sl = slice(words * off, words * (off + cnt))
            if t in theirs:   # numpy f32 dst + src; the sums' w stays 0
                want = before[sl].view(F) + other[sl].view(F)
                assert np.array_equal(after[sl], want.view(np.uint32)), (name_, t)
            else:             # not touched: the same bits, -0.0 and NaN included
                assert np.array_equal(after[sl], before[sl]), (name_, t)
    if noise:
        rec = dst.noise(FLOOR)
        assert [r.chunks for r in rec] == [k + ks for k, ks in zip(k_before, k_src)]
        assert all((ks > 0) == (t in theirs) for t, ks in enumerate(k_src))
        # the same passes taken directly, on the tiles where that is the same schedule (src's pass came last there)
        direct = fresh(s, w, h)
        add(direct, s, 0, 40)
        add(direct, s, 40, 80, tiles=extra)
        add(direct, s, 100, 140, tiles=theirs)
        ra, ea = dst.noise(FLOOR, error_map=True)
        rb, eb = direct.noise(FLOOR, error_map=True)
        only = [t for t in theirs if t not in extra]   # (0, 40) then (100, 140): acc + pass either way
        assert only
        for t in range(nt):
            assert (ra[t].samples, ra[t].chunks) == (rb[t].samples, rb[t].chunks)
            if t in only or (t not in theirs and t != quiet):
                off, cnt = spans[t]
                assert np.array_equal(u32(ea[off:off + cnt]), u32(eb[off:off + cnt])), t
                assert (bits(ra[t].mean), bits(ra[t].max)) == (bits(rb[t].mean), bits(rb[t].max)), t
        direct.close()
    # the same samples again: tiles `theirs` overlap; and an overlap on ONE tile alone
    raises(hrt.ERR_INVALID_ARG, lambda: dst.merge_tiles(src))
    one = fresh(s, w, h, noise)
    add(one, s, 60, 100, tiles=[extra[0], quiet])                                    # extra[0] holds (40, 80); quiet does not
    raises(hrt.ERR_INVALID_ARG, lambda: dst.merge_tiles(one))
    assert dst.snapshot() == d1
    raises(hrt.ERR_UNSUPPORTED, lambda: dst.merge(src))                              # merge keeps its refusal
    for x in (dst, src, one):
        x.close()


@pytest.mark.gpu
def test_merge_tiles_refuses_what_merge_refuses(scene):
    s, dst, src, extra, theirs = merge_case(scene, "A")
    w, h = dst.width, dst.height
    d0 = dst.snapshot()
    others = [fresh(s, w, h, noise=False), fresh(s, w, h, True, True), fresh(s, w, h, tile=32),
              hrt.Accumulator(s, 32, 36, hrt.tile_grid(32, 36, 16), noise=True)]
    for o in others:
        add(o, s, 100, 140)
        raises(hrt.ERR_INVALID_ARG, lambda: dst.merge_tiles(o))
        raises(hrt.ERR_INVALID_ARG, lambda: o.merge_tiles(dst))
    alien = fresh(s, w, h)
    add(alien, s, 100, 140, tiles=[3], seed=SEED + 1)                                # another identity
    raises(hrt.ERR_INVALID_ARG, lambda: dst.merge_tiles(alien))
    raises(hrt.ERR_INVALID_ARG, lambda: dst.merge_tiles(dst))
    assert dst.snapshot() == d0
    empty = fresh(s, w, h)
    dst.merge_tiles(empty)                                                           # nothing to take: nothing changes
    assert dst.snapshot() == d0
    empty.merge_tiles(dst)                                                           # into an empty one: dst's bits
    assert plane(empty.snapshot(), "sums").tobytes() == plane(d0, "sums").tobytes() and empty.tile_samples == dst.tile_samples
    assert np.array_equal(u32(empty.moments()), u32(dst.moments()))
    for x in [dst, src, alien, empty] + others:
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("noise,features", [(True, True), (False, False)])
def test_merge_tiles_of_uniform_accumulators_is_merge(scene, noise, features):
    name, w, h = INPUTS["A"]
    s = scene(name)
    made = []
    for _ in range(2):
        lo, hi = fresh(s, w, h, noise, features), fresh(s, w, h, noise, features)
        add(lo, s, 0, 40)
        add(hi, s, 40, 80)
        if features:
            lo.add_features(*setup(s, w, h, 4))
            hi.add_features(*setup(s, w, h, 4, offset=4))
        made += [lo, hi]
    made[0].merge(made[1])
    made[2].merge_tiles(made[3])
    assert made[0].snapshot() == made[2].snapshot()
    assert made[2].samples == 80 and made[2].download()[1] == [(0, 80)]
    same(answers(made[0]), answers(made[2]))
    for x in made:
        x.close()


@pytest.mark.gpu
def test_merging_until_all_tiles_agree_gives_an_ordinary_accumulator(scene):
    s, dst, src, extra, theirs = merge_case(scene, "A")
    w, h, nt = dst.width, dst.height, 12
    dst.merge_tiles(src)
    raises(hrt.ERR_STATE, lambda: dst.samples)
    rest = fresh(s, w, h)
    add(rest, s, 40, 80, tiles=[t for t in range(nt) if t not in extra])
    add(rest, s, 100, 140, tiles=[t for t in range(nt) if t not in theirs])
    dst.merge_tiles(rest)
    assert dst.samples == 120 and dst.download()[1] == [(0, 80), (100, 140)]
    assert hrt.snapshot_info(dst.snapshot())[0].uniform == 1
    assert [(r.samples, r.chunks) for r in dst.noise(FLOOR)] == [(120, 9)] * nt
    third = fresh(s, w, h)
    add(third, s, 80, 100)
    dst.merge(third)                                                                 # and hrt_accum_merge takes it again
    assert dst.download()[1] == [(0, 140)]
    for x in (dst, src, rest, third):
        x.close()


@pytest.mark.gpu
def test_merge_tiles_with_one_tile(scene):
    name, w, h = INPUTS["B"]
    s = scene(name)
    a, b, both = (hrt.Accumulator(s, w, h, noise=True) for _ in range(3))
    add(a, s, 0, 40)
    add(b, s, 40, 80, tiles=[0])
    add(both, s, 0, 40)
    add(both, s, 40, 80)
    a.merge_tiles(b)
    assert a.samples == 80
    # acc + pass_sum either way: b's sums are 0 + pass_sum = pass_sum
    assert a.snapshot() == both.snapshot()
    for x in (a, b, both):
        x.close()


# ------------------------------------------------------------------------------------------ 6. a frame split across jobs
@pytest.mark.gpu
def test_cross_job_split(scene):
    """The frame is held to numpy's evaluation of the header's expression, sqrtf(acc * (1.0f / (float)N_t)) with
    acc = a + b in f32: the resolve multiplies by the reciprocal, it does not divide."""
    name, w, h = INPUTS["A"]
    s = scene(name)
    cam, p = setup(s, w, h, 1)
    first = fresh(s, w, h)
    first.refine(cam, p, target=0.05, pass_spp=40, max_spp=160, floor=FLOOR)
    base = 1 << 20
    second = fresh(s, w, h)
    add(second, s, base, base + 40, tiles=list(range(12)))
    add(second, s, base + 40, base + 80, tiles=[2, 5, 6, 9])
    n1, n2 = first.tile_samples, second.tile_samples
    k1, k2 = [r.chunks for r in first.noise(FLOOR)], [r.chunks for r in second.noise(FLOOR)]
    b1, b2 = first.snapshot(), second.snapshot()
    carrier = fresh(s, w, h)                                                         # the other job's state arrives as a blob
    carrier.restore(b2)
    first.merge_tiles(carrier)
    rec = first.noise(FLOOR)
    assert [r.samples for r in rec] == [x + y for x, y in zip(n1, n2)] == first.tile_samples
    assert [r.chunks for r in rec] == [x + y for x, y in zip(k1, k2)]
    px = first.resolve()
    assert np.isfinite(px).all()
    acc = plane(b1, "sums").view(F).reshape(-1, 4) + plane(b2, "sums").view(F).reshape(-1, 4)
    for t, (off, cnt) in enumerate(tile_spans(first)):
        want = np.sqrt(acc[off:off + cnt, :3] * (F(1.0) / F(n1[t] + n2[t])))
        assert np.array_equal(u32(px[off:off + cnt, :3]), u32(want.astype(F))), t
    assert np.all(px[:, 3] == 1.0)
    for x in (first, second, carrier):
        x.close()
