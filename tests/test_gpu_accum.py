"""The sample accumulator on the GPU (hrt.Accumulator over hrt_accum_*): the bit contract of include/hrt/hrt.h.

One pass equals hrt_render bit for bit on every kernel family and chunk path; several passes meet the oracle's bar
and have the bits the pass schedule defines, whatever the tile split; merge, download and upload keep them; errors
change nothing; the device arithmetic equals the host's; and the existing render calls are untouched by it."""
import numpy as np
import pytest

import hrt
from oracle import oracle as O

TOL = 1e-3   # the project's bar (tests/test_gpu_parity.py)
SEED = 7
EXACT_STATS = ("segments", "samples", "pixels", "node_visits", "prim_tests", "tex_evals")


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    """Committed preset scenes, shared by the tests of this module."""
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


def setup(s, w, h, spp, offset=0, flags=0, seed=SEED, depth=50):
    cam = hrt.preset_camera(s.info, w, h)
    return cam, hrt.params(w, h, spp, depth, seed, tuple(s.info.background), sample_offset=offset, flags=flags)


def passes(s, w, h, ranges, tiles=None, **kw):
    """An accumulator holding the given [begin, end) passes, added in that order; (accumulator, [stats])."""
    a = hrt.Accumulator(s, w, h, tiles)
    stats = []
    for b, e in ranges:
        cam, p = setup(s, w, h, e - b, offset=b, **kw)
        stats.append(a.add(cam, p, stats=True))
    return a, stats


# (preset, w, h, spp, sample_offset, flags): the single-chunk and multi-chunk paths of every kernel family
ONE_PASS = [
    ("random", 40, 24, 8, 0, 0),                           # sphere kernel, one chunk
    ("random", 40, 24, 100, 0, 0),                         # head and tail chunks
    ("random", 40, 24, 100, 37, 0),                        # ... from sample 37 on
    ("random", 40, 24, 8, 0, hrt.RENDER_NO_LDS),           # the scene in global memory
    ("random", 40, 24, 8, 0, hrt.RENDER_COUNT_WORK),       # the instrumented instantiation
    ("cornell", 24, 24, 16, 0, 0),                         # general walk kernel, one chunk
    ("cornell", 24, 24, 70, 0, 0),                         # 3 chunks
    ("cornell", 24, 24, 16, 0, hrt.RENDER_REFERENCE_CULL),  # the segment kernel (finish_sample), one chunk
    ("final", 40, 40, 8, 0, 0),                            # one-sample chunks
    ("final", 40, 40, 1, 0, 0),                            # ONE one-sample chunk
    ("earth_perlin", 48, 27, 16, 0, 0),                    # the sphere kernel's HEAVY instantiation
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,spp,offset,flags", ONE_PASS)
def test_one_pass_equals_render(scene, name, w, h, spp, offset, flags):
    s = scene(name)
    cam, p = setup(s, w, h, spp, offset, flags)
    ref, st_ref = hrt.render(s, cam, p, stats=True)
    a = hrt.Accumulator(s, w, h)
    st = a.add(cam, p, stats=True)
    img = a.resolve()
    assert a.samples == spp
    assert img.shape == ref.shape and img.dtype == np.float32
    assert np.array_equal(u32(img), u32(ref))
    # the counters that are a function of the paths alone are equal field for field; the COUNT_WORK slot and cycle
    # counters (which lanes shared a wave, shader clocks) differ between two runs of the same call, so they are
    # held to being counted or not, as the reference render's are
    for f, _ in hrt.RenderStats._fields_:
        if f in EXACT_STATS:
            assert getattr(st, f) == getattr(st_ref, f), f
        elif f == "phase_cycles":
            assert [v > 0 for v in st.phase_cycles] == [v > 0 for v in st_ref.phase_cycles]
        else:
            assert (getattr(st, f) > 0) == (getattr(st_ref, f) > 0), f
    assert st.pixels == w * h and st.samples == w * h * spp
    a.close()


@pytest.mark.gpu
def test_fused_preview_equals_resolve(scene):
    """add(preview=...) resolves in the kernel that adds the pass: the same frame as a resolve after it."""
    s = scene("random")
    a = hrt.Accumulator(s, 40, 24)
    for b, e, fmt in [(0, 16, "f32"), (16, 48, "rgba8"), (48, 100, True)]:
        cam, p = setup(s, 40, 24, e - b, offset=b)
        pre = a.add(cam, p, preview=fmt)
        want = a.resolve("rgba8" if fmt == "rgba8" else "f32")
        assert pre.shape == want.shape and pre.dtype == want.dtype
        assert np.array_equal(pre.view(np.uint8), want.view(np.uint8))
    assert a.samples == 100
    a.close()


MULTI = [("random", 40, 24, [(0, 16), (16, 48), (48, 100)]), ("cornell", 24, 24, [(0, 32), (32, 70)])]
_oracle = {}


def oracle_frame(name, w, h, spp, earth):
    if name not in _oracle:
        _oracle[name] = O.OracleScene(hrt.PRESETS[name], 1, earth).render(w, h, spp, 50, seed=SEED)
    return _oracle[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,ranges", MULTI)
@pytest.mark.parametrize("order", ["in_order", "last_first"])
def test_passes_against_oracle(scene, earth, name, w, h, ranges, order):
    total = ranges[-1][1]
    ref, cnt = oracle_frame(name, w, h, total, earth)
    rs = ranges if order == "in_order" else [ranges[-1]] + ranges[:-1]
    a, stats = passes(scene(name), w, h, rs)
    assert a.samples == total
    assert a.download()[1] == [(0, total)]
    assert sum(st.segments for st in stats) == cnt["segments"]
    assert sum(st.samples for st in stats) == w * h * total
    linf = float(np.abs(a.resolve() - ref).max())
    assert linf <= TOL, f"{name} {order}: L-inf {linf}"
    a.close()


@pytest.mark.gpu
def test_defined_bits_of_passes_merge_and_upload(scene):
    s = scene("random")
    w, h, ranges = 40, 24, [(0, 16), (16, 48), (48, 100)]
    parts = [passes(s, w, h, [r])[0] for r in ranges]
    S = [a.download()[0] for a in parts]
    assert [a.download()[1] for a in parts] == [[r] for r in ranges]
    want = ((S[0] + S[1]).astype(np.float32) + S[2]).astype(np.float32)
    three, _ = passes(s, w, h, ranges)
    sums, held = three.download()
    assert held == [(0, 100)]
    assert (sums[:, 3] == 0).all()
    assert np.array_equal(u32(sums), u32(want))
    # merge: dst = dst + src
    parts[0].merge(parts[1])
    assert parts[0].download()[1] == [(0, 48)]
    parts[0].merge(parts[2])
    msums, mheld = parts[0].download()
    assert mheld == [(0, 100)] and parts[0].samples == 100
    assert np.array_equal(u32(msums), u32(want))
    assert np.array_equal(u32(parts[0].resolve()), u32(three.resolve()))
    # checkpoint: download -> a new accumulator -> upload resolves to the same bits, and goes on
    two, _ = passes(s, w, h, ranges[:2])
    csums, cheld = two.download()
    cam, p = setup(s, w, h, 1)
    resumed = hrt.Accumulator(s, w, h)
    resumed.upload(cam, p, csums, cheld)
    assert resumed.samples == 48
    assert np.array_equal(u32(resumed.resolve()), u32(two.resolve()))
    cam2, p2 = setup(s, w, h, 52, offset=48)
    resumed.add(cam2, p2)
    assert np.array_equal(u32(resumed.download()[0]), u32(want))
    # an upload into an accumulator that holds samples adds, as a merge does
    added, _ = passes(s, w, h, ranges[:1])
    added.upload(cam, p, S[1], [ranges[1]])
    added.upload(cam, p, S[2], [ranges[2]])
    assert np.array_equal(u32(added.download()[0]), u32(want))
    for a in parts + [three, two, resumed, added]:
        a.close()


@pytest.mark.gpu
def test_tiles_do_not_change_the_bits(scene):
    """A frame of two passes does not depend on the tile split: each rank's share of ragged 16-px tiles, resolved
    and scattered into the frame, equals the whole-frame accumulator's pixels."""
    s = scene("random")
    w, h, ranges = 40, 24, [(0, 16), (16, 100)]
    whole, _ = passes(s, w, h, ranges)
    ref = whole.resolve()
    frame = np.zeros_like(ref)
    for rank in range(2):
        tiles = hrt.tile_grid(w, h, 16, rank, 2)
        assert any(t[2] == 8 for t in tiles) or any(t[3] == 8 for t in tiles)   # the ragged 8-wide / 8-high tiles
        a, stats = passes(s, w, h, ranges, tiles=tiles)
        px = a.resolve()
        assert px.shape == (sum(t[2] * t[3] for t in tiles), 4)
        off = 0
        for x, y, tw, th in tiles:
            frame[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, 4)
            off += tw * th
        assert sum(st.pixels for st in stats) == 2 * off
        a.close()
    assert np.array_equal(u32(frame), u32(ref))
    whole.close()


@pytest.mark.gpu
def test_rgba8_resolve(scene):
    s = scene("simple_light")   # the light's radiance resolves to values above 1
    cam, p = setup(s, 48, 27, 16)
    a = hrt.Accumulator(s, 48, 27)
    a.add(cam, p)
    f = a.resolve("f32")
    b = a.resolve("rgba8")
    assert b.shape == (27, 48, 4) and b.dtype == np.uint8
    assert float(f[..., :3].max()) > 1.0
    v = f[..., :3]
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(0.999)).astype(np.float32)
    assert np.array_equal(b[..., :3], (np.float32(256) * v).astype(np.float32).astype(np.uint8))
    assert (b[..., 3] == 255).all()
    a.close()


def _rejected(fn):
    with pytest.raises(hrt.HrtError) as e:
        fn()
    assert e.value.status == hrt.ERR_INVALID_ARG, e.value


@pytest.mark.gpu
def test_errors_change_nothing(scene):
    s = scene("random")
    w, h = 40, 24
    empty = hrt.Accumulator(s, w, h)
    with pytest.raises(hrt.HrtError) as e:
        empty.resolve()
    assert e.value.status == hrt.ERR_STATE
    a, _ = passes(s, w, h, [(0, 16)])
    before = a.resolve().copy()

    def unchanged():
        assert a.samples == 16 and a.download()[1] == [(0, 16)]
        assert np.array_equal(u32(a.resolve()), u32(before))

    cam, p = setup(s, w, h, 16, offset=8)
    _rejected(lambda: a.add(cam, p))                                        # [8, 24) overlaps [0, 16)
    unchanged()
    _rejected(lambda: a.add(*setup(s, w, h, 16, offset=16, seed=SEED + 1)))   # another seed
    _rejected(lambda: a.add(*setup(s, w, h, 16, offset=16, depth=49)))        # another max_depth
    cam2 = hrt.camera((13, 2, 4), (0, 0, 0), 20, 0.1, 10.0, 0.0, 1.0, w, h)
    _rejected(lambda: a.add(cam2, setup(s, w, h, 16, offset=16)[1]))          # another camera
    _rejected(lambda: a.add(*setup(s, w + 8, h, 16, offset=16)))              # another image size
    cam3, p3 = setup(s, w, h, 16, offset=16)
    p3.sample_offset, p3.samples = 0xFFFFFFF0, 32                             # ends past 2^32
    _rejected(lambda: a.add(cam3, p3))
    unchanged()
    over, _ = passes(s, w, h, [(8, 24)])
    _rejected(lambda: a.merge(over))                                         # overlapping ranges
    other, _ = passes(s, w, h, [(16, 32)], seed=SEED + 1)
    _rejected(lambda: a.merge(other))                                        # another identity
    sums, _ = over.download()
    _rejected(lambda: a.upload(cam, p, sums, [(8, 24)]))
    unchanged()
    a.merge(empty)   # nothing to add: a no-op
    unchanged()
    # reset allows a new identity
    a.reset()
    assert a.samples == 0 and a.download()[1] == []
    cam4, p4 = setup(s, w, h, 8, seed=SEED + 1)
    a.add(cam4, p4)
    assert np.array_equal(u32(a.resolve()), u32(hrt.render(s, cam4, p4)))
    for x in (empty, a, over, other):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])   # the last: a second trip of the grid-stride loop
def test_device_arithmetic_equals_host(n):
    rng = np.random.default_rng(n)
    partial = np.zeros((3, n, 4), np.float32)
    partial[:, :, :3] = rng.uniform(0, 50, (3, n, 3)).astype(np.float32)
    acc = np.zeros((n, 4), np.float32)
    acc[:, :3] = rng.uniform(0, 500, (n, 3)).astype(np.float32)
    for fmt in (None, "f32", "rgba8"):
        ha, ho = hrt.debug_accumulate(partial, acc, 1000, fmt, on_device=False)
        da, do = hrt.debug_accumulate(partial, acc, 1000, fmt, on_device=True)
        assert np.array_equal(u32(da), u32(ha)), fmt
        if fmt is None:
            assert ho is None and do is None
        else:
            assert np.array_equal(do.view(np.uint8), ho.view(np.uint8)), fmt


@pytest.mark.gpu
def test_existing_calls_are_untouched(earth):
    """After accumulate calls on a scene, hrt.render of a multi-chunk and a one-chunk case still equals a render on
    a fresh scene: the slots' shared partial buffers and the kernels' raw-sum path do not leak between calls."""
    used, fresh = hrt.preset("random", 1, earth), hrt.preset("random", 1, earth)
    used.commit()
    fresh.commit()
    w, h = 40, 24
    a = hrt.Accumulator(used, w, h)
    for spp, off in [(8, 0), (100, 8), (8, 108), (16, 116), (8, 132)]:   # more calls than the scene has slots
        a.add(*setup(used, w, h, spp, offset=off))
        for check in (100, 8):
            cam, p = setup(used, w, h, check)
            assert np.array_equal(u32(hrt.render(used, cam, p)), u32(hrt.render(fresh, cam, p))), (spp, check)
    a.close()
    used.close()
    fresh.close()
