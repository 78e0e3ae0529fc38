"""The demodulated guided resolve on the GPU (hrt_accum_resolve_guided_ex with HRT_GUIDED_DEMODULATE; include/hrt/hrt.h,
"THE BIT CONTRACT of the demodulated frame"): the kernels against the host's arithmetic and against the numpy
restatement (tests/demod_restated.py) from an accumulator's downloaded planes, bit for bit; the tile cut; that the
resolve writes nothing; flags == 0; snapshots; errors; and examples/render_demod.c."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import tool_env

import demod_restated as D
import filter_restated as FR
import hrt

SEED = 7
F = np.float32
W, H = 64, 36                     # 16-px tiles: 4 x 3, the top row of tiles 4 px high
SPP, FSPP = 8, 4
SUBSET = [1, 4, 11]               # the tiles the third pass goes to
RAGGED = [(0, 0, 37, 36), (37, 0, 27, 9), (37, 9, 27, 27)]
FLOOR = 0.01
TOL = dict(normal=0.1, albedo=0.1, depth=0.1)
OFF = dict(normal=0, albedo=0, depth=0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def scene(earth):
    s = hrt.preset("random", 1, earth)
    s.commit()
    yield s
    s.close()


def setup(s, spp, offset=0):
    cam = hrt.preset_camera(s.info, W, H)
    return cam, hrt.params(W, H, spp, 50, SEED, tuple(s.info.background), sample_offset=offset)


def accumulator(s, passes=2, subset=None, features=True, noise=True, fspp=FSPP, tiles="grid"):
    """`passes` radiance passes of SPP samples to every tile, one more to `subset`, and one feature pass of fspp."""
    a = hrt.Accumulator(s, W, H, hrt.tile_grid(W, H, 16) if tiles == "grid" else tiles, noise=noise, features=features)
    for k in range(passes):
        a.add(*setup(s, SPP, offset=SPP * k))
    if subset:
        a.add(*setup(s, SPP, offset=SPP * passes), tiles=subset)
    if features and fspp:
        a.add_features(*setup(s, fspp))
    return a


def unpack(a, px):
    frame = np.zeros((H, W, px.shape[-1]), px.dtype)
    off = 0
    for x, y, tw, th in a.tiles:
        frame[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, -1)
        off += tw * th
    return frame


def scales_of(a):
    return [FR.tile_scales(r.samples, r.chunks) for r in a.noise(0.05)]


def restated(a, sums, it, sigma, tol, floor):
    al, no = a.features()
    return D.demod_frame(sums, a.moments(), a.tiles, scales_of(a), al.reshape(-1, 4), no.reshape(-1, 4), W, H, it, sigma, tol, floor)


@pytest.fixture(scope="module")
def mixed(scene):
    """(a, sums): tiles that hold different passes (N = 16 or 24, K = 2 or 3), and their sums, which a uniform
    accumulator with a tile's passes gives for that tile (tests/test_gpu_filter.py)."""
    a = accumulator(scene, 2, SUBSET)
    two, three = accumulator(scene, 2, features=False), accumulator(scene, 3, features=False)
    sums, more, off = two.download()[0].copy(), three.download()[0], 0
    for t, (_, _, tw, th) in enumerate(a.tiles):
        if t in SUBSET:
            sums[off:off + tw * th] = more[off:off + tw * th]
        off += tw * th
    two.close()
    three.close()
    assert len(set(scales_of(a))) == 2 and a.tiles[-1][3] == 4
    yield a, sums
    a.close()


# ------------------------------------------------------------------------------------------ 1. kernels against the host
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(70, 21), (33, 9)])
def test_device_demodulated_equals_host(w, h):
    """Iterations 1 to 5 pass the staged steps 1, 2 and 4 and the global steps 8 and 16, each as the LAST (remodulating)
    iteration; with the flag on and off, with the feature terms and without."""
    import test_demod_host as TD

    r, a, n = TD.rasters(w, h)
    L = hrt.load()
    for k in (dict(kn=2.0, ka=10.0, kz=10.0), dict()):
        for it in (1, 2, 3, 4, 5):
            host = hrt.debug_guided(r, a, n, it, 4.0, demodulate=FLOOR, **k)
            dev = hrt.debug_guided(r, a, n, it, 4.0, demodulate=FLOOR, on_device=True, **k)
            assert np.array_equal(u32(dev), u32(host)), (w, h, k, it)
            off = np.zeros_like(r)
            kk = (k.get("kn", 0.0), k.get("ka", 0.0), k.get("kz", 0.0))
            assert L.hrt_debug_guided_ex(1, r.ctypes.data, a.ctypes.data, n.ctypes.data, w, h, it, 4.0, *kk, 0, 0.0, off.ctypes.data) == hrt.OK
            assert np.array_equal(u32(off), u32(hrt.debug_guided(r, a, n, it, 4.0, **k))), (w, h, k, it)
            assert not np.array_equal(u32(off), u32(dev))


@pytest.mark.gpu
def test_staging_variants_are_bit_identical(monkeypatch):
    """The existing staging knobs reach the remodulating kernel too: features from global memory, and nothing staged."""
    import test_demod_host as TD

    r, a, n = TD.rasters(70, 21)
    k = dict(kn=2.0, ka=10.0, kz=10.0)
    want = hrt.debug_guided(r, a, n, 3, 4.0, demodulate=FLOOR, **k)
    for knob, v in (("HRT_GUIDED_LDS_STEP", "0"), ("HRT_GUIDED_LDS_STEP", "2"), ("HRT_FILTER_LDS_STEP", "0")):
        monkeypatch.setenv(knob, v)
        assert np.array_equal(u32(hrt.debug_guided(r, a, n, 3, 4.0, demodulate=FLOOR, on_device=True, **k)), u32(want)), (knob, v)
        monkeypatch.delenv(knob)


# ------------------------------------------------------------------------------------------ 2. the accumulator's frame
@pytest.mark.gpu
def test_demodulated_resolve_equals_the_restatement(mixed):
    a, sums = mixed
    want = restated(a, sums, 3, 4.0, TOL, FLOOR)
    got = a.resolve_guided(guide=TOL, demodulate=FLOOR)
    assert got.shape == (W * H, 4) and got.dtype == F and (got[:, 3] == 1).all()
    assert np.array_equal(u32(got), u32(want))
    assert np.array_equal(a.resolve_guided("rgba8", guide=TOL, demodulate=FLOOR), FR.quantize(want))
    assert not np.array_equal(u32(got), u32(a.resolve_guided(guide=TOL)))
    # demodulate=True is the default floor with the default tolerances under demodulation
    assert np.array_equal(u32(a.resolve_guided(demodulate=True)), u32(restated(a, sums, 3, 4.0, hrt.DEMOD_DEFAULTS, hrt.DEMOD_FLOOR)))
    # 1 and 5 iterations (the last one staged and not), another sigma and floor, and the demodulated variance-only filter
    for it, sigma, tol, floor in ((1, 4.0, TOL, FLOOR), (5, 2.0, TOL, 0.1), (4, 4.0, OFF, 0.003)):
        got = a.resolve_guided(denoise=dict(iterations=it, sigma=sigma), guide=tol, demodulate=floor)
        assert np.array_equal(u32(got), u32(restated(a, sums, it, sigma, tol, floor))), (it, sigma, tol, floor)


@pytest.mark.gpu
def test_demodulated_frame_does_not_depend_on_the_tile_cut(scene):
    tiled, whole, ragged = (accumulator(scene, 2, tiles=t) for t in ("grid", None, RAGGED))
    for fmt, kw in (("f32", dict(demodulate=FLOOR)), ("rgba8", dict(denoise=dict(iterations=5, sigma=2.0), guide=dict(normal=0.25), demodulate=0.03))):
        fw = whole.resolve_guided(fmt, **kw)
        assert fw.shape == (H, W, 4)
        assert np.array_equal(unpack(tiled, tiled.resolve_guided(fmt, **kw)), fw)
        assert np.array_equal(unpack(ragged, ragged.resolve_guided(fmt, **kw)), fw)
    assert np.array_equal(u32(tiled.resolve_guided(guide=TOL, demodulate=FLOOR)),
                          u32(restated(tiled, tiled.download()[0], 3, 4.0, TOL, FLOOR)))
    for x in (tiled, whole, ragged):
        x.close()


@pytest.mark.gpu
def test_demodulated_resolve_writes_nothing(scene, mixed):
    def state(x, uniform):
        return ([x.download()[0]] if uniform else []) + [x.moments(), *x.debug_features(), x.resolve(), x.resolve_guided(guide=TOL),
                                                         x.resolve(denoise=True), x.noise(0.05, error_map=True)[1]]

    for x, uniform in ((mixed[0], False), (accumulator(scene, 2), True)):
        before = state(x, uniform)
        first = x.resolve_guided(guide=TOL, demodulate=FLOOR)
        x.resolve_guided("rgba8", denoise=dict(iterations=5), guide=OFF, demodulate=0.1)
        for p, q in zip(before, state(x, uniform)):
            assert np.array_equal(u32(p), u32(q))
        assert np.array_equal(u32(first), u32(x.resolve_guided(guide=TOL, demodulate=FLOOR)))
        if uniform:
            x.close()


@pytest.mark.gpu
def test_flags_zero_is_the_guided_resolve(mixed):
    import torch

    a, _ = mixed
    L = hrt.load()
    for fmt, dt in (("f32", F), ("rgba8", np.uint8)):
        for it, tol in ((3, TOL), (5, dict(normal=0.5, albedo=0, depth=0)), (3, OFF)):
            # the floor is not read when the flag is clear
            for floor in (0.0, float("nan")):
                g = hrt.GuidedExParams(it, 4.0, float(tol["normal"]), float(tol["albedo"]), float(tol["depth"]), 0, floor, 0)
                out = np.zeros(W * H * 4, dt)
                assert L.hrt_accum_resolve_guided_ex_host(a.h, ctypes.byref(g), hrt._ACCUM_FORMATS[fmt], out.ctypes.data) == hrt.OK
                assert np.array_equal(out.reshape(-1, 4), a.resolve_guided(fmt, denoise=dict(iterations=it), guide=tol))
                if tol is OFF:
                    assert np.array_equal(out.reshape(-1, 4), a.resolve(fmt, denoise=dict(iterations=it)))
    # the stream-ordered entry point into device memory, with the flag off and on, on the stream torch works on (the
    # default one; the suite's other stream tests keep the streams they always drew from torch's pool)
    stream = torch.cuda.current_stream()
    for g, want in ((hrt.guided_ex_params(demodulate=False), a.resolve_guided()),
                    (hrt.guided_ex_params(demodulate=FLOOR), a.resolve_guided(demodulate=FLOOR))):
        buf = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        assert L.hrt_accum_resolve_guided_ex(a.h, ctypes.byref(g), hrt.ACCUM_F32, ctypes.c_void_p(buf.data_ptr()),
                                             ctypes.c_void_p(stream.cuda_stream)) == hrt.OK
        stream.synchronize()
        assert np.array_equal(u32(buf.cpu().numpy().reshape(-1, 4)), u32(want))


@pytest.mark.gpu
def test_snapshot_restore_then_a_demodulated_resolve(scene):
    a = accumulator(scene, 2, SUBSET)
    want = a.resolve_guided(guide=TOL, demodulate=FLOOR), a.resolve_guided("rgba8", denoise=dict(iterations=5), demodulate=0.03)
    blob = a.snapshot()
    a.close()
    b = hrt.Accumulator(scene, W, H, hrt.tile_grid(W, H, 16), noise=True, features=True)
    b.restore(blob)
    assert np.array_equal(u32(b.resolve_guided(guide=TOL, demodulate=FLOOR)), u32(want[0]))
    assert np.array_equal(b.resolve_guided("rgba8", denoise=dict(iterations=5), demodulate=0.03), want[1])
    b.close()


# ------------------------------------------------------------------------------------------ 3. errors
@pytest.mark.gpu
def test_errors_change_nothing(scene):
    a = accumulator(scene, 2)
    no_feat = accumulator(scene, 2, features=False)
    no_fsamples = accumulator(scene, 2, fspp=0)
    no_noise = accumulator(scene, 2, noise=False)
    one = accumulator(scene, 1)                                       # K = 1
    every = (a, no_feat, no_fsamples, no_noise, one)
    state = {x: (x.download()[0], x.resolve()) for x in every}

    def raises(status, fn):
        with pytest.raises(hrt.HrtError) as e:
            fn()
        assert e.value.status == status, e.value

    for x in (no_feat, no_fsamples, no_noise, one):
        for fmt in ("f32", "rgba8"):
            raises(hrt.ERR_STATE, lambda: x.resolve_guided(fmt, demodulate=FLOOR))
    for floor in (0.0, -0.01, float("nan")):
        raises(hrt.ERR_INVALID_ARG, lambda: a.resolve_guided(demodulate=floor))
        raises(hrt.ERR_INVALID_ARG, lambda: no_feat.resolve_guided(demodulate=floor))     # argument errors come first
    for it in (0, 6):
        raises(hrt.ERR_INVALID_ARG, lambda: a.resolve_guided(denoise=dict(iterations=it), demodulate=FLOOR))
    raises(hrt.ERR_INVALID_ARG, lambda: a.resolve_guided(denoise=dict(sigma=0.0), demodulate=FLOOR))
    raises(hrt.ERR_INVALID_ARG, lambda: a.resolve_guided(guide=dict(albedo=-1), demodulate=FLOOR))
    L = hrt.load()
    out = np.zeros(W * H * 4, F)

    def call(flags, floor, reserved, fmt=hrt.ACCUM_F32, dst=out.ctypes.data, acc=a):
        g = hrt.GuidedExParams(3, 4.0, 0.1, 0.1, 0.1, flags, floor, reserved)
        return L.hrt_accum_resolve_guided_ex_host(acc.h, ctypes.byref(g), fmt, dst)

    for flags in (2, 3, 0x80000001, 0xFFFFFFFE):
        assert call(flags, FLOOR, 0) == hrt.ERR_INVALID_ARG, flags
    for flags in (0, 1):
        for reserved in (1, 0xFFFFFFFF):
            assert call(flags, FLOOR, reserved) == hrt.ERR_INVALID_ARG
    assert call(1, FLOOR, 0, fmt=2) == hrt.ERR_INVALID_ARG
    assert call(1, FLOOR, 0, dst=None) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_resolve_guided_ex_host(a.h, None, hrt.ACCUM_F32, out.ctypes.data) == hrt.ERR_INVALID_ARG
    g = hrt.guided_ex_params()
    assert L.hrt_accum_resolve_guided_ex(a.h, ctypes.byref(g), hrt.ACCUM_F32, None, None) == hrt.ERR_INVALID_ARG
    assert call(1, FLOOR, 0, acc=no_feat) == hrt.ERR_STATE and call(0, FLOOR, 0, acc=no_feat) == hrt.ERR_STATE
    assert not out.any()
    for x, (sums, px) in state.items():
        assert np.array_equal(u32(x.download()[0]), u32(sums)) and np.array_equal(u32(x.resolve()), u32(px))
    assert call(1, FLOOR, 0) == hrt.OK and out.any()
    for x in every:
        x.close()


# ------------------------------------------------------------------------------------------ 4. the C example
@pytest.mark.gpu
def test_demod_example_writes_the_library_frames(scene, tmp_path):
    """examples/render_demod.c at 48x40, two passes of 8 spp and a 16-sample feature pass: the three PFMs are the
    Python binding's."""
    exe = str(tmp_path / "render_demod")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_demod.c"), "-o", exe,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    paths = [tmp_path / n for n in ("plain.pfm", "guided.pfm", "demod.pfm")]
    r = subprocess.run([exe, "48", "40", "8", "2", "16", *[str(p) for p in paths]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "16 spp and 16 feature samples" in r.stdout
    w, h = 48, 40
    a = hrt.Accumulator(scene, w, h, noise=True, features=True)
    cam = hrt.preset_camera(scene.info, w, h)
    for k in range(2):
        a.add(cam, hrt.params(w, h, 8, 50, 1, tuple(scene.info.background), sample_offset=8 * k))
    a.add_features(cam, hrt.params(w, h, 16, 50, 1, tuple(scene.info.background)))
    want = a.resolve(), a.resolve_guided(guide=TOL), a.resolve_guided(guide=dict(normal=0.05, albedo=0.2, depth=0.2), demodulate=0.01)
    assert not np.array_equal(want[1], want[2]) and not np.array_equal(want[0], want[2])
    for path, frame in zip(paths, want):
        img = hrt.read_pfm(str(path))
        assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    a.close()
