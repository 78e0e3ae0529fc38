"""The demodulated guided filter's arithmetic (csrc/filter.h through hrt_debug_guided_ex on the host) against the
independent numpy restatement (tests/demod_restated.py), without a GPU: "THE BIT CONTRACT of the demodulated frame" of
include/hrt/hrt.h, the new struct's layout, the argument errors, and that demodulation helps where it should."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from conftest import tool_env

import demod_restated as D
import guided_restated as R
import hrt

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 0.01
SHAPES = [(70, 21), (33, 9)]   # no multiples of the 32 x 8 block, more than one block each way
TERMS = [dict(), dict(ka=10.0), dict(kn=2.0, ka=10.0, kz=10.0)]


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rasters(w, h):
    """gather's (c, v) of a textured raster: irradiance times a blocky albedo, with absent pixels (a column, scattered
    ones and one fully absent row), and albedo planes that hold every special value of the contract: a 0 channel (the
    floor engages), -0.0, an emitter's 15, NaN, and c = 0 where a = 0."""
    rng = np.random.default_rng(1000 * w + h)
    region = (np.arange(w)[None, :] // 5 + np.arange(h)[:, None] // 3) % 3
    base_a = np.array([[0.2, 0.3, 0.1], [0.9, 0.9, 0.9], [0.6, 0.05, 0.4]])
    a, n = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    a[..., :3] = np.abs(base_a[region] + rng.normal(0, 0.02, (h, w, 3))).astype(F)
    a[..., 3] = rng.uniform(0, 1, (h, w)).astype(F)
    base_n = rng.normal(size=(3, 3))
    base_n /= np.linalg.norm(base_n, axis=1, keepdims=True)
    n[..., :3] = (base_n[region] + rng.normal(0, 0.1, (h, w, 3))).astype(F)
    n[..., 3] = (np.array([1.0, 5.0, 20.0])[region] * rng.uniform(0.9, 1.1, (h, w))).astype(F)
    r = np.zeros((h, w, 4), F)
    r[..., :3] = (a[..., :3] * rng.uniform(0.3, 0.7, (h, w, 1))).astype(F)
    r[..., 3] = (10.0 ** rng.uniform(-6.0, -2.0, (h, w))).astype(F)
    # the special albedos, each at a present pixel away from the absent ones below
    a[1, 2, 0] = F(0)                      # one channel 0: the floor divides it
    a[1, 4, :3] = F(-0.0)
    a[2, 6, :3] = F(15)                    # an emitter
    r[2, 6, :3] = F(15) * F(0.5)
    a[2, 8, 1] = F("nan")                  # a NaN channel gives the floor
    a[3, 10, :3], r[3, 10, :3] = F(0), F(0)  # c = 0 with a = 0: l = 0, so g = 0
    a[3, 12, :3] = F(0.002)                # below the floor
    gone = rng.uniform(size=(h, w)) < 0.06
    gone[:4, :14] = False
    gone[:, w // 2] = True
    gone[h - 2, :] = True                  # a fully absent row
    r[gone, :3] = rng.uniform(-5.0, 5.0, (int(gone.sum()), 3)).astype(F)
    r[gone, 3] = -rng.uniform(0.5, 2.0, int(gone.sum())).astype(F)
    a[gone, :3] = F("nan")                 # read at present pixels only
    return r, a, n


@pytest.mark.parametrize("w,h", SHAPES)
def test_host_demodulated_equals_the_restatement(w, h):
    r, a, n = rasters(w, h)
    gone = r[..., 3] < 0
    for k in TERMS:
        for it in (1, 2, 3, 4, 5):
            got = hrt.debug_guided(r, a, n, it, 4.0, demodulate=FLOOR, **k)
            want = D.demod_raster(r, a, n, it, 4.0, FLOOR, **k)
            assert np.array_equal(u32(got), u32(want)), (w, h, k, it)
            assert np.array_equal(u32(got[gone]), u32(r[gone])), "an absent pixel comes out as it went in"
            assert not np.array_equal(u32(got), u32(hrt.debug_guided(r, a, n, it, 4.0, **k))), "the flag changed nothing"
    # another floor is another frame, and the floor's pixels are the ones that differ
    lo, hi = (hrt.debug_guided(r, a, n, 2, 4.0, demodulate=f) for f in (0.003, 0.03))
    assert np.array_equal(u32(hi), u32(D.demod_raster(r, a, n, 2, 4.0, 0.03))) and not np.array_equal(u32(lo), u32(hi))


def test_special_albedos_follow_the_contract():
    """The restatement's steps 1 and 2 on single pixels, written out from the contract."""
    r, a, _ = rasters(33, 9)
    m = D.divisor(a, FLOOR)
    assert m[1, 2, 0] == F(FLOOR) and (m[1, 4] == F(FLOOR)).all() and (m[2, 6] == F(15)).all()
    assert m[2, 8, 1] == F(FLOOR) and (m[3, 12] == F(FLOOR)).all()
    d = D.demodulate(r, m)
    assert (d[3, 10, :3] == 0).all() and d[3, 10, 3] == 0          # l = 0: g = 0
    assert (d[2, 6, :3] == F(0.5)).all()
    c, v, mm = r[1, 2], r[1, 2, 3], m[1, 2]
    dc = np.array([c[0] / mm[0], c[1] / mm[1], c[2] / mm[2]], F)
    g = ((dc[0] + dc[1]) + dc[2]) / ((c[0] + c[1]) + c[2])
    assert np.array_equal(u32(d[1, 2]), u32(np.array([*dc, v * (g * g)], F)))


def test_a_grey_albedo_is_exact_and_flat_irradiance_stays_flat():
    """A power-of-two grey albedo commutes with every rounding: demodulated variance-only filtering of a * c is a times
    the filter of c.  And a constant irradiance under any texture comes back as the texture times that constant."""
    r, a, n = rasters(33, 9)
    a[..., :3] = F(0.25)
    r[3, 10, :3] = F(0.125)    # every present pixel has l > 0
    plain = hrt.debug_guided(r, a, n, 3, 4.0)
    scaled = r.copy()
    scaled[..., :3] *= F(4)
    scaled[..., 3] = np.where(r[..., 3] < 0, r[..., 3], r[..., 3] * F(16))
    want = hrt.debug_guided(scaled, a, n, 3, 4.0)
    got = hrt.debug_guided(r, a, n, 3, 4.0, demodulate=FLOOR)
    there = ~(r[..., 3] < 0)
    assert np.array_equal(u32(got[there][:, :3]), u32(want[there][:, :3] * F(0.25)))
    assert np.array_equal(u32(got[there][:, 3]), u32(want[there][:, 3])) and not np.array_equal(u32(got), u32(plain))
    r2, a2, n2 = rasters(70, 21)
    a2 = np.where(a2 == a2, a2, F(0.5)).astype(F)
    a2[..., :3] = np.where(a2[..., :3] > F(0.0625), a2[..., :3], F(0.0625))
    r2[..., :3], r2[..., 3] = a2[..., :3] * F(0.5), F(1e-4)
    out = hrt.debug_guided(r2, a2, n2, 3, 4.0, demodulate=FLOOR)
    assert np.allclose(out[..., :3], r2[..., :3], rtol=1e-6, atol=0)


@pytest.mark.parametrize("w,h", SHAPES)
def test_flags_zero_is_the_guided_filter(w, h):
    r, a, n = rasters(w, h)
    L = hrt.load()
    for k in ((0.0, 0.0, 0.0), (2.0, 10.0, 10.0)):
        for it in (1, 3, 5):
            out = np.zeros_like(r)
            # the floor is not read when the flag is clear
            for floor in (0.0, float("nan"), 0.5):
                out[:] = 0
                st = L.hrt_debug_guided_ex(0, r.ctypes.data, a.ctypes.data, n.ctypes.data, w, h, it, 4.0, *k, 0, floor, out.ctypes.data)
                assert st == hrt.OK
                assert np.array_equal(u32(out), u32(hrt.debug_guided(r, a, n, it, 4.0, *k)))
                assert np.array_equal(u32(out), u32(R.guided_raster(r, a, n, it, 4.0, *k)))


def test_argument_errors():
    r, a, n = rasters(33, 9)
    L = hrt.load()
    out = np.zeros_like(r)

    def call(flags, floor, it=3, sigma=4.0, ka=0.0):
        return L.hrt_debug_guided_ex(0, r.ctypes.data, a.ctypes.data, n.ctypes.data, 33, 9, it, sigma, 0.0, ka, 0.0, flags, floor,
                                     out.ctypes.data)

    assert call(hrt.GUIDED_DEMODULATE, FLOOR) == hrt.OK and out.any()
    out[:] = 0
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert call(flags, FLOOR) == hrt.ERR_INVALID_ARG, flags
    for floor in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
        assert call(hrt.GUIDED_DEMODULATE, floor) == hrt.ERR_INVALID_ARG, floor
    assert call(hrt.GUIDED_DEMODULATE, FLOOR, it=0) == hrt.ERR_INVALID_ARG
    assert call(hrt.GUIDED_DEMODULATE, FLOOR, it=6) == hrt.ERR_INVALID_ARG
    assert call(hrt.GUIDED_DEMODULATE, FLOOR, sigma=0.0) == hrt.ERR_INVALID_ARG
    assert call(hrt.GUIDED_DEMODULATE, FLOOR, ka=-1.0) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_guided_ex(0, r.ctypes.data, None, n.ctypes.data, 33, 9, 3, 4.0, 0.0, 0.0, 0.0, 1, FLOOR, out.ctypes.data) \
        == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_guided_ex(0, r.ctypes.data, a.ctypes.data, n.ctypes.data, 33, 9, 3, 4.0, 0.0, 0.0, 0.0, 1, FLOOR, None) \
        == hrt.ERR_INVALID_ARG
    assert not out.any(), "an error writes nothing"
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(hrt.HrtError) as e:
            hrt.debug_guided(r, a, n, 3, 4.0, demodulate=bad)
        assert e.value.status == hrt.ERR_INVALID_ARG
    # the resolve's own checks come before it looks at the accumulator: a null one is INVALID_ARG, as the guided call's
    g = hrt.guided_ex_params()
    assert L.hrt_accum_resolve_guided_ex_host(None, ctypes.byref(g), hrt.ACCUM_F32, out.ctypes.data) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_resolve_guided_ex(None, ctypes.byref(g), hrt.ACCUM_F32, out.ctypes.data, None) == hrt.ERR_INVALID_ARG


def test_guided_ex_params_layout_and_abi_version(tmp_path):
    """hrt_guided_ex_params in C (compiled with gcc) and in the Python binding: 32 bytes, hrt_guided_params' five fields
    at their offsets, then flags, albedo_floor and reserved; no existing struct grew, so HRT_ABI_VERSION stays 6."""
    fields = ["iterations", "sigma", "normal", "albedo", "depth", "flags", "albedo_floor", "reserved"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt/hrt.h"\nint main(void) {\n'
                   '  printf("%zu %zu %d %d\\n", sizeof(hrt_guided_ex_params), sizeof(hrt_guided_params), (int)HRT_ABI_VERSION,\n'
                   '         (int)HRT_GUIDED_DEMODULATE);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(hrt_guided_ex_params, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          env=tool_env())
    head, *offs = subprocess.check_output([str(exe)], text=True).splitlines()
    assert [int(v) for v in head.split()] == [32, 20, 6, 1]
    assert [int(v) for v in offs] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert ctypes.sizeof(hrt.GuidedExParams) == 32 and ctypes.sizeof(hrt.GuidedParams) == 20
    assert [(nm, getattr(hrt.GuidedExParams, nm).offset) for nm, _ in hrt.GuidedExParams._fields_] == list(zip(fields, range(0, 32, 4)))
    assert [t for _, t in hrt.GuidedExParams._fields_] == [ctypes.c_uint32] + [ctypes.c_float] * 4 + [ctypes.c_uint32, ctypes.c_float,
                                                                                                      ctypes.c_uint32]
    assert hrt.ABI_VERSION == 6 and hrt.load().hrt_abi_version() == 6 and hrt.GUIDED_DEMODULATE == 1
    header = open(os.path.join(ROOT, "include", "hrt", "hrt.h")).read()
    assert "#define HRT_ABI_VERSION 6u" in header and "struct hrt_guided_params { /* 20 bytes */" in header
    assert "struct hrt_guided_ex_params { /* 32 bytes */" in header
    for name in ("hrt_accum_resolve_guided_ex", "hrt_accum_resolve_guided_ex_host", "hrt_debug_guided_ex"):
        assert name in hrt.EXPORTS and name in hrt.OPTIONAL
    g = hrt.guided_ex_params()
    assert (g.iterations, g.sigma, g.flags, g.albedo_floor, g.reserved) == (3, 4.0, 1, F(hrt.DEMOD_FLOOR), 0)
    assert (g.normal, g.albedo, g.depth) == tuple(F(hrt.DEMOD_DEFAULTS[k]) for k in ("normal", "albedo", "depth"))
    g = hrt.guided_ex_params(iterations=5, albedo=0.0, demodulate=0.03)
    assert (g.iterations, g.albedo, g.flags, g.albedo_floor) == (5, 0.0, 1, F(0.03))
    g = hrt.guided_ex_params(demodulate=False)
    assert (g.flags, g.albedo_floor, g.albedo) == (0, 0.0, F(hrt.GUIDED_DEFAULTS["albedo"]))


def checker_raster(seed, w=64, h=48):
    """The issue's synthetic input: an albedo checker of 4-pixel squares in C2's ground colours, irradiance
    0.5 + N(0, 0.05^2) identical in the three channels, v the exact variance of the luminance."""
    rng = np.random.default_rng(seed)
    odd = ((np.arange(w)[None, :] // 4 + np.arange(h)[:, None] // 4) % 2).astype(bool)
    a, n = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    a[..., :3] = np.where(odd[..., None], np.array([0.9, 0.9, 0.9], F), np.array([0.2, 0.3, 0.1], F))
    a[..., 3] = 1
    n[..., :3], n[..., 3] = (F(0), F(1), F(0)), F(10)
    e = (0.5 + rng.normal(0.0, 0.05, (h, w))).astype(F)
    r = np.zeros((h, w, 4), F)
    r[..., :3] = a[..., :3] * e[..., None]
    r[..., 3] = (F(0.05) * ((a[..., 0] + a[..., 1]) + a[..., 2])) ** 2
    return r, a, n, (a[..., :3] * F(0.5)).astype(F)


def display_rmse(c, truth):
    with np.errstate(all="ignore"):
        d = np.sqrt(np.maximum(c[..., :3], 0).astype(np.float64)) - np.sqrt(truth.astype(np.float64))
    return float(np.sqrt(np.mean(d * d)))


def test_demodulation_helps_on_a_noisy_checker():
    """It helps where it should: display-unit RMSE against albedo * 0.5 at 3 iterations, sigma 4, floor 0.01, all
    feature terms off.  The restatement alone gives a ratio of 0.78 for this seed (0.75 to 0.78 over seeds 0 to 3; one
    iteration gives 0.86 to 0.88, which is why that is not the case tested), so 0.85 has margin without being vacuous."""
    r, a, n, truth = checker_raster(0)
    plain = display_rmse(r, truth)
    variance_only = display_rmse(hrt.debug_guided(r, a, n, 3, 4.0), truth)
    demod = display_rmse(hrt.debug_guided(r, a, n, 3, 4.0, demodulate=0.01), truth)
    print(f"checker RMSE: unfiltered {plain:.4f}, variance-only {variance_only:.4f}, demodulated {demod:.4f}, "
          f"ratio {demod / variance_only:.3f}")
    assert demod <= 0.85 * variance_only
    assert demod < plain


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cdemod") / "render_demod")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_demod.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_demod_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count("render_demod") == 2   # built by `all`, removed by `clean`


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_demod_example_fails_loudly_without_a_device(exe, tmp_path):
    """examples/render_demod.c builds warning-free and, without a device, ends with the scene upload's status and
    writes nothing (tests/test_gpu_demod.py runs it on one)."""
    paths = [str(tmp_path / n) for n in ("a.pfm", "b.pfm", "c.pfm")]
    r = subprocess.run([exe, "8", "8", "4", "2", "4", *paths], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not any(os.path.exists(p) for p in paths)
