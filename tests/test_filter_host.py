"""The variance-guided a-trous filter's host arithmetic (csrc/filter.h through hrt.debug_filter(on_device=False))
against the numpy restatement of the contract (tests/filter_restated.py), its invariants, its argument errors and the
Python and C surface.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import tool_env

import filter_restated as R
import hrt

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (33, 9), (64, 36)]


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulps(a, b):
    """The distance of two positive finite f32 arrays in units in the last place."""
    return np.abs(u32(a).astype(np.int64) - u32(b).astype(np.int64))


def raster(w, h, seed=0, absent=True):
    """Random c in [0, 2), v log-uniform in 1e-8 .. 1, and (absent) about 10% absent pixels with garbage contents,
    a whole absent column among them."""
    rng = np.random.default_rng(1000 * w + h + seed)
    r = np.zeros((h, w, 4), F)
    r[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)).astype(F)
    r[..., 3] = (10.0 ** rng.uniform(-8.0, 0.0, (h, w))).astype(F)
    if absent and w * h > 1:
        gone = rng.uniform(size=(h, w)) < 0.08
        gone[:, w // 2] = True
        r[gone, :3] = rng.uniform(-5.0, 5.0, (int(gone.sum()), 3)).astype(F)
        r[gone, 3] = -rng.uniform(0.5, 2.0, int(gone.sum())).astype(F)
    return r


def test_the_restatement_agrees_with_its_scalar_loop():
    """The shifted-plane form and the pixel-by-pixel loop of tests/filter_restated.py: same bits."""
    for w, h in [(1, 1), (5, 3), (9, 7)]:
        r = raster(w, h)
        for it in (1, 2, 3):
            assert np.array_equal(u32(R.filter_raster(r, it, 4.0)), u32(R.filter_raster_loops(r, it, 4.0))), (w, h, it)


@pytest.mark.parametrize("sigma", [0.5, 4.0])
@pytest.mark.parametrize("w,h", SIZES)
def test_host_filter_equals_the_restatement(w, h, sigma):
    r = raster(w, h)
    assert w * h == 1 or ((r[..., 3] < 0).all(axis=0).any() and 0.05 < (r[..., 3] < 0).mean() < 0.3 + 1.0 / w)
    for it in range(1, 6):
        got, want = hrt.debug_filter(r, it, sigma), R.filter_raster(r, it, sigma)
        assert got.shape == want.shape == (h, w, 4) and got.dtype == F
        assert np.array_equal(u32(got), u32(want)), (w, h, it, sigma)
        there = r[..., 3] >= 0
        assert np.isfinite(got[there]).all() and (got[there][:, 3] >= 0).all()
        assert np.array_equal(u32(got[~there]), u32(r[~there]))   # absent pixels come out as they went in


def test_a_constant_image_stays_constant():
    """Any v, absent pixels included: d = 0 at every tap, so the weights are the H products, multiples of 1/256, and
    c' = (sum w c) / (sum w).  The contract rounds after each of the 25 products and sums, so what "constant" can
    mean depends on the constant's significand: with at most 16 significant bits every product (w up to 36/256: 6
    bits) and every partial sum (up to 256/256: 8 bits) is exact and so is the quotient, and the 2-ulp bound holds
    with room.  A constant that fills all 24 bits is rounded at most taps: the restatement and the library agree bit
    for bit there too (test_host_filter_equals_the_restatement) and both are up to 3 ulp off after one iteration on
    the 33x9 raster, which is the contract's summation order, not an error of either."""
    rng = np.random.default_rng(3)
    for w, h in [(5, 3), (33, 9)]:
        r = raster(w, h, absent=True)
        c = (rng.integers(1 << 15, 1 << 16, 3) * 2.0 ** -15).astype(F)   # 16 significant bits, in [1, 2)
        r[..., :3] = c
        there = r[..., 3] >= 0
        for it in (1, 3, 5):
            got = hrt.debug_filter(r, it, 4.0)
            assert ulps(got[there][:, :3], np.broadcast_to(c, got[there][:, :3].shape)).max() <= 2, (w, h, it)


def test_a_noise_free_image_of_distinct_pixels_is_left_alone():
    """v = 0 everywhere and every pair of pixels differs in luminance by more than 1e-3: each neighbour's weight is
    zero (d > 1e-3 / 1e-6 = 1e3), so a pixel is (w c) / w of itself."""
    w, h = 33, 9
    rng = np.random.default_rng(11)
    lum = (np.arange(w * h) * 3e-3 + 0.3).astype(F)
    rng.shuffle(lum)
    split = rng.dirichlet((2.0, 2.0, 2.0), w * h).astype(F)
    r = np.zeros((h, w, 4), F)
    r[..., :3] = (split * lum[:, None]).reshape(h, w, 3)
    l = R.luma(r[..., :3]).reshape(-1)
    assert np.diff(np.sort(l)).min() > 1e-3
    for it in (1, 3, 5):
        got = hrt.debug_filter(r, it, 4.0)
        assert ulps(got[..., :3], r[..., :3]).max() <= 2, it
        assert not got[..., 3].any()


def test_absent_pixels_are_never_read():
    w, h = 33, 9
    r = raster(w, h)
    gone = r[..., 3] < 0
    other = r.copy()
    rng = np.random.default_rng(5)
    other[gone, :3] = rng.uniform(-100.0, 100.0, (int(gone.sum()), 3)).astype(F)
    other[gone, 3] = -rng.uniform(1e-3, 1e3, int(gone.sum())).astype(F)
    ys, xs = np.nonzero(gone)
    other[ys[::3], xs[::3], :3] = np.nan
    for it in (1, 3, 5):
        a, b = hrt.debug_filter(r, it, 4.0), hrt.debug_filter(other, it, 4.0)
        assert np.array_equal(u32(a[~gone]), u32(b[~gone])), it


def _raises(status, fn):
    with pytest.raises(hrt.HrtError) as e:
        fn()
    assert e.value.status == status, e.value


def test_argument_errors():
    r = raster(5, 3)
    for it in (0, 6, 2 ** 31):
        _raises(hrt.ERR_INVALID_ARG, lambda: hrt.debug_filter(r, it, 4.0))
    for sigma in (0.0, -1.0, float("nan")):
        _raises(hrt.ERR_INVALID_ARG, lambda: hrt.debug_filter(r, 3, sigma))
    L = hrt.load()
    out = np.zeros_like(r)
    assert L.hrt_debug_filter(0, None, 5, 3, 1, 4.0, out.ctypes.data) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_filter(0, r.ctypes.data, 5, 3, 1, 4.0, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_filter(0, r.ctypes.data, 0, 3, 1, 4.0, out.ctypes.data) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_filter(0, r.ctypes.data, 5, 65536, 1, 4.0, out.ctypes.data) == hrt.ERR_INVALID_ARG
    assert not out.any()
    # null accumulator, null params: no device needed to refuse them
    f = hrt.filter_params()
    assert L.hrt_accum_resolve_filtered(None, ctypes.byref(f), hrt.ACCUM_F32, out.ctypes.data, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_resolve_filtered_host(None, ctypes.byref(f), hrt.ACCUM_F32, out.ctypes.data) == hrt.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        hrt.debug_filter(np.zeros((3, 5, 3), F), 1, 4.0)


def test_python_signature():
    sig = inspect.signature(hrt.Accumulator.resolve)
    assert list(sig.parameters) == ["self", "fmt", "denoise"]
    assert sig.parameters["fmt"].default == "f32" and sig.parameters["denoise"].default is None
    sig = inspect.signature(hrt.debug_filter)
    assert list(sig.parameters) == ["raster", "iterations", "sigma", "on_device"]
    assert sig.parameters["on_device"].default is False
    f = hrt.filter_params()
    assert (f.iterations, f.sigma) == (3, 4.0)
    f = hrt.filter_params(**dict(sigma=2.5))
    assert (f.iterations, f.sigma) == (3, 2.5)


def test_filter_params_layout_matches_c_and_the_rust_listing(tmp_path):
    """hrt_filter_params in include/hrt/hrt.h, hrt.FilterParams and INTEGRATION.md's Rust declaration: 8 bytes, a u32
    and an f32; HRT_ABI_VERSION stays 6 (no existing struct grew)."""
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt/hrt.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d\\n", sizeof(hrt_filter_params), offsetof(hrt_filter_params, iterations),\n'
                   '         offsetof(hrt_filter_params, sigma), (int)HRT_ABI_VERSION);\n  return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          env=tool_env())
    size, o_it, o_sigma, abi = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert (size, o_it, o_sigma, abi) == (8, 0, 4, 6) and hrt.ABI_VERSION == 6
    assert ctypes.sizeof(hrt.FilterParams) == 8
    assert [(n, t) for n, t in hrt.FilterParams._fields_] == [("iterations", ctypes.c_uint32), ("sigma", ctypes.c_float)]
    assert hrt.FilterParams.sigma.offset == 4
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub struct hrt_filter_params \{ pub iterations: u32, pub sigma: f32 \}", doc)
