"""The accumulator's noise estimate without a GPU: the arithmetic of csrc/accum.h (hrt_debug_noise with
on_device = 0) against a numpy-float32 restatement of the bit contract in include/hrt/hrt.h and of accum_noise's
reduction tree, the estimator's unbiasedness on synthetic samples, and the error codes that need no device."""
import ctypes

import numpy as np
import pytest

import hrt

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def luma(s):
    return ((s[..., 0] + s[..., 1]).astype(F) + s[..., 2]).astype(F)


def restate_pass(partial, sizes, acc, m2):
    """acc + pass_sum and m2 + pass_moment: chunk sums and chunk terms in chunk order from chunk 0's, ONE addend each."""
    s = partial[0, :, :3].astype(F)
    mom = ((luma(partial[0]) * luma(partial[0])).astype(F) * (F(1) / F(sizes[0]))).astype(F)
    for c in range(1, partial.shape[0]):
        s = (s + partial[c, :, :3]).astype(F)
        y = luma(partial[c])
        mom = (mom + ((y * y).astype(F) * (F(1) / F(sizes[c]))).astype(F)).astype(F)
    out = np.zeros((partial.shape[1], 4), F)
    out[:, :3] = (acc[:, :3] + s).astype(F)
    return out, (m2 + mom).astype(F)


def restate_err(acc, m2, samples, chunks, floor):
    n = len(acc)
    if chunks < 2:
        return np.full(n, np.inf, F)
    inv_n, inv_k1 = F(1) / F(samples), F(1) / F(chunks - 1)
    y = luma(acc)
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((m2 - ((y * y).astype(F) * inv_n).astype(F)).astype(F) * inv_k1).astype(F)
        var = np.where(v > F(0), v, F(0)).astype(F)
        mean = (y * inv_n).astype(F)
        den = np.where(mean > F(floor), mean, F(floor)).astype(F)
        return (np.sqrt((var * inv_n).astype(F)).astype(F) / den).astype(F)


def restate_reduce(err):
    """Thread j of 256 folds pixels j, j + 256, ... in order from 0; then x[j] = x[j] (op) x[j + s], s = 128 ... 1."""
    n = len(err)
    xs, xm = np.zeros(256, F), np.zeros(256, F)
    for k0 in range(0, n, 256):
        row = np.zeros(256, F)
        m = min(256, n - k0)
        row[:m] = err[k0:k0 + m]
        live = np.arange(256) < m
        xs = np.where(live, (xs + row).astype(F), xs)
        xm = np.where(live & (row > xm), row, xm)
    s = 128
    while s >= 1:
        xs[:s] = (xs[:s] + xs[s:2 * s]).astype(F)
        xm[:s] = np.where(xm[s:2 * s] > xm[:s], xm[s:2 * s], xm[:s])
        s //= 2
    return (xs[0] * (F(1) / F(n))).astype(F), xm[0]


SIZES = {1: [16], 2: [8, 32], 3: [8, 16, 16], 11: [8, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]}


def synthetic_pass(rng, sizes, n, scale=1.0):
    """Chunk sums of n pixels whose per-sample value is ~ U(0, scale) per channel: sums grow with the chunk size."""
    p = np.zeros((len(sizes), n, 4), F)
    for c, nc in enumerate(sizes):
        p[c, :, :3] = (rng.uniform(0.2, 1.0, (n, 3)) * scale * nc).astype(F)
    return p


@pytest.mark.parametrize("n_chunks", [1, 2, 3, 11])
@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 6400])
def test_host_noise_matches_restatement(n_chunks, n):
    rng = np.random.default_rng(100 * n + n_chunks)
    sizes = SIZES[n_chunks]
    floor = 0.05
    p1 = synthetic_pass(rng, sizes, n)
    p1[0, 0, :3] = 0.0   # pixel 0 of chunk 0 contributes nothing
    zero, zero_m = np.zeros((n, 4), F), np.zeros(n, F)
    N1, K1 = sum(sizes), n_chunks
    acc, m2, err, mean, mx = hrt.debug_noise(p1, sizes, zero, zero_m, N1, K1, floor)
    want_acc, want_m2 = restate_pass(p1, sizes, zero, zero_m)
    assert np.array_equal(bits(acc), bits(want_acc)) and np.array_equal(bits(m2), bits(want_m2))
    want_err = restate_err(want_acc, want_m2, N1, K1, floor)
    assert np.array_equal(bits(err), bits(want_err))
    wm, wx = restate_reduce(want_err)
    assert bits(mean) == bits(wm) and bits(mx) == bits(wx)
    if n_chunks == 1:   # K = 1: no estimate, and +inf propagates into both figures
        assert np.isinf(err).all() and np.isinf(mean) and np.isinf(mx)
    else:
        assert np.isfinite(err).all() and (err >= 0).all() and mx == err.max()
    # a second pass with another schedule into the state of the first: the moment is one addend
    sizes2 = SIZES[3] if n_chunks != 3 else SIZES[11]
    p2 = synthetic_pass(rng, sizes2, n, 0.5)
    N2, K2 = N1 + sum(sizes2), K1 + len(sizes2)
    acc2, m22, err2, mean2, mx2 = hrt.debug_noise(p2, sizes2, acc, m2, N2, K2, floor)
    want_acc2, want_m22 = restate_pass(p2, sizes2, want_acc, want_m2)
    assert np.array_equal(bits(acc2), bits(want_acc2)) and np.array_equal(bits(m22), bits(want_m22))
    want_err2 = restate_err(want_acc2, want_m22, N2, K2, floor)
    assert np.array_equal(bits(err2), bits(want_err2))
    wm2, wx2 = restate_reduce(want_err2)
    assert bits(mean2) == bits(wm2) and bits(mx2) == bits(wx2)
    assert np.isfinite(err2).all() and err2.max() > 0


def test_black_constant_and_dark_pixels():
    sizes = [8, 16, 16]
    p = np.zeros((3, 4, 4), F)
    for c, nc in enumerate(sizes):
        p[c, 1, :3] = np.array([0.25, 0.5, 0.25], F) * nc      # every sample has value 1: no variance
        p[c, 2, :3] = np.array([0.001, 0.001, 0.001], F) * nc * (1 + c)  # a dark pixel, below the floor
        p[c, 3, :3] = np.array([1.0, 2.0, 3.0], F) * nc * (1 + c)
    acc, m2, err, mean, mx = hrt.debug_noise(p, sizes, np.zeros((4, 4), F), np.zeros(4, F), 40, 3, 0.05)
    assert err[0] == 0 and bits(err[:1])[0] == 0     # black: Y = 0 -> 0 / floor = +0
    assert m2[1] == 40 and err[1] == 0               # constant: m2 = Y^2 / N exactly
    assert err[2] > 0 and err[3] > 0
    # the dark pixel is measured against the floor, the bright one against its own mean
    small, _ = restate_pass(p, sizes, np.zeros((4, 4), F), np.zeros(4, F))
    lo = hrt.debug_noise(p, sizes, np.zeros((4, 4), F), np.zeros(4, F), 40, 3, 0.5)[2]
    assert np.isclose(lo[2], err[2] / 10, rtol=1e-5) and lo[3] == err[3]
    assert luma(small)[2] / 40 < 0.05 < luma(small)[3] / 40


def chunk_sizes(sched):
    """The samples of every chunk of a schedule (hrt.sample_chunks): the first head chunk, the others, the halving tail."""
    c = sched["chunk"]
    return [sched["first"]] + [c] * (sched["head"] - 1) + [c >> (1 + (j >> 1)) for j in range(sched["tail"])]


def test_schedules_of_the_test_inputs():
    """The chunk sizes the GPU tests' passes are summed in (tests/test_gpu_accum_noise.py builds the oracle's chunk
    sums from these)."""
    rnd, cor = hrt.preset("random", 1), hrt.preset("cornell", 1)
    def sizes(s, w, h, spp):
        return chunk_sizes(hrt.sample_chunks(s, hrt.params(w, h, spp)))
    assert sizes(rnd, 64, 36, 40) == [8, 16, 16]
    assert sizes(rnd, 64, 36, 70) == [8, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
    assert sizes(rnd, 64, 36, 16) == [16]
    assert sizes(cor, 32, 32, 40) == [8, 32]
    assert sizes(cor, 32, 32, 70) == [6, 32, 32]
    rnd.close()
    cor.close()


def test_estimator_is_unbiased():
    """4096 pixels of i.i.d. normal samples (mu = 1, sigma = 0.5 per channel) summed into the 500-spp schedule's 38
    chunks of unequal sizes: the mean of var over the pixels is the variance of one sample's value, 3 * 0.25, within
    2% (~5 standard deviations: one pixel's estimate has relative spread sqrt(2 / 37) = 0.23, and 0.23 / 64 = 0.0036)."""
    s = hrt.preset("random", 1)
    sizes = chunk_sizes(hrt.sample_chunks(s, hrt.params(64, 36, 500)))
    s.close()
    assert len(sizes) == 38 and sum(sizes) == 500 and len(set(sizes)) > 3
    n = 4096
    x = np.random.default_rng(0).normal(1.0, 0.5, (n, 500, 3))
    partial = np.zeros((38, n, 4), F)
    at = 0
    for c, nc in enumerate(sizes):
        partial[c, :, :3] = x[:, at:at + nc].sum(axis=1).astype(F)
        at += nc
    acc, m2, err, mean, mx = hrt.debug_noise(partial, sizes, np.zeros((n, 4), F), np.zeros(n, F), 500, 38, 0.05)
    y_mean = acc[:, :3].astype(np.float64).sum(axis=1) / 500
    assert (y_mean > 0.05).all()
    var = (err.astype(np.float64) * y_mean) ** 2 * 500      # err = sqrt(var / N) / mean
    assert abs(var.mean() / 0.75 - 1) <= 0.02, var.mean()
    # and err is the relative standard error of the pixel's mean: sigma_Y / sqrt(N) / mu_Y
    assert abs(float(mean) / (np.sqrt(0.75 / 500) / 3.0) - 1) <= 0.02


def test_errors_without_a_device():
    L = hrt.load()
    p = synthetic_pass(np.random.default_rng(1), [8, 8], 4)
    z, zm = np.zeros((4, 4), F), np.zeros(4, F)
    for floor in (0.0, -1.0, float("nan")):
        with pytest.raises(hrt.HrtError) as e:
            hrt.debug_noise(p, [8, 8], z, zm, 16, 2, floor)
        assert e.value.status == hrt.ERR_INVALID_ARG
    with pytest.raises(hrt.HrtError) as e:
        hrt.debug_noise(p, [8, 0], z, zm, 16, 2)     # an empty chunk
    assert e.value.status == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_noise(0, None, None, 1, 1, None, None, 1, 1, 0.05, None, None) == hrt.ERR_INVALID_ARG
    # null handles
    rec = (hrt.TileNoise * 1)()
    n = ctypes.c_uint64()
    idx = (ctypes.c_uint32 * 1)(0)
    assert L.hrt_accum_noise(None, 0.05, None, None, ctypes.cast(rec, ctypes.c_void_p)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_tile_samples(None, ctypes.byref(n)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_add_tiles(None, None, None, ctypes.cast(idx, ctypes.c_void_p), 1, None, None) == hrt.ERR_INVALID_ARG
    assert L.hrt_debug_accum_moments(None, None) == hrt.ERR_INVALID_ARG
    # create_ex: the checks of hrt_accum_create, and unknown flags
    s = hrt.preset("two_spheres", 1)   # not committed
    out = ctypes.c_void_p()
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, 16, 16))
    tp = ctypes.cast(tile, ctypes.c_void_p)
    assert L.hrt_accum_create_ex(s.h, 16, 16, tp, 1, hrt.ACCUM_NOISE, ctypes.byref(out)) == hrt.ERR_STATE
    assert not out.value
    assert L.hrt_accum_create_ex(s.h, 16, 16, tp, 1, 2, ctypes.byref(out)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_create_ex(s.h, 16, 16, tp, 0, hrt.ACCUM_NOISE, ctypes.byref(out)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_create_ex(None, 16, 16, tp, 1, 0, ctypes.byref(out)) == hrt.ERR_INVALID_ARG
    with pytest.raises(hrt.HrtError) as e:
        hrt.Accumulator(s, 16, 16, noise=True)
    assert e.value.status == hrt.ERR_STATE
    s.close()


def test_tile_noise_record_layout(tmp_path):
    """hrt_tile_noise in C (compiled with gcc), in the Python binding and in INTEGRATION.md's Rust declaration: the
    same fields at the same offsets, 24 bytes."""
    import os
    import re
    import subprocess

    from conftest import ROOT, tool_env

    fields = ["mean", "max", "samples", "chunks"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hrt/hrt.h"', "int main(void) {",
             '  printf("%zu", sizeof(hrt_tile_noise));']
    lines += [f'  printf(" %zu", offsetof(hrt_tile_noise, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], env=tool_env())
    size, *offs = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert size == 24 and offs == [0, 4, 8, 16]
    assert ctypes.sizeof(hrt.TileNoise) == size
    assert [f for f, _ in hrt.TileNoise._fields_] == fields
    assert [getattr(hrt.TileNoise, f).offset for f in fields] == offs
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"#\[repr\(C\)\][^\n]*\npub struct hrt_tile_noise \{(.*?)\}", doc)
    assert m, "INTEGRATION.md declares hrt_tile_noise"
    rust = [tuple(x.strip() for x in part.replace("pub ", "").split(":")) for part in m.group(1).split(",")]
    assert rust == [("mean", "f32"), ("max", "f32"), ("samples", "u64"), ("chunks", "u64")]
