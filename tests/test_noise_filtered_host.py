"""The filtered noise estimate's arithmetic on the host (hrt_debug_noise_filtered with on_device = 0; include/hrt/hrt.h,
"noise estimate of the FILTERED frame") against the numpy restatement (tests/noise_filtered_restated.py), bit for bit;
its calibration on a synthetic flat field; and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import filter_restated as FR
import hrt
import noise_filtered_restated as NF

F = np.float32
FLOOR = 0.05
DEMOD_FLOOR = 0.01
ALL = dict(kn=2.0, ka=10.0, kz=10.0)
# (width, height, tiles): 37x23 with ragged tiles and gaps; 1xN both ways; a 257-pixel tile, whose fold wraps once
CASES = {
    "37x23": (37, 23, [(0, 0, 20, 23), (20, 0, 17, 10), (22, 12, 13, 9)]),
    "1xN": (1, 41, [(0, 3, 1, 30)]),
    "Nx1": (41, 1, [(2, 0, 17, 1), (19, 0, 20, 1)]),
    "257": (260, 3, [(0, 0, 257, 1), (0, 1, 260, 2)]),
}


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rasters(w, h, tiles):
    """gather's (c, v) of a textured raster with the feature planes of tests/test_demod_host.py (their special albedos
    included), every pixel of `tiles` present and a random half of the others absent."""
    rng = np.random.default_rng(77 * w + h)
    if w >= 15 and h >= 5:
        import test_demod_host as TD

        r, a, n = TD.rasters(w, h)
    else:  # a strip: blocky albedo, noisy normals and depths, and the special albedos along it
        k = (np.arange(w)[None, :] + np.arange(h)[:, None]) // 5 % 3
        a, n = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
        a[..., :3] = np.abs(np.array([[0.2, 0.3, 0.1], [0.9, 0.9, 0.9], [0.6, 0.05, 0.4]])[k] + rng.normal(0, 0.02, (h, w, 3))).astype(F)
        n[..., :3] = (np.eye(3)[k] + rng.normal(0, 0.1, (h, w, 3))).astype(F)
        n[..., 3] = (np.array([1.0, 5.0, 20.0])[k] * rng.uniform(0.9, 1.1, (h, w))).astype(F)
        r = np.zeros((h, w, 4), F)
        r[..., :3] = (a[..., :3] * rng.uniform(0.3, 0.7, (h, w, 1))).astype(F)
        r[..., 3] = F(-1)
        flat_a, flat_r = a.reshape(-1, 4), r.reshape(-1, 4)
        flat_a[5, 0], flat_a[7, 1], flat_a[9, :3], flat_r[9, :3], flat_a[11, :3] = F(0), F("nan"), F(0), F(0), F(0.002)
    inside = np.zeros((h, w), bool)
    for x, y, tw, th in tiles:
        inside[y:y + th, x:x + tw] = True
    v = (10.0 ** rng.uniform(-6.0, -2.0, (h, w))).astype(F)
    r[..., 3] = np.where(r[..., 3] < 0, v, r[..., 3])
    r[~inside & (rng.uniform(size=(h, w)) < 0.5), 3] = F(-1)
    return r, a, n


def both(r, a, n, tiles, it, sigma=4.0, floor=FLOOR, demod=None, on_device=False, **k):
    got = hrt.debug_noise_filtered(r, a, n, it, sigma, tiles, demodulate=demod if demod else False, floor=floor,
                                   on_device=on_device, **k)
    want = NF.noise_filtered(r, a, n, tiles, it, sigma, floor, demod_floor=demod, **k)
    return got, want


def same(got, want, what):
    assert got[0].dtype == F and got[1].dtype == F
    assert np.array_equal(u32(got[0]), u32(want[0])), what
    assert np.array_equal(u32(got[1]), u32(want[1])), what


# ------------------------------------------------------------------------------------------ 1. host against restatement
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("it", [1, 3, 5])
def test_host_equals_the_restatement(case, it):
    w, h, tiles = CASES[case]
    r, a, n = rasters(w, h, tiles)
    for k in (dict(), ALL, dict(kn=2.0), dict(ka=10.0), dict(kz=10.0)):
        for demod in (None, DEMOD_FLOOR):
            same(*both(r, a, n, tiles, it, demod=demod, **k), (case, it, k, demod))
    # the variance-only filter reads no feature raster
    same(hrt.debug_noise_filtered(r, None, None, it, 4.0, tiles, floor=FLOOR), NF.noise_filtered(r, None, None, tiles, it, 4.0, FLOOR),
         (case, it, "no rasters"))


def test_reduce_restated_is_the_scalar_fold():
    """The restatement's vectorised tile_reduce against the contract's scalar loops, NaN and +inf included."""
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 700):
        e = rng.uniform(0, 1, n).astype(F)
        if n == 700:
            e[300], e[10] = F("inf"), F("nan")
        xs, xm = np.zeros(256, F), np.zeros(256, F)
        with np.errstate(all="ignore"):
            for j in range(256):
                for k in range(j, n, 256):
                    xs[j] = xs[j] + e[k]
                    xm[j] = e[k] if e[k] > xm[j] else xm[j]
            s = 128
            while s >= 1:
                for j in range(s):
                    xs[j] = xs[j] + xs[j + s]
                    xm[j] = xm[j + s] if xm[j + s] > xm[j] else xm[j]
                s >>= 1
            want = (xs[0] * (F(1) / F(n)), xm[0])
        got = NF.tile_reduce(e)
        assert np.array_equal(u32(got), u32(want)), n


def test_a_black_pixel_is_measured_against_the_floor():
    """A lone black pixel (every neighbour absent): c' = c = 0, so l' = 0 and err = sqrtf(v) / floor; with demodulation
    l_d = 0 gives gr = 0, so err = 0."""
    r = np.zeros((9, 9, 4), F)
    r[..., 3] = -1
    r[4, 4] = (0, 0, 0, 4e-4)
    a, n = np.full((9, 9, 4), 0.5, F), np.ones((9, 9, 4), F)
    tiles = [(4, 4, 1, 1)]
    for it in (1, 3):
        got, want = both(r, a, n, tiles, it)
        same(got, want, it)
        # v' = ((w * w) * v) / (w * w) is v up to its two roundings, and a 1-pixel tile's mean and max are its err
        assert np.isclose(got[0][0], np.sqrt(4e-4) / FLOOR, rtol=1e-6, atol=0) and got[1][0, 0] == got[0][0] == got[1][0, 1]
        got, want = both(r, a, n, tiles, it, demod=DEMOD_FLOOR, **ALL)
        same(got, want, it)
        assert got[0][0] == 0
    # a black 9x9 field under one 5x5 iteration: the centre's taps are all black
    r[..., :3], r[..., 3] = 0, 1e-4
    got, want = both(r, a, n, [(0, 0, 9, 9)], 1)
    same(got, want, "field")
    assert got[0][4 * 9 + 4] > 0 and np.isfinite(got[0]).all()


# ------------------------------------------------------------------------------------------ 2. calibration
SIZE, CHUNKS, LEVEL, SD, SEEDS = 64, 8, 0.6, 0.3, 8


def flat_field(seed):
    """gather's raster of a flat grey field: every pixel's luminance is LEVEL, its CHUNKS chunk means carry iid normal
    noise of standard deviation SD; c is their mean (a third per channel) and v the sample variance of the mean."""
    rng = np.random.default_rng(seed)
    y = LEVEL + SD * rng.standard_normal((CHUNKS, SIZE, SIZE))
    mean, var = y.mean(0), y.var(0, ddof=1) / CHUNKS
    r = np.zeros((SIZE, SIZE, 4), F)
    r[..., :3] = (mean / 3)[..., None]
    r[..., 3] = var
    return r


def calibration(frame, err):
    """The empirical RMS relative error of the filtered frame's luminance over the mean predicted err."""
    l = FR.luma(frame[..., :3].astype(np.float64))
    return float(np.sqrt(np.mean(((l - LEVEL) / LEVEL) ** 2)) / np.mean(err.astype(np.float64)))


def test_calibration_on_a_flat_field():
    """The band comes from the numpy restatement over SEEDS seeds, widened by their standard deviation; the library's
    mean ratio over SEEDS other seeds must lie inside it, and on the same seeds the library's ratio is the restatement's.
    Measured (3 iterations, sigma 4, 64x64, K = 8): see DESIGN.md section 6.11."""
    tiles = [(0, 0, SIZE, SIZE)]
    ref = []
    for seed in range(SEEDS):
        r = flat_field(seed)
        err, _ = NF.noise_filtered(r, None, None, tiles, 3, 4.0, FLOOR)
        ref.append(calibration(FR.filter_raster(r, 3, 4.0), err))
        lib_err, _ = hrt.debug_noise_filtered(r, None, None, 3, 4.0, tiles, floor=FLOOR)
        assert calibration(hrt.debug_filter(r, 3, 4.0), lib_err) == ref[-1]
    lo, hi = min(ref) - np.std(ref), max(ref) + np.std(ref)
    lib = []
    for seed in range(100, 100 + SEEDS):
        r = flat_field(seed)
        err, _ = hrt.debug_noise_filtered(r, None, None, 3, 4.0, tiles, floor=FLOOR)
        lib.append(calibration(hrt.debug_filter(r, 3, 4.0), err))
    print("calibration: restatement", np.round(ref, 4), "band", round(lo, 4), round(hi, 4), "library", np.round(lib, 4),
          "mean", round(float(np.mean(lib)), 4))
    assert lo <= np.mean(lib) <= hi


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing():
    w, h, tiles = CASES["37x23"]
    r, a, n = rasters(w, h, tiles)
    L = hrt.load()
    npx = sum(t[2] * t[3] for t in tiles)
    err, mm = np.full(npx, 7, F), np.full((len(tiles), 2), 7, F)

    def call(raster=r, albedo=a, normal=n, width=w, height=h, it=3, sigma=4.0, kn=2.0, ka=10.0, kz=10.0, flags=0, afloor=0.0,
             floor=FLOOR, tl=tiles, nt=None, e=err, m=mm):
        arr = None if tl is None else (hrt.Tile * max(1, len(tl)))(*[hrt.Tile(*t) for t in tl])
        p = lambda x: None if x is None else x.ctypes.data
        return L.hrt_debug_noise_filtered(0, p(raster), p(albedo), p(normal), width, height, it, sigma, kn, ka, kz, flags, afloor, floor,
                                          ctypes.cast(arr, ctypes.c_void_p) if tl is not None else None, nt if nt is not None else len(tl),
                                          p(e), p(m))

    absent = tuple(int(v) for v in np.argwhere(r[..., 3] < 0)[0])
    bad = [dict(raster=None), dict(tl=None, nt=1), dict(nt=0), dict(e=None), dict(m=None), dict(width=0), dict(height=0), dict(width=65536),
           dict(it=0), dict(it=6), dict(sigma=0.0), dict(sigma=float("nan")), dict(kn=-1.0), dict(ka=float("nan")), dict(kz=-0.5),
           dict(flags=2), dict(flags=3), dict(flags=1, afloor=0.0), dict(flags=1, afloor=float("nan")),
           dict(floor=0.0), dict(floor=-0.05), dict(floor=float("nan")),
           dict(albedo=None), dict(normal=None), dict(albedo=None, normal=None, kn=0.0, ka=0.0, kz=0.0, flags=1, afloor=DEMOD_FLOOR),
           dict(tl=[(0, 0, 38, 23)]), dict(tl=[(36, 0, 2, 1)]), dict(tl=[(0, 22, 1, 2)]), dict(tl=[(37, 0, 1, 1)]), dict(tl=[(0, 0, 0, 1)]),
           dict(tl=[(0, 0, 0xFFFFFFFF, 2)]), dict(tl=[(0, 0, 20, 23), (19, 0, 2, 2)]), dict(tl=[(absent[1], absent[0], 1, 1)])]
    for kw in bad:
        assert call(**kw) == hrt.ERR_INVALID_ARG, kw
        assert (err == 7).all() and (mm == 7).all(), kw
    # the accumulator entry without an accumulator, a parameter block or records
    g = hrt.guided_ex_params(demodulate=False)
    rec = (hrt.TileNoise * 1)()
    rec[0].mean, rec[0].samples = 7.0, 7
    assert L.hrt_accum_noise_filtered(None, ctypes.byref(g), FLOOR, None, None, ctypes.cast(rec, ctypes.c_void_p)) == hrt.ERR_INVALID_ARG
    assert rec[0].mean == 7.0 and rec[0].samples == 7
    # and the same arguments are accepted once they are right
    assert call() == hrt.OK and call(albedo=None, normal=None, kn=0.0, ka=0.0, kz=0.0) == hrt.OK
    assert not (err == 7).any() and not (mm == 7).any()
