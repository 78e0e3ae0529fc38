"""An independent restatement of the filtered noise estimate (include/hrt/hrt.h, "noise estimate of the FILTERED frame")
in numpy float32, on top of the filters' restatements (tests/filter_restated.py, guided_restated.py, demod_restated.py),
which are imported as they stand.  It never calls the library.

Here are the err expression of the last iteration's (c', v'), its demodulated form, and the tile reduction of
hrt_accum_noise (thread j of 256 folds pixels j, j + 256, ...; then the halving tree).  A raster is (height, width, 4)
float32 (c.xyz, v), v < 0 an absent pixel; tiles are (x, y, w, h) and cover present pixels only."""
import numpy as np

import demod_restated as D
import filter_restated as FR
import guided_restated as GR
from filter_restated import F, luma

BLOCK = 256


def at_least(x, lo):
    """x > lo ? x : lo, so a NaN x gives lo."""
    with np.errstate(all="ignore"):
        return np.where(x > F(lo), x, F(lo)).astype(F)


def err_of(c, v, floor):
    """err = sqrtf(v') / at_least(l', floor) with l' = (c'.x + c'.y) + c'.z."""
    c, v = np.asarray(c, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        e = np.sqrt(v) / at_least(luma(c), floor)
    assert e.dtype == F
    return e


def err_of_demodulated(d, v, m, floor):
    """The demodulated form: c'' = d' * m, gr = l_d > 0 ? l'' / l_d : 0, v'' = v' * (gr * gr), then err_of (c'', v'')."""
    d, v, m = np.asarray(d, F), np.asarray(v, F), np.asarray(m, F)
    with np.errstate(all="ignore"):
        c = d * m
        ld, l = luma(d), luma(c)
        gr = np.where(ld > 0, l / ld, F(0)).astype(F)
        vv = v * (gr * gr)
    return err_of(c, vv, floor)


def err_raster(raster, albedo, normal, iterations, sigma, floor, kn=0.0, ka=0.0, kz=0.0, demod_floor=None):
    """The per-pixel err of a raster, (height, width) float32, 0 at absent pixels.  albedo and normal may be None when
    no term is on and demod_floor is None: the variance-only filter."""
    r = np.array(raster, F)
    there = ~(r[..., 3] < 0)
    if demod_floor is not None:
        m = D.divisor(albedo, demod_floor)
        d = GR.guided_raster(D.demodulate(r, m), albedo, normal, iterations, sigma, kn, ka, kz)
        e = err_of_demodulated(d[..., :3], d[..., 3], m, floor)
    else:
        if kn == 0 and ka == 0 and kz == 0:
            f = FR.filter_raster(r, iterations, sigma)
        else:
            f = GR.guided_raster(r, albedo, normal, iterations, sigma, kn, ka, kz)
        e = err_of(f[..., :3], f[..., 3], floor)
    return np.where(there, e, F(0)).astype(F)


def pack_plane(plane, tiles):
    """A (height, width) plane's pixels in the tiles' packed order."""
    return np.concatenate([plane[y:y + th, x:x + tw].reshape(-1) for x, y, tw, th in tiles])


def _larger(a, b):
    """b > a ? b : a, so a NaN b keeps a and a NaN a is replaced by any b that compares (never: NaN compares false)."""
    with np.errstate(all="ignore"):
        return np.where(b > a, b, a).astype(F)


def tile_reduce(err):
    """(mean, max) of one tile's packed errs, in hrt_accum_noise's order."""
    err = np.asarray(err, F)
    n = err.size
    rows = -(-n // BLOCK)
    grid = np.zeros(rows * BLOCK, F)
    grid[:n] = err
    live = (np.arange(rows * BLOCK) < n).reshape(rows, BLOCK)
    grid = grid.reshape(rows, BLOCK)
    xs, xm = np.zeros(BLOCK, F), np.zeros(BLOCK, F)
    with np.errstate(all="ignore"):
        for k in range(rows):  # thread j's fold, in order, from 0
            xs = np.where(live[k], xs + grid[k], xs).astype(F)
            xm = np.where(live[k], _larger(xm, grid[k]), xm).astype(F)
        s = BLOCK // 2
        while s >= 1:
            xs[:s] = xs[:s] + xs[s:2 * s]
            xm[:s] = _larger(xm[:s], xm[s:2 * s])
            s >>= 1
        mean = xs[0] * (F(1) / F(n))
    return F(mean), F(xm[0])


def noise_filtered(raster, albedo, normal, tiles, iterations, sigma, floor, kn=0.0, ka=0.0, kz=0.0, demod_floor=None):
    """What hrt_debug_noise_filtered must give: (err packed as the tiles are, (n_tiles, 2) mean and max)."""
    plane = err_raster(raster, albedo, normal, iterations, sigma, floor, kn, ka, kz, demod_floor)
    err = pack_plane(plane, tiles)
    mm, off = np.zeros((len(tiles), 2), F), 0
    for t, (_, _, tw, th) in enumerate(tiles):
        mm[t] = tile_reduce(err[off:off + tw * th])
        off += tw * th
    return err, mm


def accumulator_noise_filtered(sums, m2, tiles, scales, albedo, normal, width, height, iterations, sigma, floor, tol=None,
                               demod_floor=None):
    """What Accumulator.noise_filtered(error_map=True) must give from the accumulator's downloaded state: sums (n_pixels,
    4), m2, scales[t] = filter_restated.tile_scales of tile t, albedo and normal the packed mean planes (or None), tol the
    tolerances dict(normal=, albedo=, depth=) or None for the variance-only filter."""
    kn, ka, kz = GR.terms(**tol) if tol else (F(0), F(0), F(0))
    al = None if albedo is None else GR.unpack_plane(albedo, tiles, width, height)
    no = None if normal is None else GR.unpack_plane(normal, tiles, width, height)
    return noise_filtered(FR.gather(sums, m2, tiles, scales, width, height), al, no, tiles, iterations, sigma, floor, kn, ka, kz,
                          demod_floor)
