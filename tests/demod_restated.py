"""An independent restatement of the DEMODULATED guided filter (include/hrt/hrt.h, "THE BIT CONTRACT of the demodulated
frame") in numpy float32, on top of tests/guided_restated.py's iterations.  It never calls the library.

Steps 1, 2 and 4 of the contract are here; step 3 is guided_restated.guided_raster as it stands.  A raster is (height,
width, 4) float32 (c.xyz, v), v < 0 an absent pixel, which is neither demodulated nor remodulated; `albedo` is (height,
width, 4) (a.xyz, -), read at present pixels only."""
import numpy as np

from filter_restated import F, gather, luma, pack, resolve_f32
from guided_restated import guided_raster, terms, unpack_plane


def divisor(albedo, floor):
    """Step 1: at_least(a, floor) per channel, x > lo ? x : lo, so a NaN albedo gives the floor."""
    a = np.asarray(albedo, F)[..., :3]
    with np.errstate(all="ignore"):
        return np.where(a > F(floor), a, F(floor)).astype(F)


def demodulate(raster, m):
    """Step 2 on the present pixels of gather's raster (c, v)."""
    r = np.array(raster, F)
    c, v = r[..., :3], r[..., 3]
    with np.errstate(all="ignore"):
        d = c / m
        l, ld = luma(c), luma(d)
        g = np.where(l > 0, ld / l, F(0)).astype(F)
        vd = v * (g * g)
    there = ~(v < 0)
    out = r.copy()
    out[there, :3] = d[there]
    out[there, 3] = vd[there]
    assert out.dtype == F
    return out


def remodulate(filtered, m, there):
    """Step 4: the last iteration's d' times the divisor, at the present pixels; v' stays in demodulated units."""
    out = np.array(filtered, F)
    with np.errstate(all="ignore"):
        c = out[..., :3] * m
    out[there, :3] = c[there]
    assert out.dtype == F
    return out


def demod_raster(raster, albedo, normal, iterations, sigma, floor, kn=0.0, ka=0.0, kz=0.0):
    """What hrt_debug_guided_ex with HRT_GUIDED_DEMODULATE must give: (c'' before the sqrt, v')."""
    r = np.array(raster, F)
    m = divisor(albedo, floor)
    d = guided_raster(demodulate(r, m), albedo, normal, iterations, sigma, kn, ka, kz)
    return remodulate(d, m, ~(r[..., 3] < 0))


def demod_frame(sums, m2, tiles, scales, albedo, normal, width, height, iterations, sigma, tol, floor):
    """What Accumulator.resolve_guided(denoise=dict(iterations, sigma), guide=tol, demodulate=floor) must give: packed
    (n_pixels, 4).  albedo, normal: the packed mean planes; tol: dict(normal=, albedo=, depth=)."""
    kn, ka, kz = terms(**tol)
    r = demod_raster(gather(sums, m2, tiles, scales, width, height), unpack_plane(albedo, tiles, width, height),
                     unpack_plane(normal, tiles, width, height), iterations, sigma, floor, kn, ka, kz)
    return resolve_f32(pack(r, tiles))
