"""An independent restatement of the feature-guided a-trous filter (include/hrt/hrt.h, "THE BIT CONTRACT of the guided
frame") in numpy float32, on the plane-shifting form of tests/filter_restated.py.  It never calls the library.

A raster is (height, width, 4) float32 (c.xyz, v), v < 0 an absent pixel; `albedo` is (height, width, 4) (a.xyz, -) and
`normal` (n.xyz, z), read at present pixels only.  kn, ka, kz are 1 / tolerance per term; 0 skips the term."""
import numpy as np

from filter_restated import F, G, H, _shift, gather, luma, pack, resolve_f32


def _sq_dist(q, p):
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _term(d, k):
    t = F(1) - d * k
    t = np.where(t > 0, t, F(0))
    return t * t


def iteration(r, albedo, normal, s, sigma, kn, ka, kz):
    """One iteration with step s on the raster r."""
    assert r.dtype == F and albedo.dtype == F and normal.dtype == F
    c, v = r[..., :3], r[..., 3]
    sigma, kn, ka, kz = F(sigma), F(kn), F(ka), F(kz)
    lp = luma(c)
    with np.errstate(all="ignore"):
        num, den = np.zeros_like(v), np.zeros_like(v)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq = _shift(v, dx, dy, F(-1))
                there = ~(vq < 0)
                g = F(G[dy + 1]) * F(G[dx + 1])
                num = np.where(there, num + g * vq, num)
                den = np.where(there, den + g, den)
        vb = num / den
        rr = F(1) / (sigma * np.sqrt(vb) + F(1e-6))
        sc, sv, sw = np.zeros_like(c), np.zeros_like(v), np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                q = _shift(r, s * dx, s * dy, F(-1))
                aq, nq = _shift(albedo, s * dx, s * dy, F(0)), _shift(normal, s * dx, s * dy, F(0))
                cq, vq = q[..., :3], q[..., 3]
                there = ~(vq < 0)
                d = np.abs(luma(cq) - lp) * rr
                t = F(1) - d * F(0.5)
                t = np.where(t > 0, t, F(0))
                e = t * t
                e = e * e
                if kn > 0:
                    e = e * _term(_sq_dist(nq, normal), kn)
                if ka > 0:
                    e = e * _term(_sq_dist(aq, albedo), ka)
                if kz > 0:
                    zq, zp = nq[..., 3], normal[..., 3]
                    e = e * _term(np.abs(zq - zp) / ((zq + zp) + F(1e-6)), kz)
                w = (F(H[dy + 2]) * F(H[dx + 2])) * e
                sc = np.where(there[..., None], sc + w[..., None] * cq, sc)
                sv = np.where(there, sv + (w * w) * vq, sv)
                sw = np.where(there, sw + w, sw)
        out = np.empty_like(r)
        out[..., :3] = sc / sw[..., None]
        out[..., 3] = sv / (sw * sw)
    keep = (v < 0) | (sw == 0)
    out[keep] = r[keep]
    assert out.dtype == F
    return out


def guided_raster(raster, albedo, normal, iterations, sigma, kn=0.0, ka=0.0, kz=0.0):
    r, a, n = np.array(raster, F), np.ascontiguousarray(albedo, F), np.ascontiguousarray(normal, F)
    for i in range(iterations):
        r = iteration(r, a, n, 1 << i, sigma, kn, ka, kz)
    return r


def terms(normal=0.0, albedo=0.0, depth=0.0):
    """(kn, ka, kz) of the tolerances, as the library computes them once on the host."""
    return tuple(F(1) / F(t) if t > 0 else F(0) for t in (normal, albedo, depth))


# ---- from an accumulator's feature sums ----
def mean_planes(fa, fn, nf):
    """The mean planes of hrt_accum_features from the raw sums (n_pixels, 4) of nf feature samples."""
    fa, fn = np.asarray(fa, F), np.asarray(fn, F)
    inv = F(1) / F(nf)
    albedo = fa * inv
    normal = fn * inv
    with np.errstate(all="ignore"):
        normal[..., 3] = np.where(fa[..., 3] > 0, fn[..., 3] * (F(1) / fa[..., 3]), F(0))
    return albedo.astype(F), normal.astype(F)


def unpack_plane(px, tiles, width, height):
    r = np.zeros((height, width, 4), F)
    off = 0
    for x, y, tw, th in tiles:
        r[y:y + th, x:x + tw] = np.asarray(px[off:off + tw * th], F).reshape(th, tw, 4)
        off += tw * th
    return r


def guided_frame(sums, m2, tiles, scales, albedo, normal, width, height, iterations, sigma, tol):
    """What Accumulator.resolve(denoise=dict(iterations, sigma), guide=tol) must give: packed (n_pixels, 4).  albedo,
    normal: the packed mean planes; tol: dict(normal=, albedo=, depth=)."""
    kn, ka, kz = terms(**tol)
    r = guided_raster(gather(sums, m2, tiles, scales, width, height), unpack_plane(albedo, tiles, width, height),
                      unpack_plane(normal, tiles, width, height), iterations, sigma, kn, ka, kz)
    return resolve_f32(pack(r, tiles))
