"""An independent restatement of the variance-guided a-trous filter (include/hrt/hrt.h, "THE BIT CONTRACT of the
filtered frame") in numpy float32.  It never calls the library.

Two forms: `filter_raster` shifts whole planes and adds the taps in the contract's order (every pixel sees the same
sequence of f32 operations as a scalar loop would give it), and `filter_raster_loops` is the scalar loop itself, for
small rasters, so that the two forms check each other.  A raster is (height, width, 4) float32 (c.xyz, v); v < 0 marks
an absent pixel, which comes out as it went in."""
import numpy as np

F = np.float32
G = (1.0, 2.0, 1.0)
H = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def _shift(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that is off the raster."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
    return b


def luma(c):
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def iteration(r, s, sigma):
    """One iteration with step s on the raster r."""
    assert r.dtype == F
    c, v = r[..., :3], r[..., 3]
    sigma = F(sigma)
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
                cq, vq = q[..., :3], q[..., 3]
                there = ~(vq < 0)
                d = np.abs(luma(cq) - lp) * rr
                t = F(1) - d * F(0.5)
                t = np.where(t > 0, t, F(0))
                e = t * t
                e = e * e
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


def filter_raster(raster, iterations, sigma):
    r = np.array(raster, F)
    for i in range(iterations):
        r = iteration(r, 1 << i, sigma)
    return r


def filter_raster_loops(raster, iterations, sigma):
    """The scalar loop of the contract, pixel by pixel."""
    r = np.array(raster, F)
    h, w = r.shape[:2]
    sigma = F(sigma)

    def at(src, x, y):
        if x < 0 or y < 0 or x >= w or y >= h or src[y, x, 3] < 0:
            return None
        return src[y, x]

    with np.errstate(all="ignore"):
        for i in range(iterations):
            s, src, dst = 1 << i, r, r.copy()
            for y in range(h):
                for x in range(w):
                    p = at(src, x, y)
                    if p is None:
                        continue
                    lp = (p[0] + p[1]) + p[2]
                    num = den = F(0)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            q = at(src, x + dx, y + dy)
                            if q is None:
                                continue
                            g = F(G[dy + 1]) * F(G[dx + 1])
                            num = num + g * q[3]
                            den = den + g
                    vb = num / den
                    rr = F(1) / (sigma * np.sqrt(vb) + F(1e-6))
                    sc, sv, sw = [F(0), F(0), F(0)], F(0), F(0)
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            q = at(src, x + s * dx, y + s * dy)
                            if q is None:
                                continue
                            d = np.abs(((q[0] + q[1]) + q[2]) - lp) * rr
                            t = F(1) - d * F(0.5)
                            t = t if t > 0 else F(0)
                            e = t * t
                            e = e * e
                            wt = (F(H[dy + 2]) * F(H[dx + 2])) * e
                            sc = [sc[k] + wt * q[k] for k in range(3)]
                            sv = sv + (wt * wt) * q[3]
                            sw = sw + wt
                    if sw == 0:
                        continue
                    dst[y, x] = [sc[0] / sw, sc[1] / sw, sc[2] / sw, sv / (sw * sw)]
            r = dst
    return r


# ---- from an accumulator's sums and moments ----
def tile_scales(samples, chunks):
    """(inv_n, inv_k1) of a tile that holds N samples in K chunks."""
    return F(1) / F(samples), F(1) / F(chunks - 1)


def gather(sums, m2, tiles, scales, width, height):
    """The raster of an accumulator: sums (n_pixels, 4) and m2 (n_pixels,) packed as `tiles` [(x, y, w, h)] are,
    scales[t] = tile_scales of tile t; pixels no tile covers are absent."""
    r = np.zeros((height, width, 4), F)
    r[..., 3] = -1
    off = 0
    for (x, y, tw, th), (inv_n, inv_k1) in zip(tiles, scales):
        acc = np.asarray(sums[off:off + tw * th, :3], F).reshape(th, tw, 3)
        m = np.asarray(m2[off:off + tw * th], F).reshape(th, tw)
        yl = luma(acc)
        var = (m - (yl * yl) * inv_n) * inv_k1
        var = np.where(var > 0, var, F(0))
        r[y:y + th, x:x + tw, :3] = acc * inv_n
        r[y:y + th, x:x + tw, 3] = var * inv_n
        off += tw * th
    return r


def pack(raster, tiles):
    """The raster's pixels in the tiles' packed order: (n_pixels, 4)."""
    return np.concatenate([raster[y:y + th, x:x + tw].reshape(-1, 4) for x, y, tw, th in tiles])


def resolve_f32(filtered):
    """The displayable frame of filtered (c', v') pixels: sqrt(c'), alpha 1."""
    with np.errstate(all="ignore"):
        out = np.sqrt(np.asarray(filtered, F))
    out[..., 3] = 1
    return out


def quantize(frame):
    """The PPM rule on an f32 frame (NaN -> 0, clamp to [0, 0.999], truncate 256 v), alpha 255."""
    v = np.asarray(frame, F)
    v = np.where(v != v, F(0), np.where(v < 0, F(0), np.where(v > F(0.999), F(0.999), v)))
    out = (F(256) * v).astype(np.uint8)
    out[..., 3] = 255
    return out


def filtered_frame(sums, m2, tiles, scales, width, height, iterations, sigma):
    """What Accumulator.resolve(denoise=dict(iterations, sigma)) must give for several tiles: packed (n_pixels, 4)."""
    return resolve_f32(pack(filter_raster(gather(sums, m2, tiles, scales, width, height), iterations, sigma), tiles))
