"""ctypes wrapper of liboracle.so — TEST INFRASTRUCTURE ONLY.

The CPU restatement of the reference renderer (oracle/oracle.cpp).  Imported only by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg, always as the checker / the CPU baseline,
never as the thing measured or shipped.  Parity status: UNPINNED against the reference binary (Rust,
unbuildable here, unseeded); pinned by the KAT fixtures of tests/golden (see oracle.cpp header).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("ORACLE_LIB") or os.path.join(HERE, "liboracle.so")  # ORACLE_LIB: the ASan build (scripts/sanitize.sh)
COUNTERS = ["segments", "aabb", "sphere", "moving", "rect", "medium", "tex_solid", "tex_checker", "tex_noise", "tex_image", "samples", "pixels"]

_lib = None


def build() -> None:
    subprocess.check_call(["make", "-s", "-C", HERE])


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        build()
    L = ctypes.CDLL(LIB)
    vp, f, u32, u64, i32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.oracle_last_error.restype = ctypes.c_char_p
    L.oracle_preset_build.restype = vp
    L.oracle_preset_build.argtypes = [i32, u64, vp, u32, u32, u32, vp]
    L.oracle_scene_build.restype = vp
    L.oracle_scene_build.argtypes = [vp, u64, vp, u64, vp]
    L.oracle_scene_destroy.argtypes = [vp]
    L.oracle_scene_count.restype = u32
    L.oracle_scene_count.argtypes = [vp]
    L.oracle_scene_bbox.restype = i32
    L.oracle_scene_bbox.argtypes = [vp, vp]
    L.oracle_render.restype = i32
    L.oracle_render.argtypes = [vp, u32, u32, u32, u32, u32, u64, f, u32, u32, u32, u32, vp, i32, vp]
    L.oracle_render_rows.restype = i32
    L.oracle_render_rows.argtypes = [vp, u32, u32, u32, u32, u32, u64, f, vp, u32, u32, u32, u32, vp, i32, vp]
    L.oracle_render_cam.restype = i32
    L.oracle_render_cam.argtypes = [vp, vp, u32, u32, u32, u32, u32, u64, f, u32, u32, u32, u32, vp, i32, vp]
    L.oracle_render_rows_cam.restype = i32
    L.oracle_render_rows_cam.argtypes = [vp, vp, u32, u32, u32, u32, u32, u64, f, vp, u32, u32, u32, u32, vp, i32, vp]
    L.oracle_camera.argtypes = [vp, vp, f, f, f, f, f, i32, i32, vp]
    L.oracle_camera_ray.argtypes = [vp, vp, f, f, f, i32, i32, f, f, vp, f, vp]
    L.oracle_aabb_hit.restype = i32
    L.oracle_aabb_hit.argtypes = [vp, vp, vp, vp, f, f]
    L.oracle_prim_hit.restype = i32
    L.oracle_prim_hit.argtypes = [i32, vp, vp, f, f, vp]
    L.oracle_vec_op.argtypes = [i32, vp, vp, f, vp]
    L.oracle_perlin.restype = f
    L.oracle_perlin.argtypes = [vp, vp, i32, vp, u32]
    L.oracle_perlin_tables.argtypes = [u64, vp, vp]
    L.oracle_texture.argtypes = [i32, vp, f, f, f, vp, vp, vp, u32, u32, u32, vp]
    L.oracle_math.argtypes = [i32, vp, vp, vp, u32]
    L.oracle_math_libm.argtypes = [i32, vp, vp, vp, u32]
    L.oracle_set_libm.argtypes = [i32]
    L.oracle_record_math.argtypes = [vp, u32, vp]
    L.oracle_rng.argtypes = [u64, u32, u32, i32, u32, vp]
    L.oracle_scene_hit.restype = i32
    L.oracle_scene_hit.argtypes = [vp, vp, u64, u64, vp]
    L.oracle_scene_prims.restype = u32
    L.oracle_scene_prims.argtypes = [vp, vp, u32]
    L.oracle_scene_media.restype = u32
    L.oracle_scene_media.argtypes = [vp, vp, u32]
    L.oracle_scatter.restype = i32
    L.oracle_scatter.argtypes = [vp, u32, vp, vp, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data


NO_ID = 0xFFFFFFFF
_F, _U = np.float32, np.uint32
# oracle.cpp oracle_scene_hit's records, oracle_scene_prims' and oracle_scatter's
RAY = np.dtype([("origin", _F, 3), ("direction", _F, 3), ("time", _F), ("t_min", _F), ("t_max", _F), ("pixel", _U), ("sample", _U),
                ("segment", _U)])
HIT = np.dtype([("hit", _U), ("t", _F), ("point", _F, 3), ("normal", _F, 3), ("u", _F), ("v", _F), ("front_face", _U), ("medium", _U),
                ("material", _U), ("prim", _U), ("medium_id", _U), ("pad", _U)])
PRIM = np.dtype([("kind", _U), ("boundary_of", _U), ("p", _F, 9), ("pad", _U)])
SCATTER = np.dtype([("emitted", _F, 3), ("scattered", _U), ("attenuation", _F, 3), ("origin", _F, 3), ("direction", _F, 3), ("time", _F),
                    ("rng", _U, 4)])
assert RAY.itemsize == 48 and HIT.itemsize == 64 and PRIM.itemsize == 48 and SCATTER.itemsize == 72


def _cam11(camera) -> np.ndarray:
    """(look_from, look_at, fov, aperture, focus_dist, time0, time1) as the 11 floats oracle_render_cam takes."""
    look_from, look_at, fov, aperture, focus_dist, time0, time1 = camera
    c = np.array([*look_from, *look_at, fov, aperture, focus_dist, time0, time1], np.float32)
    if c.shape != (11,):
        raise ValueError("camera: (look_from(3), look_at(3), fov, aperture, focus_dist, time0, time1)")
    return c


class OracleScene:
    def __init__(self, preset: int, scene_seed: int = 1, image: np.ndarray | None = None):
        L = load()
        img = np.zeros((1, 1, 3), np.uint8) if image is None else np.ascontiguousarray(image, np.uint8)
        self._img = img
        info = np.zeros(16, np.float32)
        h, w, c = img.shape
        self.h = L.oracle_preset_build(preset, scene_seed, _p(img), w, h, c, _p(info))
        if not self.h:
            raise RuntimeError(L.oracle_last_error().decode())
        self._set_info(info)

    @classmethod
    def from_description(cls, words: np.ndarray, blob: np.ndarray | None = None) -> "OracleScene":
        """A scene from a description instead of a preset number: the u32 words and the image byte blob of
        oracle.cpp build_desc (tests/scene_desc.py Desc.to_oracle encodes them)."""
        L = load()
        self = cls.__new__(cls)
        w = np.ascontiguousarray(words, np.uint32).reshape(-1)
        b = np.zeros(1, np.uint8) if blob is None or len(blob) == 0 else np.ascontiguousarray(blob, np.uint8).reshape(-1)
        n_blob = 0 if blob is None else len(blob)
        info = np.zeros(16, np.float32)
        self.h = L.oracle_scene_build(_p(w), w.size, _p(b), n_blob, _p(info))
        if not self.h:
            raise RuntimeError(L.oracle_last_error().decode())
        self._set_info(info)
        return self

    def _set_info(self, info):
        self.look_from, self.look_at = info[0:3].copy(), info[3:6].copy()
        self.fov, self.aperture, self.focus_dist, self.time0, self.time1 = [float(x) for x in info[6:11]]
        self.background = info[11:14].copy()
        self.n_media = int(info[14])

    def __del__(self):
        try:
            if self.h:
                load().oracle_scene_destroy(self.h)
        except Exception:
            pass

    def count(self) -> int:
        return load().oracle_scene_count(self.h)

    def bbox(self):
        b = np.zeros(6, np.float32)
        return b if load().oracle_scene_bbox(self.h, _p(b)) else None

    def hit(self, rays: np.ndarray, seed: int = 0) -> np.ndarray:
        """world.hit(ray, t_min, t_max) of every RAY record, with the media's draws keyed by (seed, pixel, sample,
        segment): HIT records.  No validity rule: a NaN goes where the reference's arithmetic takes it."""
        r = np.ascontiguousarray(rays, RAY).reshape(-1)
        out = np.zeros(r.size, HIT)
        if load().oracle_scene_hit(self.h, _p(r), r.size, seed, _p(out)) != 0:
            raise RuntimeError(load().oracle_last_error().decode())
        return out

    def prims(self) -> np.ndarray:
        """The world's leaves in the oracle's pre-order: PRIM records (kind and p as oracle_prim_hit takes them)."""
        n = load().oracle_scene_prims(self.h, None, 0)
        out = np.zeros(max(n, 1), PRIM)
        load().oracle_scene_prims(self.h, _p(out), n)
        return out[:n]

    def media(self) -> np.ndarray:
        """medium_id of the world's ConstantMedium nodes in pre-order (their phase functions' material ids follow the
        description's materials in this order)."""
        n = load().oracle_scene_media(self.h, None, 0)
        out = np.zeros(max(n, 1), np.uint32)
        load().oracle_scene_media(self.h, _p(out), n)
        return out[:n]

    def scatter(self, material, rays: np.ndarray, hits: np.ndarray, rng: np.ndarray) -> np.ndarray:
        """emitted(u, v, point) and then scatter(ray, rec) of material[i] for ray i (RAY) and record i (HIT), drawing from
        the xoshiro state rng[i] (4 words): SCATTER records, the state afterwards included."""
        r = np.ascontiguousarray(rays, RAY).reshape(-1)
        h = np.ascontiguousarray(hits, HIT).reshape(-1)
        g = np.ascontiguousarray(rng, np.uint32).reshape(-1, 4)
        m = np.broadcast_to(np.asarray(material, np.uint32), r.shape)
        out = np.zeros(r.size, SCATTER)
        L = load()
        ray7, rec10 = np.zeros(7, np.float32), np.zeros(10, np.float32)
        for i in range(r.size):
            ray7[0:3], ray7[3:6], ray7[6] = r["origin"][i], r["direction"][i], r["time"][i]
            rec10[0], rec10[1:4], rec10[4:7] = h["t"][i], h["point"][i], h["normal"][i]
            rec10[7], rec10[8], rec10[9] = h["u"][i], h["v"][i], 1.0 if h["front_face"][i] else 0.0
            if L.oracle_scatter(self.h, int(m[i]), _p(ray7), _p(rec10), _p(g[i:i + 1]), _p(out[i:i + 1])) != 0:
                raise RuntimeError(L.oracle_last_error().decode())
        return out

    def render(self, width, height, spp, depth=50, seed=1, region=None, threads=8, sample_offset=0, t_min=0.001,
               camera=None):
        """camera: (look_from, look_at, fov, aperture, focus_dist, time0, time1) in place of the preset's own."""
        x0, y0, w, h = region if region is not None else (0, 0, width, height)
        out = np.zeros((h, w, 4), np.float32)
        cnt = np.zeros(16, np.uint64)
        if camera is None:
            st = load().oracle_render(self.h, width, height, spp, depth, sample_offset, seed, t_min, x0, y0, w, h, _p(out), threads, _p(cnt))
        else:
            c = _cam11(camera)
            st = load().oracle_render_cam(self.h, _p(c), width, height, spp, depth, sample_offset, seed, t_min, x0, y0, w, h,
                                          _p(out), threads, _p(cnt))
        if st != 0:
            raise RuntimeError(load().oracle_last_error().decode())
        return out, dict(zip(COUNTERS, [int(c) for c in cnt[: len(COUNTERS)]]))

    def render_rows(self, width, height, spp, rows, depth=50, seed=1, threads=8, sample_offset=0, t_min=0.001,
                    x0=0, w=None, task_w=80, camera=None):
        """Columns [x0, x0 + w) (default: all) of rows `rows` of the width x height frame, in tasks of
        task_w pixels: (len(rows), w, 4) f32 and counters.  camera: as in render."""
        r = np.ascontiguousarray(rows, np.uint32)
        w = width - x0 if w is None else w
        out = np.zeros((r.size, w, 4), np.float32)
        cnt = np.zeros(16, np.uint64)
        if camera is None:
            st = load().oracle_render_rows(self.h, width, height, spp, depth, sample_offset, seed, t_min, _p(r), r.size,
                                           x0, w, task_w, _p(out), threads, _p(cnt))
        else:
            c = _cam11(camera)
            st = load().oracle_render_rows_cam(self.h, _p(c), width, height, spp, depth, sample_offset, seed, t_min, _p(r),
                                               r.size, x0, w, task_w, _p(out), threads, _p(cnt))
        if st != 0:
            raise RuntimeError(load().oracle_last_error().decode())
        return out, dict(zip(COUNTERS, [int(c) for c in cnt[: len(COUNTERS)]]))


def math(op: int, x: np.ndarray, y: np.ndarray | None = None) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    yy = None if y is None else np.ascontiguousarray(y, np.float32)
    load().oracle_math(op, _p(x), None if yy is None else _p(yy), _p(out), x.size)
    return out


def math_libm(op: int, x: np.ndarray, y: np.ndarray | None = None) -> np.ndarray:
    """glibc's f32 function for op (0 sinf, 1 cosf, 2 acosf, 3 atan2f(x, y), 4 logf, 5 powf(x, 5), 6 tanf):
    the reference platform's arithmetic (Rust f32 methods call these on Linux)."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    yy = None if y is None else np.ascontiguousarray(y, np.float32)
    load().oracle_math_libm(op, _p(x), None if yy is None else _p(yy), _p(out), x.size)
    return out


class libm_arithmetic:
    """Context manager: oracle renders and scene builds inside use glibc's f32 transcendentals."""

    def __enter__(self):
        load().oracle_set_libm(1)
        return self

    def __exit__(self, *exc):
        load().oracle_set_libm(0)
        return False


N_OPS = 7


def record_math(fn, cap: int = 1 << 22):
    """Run fn() (single-threaded oracle renders) and return {op: (n_calls, args[:min(n, cap), 2])}."""
    bufs = [np.zeros(2 * cap, np.float32) for _ in range(N_OPS)]
    ptrs = (ctypes.c_void_p * N_OPS)(*[b.ctypes.data for b in bufs])
    counts = np.zeros(N_OPS, np.uint32)
    L = load()
    L.oracle_record_math(ptrs, cap, None)
    try:
        fn()
    finally:
        L.oracle_record_math(None, 0, counts.ctypes.data)
    return {k: (int(counts[k]), bufs[k][: 2 * min(int(counts[k]), cap)].reshape(-1, 2)) for k in range(N_OPS)}
