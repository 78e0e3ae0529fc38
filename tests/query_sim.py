"""Helper of the ray-query tests: builds tests/native/query_sim.hip (csrc/query.h on the host, as tests/feature_sim.py
builds feature_sim.hip) and runs it over a scene's flattened blob."""
import ctypes
import os
import subprocess

import numpy as np

import hrt
from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
MISS = 0xFFFFFFFF
INF = F(np.inf)


def build(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("querysim") / "libquerysim.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-host-only",
                    "-no-hip-rt",  # host code only: a GPU test process must not map a second HIP runtime beside torch's
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", "query_sim.hip"), "-o", so], check=True, env=tool_env())
    hrt.load()  # the process's one HIP runtime first (hrt.load)
    L = ctypes.CDLL(so)
    L.query_sim.restype = ctypes.c_int
    L.query_sim.argtypes = [ctypes.c_void_p, ctypes.POINTER(hrt.BlobInfo), ctypes.POINTER(hrt.QueryParams), ctypes.c_void_p,
                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    L.camera_rays_sim.restype = ctypes.c_int
    L.camera_rays_sim.argtypes = [ctypes.POINTER(hrt.Camera), ctypes.POINTER(hrt.RenderParams)] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p]
    return L


def aligned(n, dtype):
    """n records of a 48-byte dtype at a 16-byte aligned address, zeroed."""
    raw = np.zeros(n * dtype.itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * dtype.itemsize].view(dtype)


def make_rays(origin, direction, time=0.0, t_min=0.001, t_max=np.inf, pixel=0, sample=0, segment=0):
    """A RAY_DTYPE array from broadcastable columns."""
    origin = np.asarray(origin, F).reshape(-1, 3)
    direction = np.asarray(direction, F).reshape(-1, 3)
    n = max(len(origin), len(direction))
    r = aligned(n, hrt.RAY_DTYPE)
    r["origin"], r["direction"] = origin, direction
    r["time"], r["t_min"], r["t_max"] = time, t_min, t_max
    r["pixel"], r["sample"], r["segment"] = pixel, sample, segment
    return r


def intersect(L, scene, rays, flags=0, seed=0, shutter=(0.0, 1.0), full=-1, blob=None):
    """hrt_scene_intersect's answer on the host: a HIT_DTYPE array."""
    buf, info = blob if blob is not None else hrt.scene_blob(scene)
    src = aligned(len(rays), hrt.RAY_DTYPE)
    src[:] = rays
    hits = aligned(len(rays), hrt.HIT_DTYPE)
    q = hrt.query_params(flags, seed, shutter)
    rc = L.query_sim(buf, ctypes.byref(info), ctypes.byref(q), src.ctypes.data, len(rays), hits.ctypes.data, full)
    assert rc == 0
    return hits


def camera_rays(L, cam, p, region=None):
    """hrt_camera_rays' rays for region (x0, y0, w, h) (default: the frame) as one tile: a RAY_DTYPE array."""
    x0, y0, w, h = region if region is not None else (0, 0, p.width, p.height)
    rays = aligned(w * h * p.samples, hrt.RAY_DTYPE)
    assert L.camera_rays_sim(ctypes.byref(cam), ctypes.byref(p), x0, y0, w, h, rays.ctypes.data) == 0
    return rays


def words(a):
    """Records as uint32 words, (n, 12)."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 12)
