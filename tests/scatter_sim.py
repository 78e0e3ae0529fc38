"""Helper of the scatter-query tests: builds tests/native/scatter_sim.hip (csrc/scatter.h on the host), query_sim.hip and
lane_sim.hip (the reference frames) the way query_sim.py builds, host-only and without a HIP runtime, and runs the loop
camera paths -> (intersect -> scatter) until done over a scene's flattened blob."""
import ctypes
import os
import subprocess

import numpy as np

import hrt
import query_sim as QS
from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
MAT_BYTES = 32  # layout.h Mat


def _compile(src, so):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-host-only",
                    "-no-hip-rt",  # host code only: a GPU test process must not map a second HIP runtime beside torch's
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", src), "-o", so], check=True, env=tool_env())


class Sims:
    """The three host simulators: S scatter_sim.hip, Q query_sim.hip, L lane_sim.hip."""


def build(tmp_path_factory, lane=True):
    d = tmp_path_factory.mktemp("scattersim")
    sims = Sims()
    sims.Q = QS.build(tmp_path_factory)
    so = str(d / "libscattersim.so")
    _compile("scatter_sim.hip", so)
    S = ctypes.CDLL(so)
    S.scatter_sim.restype = ctypes.c_int
    S.scatter_sim.argtypes = [ctypes.c_void_p, ctypes.POINTER(hrt.BlobInfo), ctypes.POINTER(hrt.ScatterParams), ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]
    S.camera_paths_sim.restype = ctypes.c_int
    S.camera_paths_sim.argtypes = [ctypes.POINTER(hrt.Camera), ctypes.POINTER(hrt.RenderParams)] + [ctypes.c_uint32] * 4 + \
        [ctypes.c_void_p, ctypes.c_void_p]
    sims.S = S
    sims.L = None
    if lane:
        so = str(d / "liblanesim.so")
        _compile("lane_sim.hip", so)
        sims.L = ctypes.CDLL(so)
        sims.L.lane_sim_render.restype = ctypes.c_int
    return sims


def material_bound(info):
    """An upper bound of the scene's material count from the blob alone: its material section, which is zero-padded to
    256 bytes (a padding record reads as a Lambertian of texture 0, so the bound is safe to index).  Enough wherever every
    hit comes from the scene's own intersect; a test of the range check passes the true count."""
    return (info.off_texs - info.off_mats) // MAT_BYTES


def camera_paths(sims, cam, p, region=None):
    """hrt_camera_paths' (rays, paths) for region (x0, y0, w, h) (default: the frame) as one tile."""
    x0, y0, w, h = region if region is not None else (0, 0, p.width, p.height)
    n = w * h * p.samples
    rays, paths = QS.aligned(n, hrt.RAY_DTYPE), QS.aligned(n, hrt.PATH_DTYPE)
    assert sims.S.camera_paths_sim(ctypes.byref(cam), ctypes.byref(p), x0, y0, w, h, rays.ctypes.data, paths.ctypes.data) == 0
    return rays, paths


def scatter(sims, blob, rays, hits, paths, background, n_mats=None):
    """hrt_scene_scatter's effect on the host: new (rays, paths) arrays; blob = hrt.scene_blob(scene)."""
    buf, info = blob
    n = len(rays)
    r, h, q = QS.aligned(n, hrt.RAY_DTYPE), QS.aligned(n, hrt.HIT_DTYPE), QS.aligned(n, hrt.PATH_DTYPE)
    r[:], h[:], q[:] = rays, hits, paths
    sp = hrt.scatter_params(background)
    rc = sims.S.scatter_sim(buf, ctypes.byref(info), ctypes.byref(sp), r.ctypes.data, h.ctypes.data, q.ctypes.data, n,
                            material_bound(info) if n_mats is None else n_mats)
    assert rc == 0
    return r, q


def loop(sims, scene, cam, p, blob=None, region=None, on_round=None, n_mats=None):
    """The contract's loop on the host.  Returns (paths, n_rays, scattered) with n_rays the valid, not-DONE rays handed to
    intersect over all rounds and scattered[kind] the scatter steps made at a material of that kind (from the hits'
    material ids).  on_round(i, rays, hits, paths): called after every scatter with the batch's state."""
    blob = hrt.scene_blob(scene) if blob is None else blob
    buf, info = blob
    kinds = np.frombuffer(buf, np.uint32, offset=info.off_mats, count=material_bound(info) * (MAT_BYTES // 4)).reshape(-1, 8)[:, 4]
    rays, paths = camera_paths(sims, cam, p, region)
    n_rays, scattered = 0, np.zeros(8, np.int64)
    bg = tuple(p.background)
    for i in range(p.max_depth):
        live = (paths["flags"] & hrt.PATH_DONE) == 0
        if not live.any():
            break
        hits = QS.intersect(sims.Q, scene, rays, seed=p.seed, shutter=(cam.time0, cam.time1), blob=blob)
        n_rays += int(((hits["flags"] & hrt.HIT_INVALID) == 0).sum())
        stepped = live & ((hits["flags"] & hrt.HIT_HIT) != 0)
        scattered += np.bincount(kinds[hits["material"][stepped]], minlength=8)[:8]
        rays, paths = scatter(sims, blob, rays, hits, paths, bg, n_mats)
        if on_round is not None:
            on_round(i, rays, hits, paths)
    return paths, n_rays, scattered


def frame(paths, w, h):
    """sqrtf(radiance * 1.0f) of a one-sample batch as the (h, w, 3) frame a render returns."""
    return np.sqrt(paths["radiance"].astype(F) * F(1.0)).reshape(h, w, 3)


def lane_render(sims, scene, cam, p, blob=None, kernel=1, cull=2):
    """lane_sim_render of the frame: (h, w, 4) float32 and the segment count."""
    buf, info = hrt.scene_blob(scene) if blob is None else blob
    out = np.zeros((p.height, p.width, 4), F)
    cnt = np.zeros(8, np.uint64)
    rc = sims.L.lane_sim_render(buf, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), kernel, cull, 0, 0, p.width, p.height,
                                out.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out, int(cnt[0])


def words(a):
    return QS.words(a)
