"""Helper of the feature-pass tests: builds tests/native/feature_sim.hip (csrc/feature_pass.h on the host, as
tests/test_lane_sim.py builds lane_sim.hip) and runs it over a preset's flattened scene."""
import ctypes
import os
import subprocess

import numpy as np

import hrt
from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
CULL_REFERENCE, CULL_EXACT = 0, 2
MISS = 0xFFFFFFFF
# layout.h M_*
M_LAMBERTIAN, M_METAL, M_DIELECTRIC, M_DIFFUSE_LIGHT, M_ISOTROPIC = range(5)


def build(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("featuresim") / "libfeaturesim.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-host-only",
                    "-no-hip-rt",  # host code only: a GPU test process must not map a second HIP runtime beside torch's
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", "feature_sim.hip"), "-o", so], check=True, env=tool_env())
    hrt.load()  # the process's one HIP runtime first (hrt.load)
    L = ctypes.CDLL(so)
    L.feature_sim.restype = ctypes.c_int
    return L


def run(L, scene, cam, p, region=None, cull=CULL_EXACT, full=-1, per_sample=True):
    """One feature pass (p.sample_offset, p.samples) over region (x0, y0, w, h) (default: the frame).  Returns
    (samples (h, w, spp, 8) or None, kinds (h, w, spp) uint32 or None, sums (h, w, 8)): albedo.xyz, hit, normal.xyz, depth."""
    blob, info = hrt.scene_blob(scene)
    x0, y0, w, h = region if region is not None else (0, 0, p.width, p.height)
    samples = np.zeros((h, w, p.samples, 8), F) if per_sample else None
    kinds = np.zeros((h, w, p.samples), np.uint32) if per_sample else None
    sums = np.zeros((h, w, 8), F)
    rc = L.feature_sim(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), cull, full, x0, y0, w, h,
                       samples.ctypes.data_as(ctypes.c_void_p) if per_sample else None,
                       kinds.ctypes.data_as(ctypes.c_void_p) if per_sample else None, sums.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return samples, kinds, sums


def planes(L, scene, cam, make_params, passes, region=None, **kw):
    """The planes (h, w, 8) after the feature passes [(begin, end), ...]: plane = plane + pass_sum, from zero."""
    plane = None
    for b, e in passes:
        _, _, s = run(L, scene, cam, make_params(e - b, b), region, per_sample=False, **kw)
        plane = (np.zeros_like(s) + s) if plane is None else plane + s
    return plane


def pack(plane, tiles):
    """(h, w, 8) -> (fa, fn), each (n_pixels, 4) in the tiles' packed order."""
    px = np.concatenate([plane[y:y + th, x:x + tw].reshape(-1, 8) for x, y, tw, th in tiles])
    return np.ascontiguousarray(px[:, :4]), np.ascontiguousarray(px[:, 4:])
