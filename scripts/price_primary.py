"""Price the camera segment's per-cell leaf lists on the host before building the kernel phase (DESIGN.md
section 10): for a sample of 8x8-pixel cells spread over the frame, build each cell's list (csrc/primary_list.h),
generate the cell's camera rays as the kernels do, and run both the stream walk and the list walk for every ray
(tests/native/primary_list.hip pl_check_cell).

  python scripts/price_primary.py [--preset random] [--width 1920 --height 1080] [--spp 4] [--cells 400] [--cap 8]

Output: the distribution of list lengths (leaves a cell's beam meets), the share of overflow cells at the capacity,
the camera segment's box tests per ray (list steps; overflow cells walk the stream) against the stream walk's node
visits per ray, and the checks (leaves the walk tested that a list lacks, rays whose list walk differs): both 0."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-ray-tracer_amd"), ROOT]
import hrt  # noqa: E402

STAT_NAMES = ("rays", "nan_rays", "walk_nodes", "walk_leaf", "list_steps", "list_leaf", "missing", "mismatch", "hull_out")


def build(out="/tmp/hrt_price/libprimarylist.so", extra=()):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                    "--offload-host-only", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "primary_list.hip"), "-o", out], check=True)
    return ctypes.CDLL(out)


def sample_cells(W, H, n, seed=1):
    """n cells spread over the frame: a seeded draw without replacement (all of them when the frame has fewer)."""
    cx, cy = (W + 7) // 8, (H + 7) // 8
    if n >= cx * cy:
        return [(i % cx, i // cx) for i in range(cx * cy)]
    pick = np.random.default_rng(seed).choice(cx * cy, size=n, replace=False)
    return [(int(i) % cx, int(i) // cx) for i in sorted(pick)]


def price(L, preset, W, H, spp, cells, cap=8, seed=1, view=True):
    earth = hrt.load_image(os.path.join(ROOT, "tests", "golden", "earthmap_rgb8.png"))
    s = hrt.preset(preset, 1, earth)
    cam = hrt.preset_camera(s.info, W, H)
    if view:
        s.set_view(cam)
    blob, info = hrt.scene_blob(s)
    p = hrt.params(W, H, spp, 50, seed, tuple(s.info.background))
    tot = np.zeros(9, np.uint64)
    used = np.zeros(9, np.uint64)  # the cells whose list is usable (no overflow)
    lengths = []
    for bx, by in cells:
        st = np.zeros(9, np.uint64)
        n = ctypes.c_uint32()
        rc = L.pl_check_cell(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), cap, bx, by,
                             st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
        assert rc == 0, rc
        tot += st
        if n.value <= cap:
            used += st
        lengths.append(n.value)
    return dict(zip(STAT_NAMES, (int(v) for v in tot))), dict(zip(STAT_NAMES, (int(v) for v in used))), lengths


def summary(tot, used, lengths, cap):
    ln = np.array(lengths)
    rays = max(1, tot["rays"])
    over = float((ln > cap).mean())
    # camera-segment box tests per ray with the lists: list steps where a list is usable, the stream walk elsewhere
    with_lists = (used["list_steps"] + (tot["walk_nodes"] - used["walk_nodes"])) / rays
    return {
        "cells": len(lengths), "rays": tot["rays"], "cap": cap,
        "list_len": {"min": int(ln.min()), "median": float(np.median(ln)), "mean": round(float(ln.mean()), 2),
                     "p90": float(np.percentile(ln, 90)), "max": int(ln.max()),
                     "hist": {str(k): int((ln == k).sum()) for k in range(int(ln.max()) + 1) if (ln == k).any()}},
        "overflow_share": round(over, 4),
        "walk_nodes_per_ray": round(tot["walk_nodes"] / rays, 2),
        "walk_leaf_tests_per_ray": round(tot["walk_leaf"] / rays, 2),
        "box_tests_per_ray_with_lists": round(with_lists, 2),
        "list_steps_per_ray_listed_cells": round(used["list_steps"] / max(1, used["rays"]), 2),
        "walk_nodes_per_ray_listed_cells": round(used["walk_nodes"] / max(1, used["rays"]), 2),
        "walk_nodes_per_ray_overflow_cells": round((tot["walk_nodes"] - used["walk_nodes"]) / max(1, tot["rays"] - used["rays"]), 2),
        "missing": tot["missing"], "mismatch": tot["mismatch"], "nan_rays": tot["nan_rays"], "hull_out": tot["hull_out"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="random")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--cells", type=int, default=400)
    ap.add_argument("--cap", type=int, default=8)
    ap.add_argument("--no-view", action="store_true", help="the stream without hrt_scene_set_view")
    a = ap.parse_args()
    L = build()
    cells = sample_cells(a.width, a.height, a.cells)
    tot, used, lengths = price(L, a.preset, a.width, a.height, a.spp, cells, a.cap, view=not a.no_view)
    print(json.dumps({"preset": a.preset, "width": a.width, "height": a.height, "spp": a.spp, **summary(tot, used, lengths, a.cap)}))


if __name__ == "__main__":
    main()
