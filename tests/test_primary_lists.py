"""The camera segment's per-cell leaf lists (csrc/primary_list.h) against the walk they replace, on the host.

tests/native/primary_list.hip builds a cell's list, generates the cell's camera rays with lane.h start_sample
(every pixel of the cell x 8 samples) plus the pixel footprint's four corners at jitter 0 and 1 - 2^-24 with lens
samples at the disk's centre and around its rim, and runs for each ray the stream walk (walk_box / walk_prim, what
render_basic_kernel's lane does) and the list walk (list_step per entry, then walk_leaf_test).  Per cell:
- every leaf the walk hands to walk_leaf_test is on the cell's list, or the cell is an overflow cell (`missing`);
- the list walk returns the same (closest, winner) bits (`mismatch`); NaN-mode rays take the stream walk in the
  kernel, so only their result counts;
- every ray lies inside the padded hull the builder tests boxes against: its origin in the lens range and
  origin + direction in the target range, per axis (`hull_out`).  A shim built with -DHRT_PL_NO_PAD (the hull
  without its pads) fails this check: the f32 rounding of start_sample's ray puts corner rays outside the exact
  ranges, which is what the pads are for.

Presets: random, motion (per-sphere shutters), two_spheres (lens radius 0).  Frames: 1920x1080 on 200 seeded cells,
all of 40x24 and of 37x23 (not multiples of 8).  Each from the preset's own camera; tests/test_cameras.py runs the
same check (_check with camera=) from the cameras of tests/cameras.py.

The overflow cap: no preset may overflow more than 10% of its cells at capacity 8.  It is asserted on the 1920x1080
frame, the size the lists are made for.  On the two tiny frames a cell's footprint is a fifth of the frame's width
and its beam meets 9 to 61 leaves of `random`, so no builder can keep those cells within 8 entries: there the share
is measured and printed, the cells take the walk, and the checks above still hold for every ray.
Measured overflow shares at capacity 8 (cells with more than 8 leaves / cells):
  random      1920x1080 15/200 = 7.5% (164/2000 = 8.2% on scripts/price_primary.py's sample), 40x24 15/15, 37x23 15/15
  motion      1920x1080 9/200 = 4.5%, 40x24 8/15, 37x23 5/15
  two_spheres 0 everywhere (2 leaves)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hrt
from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STAT_NAMES = ("rays", "nan_rays", "walk_nodes", "walk_leaf", "list_steps", "list_leaf", "missing", "mismatch", "hull_out")
CAP = 8
SPP = 8


def _build(tmp_path_factory, extra=()):
    so = str(tmp_path_factory.mktemp("primarylist") / "libprimarylist.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                    "--offload-host-only", *extra, *os.environ.get("LANE_SIM_CFLAGS", "").split(),
                    "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", "primary_list.hip"), "-o", so], check=True, env=tool_env())
    L = ctypes.CDLL(so)
    L.pl_check_cell.restype = ctypes.c_int
    L.pl_build.restype = ctypes.c_int
    L.pl_listable.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _build(tmp_path_factory)


@pytest.fixture(scope="module")
def lib_no_pad(tmp_path_factory):
    return _build(tmp_path_factory, ("-DHRT_PL_NO_PAD",))


def _cells(W, H, n=None, seed=7):
    cx, cy = (W + 7) // 8, (H + 7) // 8
    if n is None or n >= cx * cy:
        return [(i % cx, i // cx) for i in range(cx * cy)]
    pick = np.random.default_rng(seed).choice(cx * cy, size=n, replace=False)
    return [(int(i) % cx, int(i) // cx) for i in sorted(pick)]


def _check(L, earth, name, W, H, cells, cap=CAP, camera=None):
    """Totals of pl_check_cell over the cells, and each cell's leaf count.  camera: a tests/cameras.py spec
    (look_from, look_at, fov, aperture, focus_dist, time0, time1) in place of the preset's own."""
    s = hrt.preset(name, 1, earth)
    cam = hrt.preset_camera(s.info, W, H) if camera is None else hrt.camera(*camera, W, H)
    blob, info = hrt.scene_blob(s)
    assert L.pl_listable(ctypes.byref(info)) == 1, name
    p = hrt.params(W, H, SPP, 50, 3, tuple(s.info.background))
    tot = np.zeros(len(STAT_NAMES), np.uint64)
    counts = []
    for bx, by in cells:
        st = np.zeros(len(STAT_NAMES), np.uint64)
        n = ctypes.c_uint32()
        rc = L.pl_check_cell(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), cap, bx, by,
                             st.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n))
        assert rc == 0, (name, bx, by, rc)
        tot += st
        counts.append(n.value)
    return dict(zip(STAT_NAMES, (int(v) for v in tot))), np.array(counts)


FRAMES = [(1920, 1080, 200), (40, 24, None), (37, 23, None)]


@pytest.mark.parametrize("W,H,n", FRAMES)
@pytest.mark.parametrize("name", ["random", "motion", "two_spheres"])
def test_list_holds_every_leaf_the_walk_tests(lib, earth, name, W, H, n):
    cells = _cells(W, H, n)
    tot, counts = _check(lib, earth, name, W, H, cells)
    overflow = float((counts > CAP).mean())
    print(f"{name} {W}x{H}: {len(cells)} cells, {tot['rays']} rays, list length median {np.median(counts):.0f} "
          f"max {counts.max()}, overflow share {overflow:.4f}, walk nodes/ray {tot['walk_nodes'] / tot['rays']:.1f}")
    assert tot["rays"] >= len(cells) * 36  # at least the corner rays of every cell
    assert tot["missing"] == 0
    assert tot["mismatch"] == 0
    assert tot["hull_out"] == 0
    if W == 1920:
        assert overflow <= 0.10, overflow
    if name == "random" and W == 1920:
        assert tot["list_steps"] > 0 and tot["list_leaf"] > 0  # usable lists were walked


def test_check_fails_without_the_hulls_pads(lib_no_pad, earth):
    """The same check on lists built without the pads: rays fall outside the unpadded hull, so the test above can fail."""
    tot, _ = _check(lib_no_pad, earth, "random", 1920, 1080, _cells(1920, 1080, 200))
    assert tot["hull_out"] > 0


def test_capacity_and_record_format(lib, earth):
    """pl_build: entries in increasing leaf order, unused entries 0xFFFF, an overflow record 0xFFFE then 0xFFFF, and a
    smaller capacity turns exactly the longer lists into overflow records."""
    W, H = 320, 184
    s = hrt.preset("random", 1, earth)
    cam = hrt.preset_camera(s.info, W, H)
    blob, info = hrt.scene_blob(s)
    p = hrt.params(W, H, SPP, 50, 3, tuple(s.info.background))
    cells = np.array(_cells(W, H), np.uint32)
    n = len(cells)
    out = {}
    for cap in (8, 2):
        rec = np.zeros((n, 8), np.uint16)
        cnt = np.zeros(n, np.uint32)
        assert lib.pl_build(blob, ctypes.byref(info), ctypes.byref(cam), ctypes.byref(p), cap,
                            cells.ctypes.data_as(ctypes.c_void_p), n, rec.ctypes.data_as(ctypes.c_void_p),
                            cnt.ctypes.data_as(ctypes.c_void_p)) == 0
        out[cap] = (rec, cnt)
        for r, c in zip(rec, cnt):
            if c > cap:
                assert r[0] == 0xFFFE and (r[1:] == 0xFFFF).all()
            else:
                assert (r[c:] == 0xFFFF).all() and (np.diff(r[:c].astype(np.int64)) > 0).all()
                assert (r[:c].astype(np.int64) * 16 < info.walk_bytes).all()
    assert np.array_equal(out[8][1], out[2][1])  # the leaf count does not depend on the capacity
    assert (out[2][1] > 2).any() and (out[2][1] <= 2).any()
    short = out[8][1] <= 2
    assert np.array_equal(out[8][0][short], out[2][0][short])
