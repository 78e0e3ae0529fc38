"""The block decode of the sphere kernel's claim against the per-item decode, for every item of a launch, on the host.

csrc/lane.h holds both: decode_item (what claim_work runs per lane) and decode_block + take_from_block (what
claim_blocks runs once per claimed 64-item block, then per lane).  tests/native/claim_decode.hip fills the
launch parameters the way hrt_render_tiles_device does and walks every work item.  For each w it checks:
- decode_block(w & ~63) + take_from_block(w) == decode_item(w) in (valid, pxy, slot, sample, sample_end);
- every valid slot < n_chunks * n_out (a wrong slot is an out-of-bounds store on the device);
- every valid pixel lies in a tile of the call, and its slot is the one the tile list gives it;
- each (pixel, chunk) appears exactly once, and none is missing.

Each tile set asserts which tile-lookup path it took, so a case cannot silently stop covering its path.
"""
import ctypes
import os
import subprocess

import pytest

import hrt
from conftest import tool_env
from hrt.tiling import split_tiles

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FAILS = {1: "valid differs", 2: "pxy differs", 3: "slot differs", 4: "samples differ", 5: "slot out of range",
         6: "pixel outside the call's tiles", 7: "(pixel, chunk) twice", 8: "(pixel, chunk) missing",
         9: "a multiple-of-64 rule is broken"}


class Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "total_work", "pad_px", "tile_stride", "n_head", "n_tail", "chunk", "chunk_first", "n_out",
        "padding_items", "past_blocks", "fail_w", "fail_what")]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("claimdecode") / "libclaimdecode.so")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                    "--offload-host-only", *os.environ.get("LANE_SIM_CFLAGS", "").split(),
                    "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc"),
                    os.path.join(HERE, "native", "claim_decode.hip"), "-o", so], check=True, env=tool_env())
    L = ctypes.CDLL(so)
    L.claim_decode_check.restype = ctypes.c_int
    L.claim_decode_check.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_void_p]
    return L


# (name, frame size, the call's tile list, lookup path)
#   one:    a single tile: no lookup
#   search: several tiles the stride rule refuses: binary search over pad_start
#   stride: equal tiles: tile = item / stride, nothing added
#   padded: unequal tiles padded to one stride: blocks past their tile
def _tile_sets():
    sets = [("one_37x19", 37, 19, [(0, 0, 37, 19)], "one")]
    for rank in range(3):
        sets.append((f"grid80_200x90_r{rank}", 200, 90, hrt.tile_grid(200, 90, 80, rank, 3), "search"))
    for rank in range(2):
        sets.append((f"grid16_48x32_r{rank}", 48, 32, split_tiles(48, 32, 2, rank), "stride"))
    # 40x24 over 2 ranks: each share is a 16x16, a half and a half or quarter tile; padding them to one stride would add
    # more than 1/8 idle items, so the stride rule refuses both shares and they take the search
    for rank in range(2):
        sets.append((f"grid16_40x24_r{rank}", 40, 24, split_tiles(40, 24, 2, rank), "search"))
    # eight 16x16 tiles and one 8x16: the rule accepts (2304 <= 2176 x 9/8), and the last tile's second block is padding
    sets.append(("grid16_136x16", 136, 16, split_tiles(136, 16, 1, 0), "padded"))
    return sets


# spp -> (head chunks, tail chunks): one chunk; 3 head, no tail; 2 head + 8 tail; the headline's 30 + 8
SCHEDULES = {1: (1, 0), 40: (3, 0), 48: (2, 8), 500: (30, 8)}


@pytest.mark.parametrize("spp", sorted(SCHEDULES))
def test_block_decode_equals_item_decode(lib, spp):
    for name, W, H, tiles, path in _tile_sets():
        arr = (hrt.Tile * len(tiles))(*[hrt.Tile(*t) for t in tiles])
        info = Info()
        rc = lib.claim_decode_check(ctypes.cast(arr, ctypes.c_void_p), len(tiles), W, H, spp, ctypes.byref(info))
        assert rc == 0, (name, spp, FAILS.get(info.fail_what, rc), info.fail_w)
        assert (info.n_head, info.n_tail) == SCHEDULES[spp], (name, spp)
        n_chunks = info.n_head + info.n_tail
        pixels = sum(t[2] * t[3] for t in tiles)
        assert info.n_out == pixels
        assert info.total_work == info.pad_px * n_chunks
        assert info.total_work - info.padding_items == pixels * n_chunks
        padded = sum(((t[2] + 7) // 8) * ((t[3] + 7) // 8) * 64 for t in tiles)
        if path == "one":
            assert len(tiles) == 1 and info.tile_stride == 0
            assert info.padding_items > 0  # 37x19: partial blocks on both axes
        elif path == "search":
            assert len(tiles) > 1 and info.tile_stride == 0, name
            assert len({t[2] * t[3] for t in tiles}) > 1, name  # uneven tiles
        elif path == "stride":
            assert info.tile_stride > 0 and info.pad_px == padded and info.past_blocks == 0, name
        else:
            assert info.tile_stride > 0 and info.pad_px > padded and info.past_blocks > 0, name
