"""The ABI of the snapshot and per-tile merge entry points without a GPU: libhrt.so exports them, hrt_snapshot_info has
the layout include/hrt/hrt.h states (in C, in the Python binding and in INTEGRATION.md's Rust declaration), no struct
grew (HRT_ABI_VERSION is still 6), and the calls that need no device answer their argument errors."""
import ctypes
import os
import re
import subprocess

import hrt
from conftest import ROOT, tool_env

NEW = ["hrt_accum_snapshot", "hrt_accum_restore", "hrt_accum_snapshot_info", "hrt_accum_merge_tiles"]


def test_new_symbols_are_exported_and_bound():
    L = hrt.load()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in hrt.EXPORTS and getattr(L, name).argtypes is not None
    for method in ("snapshot", "restore", "save", "load", "merge_tiles"):
        assert callable(getattr(hrt.Accumulator, method))
    assert L.hrt_abi_version() == 6 == hrt.ABI_VERSION


def test_snapshot_info_layout(tmp_path):
    fields = ["version", "flags", "width", "height", "n_tiles", "uniform", "n_pixels", "bytes"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hrt/hrt.h"', "int main(void) {",
             '  printf("%d %zu", (int)HRT_ABI_VERSION, sizeof(hrt_snapshot_info));']
    lines += [f'  printf(" %zu", offsetof(hrt_snapshot_info, {f}));' for f in fields]
    lines.append("  return 0;\n}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                          env=tool_env())
    abi, size, *offs = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert abi == 6
    assert size == 40 and offs == [0, 4, 8, 12, 16, 20, 24, 32]
    assert ctypes.sizeof(hrt.SnapshotInfo) == size
    assert [f for f, _ in hrt.SnapshotInfo._fields_] == fields
    assert [getattr(hrt.SnapshotInfo, f).offset for f in fields] == offs
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"#\[repr\(C\)\][^\n]*\npub struct hrt_snapshot_info \{(.*?)\}", doc)
    assert m, "INTEGRATION.md declares hrt_snapshot_info"
    rust = [tuple(x.strip() for x in part.replace("pub ", "").split(":")) for part in m.group(1).split(",")]
    assert rust == [(f, "u32") for f in fields[:6]] + [("n_pixels", "u64"), ("bytes", "u64")]


def test_null_arguments_without_a_device():
    L = hrt.load()
    info, size = hrt.SnapshotInfo(), ctypes.c_uint64()
    assert L.hrt_accum_snapshot_info(None, 0, ctypes.byref(info), None, 0) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_snapshot_info(b"x" * 64, 64, None, None, 0) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_snapshot_info(b"x" * 400, 400, ctypes.byref(info), None, 0) == hrt.ERR_INVALID_ARG
    assert b"malformed" in L.hrt_last_error()
    assert L.hrt_accum_snapshot(None, None, 0, ctypes.byref(size)) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_restore(None, b"x", 1) == hrt.ERR_INVALID_ARG
    assert L.hrt_accum_merge_tiles(None, None, None) == hrt.ERR_INVALID_ARG
