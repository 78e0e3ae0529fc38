#!/usr/bin/env python3
"""What a checkpoint costs: BASELINE config C2's accumulator (1920x1080 in 336 tiles of 80 px) with the noise plane and
the feature planes, holding a whole-frame pass, a pass over a third of the tiles and a feature pass.  One JSON line per
figure, appended to --out (default profiles/snapshot.jsonl):

  bare_copy_d2h / _h2d   the yardstick, in the same run: one copy of the same plane bytes (52 B per pixel) between a
                         device tensor and a pageable host tensor through torch (hipMemcpy), each direction;
  snapshot               hrt_accum_snapshot into a caller-owned buffer (device wait, header and ledgers, four plane copies,
                         checksum);
  snapshot_bytes_object  Accumulator.snapshot(): the same plus the buffer's allocation and its copy into a bytes object;
  snapshot_info          hrt_accum_snapshot_info alone: validation and the checksum pass over the blob, no device;
  restore                hrt_accum_restore into a reset accumulator (validation, checksum, four plane copies);
  merge_tiles_subset     hrt_accum_merge_tiles of an accumulator that holds a pass on a third of the tiles;
  merge_tiles_all / merge  hrt_accum_merge_tiles and hrt_accum_merge of one that holds a whole-frame pass.

Every line carries its ratio to the bare copy of its direction where there is one.  No GPU: the script fails (there is
no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))

import torch  # noqa: E402

import hrt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tile", type=int, default=80)
    ap.add_argument("--pass-spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--preset", default="random")
    ap.add_argument("--reps", type=int, default=7, help="timed runs per figure (the median is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    W, H, spp = args.width, args.height, args.pass_spp
    s = hrt.preset(args.preset, 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    tiles = hrt.tile_grid(W, H, args.tile)
    third = list(range(0, len(tiles), 3))
    L = hrt.load()
    sink = open(args.out, "a")

    def params(offset):
        return hrt.params(W, H, spp, args.depth, 1, bg, sample_offset=offset)

    def accumulator(passes):
        a = hrt.Accumulator(s, W, H, tiles, noise=True, features=True)
        for offset, subset in passes:
            a.add(cam, params(offset), tiles=subset)
        return a

    def timed(run, before=None):
        ts = []
        for _ in range(args.reps + 1):   # the first run warms up (first-touch page faults, lazy allocations) and is dropped
            if before:
                before()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[1:]), ts[1:]

    acc = accumulator([(0, None), (spp, third)])
    acc.add_features(cam, hrt.params(W, H, 4, args.depth, 1, bg))
    size = acc.snapshot_size()
    plane_bytes = acc.n_pixels * 52
    config = {"preset": args.preset, "width": W, "height": H, "tile": args.tile, "tiles": len(tiles), "pass_spp": spp,
              "flags": "NOISE|FEATURES", "blob_bytes": size, "plane_bytes": plane_bytes, "reps": args.reps}

    def emit(variant, ms, runs, **more):
        rec = {"metric": "snapshot", "variant": variant, "ms": round(ms, 3), "ms_runs": [round(t, 3) for t in runs], **more,
               "config": config}
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    # the yardstick: the same bytes through torch, pageable host memory as a caller's buffer is
    d_bytes = torch.empty(plane_bytes, dtype=torch.uint8, device=dev)
    h_bytes = torch.empty(plane_bytes, dtype=torch.uint8)
    d2h, runs = timed(lambda: h_bytes.copy_(d_bytes))
    emit("bare_copy_d2h", d2h, runs, gb_per_s=round(plane_bytes / d2h / 1e6, 2))
    h2d, runs = timed(lambda: d_bytes.copy_(h_bytes))
    emit("bare_copy_h2d", h2d, runs, gb_per_s=round(plane_bytes / h2d / 1e6, 2))

    buf = np.empty(size, np.uint8)
    ms, runs = timed(lambda: acc.snapshot_into(buf))
    emit("snapshot", ms, runs, ratio_to_bare_copy=round(ms / d2h, 3))
    snap_ms = ms
    ms, runs = timed(lambda: acc.snapshot())
    emit("snapshot_bytes_object", ms, runs, ratio_to_bare_copy=round(ms / d2h, 3))
    info = hrt.SnapshotInfo()
    ms, runs = timed(lambda: hrt._check(L.hrt_accum_snapshot_info(buf.ctypes.data, size, ctypes.byref(info), None, 0)))
    emit("snapshot_info", ms, runs, gb_per_s=round(size / ms / 1e6, 2), share_of_snapshot=round(ms / snap_ms, 3),
         note="validation and the checksum pass alone, no device")
    target = hrt.Accumulator(s, W, H, tiles, noise=True, features=True)
    ms, runs = timed(lambda: hrt._check(L.hrt_accum_restore(target.h, buf.ctypes.data, size)), before=target.reset)
    emit("restore", ms, runs, ratio_to_bare_copy=round(ms / h2d, 3))
    assert target.snapshot() == buf.tobytes()

    # merges: dst is put back from the blob before every run
    def put_back():
        target.reset()
        target.restore(buf)

    src_subset = accumulator([(4 * spp, third)])
    ms, runs = timed(lambda: target.merge_tiles(src_subset), before=put_back)
    emit("merge_tiles_subset", ms, runs, tiles=len(third), pixels=sum(tiles[t][2] * tiles[t][3] for t in third))
    src_all = accumulator([(4 * spp, None)])
    ms, runs = timed(lambda: target.merge_tiles(src_all), before=put_back)
    emit("merge_tiles_all", ms, runs, tiles=len(tiles), pixels=acc.n_pixels)
    uniform = accumulator([(0, None)])
    u_blob = uniform.snapshot()

    def put_back_uniform():
        uniform.reset()
        uniform.restore(u_blob)

    ms, runs = timed(lambda: uniform.merge(src_all), before=put_back_uniform)
    emit("merge", ms, runs, tiles=len(tiles), pixels=acc.n_pixels, note="hrt_accum_merge of two uniform accumulators: two kernels")
    for a in (acc, target, src_subset, src_all, uniform):
        a.close()
    sink.close()


if __name__ == "__main__":
    main()
