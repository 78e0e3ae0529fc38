#!/usr/bin/env python3
"""What the variance-guided preview filter costs and what it buys (hrt_accum_resolve_filtered).  JSON lines, appended
to --out (default profiles/filter_refine.jsonl):

  filter_wall      at 1920x1080 (C2, whole-frame HRT_ACCUM_NOISE accumulator): one filtered resolve into device memory
                   for iterations 1, 3 and 5, beside the plain hrt_accum_resolve and a 16-spp and a 50-spp pass of
                   the same run (median of --reps, each between two stream synchronisations);
  filter_lds_switch  5 iterations with the steps up to K = 0, 1, 2, 4, 8 staged in LDS and the others read from global
                   memory (HRT_FILTER_LDS_STEP): where the switch belongs;
  filter_quality   C2 after 1, 2 and 4 passes of 16 spp: RMSE (display units) of the plain and of the filtered frame
                   against the 500-spp frame; Cornell at 512x512 after 2 and 8 passes of 50 spp against its 5000-spp
                   frame.  A state the filter refuses (one chunk: no variance estimate) is reported as such.
  filter_kernel    with --stats CSV (the kernel stats of a run of this script under
                   `rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/filter_bench.py --reps 1
                   --wall-only`): every filter kernel's calls and average time, and for filter_atrous the achieved
                   bytes/s over its compulsory traffic (read one plane, write one: 2 x 16 B per pixel); the rows are
                   copied to --stats-out (default profiles/filter_kernel_stats.csv).

The profiler slows the host, so that run's wall times mean nothing.  No GPU: the script fails (there is no fallback)."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))


def kernel_stats(args, emit):
    rows = [r for r in csv.DictReader(open(args.stats)) if "filter_" in r["Name"] or "accum_resolve" in r["Name"]]
    if not rows:
        raise SystemExit(f"{args.stats}: no filter kernels in it")
    with open(args.stats_out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        wr.writeheader()
        wr.writerows(rows)
    compulsory = 2 * 16 * args.width * args.height
    for r in rows:
        name = r["Name"].split("(anonymous namespace)::")[-1].split("(")[0]
        rec = {"metric": "filter_kernel", "kernel": name, "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
               "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        if name.startswith("filter_atrous"):
            rec["compulsory_bytes"] = compulsory
            rec["achieved_GBps_avg"] = round(compulsory / float(r["AverageNs"]), 1)
            rec["achieved_GBps_best"] = round(compulsory / float(r["MinNs"]), 1)
        emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5, help="timed runs per figure (the median is reported)")
    ap.add_argument("--wall-only", action="store_true", help="skip the quality lines (a run under the profiler)")
    ap.add_argument("--tile", type=int, default=0, help="tile size of the timed accumulator (0: one whole-frame tile)")
    ap.add_argument("--stats", help="a rocprofv3 kernel-stats CSV to summarise instead of running anything")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "filter_kernel_stats.csv"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_refine.jsonl"))
    args = ap.parse_args()
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    if args.stats:
        kernel_stats(args, emit)
        return
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("filter_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()

    def timed(run):
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return round(statistics.median(ts) * 1e3, 3), [round(t * 1e3, 3) for t in ts]

    def rmse(img, ref):
        d = (img[..., :3] - ref[..., :3]).astype(np.float64)
        return float(np.sqrt((d * d).mean()))

    # ---- wall time at the C2 frame size
    W, H = args.width, args.height
    s = hrt.preset("random", 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    tiles = hrt.tile_grid(W, H, args.tile) if args.tile else None
    config = {"preset": "random", "width": W, "height": H, "tile": args.tile, "sigma": args.sigma, "depth": args.depth, "reps": args.reps}
    acc = hrt.Accumulator(s, W, H, tiles, noise=True)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    buf = torch.empty(W * H * 4, dtype=torch.float32, device=dev)
    bp = ctypes.c_void_p(buf.data_ptr())
    offset = [0]

    def a_pass(spp):
        def run():
            acc.add(cam, hrt.params(W, H, spp, args.depth, 1, bg, sample_offset=offset[0]))
            offset[0] += spp
        return run

    a_pass(16)()   # warm-up: kernels loaded, the scene's buffers made
    a_pass(50)()
    wall = {"metric": "filter_wall", "config": config}
    wall["pass_16spp_ms"], wall["pass_16spp_runs"] = timed(a_pass(16))
    wall["pass_50spp_ms"], wall["pass_50spp_runs"] = timed(a_pass(50))

    def plain():
        hrt._check(L.hrt_accum_resolve(acc.h, hrt.ACCUM_F32, bp, sp))

    plain()
    wall["accum_resolve_ms"], wall["accum_resolve_runs"] = timed(plain)
    for it in (1, 3, 5):
        f = hrt.filter_params(it, args.sigma)

        def filtered():
            hrt._check(L.hrt_accum_resolve_filtered(acc.h, ctypes.byref(f), hrt.ACCUM_F32, bp, sp))

        filtered()   # the first call allocates the planes
        wall[f"filtered_{it}_ms"], wall[f"filtered_{it}_runs"] = timed(filtered)
    wall["samples_held"] = acc.samples
    emit(wall)
    # where the LDS / global switch belongs: 5 iterations (steps 1 .. 16) with the steps up to K staged in LDS
    # (HRT_FILTER_LDS_STEP, an A/B knob between bit-identical variants; unset: the library's default)
    f5 = hrt.filter_params(5, args.sigma)

    def five():
        hrt._check(L.hrt_accum_resolve_filtered(acc.h, ctypes.byref(f5), hrt.ACCUM_F32, bp, sp))

    switch = {"metric": "filter_lds_switch", "iterations": 5, "config": config}
    for k in (0, 1, 2, 4, 8):
        os.environ["HRT_FILTER_LDS_STEP"] = str(k)
        five()
        switch[f"lds_up_to_{k}_ms"], switch[f"lds_up_to_{k}_runs"] = timed(five)
    del os.environ["HRT_FILTER_LDS_STEP"]
    emit(switch)
    acc.close()
    if args.wall_only:
        return

    # ---- quality
    def quality(name, scene, w, h, pass_spp, after, ref_spp):
        c = hrt.preset_camera(scene.info, w, h)
        b = tuple(scene.info.background)
        ref = hrt.render(scene, c, hrt.params(w, h, ref_spp, args.depth, 1, b))
        a = hrt.Accumulator(scene, w, h, noise=True)
        for k in range(max(after)):
            a.add(c, hrt.params(w, h, pass_spp, args.depth, 1, b, sample_offset=k * pass_spp))
            if k + 1 not in after:
                continue
            rec = {"metric": "filter_quality", "preset": name, "width": w, "height": h, "pass_spp": pass_spp, "passes": k + 1,
                   "spp": (k + 1) * pass_spp, "ref_spp": ref_spp, "sigma": args.sigma, "chunks": a.noise()[0].chunks,
                   "rmse_plain": rmse(a.resolve(), ref)}
            for it in (1, 3, 5):
                try:
                    rec[f"rmse_filtered_{it}"] = rmse(a.resolve(denoise=dict(iterations=it, sigma=args.sigma)), ref)
                    rec[f"ratio_{it}"] = round(rec[f"rmse_filtered_{it}"] / rec["rmse_plain"], 4)
                except hrt.HrtError as e:
                    rec[f"rmse_filtered_{it}"] = None
                    rec["refused"] = f"status {e.status}: {e}"
            emit(rec)
        a.close()

    quality("random", s, W, H, 16, (1, 2, 4), 500)
    s.close()
    c5 = hrt.preset("cornell", 1)
    c5.commit(0)
    quality("cornell", c5, 512, 512, 50, (2, 8), 5000)
    c5.close()
    sink.close()


if __name__ == "__main__":
    main()
