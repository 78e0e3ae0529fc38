#!/usr/bin/env python3
"""What the first-hit feature pass and the feature-guided preview filter cost and what they buy
(hrt_accum_add_features, hrt_accum_resolve_guided).  JSON lines, appended to --out (default
profiles/guided_refine.jsonl):

  guided_wall       at 1920x1080 (C2, whole-frame accumulator with noise and feature planes): a feature pass of 4 and of
                    16 samples beside a radiance pass of the same sample counts; one guided resolve into device memory
                    for iterations 1, 3 and 5 beside the variance-only filtered resolve of the same iterations (median
                    of --reps, each between two stream synchronisations);
  guided_block      the 16-sample feature pass with the wave's pixel block 64x1, 32x2, 16x4, 8x8, 4x16
                    (HRT_FEATURE_BLOCK_W, read when the accumulator is created): which shape belongs in the kernel;
  guided_lds_switch 3 and 5 iterations with the feature planes staged in LDS for the steps up to K = 0, 1, 2, 4
                    (HRT_GUIDED_LDS_STEP): where that switch belongs;
  guided_quality    RMSE (display units) of the plain, variance-only and guided frame with the default tolerances: C2
                    after 2 and 4 passes of 16 spp against its 500-spp frame, Cornell at 512x512 after 2 and 8 passes of
                    50 spp against its 5000-spp frame, each with a 16-sample feature pass;
  guided_sweep      the same two states (C2 at 32 spp, Cornell at 100 spp) over a grid of tolerances.
  guided_kernel     with --stats CSV (the kernel stats of `rocprofv3 --kernel-trace --stats --output-format csv -- python
                    scripts/guided_bench.py --reps 1 --wall-only`): every feature / guided kernel's calls and average
                    time; the rows are copied to --stats-out (default profiles/guided_kernel_stats.csv).

The profiler slows the host, so that run's wall times mean nothing.  No GPU: the script fails (there is no fallback)."""
import argparse
import csv
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))


def kernel_stats(args, emit):
    rows = [r for r in csv.DictReader(open(args.stats)) if any(k in r["Name"] for k in ("feature_", "guided_", "filter_"))]
    if not rows:
        raise SystemExit(f"{args.stats}: no feature or guided kernels in it")
    with open(args.stats_out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
        wr.writeheader()
        wr.writerows(rows)
    for r in rows:
        name = r["Name"].split("(anonymous namespace)::")[-1].split("(")[0]
        emit({"metric": "guided_kernel", "kernel": name, "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
              "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=5, help="timed runs per figure (the median is reported)")
    ap.add_argument("--wall-only", action="store_true", help="skip the quality and sweep lines (a run under the profiler)")
    ap.add_argument("--stats", help="a rocprofv3 kernel-stats CSV to summarise instead of running anything")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "guided_kernel_stats.csv"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_refine.jsonl"))
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
        raise SystemExit("guided_bench.py: no GPU")
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

    W, H = args.width, args.height
    s = hrt.preset("random", 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    config = {"preset": "random", "width": W, "height": H, "sigma": args.sigma, "depth": args.depth, "reps": args.reps,
              "tolerances": hrt.GUIDED_DEFAULTS}
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    buf = torch.empty(W * H * 4, dtype=torch.float32, device=dev)
    bp = ctypes.c_void_p(buf.data_ptr())

    def passes(acc):
        offset, foffset = [0], [0]

        def radiance(spp):
            def run():
                acc.add(cam, hrt.params(W, H, spp, args.depth, 1, bg, sample_offset=offset[0]))
                offset[0] += spp
            return run

        def features(spp):
            def run():
                p = hrt.params(W, H, spp, args.depth, 1, bg, sample_offset=foffset[0])
                hrt._check(L.hrt_accum_add_features(acc.h, ctypes.byref(cam), ctypes.byref(p), sp))
                foffset[0] += spp
            return run
        return radiance, features

    # ---- wall time at the C2 frame size
    acc = hrt.Accumulator(s, W, H, None, noise=True, features=True)
    radiance, features = passes(acc)
    radiance(16)()   # warm-up: kernels loaded, the scene's buffers made
    radiance(16)()
    features(16)()
    wall = {"metric": "guided_wall", "config": config}
    for n in (4, 16):
        wall[f"feature_pass_{n}_ms"], wall[f"feature_pass_{n}_runs"] = timed(features(n))
        wall[f"radiance_pass_{n}_ms"], wall[f"radiance_pass_{n}_runs"] = timed(radiance(n))
    for it in (1, 3, 5):
        f, g = hrt.filter_params(it, args.sigma), hrt.guided_params(it, args.sigma)

        def filtered():
            hrt._check(L.hrt_accum_resolve_filtered(acc.h, ctypes.byref(f), hrt.ACCUM_F32, bp, sp))

        def guided():
            hrt._check(L.hrt_accum_resolve_guided(acc.h, ctypes.byref(g), hrt.ACCUM_F32, bp, sp))

        filtered()   # the first calls allocate the planes
        guided()
        wall[f"filtered_{it}_ms"], wall[f"filtered_{it}_runs"] = timed(filtered)
        wall[f"guided_{it}_ms"], wall[f"guided_{it}_runs"] = timed(guided)
    wall["samples_held"], wall["feature_samples_held"] = acc.samples, acc.feature_samples
    emit(wall)
    # where the feature planes' LDS / global switch belongs (an A/B knob between bit-identical variants)
    for it in (3, 5):
        g = hrt.guided_params(it, args.sigma)

        def guided():
            hrt._check(L.hrt_accum_resolve_guided(acc.h, ctypes.byref(g), hrt.ACCUM_F32, bp, sp))

        switch = {"metric": "guided_lds_switch", "iterations": it, "config": config}
        for k in (0, 1, 2, 4):
            os.environ["HRT_GUIDED_LDS_STEP"] = str(k)
            guided()
            switch[f"features_in_lds_up_to_{k}_ms"], switch[f"features_in_lds_up_to_{k}_runs"] = timed(guided)
        del os.environ["HRT_GUIDED_LDS_STEP"]
        emit(switch)
    acc.close()
    # the wave's block shape
    block = {"metric": "guided_block", "samples": 16, "config": config}
    for bw in (64, 32, 16, 8, 4):
        os.environ["HRT_FEATURE_BLOCK_W"] = str(bw)
        shaped = hrt.Accumulator(s, W, H, None, features=True)
        del os.environ["HRT_FEATURE_BLOCK_W"]
        _, features = passes(shaped)
        features(16)()
        block[f"block_{bw}x{64 // bw}_ms"], block[f"block_{bw}x{64 // bw}_runs"] = timed(features(16))
        shaped.close()
    emit(block)
    if args.wall_only:
        return

    # ---- quality and the tolerance sweep
    grid = list(itertools.product((0.05, 0.1, 0.2, 0.5), (0.05, 0.1, 0.2), (0.05, 0.1, 0.2)))

    def quality(name, scene, w, h, pass_spp, after, ref_spp, sweep_at):
        c = hrt.preset_camera(scene.info, w, h)
        b = tuple(scene.info.background)
        ref = hrt.render(scene, c, hrt.params(w, h, ref_spp, args.depth, 1, b))
        a = hrt.Accumulator(scene, w, h, noise=True, features=True)
        a.add_features(c, hrt.params(w, h, 16, args.depth, 1, b))
        den = dict(iterations=3, sigma=args.sigma)
        for k in range(max(after)):
            a.add(c, hrt.params(w, h, pass_spp, args.depth, 1, b, sample_offset=k * pass_spp))
            if k + 1 not in after:
                continue
            base = {"preset": name, "width": w, "height": h, "spp": (k + 1) * pass_spp, "feature_samples": 16, "ref_spp": ref_spp,
                    "sigma": args.sigma, "iterations": 3}
            plain, filt = rmse(a.resolve(), ref), rmse(a.resolve(denoise=den), ref)
            guided = rmse(a.resolve_guided(denoise=den), ref)
            emit({"metric": "guided_quality", **base, "tolerances": hrt.GUIDED_DEFAULTS, "rmse_plain": plain, "rmse_filtered": filt,
                  "rmse_guided": guided, "guided_over_filtered": round(guided / filt, 4), "guided_over_plain": round(guided / plain, 4)})
            if k + 1 != sweep_at:
                continue
            rows = [[tn, ta, td, round(rmse(a.resolve_guided(denoise=den, guide=dict(normal=tn, albedo=ta, depth=td)), ref) / plain, 4)]
                    for tn, ta, td in grid]
            emit({"metric": "guided_sweep", **base, "rmse_plain": plain, "rmse_filtered": filt,
                  "columns": ["normal", "albedo", "depth", "guided_over_plain"], "rows": rows})
        a.close()

    quality("random", s, W, H, 16, (2, 4), 500, 2)
    s.close()
    c5 = hrt.preset("cornell", 1)
    c5.commit(0)
    quality("cornell", c5, 512, 512, 50, (2, 8), 5000, 2)
    c5.close()
    sink.close()


if __name__ == "__main__":
    main()
