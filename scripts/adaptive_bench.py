#!/usr/bin/env python3
"""What noise-driven refinement buys: BASELINE config C2 (Random 1920x1080, depth 50) in 80-px tiles and passes of
50 spp.  One JSON line per variant, appended to --out (default profiles/adaptive_refine.jsonl):

  adaptive        hrt.Accumulator(noise=True).refine to --target (mean relative error of a tile): wall time of the
                  whole loop (passes, hrt_accum_noise after each, the host's decisions), the samples rendered, the
                  tiles' sample counts;
  uniform         the same passes over every tile of a plain accumulator, up to the worst tile's sample count;
  uniform_noise   ... of an accumulator that keeps the noise plane (the moment-tracking accumulate kernel end to end).

Every line carries its frame's L-inf and RMSE against the --spp (500) frame of one launch.  Kernel times of the plain
and the moment-tracking accumulate_chunks and of accum_noise come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python scripts/adaptive_bench.py --reps 1` (the profiler slows the host, so
that run's wall times mean nothing).  No GPU: the script fails (there is no fallback)."""
import argparse
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
    ap.add_argument("--spp", type=int, default=500, help="samples of the frame the variants are compared with, and their cap")
    ap.add_argument("--pass-spp", type=int, default=50)
    ap.add_argument("--target", type=float, default=0.04, help="refine until every tile's mean relative error is at most this")
    ap.add_argument("--floor", type=float, default=0.05)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--preset", default="random")
    ap.add_argument("--reps", type=int, default=3, help="timed runs per variant (the median is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_refine.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    s = hrt.preset(args.preset, 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    tiles = hrt.tile_grid(W, H, args.tile)
    config = {"preset": args.preset, "width": W, "height": H, "tile": args.tile, "tiles": len(tiles), "pass_spp": args.pass_spp,
              "target": args.target, "floor": args.floor, "max_spp": args.spp, "depth": args.depth, "reps": args.reps}
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def frame_of(acc):
        px, off = acc.resolve(), 0
        img = np.zeros((H, W, 4), np.float32)
        for x, y, tw, th in tiles:
            img[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, 4)
            off += tw * th
        return img

    def timed(run):
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    def against(img):
        d = (img[..., :3] - ref[..., :3]).astype(np.float64)
        return {"linf_to_ref": float(np.abs(d).max()), "rmse_to_ref": float(np.sqrt((d * d).mean()))}

    p_all = hrt.params(W, H, args.spp, args.depth, 1, bg)
    ref = hrt.render(s, cam, p_all)

    # adaptive: the warm-up run fixes the schedule (it is deterministic), the timed runs repeat it
    p1 = hrt.params(W, H, 1, args.depth, 1, bg)
    acc = hrt.Accumulator(s, W, H, tiles, noise=True)
    passes = []
    rec = acc.refine(cam, p1, args.target, args.pass_spp, args.spp, args.floor, on_pass=lambda t, r: passes.append(len(t)))
    held = acc.tile_samples
    px_of = [t[2] * t[3] for t in tiles]
    rendered = sum(n * c for n, c in zip(held, px_of))
    img = frame_of(acc)

    def adaptive():
        acc.reset()
        acc.refine(cam, p1, args.target, args.pass_spp, args.spp, args.floor)

    dt, ts = timed(adaptive)
    assert acc.tile_samples == held
    hist = {str(n): held.count(n) for n in sorted(set(held))}
    emit({"metric": "adaptive_refine", "variant": "adaptive", "ms": round(dt * 1e3, 2), "ms_runs": [round(t * 1e3, 2) for t in ts],
          "passes": len(passes), "tiles_per_pass": passes, "samples_rendered": rendered, "tiles_by_samples": hist,
          "worst_tile_mean": max(r.mean for r in rec), "tiles_over_target": sum(r.mean > args.target for r in rec),
          **against(img), "config": config})
    acc.close()

    worst = max(held)
    ps = [hrt.params(W, H, args.pass_spp, args.depth, 1, bg, sample_offset=b) for b in range(0, worst, args.pass_spp)]
    for variant, noise in (("uniform", False), ("uniform_noise", True)):
        u = hrt.Accumulator(s, W, H, tiles, noise=noise)

        def uniform():
            u.reset()
            for p in ps:
                u.add(cam, p)

        uniform()
        dtu, tsu = timed(uniform)
        emit({"metric": "adaptive_refine", "variant": variant, "ms": round(dtu * 1e3, 2), "ms_runs": [round(t * 1e3, 2) for t in tsu],
              "passes": len(ps), "samples_rendered": worst * W * H, "spp": worst, "adaptive_speedup": round(dtu / dt, 3),
              "adaptive_sample_ratio": round(rendered / (worst * W * H), 4), **against(frame_of(u)), "config": config})
        if noise:
            t0 = time.perf_counter()
            for _ in range(10):
                u.noise(args.floor)
            emit({"metric": "adaptive_refine", "variant": "noise_call", "ms": round((time.perf_counter() - t0) * 100, 3),
                  "note": "one hrt_accum_noise call: kernel, records back, stream synchronise", "config": config})
        u.close()
    sink.close()


if __name__ == "__main__":
    main()
