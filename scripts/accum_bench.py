#!/usr/bin/env python3
"""The cost of refining: BASELINE config C2 (Random 1920x1080, 500 spp, depth 50) as ONE hrt_render_tiles_device
launch (the yardstick) against the same 500 samples added to an hrt_accum in passes of 16 / 50 / 125 spp, with and
without a preview resolved by the pass's own accumulate kernel (hrt_accum_add_resolve).  One JSON line per variant:
Mrays/s (the frame's world.hit calls, identical for every pass split since a path is keyed by its pixel and sample
index, over the wall time of the enqueued frame ending in a device synchronise) and the ratio to the one-shot line.

    python scripts/accum_bench.py [--width 1920 --height 1080 --spp 500 --passes 16,50,125 --reps 3]

Kernel times of accumulate_chunks / accum_resolve alone come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python scripts/accum_bench.py --reps 1` (the profiler slows the host, so its
run gives no rates).  No GPU: the script fails (there is no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))

import torch  # noqa: E402

import hrt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--preset", default="random")
    ap.add_argument("--passes", default="16,50,125", help="pass sizes (spp), comma separated")
    ap.add_argument("--reps", type=int, default=3, help="timed frames per variant (the median is reported)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()
    W, H = args.width, args.height
    s = hrt.preset(args.preset, 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    out = torch.empty(W * H * 4, dtype=torch.float32, device=dev)
    config = {"preset": args.preset, "width": W, "height": H, "spp": args.spp, "depth": args.depth, "reps": args.reps}

    def timed(frame):
        """median wall seconds of `frame()` (enqueue only) + the device synchronise that ends it"""
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            frame()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), ts

    # the yardstick: one launch of all the samples (the warm-up run counts the frame's rays)
    p_all = hrt.params(W, H, args.spp, args.depth, 1, bg)
    st = hrt.render_tiles_device(s, cam, p_all, [(0, 0, W, H)], out.data_ptr(), 0, want_stats=True)
    segments = st.segments
    dt, ts = timed(lambda: hrt.render_tiles_device(s, cam, p_all, [(0, 0, W, H)], out.data_ptr(), 0))
    s.synchronize()
    one_shot = segments / dt / 1e6
    print(json.dumps({"metric": "accum_refine", "variant": "one_shot", "mrays_per_s": round(one_shot, 1),
                      "ms_per_frame": round(dt * 1e3, 2), "ms_runs": [round(t * 1e3, 2) for t in ts], "ratio_to_one_shot": 1.0,
                      "segments": segments, "config": config, "launch": hrt.last_launch()}), flush=True)

    acc = hrt.Accumulator(s, W, H)
    for n in [int(x) for x in args.passes.split(",")]:
        ranges = [(b, min(b + n, args.spp)) for b in range(0, args.spp, n)]
        ps = [hrt.params(W, H, e - b, args.depth, 1, bg, sample_offset=b) for b, e in ranges]
        # warm-up with stats: every pass shape runs once, and the passes' rays must add up to the one-shot frame's
        acc.reset()
        total = sum(acc.add(cam, p, stats=True).segments for p in ps)
        if total != segments or acc.samples != args.spp:
            raise SystemExit(f"accum_bench.py: passes of {n} traced {total} rays, the one-shot frame {segments}")
        for preview in (False, True):
            def frame():
                _check(L.hrt_accum_reset(acc.h, None))
                for p in ps:
                    if preview:
                        _check(L.hrt_accum_add_resolve(acc.h, ctypes.byref(cam), ctypes.byref(p), hrt.ACCUM_F32,
                                                       ctypes.c_void_p(out.data_ptr()), None, None))
                    else:
                        _check(L.hrt_accum_add(acc.h, ctypes.byref(cam), ctypes.byref(p), None, None))

            frame()  # warm-up of this variant's accumulate kernel
            dt, ts = timed(frame)
            s.synchronize()
            rate = segments / dt / 1e6
            print(json.dumps({"metric": "accum_refine", "variant": f"passes_{n}" + ("_preview" if preview else ""),
                              "pass_spp": n, "passes": len(ps), "preview_per_pass": preview, "mrays_per_s": round(rate, 1),
                              "ms_per_frame": round(dt * 1e3, 2), "ms_per_pass": round(dt * 1e3 / len(ps), 3),
                              "ms_runs": [round(t * 1e3, 2) for t in ts], "ratio_to_one_shot": round(rate / one_shot, 4),
                              "config": config}), flush=True)
    acc.close()


def _check(st):
    if st != hrt.OK:
        raise hrt.HrtError(st, hrt.load().hrt_last_error().decode())


if __name__ == "__main__":
    main()
