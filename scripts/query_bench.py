#!/usr/bin/env python3
"""What ray queries cost (hrt_camera_rays, hrt_scene_intersect) beside their yardstick, the feature pass.  JSON lines,
appended to --out (default profiles/query.jsonl), on C2's scene (`random` at 1920x1080), 4 samples per pixel (8.3 M rays):

  query_camera_rays   (a) hrt_camera_rays for the 4 samples;
  query_intersect     (b) hrt_scene_intersect of those rays, with the scene in LDS and under HRT_QUERY_NO_LDS;
  query_incoherent    (c) a batch of the same size whose origins are (b)'s hit points and whose directions are the normal
                      plus a random unit vector (made with torch on the device), LDS on and off;
  query_features      (d) hrt_accum_add_features of the same 4 samples: the same walk on the same rays;
  query_copy          (e) a device-to-device copy of 96 * n bytes, what a query moves beyond the feature pass;
  query_floor         (f) the same call on the same rays with their times moved outside the declared interval: every
                      ray is invalid, so no lane walks and what remains is the call itself (the counter's allocation and
                      memset, the launch, the staging) and the 96 bytes per ray it reads and writes;
  query_claim         with --claims: (b) and (c), scene in LDS, at each given number of 64-ray blocks per atomicAdd;
  query_verdict       (b) against (d) + 2 x (e), and which of LDS on / off is faster on (b) and on (c).

Every figure is the median of --reps runs, each between two stream synchronisations; the runs of (b), (d) and (e)
alternate in one loop, as the project's A/B records do.  No GPU: the script fails (there is no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9, help="timed runs per figure (the median is reported)")
    ap.add_argument("--claims", default="", help="comma-separated HRT_QUERY_CLAIM values to time (b) and (c) with, e.g. 1,2,4,8,16,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query.jsonl"))
    args = ap.parse_args()
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("query_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def once(run):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def alternate(runs):
        """{name: (median ms, [ms])} of the runs, taken in turn --reps times after one untimed round."""
        for run in runs.values():
            once(run)
        ts = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, run in runs.items():
                ts[k].append(once(run))
        return {k: (round(statistics.median(v), 4), [round(t, 4) for t in v]) for k, v in ts.items()}

    W, H, spp = args.width, args.height, args.samples
    s = hrt.preset("random", 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    p = hrt.params(W, H, spp, 50, 1, tuple(s.info.background))
    n = W * H * spp
    config = {"preset": "random", "width": W, "height": H, "samples": spp, "rays": n, "reps": args.reps}
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, W, H))
    rays = torch.empty((n, 12), dtype=torch.float32, device=dev)
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)
    spare = torch.empty((2 * n, 12), dtype=torch.float32, device=dev)

    def q(flags):
        return hrt.query_params(flags, p.seed, (cam.time0, cam.time1))

    def camera_rays():
        hrt._check(L.hrt_camera_rays(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), sp))

    def intersect(src, flags):
        qq = q(flags)
        return lambda: hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(qq), src.data_ptr(), n, hits.data_ptr(), sp))

    acc = hrt.Accumulator(s, W, H, [(0, 0, W, H)], features=True)

    def features():
        hrt._check(L.hrt_accum_reset(acc.h, sp))
        hrt._check(L.hrt_accum_add_features(acc.h, ctypes.byref(cam), ctypes.byref(p), sp))

    def reset_only():
        hrt._check(L.hrt_accum_reset(acc.h, sp))

    def copy():
        spare[n:].copy_(spare[:n])  # 48 n bytes read and 48 n written: 96 n bytes moved

    camera_rays()
    t = alternate({"camera_rays": camera_rays})
    emit({"metric": "query_camera_rays", **config, "ms": t["camera_rays"][0], "runs_ms": t["camera_rays"][1]})
    t = alternate({"lds": intersect(rays, 0), "no_lds": intersect(rays, hrt.QUERY_NO_LDS), "features": features, "reset": reset_only,
                   "copy": copy})
    b_lds, b_no = t["lds"][0], t["no_lds"][0]
    d = round(t["features"][0] - t["reset"][0], 4)  # the pass alone: the reset that makes it repeatable is timed beside it
    e = t["copy"][0]
    emit({"metric": "query_intersect", **config, "lds_ms": b_lds, "no_lds_ms": b_no, "lds_runs_ms": t["lds"][1], "no_lds_runs_ms": t["no_lds"][1],
          "mrays_per_s": round(n / min(b_lds, b_no) / 1e3, 1), "launch": hrt.last_launch()})
    emit({"metric": "query_features", **config, "ms": d, "with_reset_ms": t["features"][0], "reset_ms": t["reset"][0],
          "runs_ms": t["features"][1]})
    emit({"metric": "query_copy", **config, "bytes": 96 * n, "ms": e, "runs_ms": t["copy"][1], "gb_per_s": round(96 * n / e / 1e6, 1)})
    # (c) the bounce batch: from (b)'s hit points along normal + a random unit vector; misses keep their camera ray
    intersect(rays, 0)()
    torch.cuda.synchronize(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    v = torch.randn((n, 3), generator=gen, device=dev)
    v = v / v.norm(dim=1, keepdim=True)
    hit = (hits.view(torch.int32)[:, 3] & hrt.HIT_HIT) != 0
    bounce = rays.clone()
    bounce[:, 0:3] = torch.where(hit[:, None], hits[:, 4:7], rays[:, 0:3])
    bounce[:, 4:7] = torch.where(hit[:, None], hits[:, 8:11] + v, rays[:, 4:7])
    bounce.view(torch.int32)[:, 11] = 1  # segment 1 of the same paths
    t = alternate({"lds": intersect(bounce, 0), "no_lds": intersect(bounce, hrt.QUERY_NO_LDS)})
    c_lds, c_no = t["lds"][0], t["no_lds"][0]
    emit({"metric": "query_incoherent", **config, "hit_fraction": round(float(hit.float().mean()), 4), "lds_ms": c_lds, "no_lds_ms": c_no,
          "lds_runs_ms": t["lds"][1], "no_lds_runs_ms": t["no_lds"][1], "mrays_per_s": round(n / min(c_lds, c_no) / 1e3, 1)})
    outside = rays.clone()
    outside[:, 8] = cam.time1 + 1.0
    t = alternate({"lds": intersect(outside, 0), "no_lds": intersect(outside, hrt.QUERY_NO_LDS)})
    emit({"metric": "query_floor", **config, "lds_ms": t["lds"][0], "no_lds_ms": t["no_lds"][0], "lds_runs_ms": t["lds"][1],
          "no_lds_runs_ms": t["no_lds"][1]})
    if args.claims:  # blocks of 64 rays per atomicAdd (HRT_QUERY_CLAIM, read at each launch): where the default belongs
        for k in args.claims.split(","):
            os.environ["HRT_QUERY_CLAIM"] = k
            t = alternate({"coherent": intersect(rays, 0), "incoherent": intersect(bounce, 0)})
            emit({"metric": "query_claim", **config, "blocks_per_claim": int(k), "coherent_ms": t["coherent"][0],
                  "incoherent_ms": t["incoherent"][0], "coherent_runs_ms": t["coherent"][1], "incoherent_runs_ms": t["incoherent"][1]})
        del os.environ["HRT_QUERY_CLAIM"]
    best = min(b_lds, b_no)
    emit({"metric": "query_verdict", **config, "intersect_ms": best, "bound_ms": round(d + 2 * e, 4), "meets_bound": bool(best <= d + 2 * e),
          "faster_coherent": "lds" if b_lds <= b_no else "no_lds", "faster_incoherent": "lds" if c_lds <= c_no else "no_lds"})
    acc.close()
    s.close()


if __name__ == "__main__":
    main()
