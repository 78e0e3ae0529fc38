#!/usr/bin/env python3
"""What the noise estimate of the filtered frame (hrt_accum_noise_filtered) costs, what refining on it saves, and how far
it is from the filtered frame's real error.  JSON lines, appended to --out (default profiles/filtered_noise.jsonl):

  noise_filtered_cost   at 1920x1080 (C2, 336 tiles of 80 px, noise and feature planes): hrt_accum_noise_filtered at 1, 3
                        and 5 iterations, variance-only and guided, against a filtered resolve of the same settings into
                        device memory plus one hrt_accum_noise, in one process, the two alternating (--reps pairs, each
                        run between two stream synchronisations): median, fastest, slowest;
  resolve_timing        hrt_accum_resolve_filtered and hrt_accum_resolve_guided (the calls that existed before) at 1, 3
                        and 5 iterations, one line per run, tagged with the library that ran (--label):
                        `--resolve-only` prints this line alone, and `--against LIB` starts such runs in child processes,
                        this build and LIB (HRT_LIB) alternating, --runs each after a discarded one each, and reports this
                        build's slowest run against the other's fastest, relative to the larger spread;
  refine_saving         Accumulator.refine against refine_filtered (target 0.04, passes of 50, at most 500) on C2 at
                        1920x1080 and on Cornell at 512x512: samples rendered, wall time, passes, and the RMSE (display
                        units) of the frame each policy shows, the plain one for refine and the filtered one for
                        refine_filtered, against the 500-spp (Cornell: 5000-spp) frame; the filtered frame of refine's
                        state and the plain frame of refine_filtered's for comparison;
  calibration           per tile, the RMS relative error of the filtered frame's luminance against the converged frame
                        (floored as the estimate's denominator is) over the tile's predicted mean: the median and the
                        worst tile, on C2 at 32 spp, Cornell at 100 spp and `random` at 64x36 and 126 spp against
                        tests/golden's 4096-spp frame;
  flat_field            the same ratio on the synthetic flat field of tests/test_noise_filtered_host.py at 1 to 5
                        iterations, through the host's arithmetic (no GPU needed: --flat-only).

No GPU: everything but --flat-only fails (there is no fallback)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))
FLOOR = 0.05
TOL = dict(normal=0.1, albedo=0.1, depth=0.1)


def against(args, emit):
    """This build and args.against alternating in child processes, after one discarded run of each; which of the two
    goes first alternates from pair to pair."""
    runs = {"this": [], "other": []}
    order = ["this", "other"] + [w for k in range(args.runs) for w in (("this", "other") if k % 2 == 0 else ("other", "this"))]
    for k, which in enumerate(order):
        env = dict(os.environ)
        env.pop("HRT_LIB", None)
        if which == "other":
            env["HRT_LIB"] = os.path.abspath(args.against)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--resolve-only", "--label", which, "--reps", str(args.reps),
                              "--out", os.devnull], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            raise SystemExit(f"filtered_noise_bench.py: the {which} run failed:\n{out.stderr}")
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        if k < 2:
            rec["discarded"] = "warm-up"
        else:
            runs[which].append(rec)
        emit(rec)
    for kind in ("filtered", "guided"):
        for it in (1, 3, 5):
            key = f"{kind}_{it}_ms"
            t, o = [r[key] for r in runs["this"]], [r[key] for r in runs["other"]]
            spread = max(max(t) - min(t), max(o) - min(o))
            emit({"metric": "resolve_verdict", "resolve": kind, "iterations": it, "this_ms": t, "other_ms": o, "other": args.against,
                  "this_spread_ms": round(max(t) - min(t), 4), "other_spread_ms": round(max(o) - min(o), 4),
                  "this_slowest_minus_other_fastest_ms": round(max(t) - min(o), 4), "larger_spread_ms": round(spread, 4),
                  "beyond_spread": bool(max(t) - min(o) > spread)})


def flat_field(emit):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_noise_filtered_host as TH

    import hrt

    tiles = [(0, 0, TH.SIZE, TH.SIZE)]
    for it in (1, 2, 3, 4, 5):
        ratios = []
        for seed in range(TH.SEEDS):
            r = TH.flat_field(seed)
            err, _ = hrt.debug_noise_filtered(r, None, None, it, 4.0, tiles, floor=FLOOR)
            ratios.append(TH.calibration(hrt.debug_filter(r, it, 4.0), err))
        emit({"metric": "flat_field", "iterations": it, "sigma": 4.0, "size": TH.SIZE, "chunks": TH.CHUNKS, "seeds": TH.SEEDS,
              "actual_over_predicted": [round(x, 4) for x in ratios], "mean": round(float(np.mean(ratios)), 4),
              "sd": round(float(np.std(ratios)), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--reps", type=int, default=21, help="timed runs per figure (the median is reported)")
    ap.add_argument("--runs", type=int, default=4, help="--against: processes per library")
    ap.add_argument("--resolve-only", action="store_true", help="time the two resolves that existed before (one resolve_timing line)")
    ap.add_argument("--flat-only", action="store_true", help="the flat-field calibration alone (host arithmetic)")
    ap.add_argument("--skip", default="", help="comma-separated sections to skip: cost, saving, calibration, flat")
    ap.add_argument("--label", default="this")
    ap.add_argument("--against", help="another build's libhrt.so: alternate child processes and report the verdict")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_noise.jsonl"))
    args = ap.parse_args()
    sink = open(args.out, "a")
    skip = set(filter(None, args.skip.split(",")))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    if args.against:
        return against(args, emit)
    if args.flat_only:
        return flat_field(emit)
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("filtered_noise_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def once(run):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 4), "fastest_ms": round(min(ms), 4), "slowest_ms": round(max(ms), 4)}

    def rmse(img, ref):
        d = (img[..., :3] - ref[..., :3]).astype(np.float64)
        return float(np.sqrt((d * d).mean()))

    def unpack(a, px):
        frame = np.zeros((a.height, a.width, px.shape[-1]), px.dtype)
        off = 0
        for x, y, tw, th in a.tiles:
            frame[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, -1)
            off += tw * th
        return frame

    W, H = 1920, 1080
    c2 = hrt.preset("random", 1)
    c2.commit(0)
    cam, bg = hrt.preset_camera(c2.info, W, H), tuple(c2.info.background)
    tiles = hrt.tile_grid(W, H, 80)

    # ---- the resolves that existed before, and the new call against them
    a = hrt.Accumulator(c2, W, H, tiles, noise=True, features=True)
    for k in range(2):
        a.add(cam, hrt.params(W, H, 16, args.depth, 1, bg, sample_offset=16 * k))
    a.add_features(cam, hrt.params(W, H, 16, args.depth, 1, bg))
    out = torch.empty(a.n_pixels * 4, dtype=torch.float32, device=dev)
    err = torch.empty(a.n_pixels, dtype=torch.float32, device=dev)
    rec = (hrt.TileNoise * len(tiles))()
    recp, outp, errp = ctypes.cast(rec, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(err.data_ptr())

    def check(st):
        if st != hrt.OK:
            raise SystemExit(f"filtered_noise_bench.py: status {st}: {L.hrt_last_error().decode()}")

    def resolve(kind, it):
        if kind == "filtered":
            f = hrt.filter_params(it, 4.0)
            return lambda: check(L.hrt_accum_resolve_filtered(a.h, ctypes.byref(f), hrt.ACCUM_F32, outp, sp))
        g = hrt.guided_params(it, 4.0, **TOL)
        return lambda: check(L.hrt_accum_resolve_guided(a.h, ctypes.byref(g), hrt.ACCUM_F32, outp, sp))

    if args.resolve_only:
        line = {"metric": "resolve_timing", "label": args.label, "lib": os.environ.get("HRT_LIB", "this build"), "width": W, "height": H,
                "tiles": len(tiles), "reps": args.reps}
        for kind in ("filtered", "guided"):
            for it in (1, 3, 5):
                run = resolve(kind, it)
                for _ in range(3):
                    once(run)
                line[f"{kind}_{it}_ms"] = round(statistics.median([once(run) for _ in range(args.reps)]), 4)
        return emit(line)

    if "cost" not in skip:
        for kind in ("filtered", "guided"):
            for it in (1, 3, 5):
                g = hrt.guided_ex_params(it, 4.0, **(TOL if kind == "guided" else dict(normal=0, albedo=0, depth=0)), demodulate=False)
                res = resolve(kind, it)
                new = lambda: check(L.hrt_accum_noise_filtered(a.h, ctypes.byref(g), FLOOR, errp, sp, recp))
                new_own = lambda: check(L.hrt_accum_noise_filtered(a.h, ctypes.byref(g), FLOOR, None, sp, recp))

                def old():
                    res()
                    check(L.hrt_accum_noise(a.h, FLOOR, errp, sp, recp))

                for run in (new, new_own, old):
                    for _ in range(3):
                        once(run)
                t = {"new": [], "own_plane": [], "old": []}
                for k in range(args.reps):
                    for name, run in ((("new", new), ("own_plane", new_own), ("old", old)) if k % 2 == 0 else
                                      (("old", old), ("own_plane", new_own), ("new", new))):
                        t[name].append(once(run))
                emit({"metric": "noise_filtered_cost", "filter": "variance-only" if kind == "filtered" else "guided", "iterations": it,
                      "width": W, "height": H, "tiles": len(tiles), "reps": args.reps, "noise_filtered": stats(t["new"]),
                      "noise_filtered_own_plane": stats(t["own_plane"]), "resolve_plus_noise": stats(t["old"]),
                      "ratio_of_medians": round(statistics.median(t["new"]) / statistics.median(t["old"]), 4)})
    a.close()

    # ---- what refining on it saves
    def saving(name, scene, w, h, tile, seed, ref, ref_name):
        c, b = hrt.preset_camera(scene.info, w, h), tuple(scene.info.background)
        tl = hrt.tile_grid(w, h, tile)
        p = hrt.params(w, h, 50, args.depth, seed, b)
        line = {"metric": "refine_saving", "preset": name, "width": w, "height": h, "tiles": len(tl), "target": 0.04, "pass_spp": 50,
                "max_spp": 500, "floor": FLOOR, "ref": ref_name}
        for policy in ("refine", "refine_filtered"):
            acc = hrt.Accumulator(scene, w, h, tl, noise=True)
            passes = [0]
            t0 = time.perf_counter()
            getattr(acc, policy)(c, p, 0.04, 50, 500, FLOOR, on_pass=lambda t, r: passes.__setitem__(0, passes[0] + 1))
            scene.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            held = acc.tile_samples
            plain, filt = unpack(acc, acc.resolve()), unpack(acc, acc.resolve(denoise=True))
            fm = [r.mean for r in acc.noise_filtered(FLOOR)]
            line[policy] = {"samples": int(sum(n * t[2] * t[3] for n, t in zip(held, tl))), "wall_ms": round(ms, 2), "passes": passes[0],
                            "tiles_at_cap": int(sum(n >= 500 for n in held)), "rmse_plain": rmse(plain, ref), "rmse_filtered": rmse(filt, ref),
                            "shown": "plain" if policy == "refine" else "filtered", "filtered_mean_of_tiles": round(float(np.mean(fm)), 5),
                            "filtered_mean_worst_tile": round(float(np.max(fm)), 5)}
            acc.close()
        line["sample_ratio"] = round(line["refine_filtered"]["samples"] / line["refine"]["samples"], 4)
        line["shown_rmse_ratio"] = round(line["refine_filtered"]["rmse_filtered"] / line["refine"]["rmse_plain"], 4)
        emit(line)

    # ---- how far the estimate is from the filtered frame's real error
    def calibrate(name, scene, w, h, tile, seed, passes, ref, ref_name, fsamples=16):
        c, b = hrt.preset_camera(scene.info, w, h), tuple(scene.info.background)
        acc = hrt.Accumulator(scene, w, h, hrt.tile_grid(w, h, tile), noise=True, features=True)
        for lo, hi in passes:
            acc.add(c, hrt.params(w, h, hi - lo, args.depth, seed, b, sample_offset=lo))
        acc.add_features(c, hrt.params(w, h, fsamples, args.depth, seed, b))
        lref = np.square(ref[..., :3].astype(np.float64)).sum(-1)      # the frame is sqrt(c): back to linear luminance
        for setting, kw, frame in (("variance-only", dict(), lambda: acc.resolve(denoise=True)),
                                   ("guided", dict(guide=TOL), lambda: acc.resolve_guided(guide=TOL))):
            recs = acc.noise_filtered(FLOOR, **kw)
            lum = np.square(unpack(acc, frame())[..., :3].astype(np.float64)).sum(-1)
            rel = (lum - lref) / np.maximum(lref, FLOOR)
            # a predicted mean below 2e-4 is "converged, not a measurement" (csrc/accum.h: the f32 floor of the estimate):
            # such tiles (sky) are counted and left out of the ratios
            ratio, converged = [], 0
            for (x, y, tw, th), r in zip(acc.tiles, recs):
                if r.mean < 2e-4:
                    converged += 1
                    continue
                ratio.append(float(np.sqrt(np.mean(rel[y:y + th, x:x + tw] ** 2))) / r.mean)
            raw = [r.mean for r in acc.noise(FLOOR)]
            emit({"metric": "calibration", "preset": name, "width": w, "height": h, "tiles": len(acc.tiles), "spp": passes[-1][1],
                  "filter": setting, "ref": ref_name, "tiles_converged_left_out": converged, "actual_over_predicted_median": round(float(np.median(ratio)), 3),
                  "actual_over_predicted_worst_tile": round(float(np.max(ratio)), 3),
                  "actual_over_predicted_best_tile": round(float(np.min(ratio)), 3),
                  "predicted_mean_of_tiles": round(float(np.mean([r.mean for r in recs])), 5), "raw_mean_of_tiles": round(float(np.mean(raw)), 5)})
        acc.close()

    if "saving" not in skip or "calibration" not in skip:
        ref2 = hrt.render(c2, cam, hrt.params(W, H, 500, args.depth, 1, bg))
        c5 = hrt.preset("cornell", 1)
        c5.commit(0)
        ref5 = hrt.render(c5, hrt.preset_camera(c5.info, 512, 512), hrt.params(512, 512, 5000, args.depth, 1, tuple(c5.info.background)))
        if "saving" not in skip:
            saving("random", c2, W, H, 80, 1, ref2, "500 spp")
            saving("cornell", c5, 512, 512, 64, 1, ref5, "5000 spp")
        if "calibration" not in skip:
            calibrate("random", c2, W, H, 80, 1, [(0, 16), (16, 32)], ref2, "500 spp")
            calibrate("cornell", c5, 512, 512, 64, 1, [(0, 50), (50, 100)], ref5, "5000 spp")
            golden = os.path.join(ROOT, "tests", "golden", "random_64x36_4096spp_seed1234.npy")
            if os.path.exists(golden):
                calibrate("random", c2, 64, 36, 16, 7, [(0, 42), (42, 84), (84, 126)], np.load(golden).astype(np.float64),
                          "the oracle's 4096 spp, seed 1234")
        c5.close()
    if "flat" not in skip:
        flat_field(emit)
    c2.close()


if __name__ == "__main__":
    main()
