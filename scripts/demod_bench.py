#!/usr/bin/env python3
"""What demodulating the guided preview filter by the first-hit albedo costs and what it buys
(hrt_accum_resolve_guided_ex with HRT_GUIDED_DEMODULATE).  JSON lines, appended to --out (default
profiles/demod_refine.jsonl):

  demod_cost      at 1920x1080 (C2, whole-frame accumulator with noise and feature planes): hrt_accum_resolve_guided_ex
                  into device memory with the flag on against the same call with the flag off, at 1, 3 and 5 iterations,
                  in one process, the two alternating (--reps pairs, each run between two stream synchronisations);
  demod_quality   RMSE (display units, 3 iterations, 16 feature samples) of the plain, variance-only, guided, demodulated
                  (albedo term off and on) frames, and of the demodulated frame over the floors 0.003 / 0.01 / 0.03 / 0.1:
                  C2 after 32 and 64 spp against its 500-spp frame (and at 32 spp with 64 and 256 feature samples),
                  Cornell at 512x512 after 100 and 400 spp against its 5000-spp frame, `random` at 64x36 after 126 spp
                  against tests/golden's 4096-spp frame;
  demod_sweep     the demodulated frame over a grid of tolerances at C2 32 spp, Cornell 100 spp and `random` 126 spp:
                  the rows from which the defaults are chosen;
  guided_flag_off hrt_accum_resolve_guided (the call that existed before) at 1, 3 and 5 iterations, one line per run,
                  tagged with the library that ran (--label): `--flag-off-only` prints this line alone, and
                  `--against LIB` starts such runs in child processes, this build and LIB (HRT_LIB) alternating, four
                  each after a discarded one each, and reports the project's verdict: this build's slowest run against the other's fastest,
                  relative to the larger spread.

No GPU: the script fails (there is no fallback)."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hyper-ray-tracer_amd"))
FLOORS = (0.003, 0.01, 0.03, 0.1)


def against(args, emit):
    """This build and args.against alternating in child processes, `runs` each, after one discarded run of each (the
    first process on a box that did other work before pays for more than the library); which of the two goes first
    alternates from pair to pair."""
    runs = {"this": [], "other": [], "warmup": []}
    order = ["this", "other"] + [w for k in range(args.runs) for w in (("this", "other") if k % 2 == 0 else ("other", "this"))]
    for k, which in enumerate(order):
        env = dict(os.environ)
        env.pop("HRT_LIB", None)
        if which == "other":
            env["HRT_LIB"] = os.path.abspath(args.against)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--flag-off-only", "--label", which, "--reps", str(args.reps),
                              "--out", os.devnull], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            raise SystemExit(f"demod_bench.py: the {which} run failed:\n{out.stderr}")
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        if k < 2:
            rec["discarded"] = "warm-up"
        runs[which if k >= 2 else "warmup"].append(rec)
        emit(rec)
    for it in (1, 3, 5):
        key = f"guided_{it}_ms"
        t, o = [r[key] for r in runs["this"]], [r[key] for r in runs["other"]]
        spread = max(max(t) - min(t), max(o) - min(o))
        emit({"metric": "guided_flag_off_verdict", "iterations": it, "this_ms": t, "other_ms": o, "other": args.against,
              "this_slowest_minus_other_fastest_ms": round(max(t) - min(o), 4), "larger_spread_ms": round(spread, 4),
              "beyond_spread": bool(max(t) - min(o) > spread)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=21, help="timed runs per figure (the median is reported)")
    ap.add_argument("--runs", type=int, default=4, help="--against: processes per library")
    ap.add_argument("--cost-only", action="store_true", help="skip the quality and sweep lines")
    ap.add_argument("--flag-off-only", action="store_true", help="time hrt_accum_resolve_guided alone (one guided_flag_off line)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--against", help="another build's libhrt.so: alternate child processes and report the verdict")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demod_refine.jsonl"))
    args = ap.parse_args()
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    if args.against:
        against(args, emit)
        return
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("demod_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()

    def once(run):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def rmse(img, ref):
        d = (img[..., :3] - ref[..., :3]).astype(np.float64)
        return float(np.sqrt((d * d).mean()))

    W, H = args.width, args.height
    s = hrt.preset("random", 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    bg = tuple(s.info.background)
    config = {"preset": "random", "width": W, "height": H, "sigma": args.sigma, "depth": args.depth, "reps": args.reps}
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    buf = torch.empty(W * H * 4, dtype=torch.float32, device=dev)
    bp = ctypes.c_void_p(buf.data_ptr())

    # ---- wall time at the C2 frame size
    acc = hrt.Accumulator(s, W, H, None, noise=True, features=True)
    for k in range(2):
        acc.add(cam, hrt.params(W, H, 16, args.depth, 1, bg, sample_offset=16 * k))
    acc.add_features(cam, hrt.params(W, H, 16, args.depth, 1, bg))
    if args.flag_off_only:
        rec = {"metric": "guided_flag_off", "label": args.label, "lib": hrt.LIB_PATH if not os.environ.get("HRT_LIB") else os.environ["HRT_LIB"],
               "config": config}
        for it in (1, 3, 5):
            g = hrt.guided_params(it, args.sigma)

            def guided():
                hrt._check(L.hrt_accum_resolve_guided(acc.h, ctypes.byref(g), hrt.ACCUM_F32, bp, sp))

            guided()
            guided()
            ts = [once(guided) for _ in range(args.reps)]
            rec[f"guided_{it}_ms"], rec[f"guided_{it}_min_ms"] = round(statistics.median(ts), 4), round(min(ts), 4)
        emit(rec)
        return
    cost = {"metric": "demod_cost", "config": config, "floor": hrt.DEMOD_FLOOR, "tolerances": hrt.DEMOD_DEFAULTS}
    for it in (1, 3, 5):
        on = hrt.guided_ex_params(it, args.sigma, demodulate=True)
        off = hrt.guided_ex_params(it, args.sigma, **hrt.DEMOD_DEFAULTS, demodulate=False)

        def run(g):
            return lambda: hrt._check(L.hrt_accum_resolve_guided_ex(acc.h, ctypes.byref(g), hrt.ACCUM_F32, bp, sp))

        for g in (on, off, on, off):   # the first calls allocate the planes and load the kernels
            run(g)()
        t_on, t_off = [], []
        for k in range(args.reps):      # alternating, and the order within a pair alternating too
            for g, ts in ((on, t_on), (off, t_off)) if k % 2 == 0 else ((off, t_off), (on, t_on)):
                ts.append(once(run(g)))
        cost[f"flag_on_{it}_ms"], cost[f"flag_off_{it}_ms"] = round(statistics.median(t_on), 4), round(statistics.median(t_off), 4)
        cost[f"flag_on_{it}_range_ms"] = [round(min(t_on), 4), round(max(t_on), 4)]
        cost[f"flag_off_{it}_range_ms"] = [round(min(t_off), 4), round(max(t_off), 4)]
    emit(cost)
    acc.close()
    if args.cost_only:
        return

    # ---- quality, the floors and the tolerance sweep
    grid = list(itertools.product((0.05, 0.1, 0.2, 0.5), (0.0, 0.05, 0.1, 0.2), (0.05, 0.1, 0.2)))

    def quality(name, scene, w, h, seed, passes, after, ref, ref_what, sweep_at, fpasses=((0, 16),), tiles=None):
        c = hrt.preset_camera(scene.info, w, h)
        b = tuple(scene.info.background)
        a = hrt.Accumulator(scene, w, h, tiles, noise=True, features=True)
        for f0, f1 in fpasses:
            a.add_features(c, hrt.params(w, h, f1 - f0, args.depth, seed, b, sample_offset=f0))
        den = dict(iterations=3, sigma=args.sigma)

        def frame(px):
            if tiles is None:
                return px
            out, off = np.zeros((h, w, 4), px.dtype), 0
            for x, y, tw, th in a.tiles:
                out[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, 4)
                off += tw * th
            return out

        for k, (p0, p1) in enumerate(passes):
            a.add(c, hrt.params(w, h, p1 - p0, args.depth, seed, b, sample_offset=p0))
            if k + 1 not in after:
                continue
            base = {"preset": name, "width": w, "height": h, "spp": p1, "feature_samples": fpasses[-1][1], "ref": ref_what,
                    "sigma": args.sigma, "iterations": 3}
            err = lambda **kw: rmse(frame(a.resolve_guided(denoise=den, **kw)), ref)  # noqa: E731
            plain, filt = rmse(frame(a.resolve()), ref), rmse(frame(a.resolve(denoise=den)), ref)
            guided = err(guide=True)
            tol_on, tol_off = dict(hrt.DEMOD_DEFAULTS), dict(hrt.DEMOD_DEFAULTS, albedo=0.0)
            rec = {"metric": "demod_quality", **base, "guided_tolerances": hrt.GUIDED_DEFAULTS, "demod_tolerances": tol_on,
                   "floor": hrt.DEMOD_FLOOR, "rmse_plain": plain, "rmse_filtered": filt, "rmse_guided": guided,
                   "rmse_demod_albedo_on": err(guide=tol_on, demodulate=True), "rmse_demod_albedo_off": err(guide=tol_off, demodulate=True),
                   "rmse_demod_variance_only": err(guide=dict(normal=0, albedo=0, depth=0), demodulate=True),
                   "floors": list(FLOORS),
                   "rmse_demod_albedo_on_by_floor": [err(guide=tol_on, demodulate=f) for f in FLOORS],
                   "rmse_demod_albedo_off_by_floor": [err(guide=tol_off, demodulate=f) for f in FLOORS]}
            rec["demod_over_filtered"] = round(min(rec["rmse_demod_albedo_on"], rec["rmse_demod_albedo_off"]) / filt, 4)
            rec["demod_over_plain"] = round(min(rec["rmse_demod_albedo_on"], rec["rmse_demod_albedo_off"]) / plain, 4)
            emit(rec)
            if k + 1 != sweep_at:
                continue
            rows = [[tn, ta, td, round(err(guide=dict(normal=tn, albedo=ta, depth=td), demodulate=True) / plain, 4)] for tn, ta, td in grid]
            emit({"metric": "demod_sweep", **base, "floor": hrt.DEMOD_FLOOR, "rmse_plain": plain, "rmse_filtered": filt,
                  "columns": ["normal", "albedo", "depth", "demod_over_plain"], "rows": rows})
        a.close()

    ref = hrt.render(s, cam, hrt.params(W, H, 500, args.depth, 1, bg))
    quality("random", s, W, H, 1, [(16 * k, 16 * k + 16) for k in range(4)], (2, 4), ref, "500 spp", 2)
    for nf in (64, 256):   # the albedo plane is a Monte-Carlo estimate too: the same frame with more feature samples
        quality("random", s, W, H, 1, [(0, 16), (16, 32)], (2,), ref, "500 spp", None, fpasses=((0, nf),))
    golden = np.load(os.path.join(ROOT, "tests", "golden", "random_64x36_4096spp_seed1234.npy")).astype(np.float64)
    quality("random", s, 64, 36, 7, [(0, 40), (40, 110), (110, 126)], (3,), golden, "the oracle's 4096 spp, seed 1234", 3,
            fpasses=((0, 5), (5, 16)), tiles=hrt.tile_grid(64, 36, 16))
    s.close()
    c5 = hrt.preset("cornell", 1)
    c5.commit(0)
    c5cam = hrt.preset_camera(c5.info, 512, 512)
    ref = hrt.render(c5, c5cam, hrt.params(512, 512, 5000, args.depth, 1, tuple(c5.info.background)))
    quality("cornell", c5, 512, 512, 1, [(50 * k, 50 * k + 50) for k in range(8)], (2, 8), ref, "5000 spp", 2)
    c5.close()
    sink.close()


if __name__ == "__main__":
    main()
