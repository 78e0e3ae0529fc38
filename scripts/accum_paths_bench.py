#!/usr/bin/env python3
"""What depositing caller-traced paths costs (hrt_accum_add_paths).  JSON lines, appended to --out (default
profiles/accum_paths.jsonl), on C2's scene (`random` at 1920x1080), following scripts/step_bench.py's method: every figure
is the median of --reps runs, each --inner calls between two device synchronisations, the runs of one record alternating in
one loop.

  accum_paths_reduce   per S = samples per pixel and pass, without and with the noise plane and the preview: the call
                       against (i) a device-to-device copy of the batch's n x 48 bytes in the same loop, and (iii) the
                       route it replaces: download the paths, fold in numpy, Accumulator.upload.  `over_copy` is the
                       ratio the bar is on at S >= 4 (the copy moves twice the bytes the reduce must read).  The batch is
                       synthetic (uniform radiance, every path DONE): the kernel's time does not depend on the values.
                       With --shape TAG the record carries the tag and only the calls are timed: the kernel shapes
                       are compared as separate builds of the library (HRT_LIB), one process per build.
  accum_paths_pass     the whole pass: Accumulator.add_wavefront against Accumulator.add of the same samples.
  accum_paths_existing with --existing TAG: hrt_accum_add and round 0 of hrt_scene_step alone, for the A/B against another
                       build of the library (HRT_LIB), one process per build, run in turn by the caller.
  accum_paths_bench_py with --bench-line TAG: one run of bench.py (--steps 3 --warmup 1, no CPU leg) in a child process under
                       the same HRT_LIB, its value and ms_per_step recorded with the tag; run in turn by the caller.
  --probe              no timing: a few add and add_paths passes for a kernel trace (rocprofv3 --kernel-trace --stats in a
                       run of its own), which is where (ii), accumulate_chunks on the partial sums of a rendered pass of the
                       same samples, beside accumulate_paths comes from.

No GPU: the script fails (there is no fallback)."""
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
    ap.add_argument("--samples", default="1,4,16", help="samples per pixel and pass, comma separated")
    ap.add_argument("--reps", type=int, default=9, help="timed runs per figure (the median is reported)")
    ap.add_argument("--inner", type=int, default=10, help="calls per timed run")
    ap.add_argument("--shape", default="", help="time only the calls, and tag the record with this name (a kernel-shape build)")
    ap.add_argument("--existing", default="", help="time only the calls the parent has, and tag the record with this name")
    ap.add_argument("--bench-line", default="", help="run bench.py once and record its line with this tag")
    ap.add_argument("--probe", action="store_true", help="run a few passes untimed, for a kernel trace")
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_paths.jsonl"))
    args = ap.parse_args()
    if args.bench_line:
        import subprocess

        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                           capture_output=True, text=True, check=True)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        rec = {"metric": "accum_paths_bench_py", "tag": args.bench_line, "lib": os.environ.get("HRT_LIB", "lib/libhrt.so"),
               "value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"], "steps": line["steps"]}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        return
    import numpy as np
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("accum_paths_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def once(run, inner):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(inner):
            run()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / inner

    def alternate(runs, inner=None):
        inner = args.inner if inner is None else inner
        for run in runs.values():
            once(run, 1)
        ts = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, run in runs.items():
                ts[k].append(once(run, inner))
        return {k: (round(statistics.median(v), 4), [round(t, 4) for t in v]) for k, v in ts.items()}

    W, H = args.width, args.height
    n_px = W * H
    s = hrt.preset("random", 1)
    s.commit(0)
    cam = hrt.preset_camera(s.info, W, H)
    config = {"preset": "random", "width": W, "height": H, "reps": args.reps, "inner": args.inner, "lib": os.path.relpath(hrt.LIB_PATH, ROOT)}

    def params(spp, offset=0):
        return hrt.params(W, H, spp, 50, 1, tuple(s.info.background), sample_offset=offset)

    class Passes:
        """An accumulator and the next sample offset: every timed call adds a fresh range of S samples."""

        def __init__(self, spp, noise):
            self.acc, self.spp, self.at = hrt.Accumulator(s, W, H, noise=noise), spp, 0

        def next(self):
            if self.at + self.spp >= 1 << 31:
                self.acc.reset()
                self.at = 0
            p = params(self.spp, self.at)
            self.at += self.spp
            return p

    if args.existing:
        spp = 4
        n = n_px * spp
        a = Passes(spp, True)
        rays, paths = hrt.camera_paths(s, cam, params(spp), device=True)
        r0, p0 = rays.clone(), paths.clone()
        st = hrt.step_params(1, 1, (cam.time0, cam.time1), tuple(s.info.background))

        def step():
            rays.copy_(r0)
            paths.copy_(p0)
            hrt._check(L.hrt_scene_step(s.h, ctypes.byref(st), rays.data_ptr(), paths.data_ptr(), n, None, None, None, None, None))

        t = alternate({"accum_add": lambda: a.acc.add(cam, a.next()), "step_round0_with_restore": step}, inner=3)
        emit({"metric": "accum_paths_existing", "tag": args.existing, **config, "samples": spp, **{k + "_ms": v[0] for k, v in t.items()},
              **{k + "_runs_ms": v[1] for k, v in t.items()}})
        return

    for spp in [int(x) for x in args.samples.split(",")]:
        n = n_px * spp
        paths = torch.rand((n, 12), dtype=torch.float32, device=dev)
        paths.view(torch.int32)[:, 11] = hrt.PATH_DONE
        copy_to = None if args.shape or args.probe else torch.empty_like(paths)
        preview = torch.empty(n_px * 4, dtype=torch.float32, device=dev)
        variants = {"plain": (False, -1), "noise": (True, -1), "noise_preview": (True, hrt.ACCUM_F32)}
        accs = {k: Passes(spp, noise) for k, (noise, _) in variants.items()}

        def add_paths(k):
            a, fmt = accs[k], variants[k][1]

            def f():
                p = a.next()
                hrt._check(L.hrt_accum_add_paths(a.acc.h, ctypes.byref(cam), ctypes.byref(p), None, 0, paths.data_ptr(), n, fmt,
                                                 preview.data_ptr() if fmt >= 0 else None, None, None))
            return f

        if args.probe:
            for _ in range(3):
                add_paths("noise")()
                accs["plain"].acc.add(cam, accs["plain"].next())
                b = accs["noise_preview"]
                b.acc.add(cam, b.next())
            torch.cuda.synchronize(dev)
            continue
        runs = {"add_paths_" + k: add_paths(k) for k in variants}
        if not args.shape:
            runs["copy"] = lambda: copy_to.copy_(paths)
        t = alternate(runs)
        rec = {"metric": "accum_paths_reduce", **config, "samples": spp, "paths": n, "batch_mb": round(n * 48 / 1e6, 1),
               **{k + "_ms": v[0] for k, v in t.items()}}
        if args.shape:
            rec["shape"] = args.shape
        else:
            host = Passes(spp, False)

            def replaced():  # download the paths, fold on the host, upload the sums as the samples of a fresh accumulator
                rad = paths[:, 8:11].cpu().numpy().reshape(n_px, spp, 3)
                sums = np.zeros((n_px, 4), np.float32)
                sums[:, :3] = rad.sum(axis=1, dtype=np.float32)
                host.acc.reset()
                host.acc.upload(cam, params(spp), sums, [(0, spp)])

            reps, args.reps = args.reps, 3
            t.update(alternate({"download_fold_upload": replaced}, inner=1))
            args.reps = reps
            rec["download_fold_upload_ms"] = t["download_fold_upload"][0]
            rec.update({"over_copy_" + k: round(t["add_paths_" + k][0] / t["copy"][0], 3) for k in variants})
            rec["read_gbs_plain"] = round(n * 48 / 1e6 / t["add_paths_plain"][0], 1)  # the whole batch crosses the memory system
            rec["copy_gbs"] = round(2 * n * 48 / 1e6 / t["copy"][0], 1)
            if spp >= 4:
                rec["not_above_copy"] = bool(all(t["add_paths_" + k][0] <= t["copy"][0] for k in variants))
            host.acc.close()
        rec.update({k + "_runs_ms": v[1] for k, v in t.items()})
        emit(rec)
        for a in accs.values():
            a.acc.close()
        del paths, copy_to

    if args.shape or args.probe or args.skip_pass:
        return
    for spp in [int(x) for x in args.samples.split(",")]:
        a, b = Passes(spp, True), Passes(spp, True)
        got = {}

        def wavefront():
            got["wavefront"] = a.acc.add_wavefront(cam, a.next())

        def add():
            got["add"] = b.acc.add(cam, b.next(), stats=True).segments

        t = alternate({"add_wavefront": wavefront, "add": add}, inner=1)
        emit({"metric": "accum_paths_pass", **config, "samples": spp, **{k + "_ms": v[0] for k, v in t.items()},
              "wavefront_over_add": round(t["add_wavefront"][0] / t["add"][0], 2), "same_rays": bool(got["wavefront"] == got["add"]),
              **{k + "_runs_ms": v[1] for k, v in t.items()}})
        a.acc.close()
        b.acc.close()
    s.close()


if __name__ == "__main__":
    main()
