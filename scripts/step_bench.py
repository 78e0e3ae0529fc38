#!/usr/bin/env python3
"""What the fused step costs (hrt_scene_step) beside the pair it fuses (hrt_scene_intersect + hrt_scene_scatter).  JSON
lines, appended to --out (default profiles/step.jsonl), on C2's scene (`random` at 1920x1080), 4 samples per pixel (8.3 M
paths), following scripts/scatter_bench.py's method:

  step_round0    round 0, every path live: the step with and without d_hits against intersect + scatter on the same batch;
  step_late      a late round (--late-round, default 4): the step over the live list against the pair on the whole batch,
                 against the step without a list, and against a call on an empty list (the floor); `model` is
                 live share x round 0's step + the floor, `late_over_model` the ratio the issue asks for;
  step_loop      the whole loop to depth 50: hrt.trace_paths_fused over steps x check_every against hrt.trace_paths and
                 hrt_render_tiles_device of the same samples, all in one alternating loop;
  step_perlin    round 0 and the late round on `earth_perlin` with the Perlin tables staged in LDS (the default) and, under
                 HRT_SCATTER_PERLIN_LDS=0, read from global memory;
  step_existing  with --existing TAG: hrt_scene_intersect and hrt_scene_scatter alone in round 0, for the A/B against
                 another build of the library (HRT_LIB), one process per build, run in turn by the caller.

The step works in place, so every timed call starts from a saved copy of the round's rays and paths, restored outside the
timed interval.  Every figure is the median of --reps runs, each between two stream synchronisations; the runs of one
record alternate in one loop.  No GPU: the script fails (there is no fallback)."""
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
    ap.add_argument("--late-round", type=int, default=4)
    ap.add_argument("--existing", default="", help="time only the calls the parent has, and tag the record with this name")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step.jsonl"))
    args = ap.parse_args()
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("step_bench.py: no GPU")
    dev = torch.device("cuda", 0)
    L = hrt.load()
    sink = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def once(run):
        prep, timed = run if isinstance(run, tuple) else (None, run)
        if prep:
            prep()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        timed()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def alternate(runs):
        for run in runs.values():
            once(run)
        ts = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, run in runs.items():
                ts[k].append(once(run))
        return {k: (round(statistics.median(v), 4), [round(t, 4) for t in v]) for k, v in ts.items()}

    W, H, spp = args.width, args.height, args.samples
    n = W * H * spp
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tile = (hrt.Tile * 1)(hrt.Tile(0, 0, W, H))
    rays = torch.empty((n, 12), dtype=torch.float32, device=dev)
    paths = torch.empty((n, 12), dtype=torch.float32, device=dev)
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)
    path_flags = paths.view(torch.int32)[:, 11]
    out_index = torch.empty(n, dtype=torch.int32, device=dev)
    out_count = torch.zeros(1, dtype=torch.int32, device=dev)
    lout = hrt.PathList(out_index.data_ptr(), out_count.data_ptr(), n, 0)
    config = {"preset": "random", "width": W, "height": H, "samples": spp, "paths": n, "reps": args.reps}

    def scene_of(name):
        s = hrt.preset(name, 1)
        s.commit(0)
        cam = hrt.preset_camera(s.info, W, H)
        p = hrt.params(W, H, spp, 50, 1, tuple(s.info.background))
        return (s, cam, p, hrt.query_params(0, p.seed, (cam.time0, cam.time1)), hrt.scatter_params(tuple(p.background)),
                hrt.step_params(1, p.seed, (cam.time0, cam.time1), tuple(p.background)))

    def states_of(s, cam, p, st):
        """The batch at the start of round 0 and of the late round: [(round, live share, rays, paths, live list, count)]."""
        hrt._check(L.hrt_camera_paths(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), paths.data_ptr(), sp))
        saved = []
        for r in range(args.late_round + 1):
            live = torch.nonzero(path_flags & hrt.PATH_DONE == 0).flatten().to(torch.int32)
            if r in (0, args.late_round):
                saved.append((r, round(live.numel() / n, 4), rays.clone(), paths.clone(), live.clone(),
                              torch.tensor([live.numel()], dtype=torch.int32, device=dev)))
            hrt._check(L.hrt_scene_step(s.h, ctypes.byref(st), rays.data_ptr(), paths.data_ptr(), n, None, None, None, None, sp))
        return saved

    def round_runs(s, q, sc, st, state):
        _, _, r0, p0, live, count = state
        lin = hrt.PathList(live.data_ptr(), count.data_ptr(), max(live.numel(), 1), 0)
        empty = torch.zeros(1, dtype=torch.int32, device=dev)
        lempty = hrt.PathList(out_index.data_ptr(), empty.data_ptr(), n, 0)

        def restore():
            rays.copy_(r0)
            paths.copy_(p0)

        def step(d_hits, a, b):
            return lambda: hrt._check(L.hrt_scene_step(s.h, ctypes.byref(st), rays.data_ptr(), paths.data_ptr(), n, d_hits,
                                                       None if a is None else ctypes.byref(a), None if b is None else ctypes.byref(b),
                                                       None, sp))

        def pair():
            hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), rays.data_ptr(), n, hits.data_ptr(), sp))
            hrt._check(L.hrt_scene_scatter(s.h, ctypes.byref(sc), rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, sp))

        def in_global(run):  # the A/B variant with the Perlin tables left in global memory (the knob is read at each launch)
            def f():
                os.environ["HRT_SCATTER_PERLIN_LDS"] = "0"
                try:
                    run()
                finally:
                    del os.environ["HRT_SCATTER_PERLIN_LDS"]
            return f

        return {"pair": (restore, pair), "step": (restore, step(None, None, None)), "step_hits": (restore, step(hits.data_ptr(), None, None)),
                "step_out": (restore, step(None, None, lout)), "step_list": (restore, step(None, lin, lout)),
                "step_list_global": (restore, in_global(step(None, lin, lout))), "step_global": (restore, in_global(step(None, None, None))),
                "empty_list": step(None, lempty, None)}

    s, cam, p, q, sc, st = scene_of("random")
    if args.existing:
        hrt._check(L.hrt_camera_paths(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), paths.data_ptr(), sp))
        r0, p0 = rays.clone(), paths.clone()

        def restore():
            rays.copy_(r0)
            paths.copy_(p0)

        def scatter():
            hrt._check(L.hrt_scene_scatter(s.h, ctypes.byref(sc), rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, sp))

        hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), rays.data_ptr(), n, hits.data_ptr(), sp))
        t = alternate({"intersect": lambda: hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), r0.data_ptr(), n, hits.data_ptr(), sp)),
                       "scatter": (restore, scatter)})
        emit({"metric": "step_existing", "lib": args.existing, **config, "intersect_ms": t["intersect"][0], "scatter_ms": t["scatter"][0],
              "intersect_runs_ms": t["intersect"][1], "scatter_runs_ms": t["scatter"][1]})
        return

    round0 = None
    for name in ("random", "earth_perlin"):
        if name != "random":
            s, cam, p, q, sc, st = scene_of(name)
        saved = states_of(s, cam, p, st)
        for state in saved:
            runs = round_runs(s, q, sc, st, state)
            if name == "random":
                del runs["step_list_global"], runs["step_global"]  # no Perlin table: the knob selects nothing
            if state[0] == 0:
                for k in ("step_list", "step_list_global", "empty_list"):
                    runs.pop(k, None)
            t = alternate(runs)
            rec = {"metric": {"random": "step_round0" if state[0] == 0 else "step_late"}.get(name, "step_perlin"), **config, "preset": name,
                   "round": state[0], "live_fraction": state[1], **{k + "_ms": v[0] for k, v in t.items()},
                   **{k + "_runs_ms": v[1] for k, v in t.items()}}
            if state[0] == 0:
                rec["step_not_above_pair"] = bool(t["step"][0] <= t["pair"][0] and t["step_hits"][0] <= t["pair"][0])
                if name == "random":
                    round0 = t["step_out"][0]
            elif name == "random":
                model = state[1] * round0 + t["empty_list"][0]
                rec.update({"model_ms": round(model, 4), "late_over_model": round(t["step_list"][0] / model, 3),
                            "pair_over_step_list": round(t["pair"][0] / t["step_list"][0], 2)})
            emit(rec)
        del saved
        if name != "random":
            s.close()

    if args.skip_loop:
        return
    s, cam, p, q, sc, st = scene_of("random")
    frame = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    got = {}

    def fused(steps, check):
        def f():
            got[(steps, check)] = hrt.trace_paths_fused(s, cam, p, device=True, steps=steps, check_every=check)[1]
        return f

    def plain():
        got["trace_paths"] = hrt.trace_paths(s, cam, p, device=True)[1]

    runs = {"trace_paths": plain, "render": lambda: hrt.render_tiles_device(s, cam, p, [(0, 0, W, H)], frame.data_ptr(), sp.value)}
    for steps in (1, 2, 4, 8, p.max_depth):
        for check in (1, 4, 0):
            runs[f"fused_s{steps}_c{check or 'never'}"] = fused(steps, check)
    t = alternate(runs)
    assert len(set(got.values())) == 1, got  # every variant walked the same rays
    best = min((k for k in t if k.startswith("fused")), key=lambda k: t[k][0])
    emit({"metric": "step_loop", **config, "rays": got["trace_paths"], **{k + "_ms": v[0] for k, v in t.items()}, "best": best,
          "best_over_render": round(t[best][0] / t["render"][0], 2), "trace_paths_over_best": round(t["trace_paths"][0] / t[best][0], 2),
          **{k + "_runs_ms": v[1] for k, v in t.items()}})
    s.close()


if __name__ == "__main__":
    main()
