#!/usr/bin/env python3
"""What scatter queries cost (hrt_camera_paths, hrt_scene_scatter) beside the calls they sit between.  JSON lines,
appended to --out (default profiles/scatter.jsonl), on C2's scene (`random` at 1920x1080), 4 samples per pixel (8.3 M
paths), following scripts/query_bench.py's method:

  scatter_camera_paths  hrt_camera_paths against hrt_camera_rays for the 4 samples;
  scatter_round         hrt_scene_scatter and hrt_scene_intersect of the same batch in round 0 (every path live) and in a
                        late round (the first in which at most a tenth of the paths is live), beside a device copy of
                        120 bytes per path (240 moved: the call reads 144 and writes 96 per live path);
  scatter_loop          the whole loop to depth 50 (hrt.trace_paths) against hrt_render_tiles_device of the same samples;
  scatter_textures      the same two scatter rounds on the `earth_perlin` scene (image and noise textures, the Perlin
                        tables staged in LDS and, under HRT_SCATTER_PERLIN_LDS=0, read from global memory);
  scatter_verdict       the bar: round 0's scatter takes less time than round 0's intersect of the same batch;
  scatter_existing      with --existing TAG: hrt_camera_rays and hrt_scene_intersect alone, for the A/B against another
                        build of the library (HRT_LIB), one process per build, run in turn by the caller.

The scatter works in place, so every timed scatter starts from a saved copy of the round's rays and paths, restored
outside the timed interval.  Every figure is the median of --reps runs, each between two stream synchronisations; the
runs of one record alternate in one loop.  No GPU: the script fails (there is no fallback)."""
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
    ap.add_argument("--existing", default="", help="time only the calls the parent has, and tag the record with this name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter.jsonl"))
    args = ap.parse_args()
    import torch

    import hrt

    if not torch.cuda.is_available():
        raise SystemExit("scatter_bench.py: no GPU")
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
        """{name: (median ms, [ms])} of the runs, taken in turn --reps times after one untimed round; a run is a
        callable, or (untimed preparation, timed callable)."""
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

    def scene_of(name):
        s = hrt.preset(name, 1)
        s.commit(0)
        cam = hrt.preset_camera(s.info, W, H)
        p = hrt.params(W, H, spp, 50, 1, tuple(s.info.background))
        return s, cam, p, hrt.query_params(0, p.seed, (cam.time0, cam.time1)), hrt.scatter_params(tuple(p.background))

    def rounds_of(name):
        """The two measured rounds of a scene's loop: [(round, live fraction, rays, paths, hits at its start)]."""
        s, cam, p, q, sc = scene_of(name)
        hrt._check(L.hrt_camera_paths(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), paths.data_ptr(), sp))
        saved = []
        for r in range(p.max_depth):
            live = float((path_flags & hrt.PATH_DONE == 0).float().mean())
            hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), rays.data_ptr(), n, hits.data_ptr(), sp))
            if r == 0 or live <= 0.1:
                saved.append((r, round(live, 4), rays.clone(), paths.clone(), hits.clone()))
            if len(saved) == 2 or live == 0.0:
                break
            hrt._check(L.hrt_scene_scatter(s.h, ctypes.byref(sc), rays.data_ptr(), hits.data_ptr(), paths.data_ptr(), n, sp))
        return s, q, sc, saved

    def round_runs(s, q, sc, state):
        _, _, r0, p0, h0 = state

        def restore():
            rays.copy_(r0)
            paths.copy_(p0)

        def scatter():
            hrt._check(L.hrt_scene_scatter(s.h, ctypes.byref(sc), rays.data_ptr(), h0.data_ptr(), paths.data_ptr(), n, sp))

        def scatter_global():  # the A/B variant with the Perlin tables left in global memory (the knob is read at each launch)
            os.environ["HRT_SCATTER_PERLIN_LDS"] = "0"
            try:
                scatter()
            finally:
                del os.environ["HRT_SCATTER_PERLIN_LDS"]

        return {"scatter": (restore, scatter), "scatter_global": (restore, scatter_global),
                "intersect": lambda: hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), r0.data_ptr(), n, hits.data_ptr(), sp))}

    config = {"preset": "random", "width": W, "height": H, "samples": spp, "paths": n, "reps": args.reps}
    s, cam, p, q, sc = scene_of("random")

    def camera_rays():
        hrt._check(L.hrt_camera_rays(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), sp))

    if args.existing:
        camera_rays()
        t = alternate({"camera_rays": camera_rays,
                       "intersect": lambda: hrt._check(L.hrt_scene_intersect(s.h, ctypes.byref(q), rays.data_ptr(), n, hits.data_ptr(), sp))})
        emit({"metric": "scatter_existing", "lib": args.existing, **config, "camera_rays_ms": t["camera_rays"][0],
              "intersect_ms": t["intersect"][0], "camera_rays_runs_ms": t["camera_rays"][1], "intersect_runs_ms": t["intersect"][1]})
        return

    def camera_paths():
        hrt._check(L.hrt_camera_paths(s.h, ctypes.byref(cam), ctypes.byref(p), tile, 1, rays.data_ptr(), paths.data_ptr(), sp))

    t = alternate({"camera_rays": camera_rays, "camera_paths": camera_paths})
    emit({"metric": "scatter_camera_paths", **config, "camera_paths_ms": t["camera_paths"][0], "camera_rays_ms": t["camera_rays"][0],
          "camera_paths_runs_ms": t["camera_paths"][1], "camera_rays_runs_ms": t["camera_rays"][1]})
    s.close()

    spare = torch.empty((2 * n, 30), dtype=torch.float32, device=dev)

    def copy():
        spare[n:].copy_(spare[:n])  # 120 n bytes read and 120 n written

    verdict = {}
    for name in ("random", "earth_perlin"):
        s, q, sc, saved = rounds_of(name)
        for state in saved:
            runs = round_runs(s, q, sc, state)
            if name == "random":
                runs["copy"] = copy
                del runs["scatter_global"]  # no Perlin table: the knob selects nothing
            t = alternate(runs)
            rec = {"metric": "scatter_round" if name == "random" else "scatter_textures", **config, "preset": name, "round": state[0],
                   "live_fraction": state[1], "perlin": "none", "scatter_ms": t["scatter"][0], "intersect_ms": t["intersect"][0],
                   "scatter_runs_ms": t["scatter"][1], "intersect_runs_ms": t["intersect"][1]}
            if "scatter_global" in t:
                rec.update({"perlin": "staged in LDS (scatter_ms, the default) and global (scatter_global_ms, HRT_SCATTER_PERLIN_LDS=0)",
                            "scatter_global_ms": t["scatter_global"][0], "scatter_global_runs_ms": t["scatter_global"][1]})
            if "copy" in t:
                rec.update({"copy_ms": t["copy"][0], "copy_bytes_moved": 240 * n, "copy_gb_per_s": round(240 * n / t["copy"][0] / 1e6, 1),
                            "scatter_over_copy": round(t["scatter"][0] / t["copy"][0], 3)})
            emit(rec)
            if name == "random" and state[0] == 0:
                verdict = {"scatter_ms": t["scatter"][0], "intersect_ms": t["intersect"][0]}
        s.close()
        del saved

    s, cam, p, q, sc = scene_of("random")
    frame = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    loop = {}

    def run_loop():
        loop["rays"] = hrt.trace_paths(s, cam, p, device=True)[1]  # the radiance stays on the device, as the render's frame does

    t = alternate({"loop": run_loop, "render": lambda: hrt.render_tiles_device(s, cam, p, [(0, 0, W, H)], frame.data_ptr(), sp.value)})
    emit({"metric": "scatter_loop", **config, "loop_ms": t["loop"][0], "render_ms": t["render"][0], "loop_over_render": round(t["loop"][0] / t["render"][0], 2),
          "rays": loop["rays"], "loop_runs_ms": t["loop"][1], "render_runs_ms": t["render"][1]})
    emit({"metric": "scatter_verdict", **config, **verdict, "scatter_below_intersect": bool(verdict["scatter_ms"] < verdict["intersect_ms"])})
    s.close()


if __name__ == "__main__":
    main()
