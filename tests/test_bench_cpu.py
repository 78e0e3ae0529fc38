"""bench.py's CPU leg (the cpu_baseline object of the JSON line, and the oracle rows the parity band is
checked against) on a tiny workload: rows spread over the frame, the fields the contract names."""
import argparse

import bench


def test_cpu_leg_fields_and_rows():
    args = argparse.Namespace(preset="random", width=64, height=36, spp=4, depth=10, seed=1, cpu_seconds=0.3)
    cb, rows, img, cnt = bench.cpu_leg(args, 2.8)
    for k in ("value", "unit", "cores", "kind", "sample", "one_core_value", "host_cpu", "nproc", "label",
              "segments_per_sample", "frame_segments_per_sample", "sample_vs_frame", "cpu_quota"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["unit"] == "Mrays/s"
    assert cb["value"] > 0 and cb["one_core_value"] > 0
    assert cb["segments_per_sample"] > 1.0
    assert cb["cores"] == bench.usable_cpus()[0]
    assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < 36
    assert img.shape == (len(rows), 64, 4) and cnt["samples"] == len(rows) * 64 * 4


def test_band_rows_spread_over_the_frame():
    r = bench.band_rows(1080, 60)
    assert len(r) == 60 and r[0] < 18 and r[-1] > 1060
    assert bench.band_rows(10, 50) == list(range(10))


def test_pmc_key_names_the_share_and_rejects_counters_above_peak():
    """A tile split's launch is priced with the counters of that share's launch (key suffix _shareN), never
    with the whole frame's; counters that would put a launch above peak are rejected, not reported."""
    args = argparse.Namespace(preset="random", width=1920, height=1080, spp=500)
    assert bench.pmc_key(args, 1) == "random_1920x1080_500"
    assert bench.pmc_key(args, 8) == "random_1920x1080_500_share8"
    peak = bench.SIMDS * bench.MAX_CLOCK_HZ / bench.VALU_CYC / 1e9
    pm = {"valu_insts": 2.0e11, "source": "x", "lib_sha16": None}
    ro = {"peak": peak, "achieved": None, "frac": None}
    bench.apply_pmc(ro, "k", pm, 0.203, 2.9e9)
    assert 0.7 < ro["frac"] < 0.9 and ro["pmc_key"] == "k"
    ro = {"peak": peak, "achieved": None, "frac": None}
    bench.apply_pmc(ro, "k", pm, 0.203 / 8, 2.9e9 / 8)  # a 1/8 share's launch with the whole frame's counters
    assert ro["frac"] is None and ro["achieved"] is None and "pmc_rejected" in ro
    ro = {"peak": peak, "achieved": None, "frac": None}
    bench.apply_pmc(ro, "k", None, 0.2, 1e9)
    assert ro["frac"] is None and ro["pmc_key"] == "k"


def test_chunk_schedule_is_the_frames_at_every_gpu_count():
    """VERDICT r05 (missing 2): the sample chunks are a function of the frame alone, so the image is the same bits
    at 1, 2, 4 and 8 GPUs.  No share or GPU count enters chunk_options; only an explicit A/B value changes it."""
    import inspect

    def args(chunks="frame"):
        return argparse.Namespace(width=1920, height=1080, spp=500, chunks=chunks)
    assert bench.chunk_options(args()) is None
    assert list(inspect.signature(bench.chunk_options).parameters) == ["args"]
    assert bench.chunk_options(args("8")) == {"chunk_min": 8, "chunk_max": 64}


def test_every_gpu_count_gets_parity_and_cpu_baseline():
    """VERDICT r05 (missing 1): rank 0 runs the CPU leg at every N (the oracle rows of the delivered N-GPU frame,
    or of its replica under weak scaling); a one-GPU share line uses tiles; other ranks run none."""
    a = argparse.Namespace(no_cpu_baseline=False)
    for world in (1, 2, 4, 8):
        assert bench.parity_plan(world, 0, world, True, a) == "rows"
        assert bench.parity_plan(world, 0, 1, False, a) == "rows"
        for r in range(1, world):
            assert bench.parity_plan(world, r, world, True, a) is None
    assert bench.parity_plan(1, 0, 8, True, a) == "tiles"
    assert bench.parity_plan(2, 0, 2, True, argparse.Namespace(no_cpu_baseline=True)) is None


def test_share_tiles_for_the_cpu_leg_spread_in_two_dimensions():
    """The oracle tiles of a share's CPU leg and parity band cover the frame in x and y.  Evenly spaced list
    indices of rank 0's 1/8 share of C5 (2048^2, diagonal deal) all fell in the leftmost tile column, where
    every camera ray misses the Cornell box (r05c: 1.0 rays per sample)."""
    from hrt import tiling
    for W, H, world, rank, n in ((2048, 2048, 8, 0, 8), (3840, 2160, 8, 5, 5), (1920, 1080, 2, 1, 4), (64, 48, 2, 1, 40)):
        tiles = tiling.split_tiles(W, H, world, rank)
        picks = bench.spread_tiles(tiles, n, W, H)
        assert picks == sorted(set(picks)) and len(picks) == min(n, len(tiles))
        assert all(0 <= i < len(tiles) for i in picks)
        xs = {tiles[i][0] for i in picks}
        ys = {tiles[i][1] for i in picks}
        want_x = min(len(picks), 4, len({t[0] for t in tiles}))
        want_y = min(len(picks), 4, len({t[1] for t in tiles}))
        assert len(xs) >= want_x and len(ys) >= want_y, (W, H, world, rank, sorted(xs), sorted(ys))
        span_x = max(xs) - min(xs)
        assert len(picks) < 4 or span_x >= W / 2, (W, span_x)


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    """A plain run (no --full) does the headline's work alone; the legs with runs of their own are behind --full."""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_array_or_a_fixed_sample(tmp_path):
    """--dump-outputs: an array within the budget is written whole as float32; a larger one as a seeded sample of
    its pixels, the same pixels every time, within the budget on disk."""
    import os

    import numpy as np

    frame = np.arange(36 * 64 * 4, dtype=np.float32).reshape(36, 64, 4)
    p = bench.dump_outputs(str(tmp_path / "a"), "frame", frame, bench.DUMP_BYTES)
    got = np.load(p)
    assert os.path.basename(p) == "frame.npy" and got.dtype == np.float32 and np.array_equal(got, frame)
    budget = 4096 + 1600  # room for 100 pixels beside the header
    p1 = bench.dump_outputs(str(tmp_path / "b"), "frame", frame, budget)
    p2 = bench.dump_outputs(str(tmp_path / "c"), "frame", frame + 0.0, budget)
    s1, s2 = np.load(p1), np.load(p2)
    assert os.path.basename(p1) == "frame_sample.npy" and s1.dtype == np.float32 and s1.shape == (100, 4)
    assert np.array_equal(s1, s2) and os.path.getsize(p1) <= budget
    px = (s1[:, 0] / 4).astype(int)  # pixel i holds 4i .. 4i+3
    assert np.array_equal(s1, frame.reshape(-1, 4)[px]) and np.all(np.diff(px) > 0)
    assert bench.DUMP_BYTES <= 64 * 1000 * 1000


def test_stream_count_per_run():
    """--streams auto: two alternating streams for a GPU's share of C2 (short launches: the next step's grid fills
    the CUs the previous one's end frees), one for the whole frame and for C4's / C5's long share launches."""
    def args(w, h, spp, streams="auto"):
        return argparse.Namespace(width=w, height=h, spp=spp, streams=streams)
    assert bench.stream_count(args(1920, 1080, 500), 1) == 1
    assert [bench.stream_count(args(1920, 1080, 500), n) for n in (2, 4, 8)] == [2, 2, 2]
    assert bench.stream_count(args(3840, 2160, 2000), 8) == 1
    assert bench.stream_count(args(2048, 2048, 10000), 8) == 1
    assert bench.stream_count(args(1920, 1080, 500, "3"), 1) == 3
