"""The re-entrancy contract of include/hrt/hrt.h, held to results: "rendering is re-entrant per scene", "different
accumulators of a scene may be used from different threads, as the render calls may", the ray queries and hrt_scene_step
"re-entrant as the renders are", hrt_last_error and hrt_last_launch per thread.

tests/native/threads.c drives one committed scene from 8 pthreads through the C ABI (its header lists the jobs): every
job runs once serially, then one thread per job runs it three more times behind a barrier and compares outputs, stats,
the kernel of hrt_last_launch and the refused calls' status and text with the serial run byte for byte.  The serial
frames are held to the oracle here, so "equal to the serial run" means "equal to a frame the reference agrees with".
The binding is driven from Python threads the same way, and one sequential case covers the process-wide cache of
kernel_common.h resident_grid across scenes with different LDS sizes.

What this does not do: ThreadSanitizer cannot see the .hip translation units, so these tests check results, not races as
such (tests/test_scene_threads.py runs the host half of a scene under TSan).  No tolerance appears except the oracle's."""
import os
import re
import subprocess
import threading
import time

import numpy as np
import pytest
from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
JOBS = ("R1", "R2", "R3", "R4", "A1", "A2", "Q1", "L1")
ROUNDS = 3
TOL = 1e-3  # the project's oracle bound (tests/test_gpu_parity.py)
# threads.c LOOK_FROM_1 / LOOK_FROM_2
LOOK_FROM_1 = (10.0, 3.0, 5.0)
LOOK_FROM_2 = (12.0, 1.5, -2.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cthreads") / "threads")
    lib = os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROCM, "include"), os.path.join(HERE, "native", "threads.c"), "-o", out, "-L" + lib, "-lhrt",
                    "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_thread_driver_fails_loudly_without_a_device(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
    assert "status 6" in r.stderr  # HRT_ERR_HIP from the scene upload
    assert "threads: ok" not in r.stdout
    assert not list(tmp_path.glob("*.pfm"))


def _oracle_camera(o, look_from):
    return (look_from, tuple(o.look_at), o.fov, o.aperture, o.focus_dist, o.time0, o.time1)


@pytest.mark.gpu
def test_eight_threads_on_one_scene_equal_the_serial_run(exe, tmp_path, earth):
    """The driver exits 0 with an `equal` line for every job and round, R1 and R4 name different kernels, and the serial
    frames of the render jobs are within 1e-3 of the oracle with equal ray counts (R3 is launched without stats, as its
    job says, so only its frame is compared)."""
    import hrt
    from oracle import oracle as O

    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for k in range(ROUNDS):
        for job in JOBS:
            assert f"round {k} {job} equal" in lines, (k, job, r.stdout)
    assert "threads: ok" in lines
    serial = {}
    for ln in lines:
        m = re.fullmatch(r"serial (\w+) segments=(\d+) kernel=(.*)", ln)
        if m:
            serial[m.group(1)] = (int(m.group(2)), m.group(3))
    assert set(serial) == set(JOBS)
    assert all(kernel for _, kernel in serial.values())
    assert serial["R1"][1] != serial["R4"][1]  # the sphere kernel and the general kernel
    assert serial["R1"][1] == serial["R2"][1] == serial["R3"][1]

    rnd = O.OracleScene(hrt.PRESETS["random"], 1, earth)
    box = O.OracleScene(hrt.PRESETS["cornell"], 1, earth)
    cases = [("R1", rnd, 64, 36, None, True), ("R2", rnd, 37, 19, _oracle_camera(rnd, LOOK_FROM_1), True),
             ("R3", rnd, 64, 36, _oracle_camera(rnd, LOOK_FROM_2), False), ("R4", box, 32, 32, None, True)]
    for job, o, w, h, cam, counted in cases:
        img = hrt.read_pfm(str(tmp_path / f"{job}.pfm"))
        ref, cnt = o.render(w, h, 8, 50, seed=1, camera=cam)
        assert img.shape == (h, w, 3)
        linf = float(np.abs(img - ref[..., :3]).max())
        print(f"{job}: Linf {linf:.3e}, segments {serial[job][0]} (oracle {cnt['segments']})")
        assert np.isfinite(img).all()
        assert linf <= TOL, (job, linf)
        if counted:
            assert serial[job][0] == cnt["segments"], (job, serial[job][0], cnt["segments"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
def test_binding_under_python_threads():
    """Four Python threads behind a barrier, three rounds each: hrt.render of `random` 64x36 at 8 spp from two cameras,
    an hrt.Accumulator with two passes and resolve(), hrt.trace_paths_fused of a 32x18 frame.  Every result equals the same
    call made before the threads started, bit for bit, and hrt.last_launch()["kernel"] read inside a thread is the serial
    value for that call.  (ctypes drops the GIL for the length of a call, so the library calls do overlap.)"""
    import hrt

    s = hrt.preset("random", 1)
    s.commit()
    bg = tuple(s.info.background)
    info = s.info
    W, H = 64, 36
    cam_a = hrt.preset_camera(info, W, H)
    cam_b = hrt.camera(LOOK_FROM_1, info.look_at, info.fov, info.aperture, info.focus_dist, info.time0, info.time1, W, H)
    cam_q = hrt.preset_camera(info, 32, 18)

    def render(cam):
        img = hrt.render(s, cam, hrt.params(W, H, 8, 50, 1, bg))
        return [img], hrt.last_launch()["kernel"]

    def accumulate():
        acc = hrt.Accumulator(s, W, H)
        try:
            acc.add(cam_a, hrt.params(W, H, 8, 50, 1, bg))
            acc.add(cam_a, hrt.params(W, H, 8, 50, 1, bg, sample_offset=8))
            kernel = hrt.last_launch()["kernel"]
            return [acc.resolve()], kernel
        finally:
            acc.close()

    def paths():
        radiance, n_rays = hrt.trace_paths_fused(s, cam_q, hrt.params(32, 18, 2, 50, 1, bg))
        return [radiance, np.array([n_rays], np.uint32)], hrt.last_launch()["kernel"]

    calls = [lambda: render(cam_a), lambda: render(cam_b), accumulate, paths]
    serial = [c() for c in calls]
    assert not np.array_equal(_bits(serial[0][0][0]), _bits(serial[1][0][0]))  # two views, two frames
    barrier = threading.Barrier(len(calls))
    problems = []

    def work(k):
        try:
            for rnd in range(ROUNDS):
                barrier.wait(timeout=60)
                arrays, kernel = calls[k]()
                want_arrays, want_kernel = serial[k]
                if kernel != want_kernel:
                    problems.append(f"thread {k} round {rnd}: kernel {kernel!r}, serial {want_kernel!r}")
                for a, b in zip(arrays, want_arrays):
                    if a.shape != b.shape or not np.array_equal(_bits(a), _bits(b)):
                        problems.append(f"thread {k} round {rnd}: a result differs from the serial call")
        except Exception as e:  # a thread's exception must fail the test, not vanish
            problems.append(f"thread {k}: {e!r}")
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(calls))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 120  # a cap so that a deadlock fails the test, not a measurement
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in threads), "a thread is still running: deadlock"
    assert not problems, problems
    s.close()


@pytest.mark.gpu
def test_a_smaller_scene_does_not_lower_the_lds_limit_of_a_larger_one():
    """resident_grid (kernel_common.h) sets hipFuncAttributeMaxDynamicSharedMemorySize whenever it first sees a (kernel,
    device, LDS bytes) triple, so a scene with a smaller walk stream sets the limit of the same kernel instantiation below
    what an earlier scene needs.  `random` (a large stream), then a scene of 41 plain spheres (the same kernel, fewer LDS
    bytes; built here so that no earlier test of the process has cached its triple), then `random` again: both `random`
    frames are equal bit for bit and the small scene's frame equals its own second render."""
    import hrt

    big = hrt.preset("random", 1)
    big.commit()
    cam_big = hrt.preset_camera(big.info, 64, 36)
    p_big = hrt.params(64, 36, 8, 50, 1, tuple(big.info.background))
    small = hrt.Scene()
    grey = small.lambertian(small.solid(0.5, 0.5, 0.5))
    metal = small.metal((0.8, 0.6, 0.2), 0.1)
    # 40 spheres: above the 15 node parts up to which the sphere kernel walks a stream as one packet (another instantiation)
    balls = [small.sphere((0.7 * (k % 8 - 3.5), 0.3, -0.7 * (k // 8)), 0.3, metal if k & 1 else grey) for k in range(40)]
    small.set_root(small.bvh(balls + [small.sphere((0.0, -1000.0, 0.0), 1000.0, grey)]))
    small.commit()
    cam_small = hrt.camera((0.0, 1.0, 5.0), (0.0, 0.3, 0.0), 40.0, 0.0, 5.0, 0.0, 1.0, 32, 18)
    p_small = hrt.params(32, 18, 8, 50, 1, (0.7, 0.8, 1.0))
    first = hrt.render(big, cam_big, p_big)
    launch_big = hrt.last_launch()
    small_first = hrt.render(small, cam_small, p_small)
    launch_small = hrt.last_launch()
    # the case exercises the path only while these two hold
    assert launch_small["kernel"] == launch_big["kernel"]
    assert 0 < launch_small["lds_bytes"] < launch_big["lds_bytes"]
    again = hrt.render(big, cam_big, p_big)
    assert hrt.last_launch()["lds_bytes"] == launch_big["lds_bytes"]
    small_again = hrt.render(small, cam_small, p_small)
    assert np.array_equal(_bits(first), _bits(again))
    assert np.array_equal(_bits(small_first), _bits(small_again))
    assert np.isfinite(first).all() and float(first[..., :3].max()) > 0
    small.close()
    big.close()
