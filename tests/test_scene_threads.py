"""The host half of a scene under ThreadSanitizer: scene.cpp, presets.cpp, knobs.cpp and image_io.cpp (the constructors,
BvhNode::new, the walk-stream builders, the host part of hrt_scene_commit) compiled with -fsanitize=thread together with
tests/native/scene_threads_tsan.cpp, a stand-alone program with its own main, and run as a child process.  The driver
defines the only two symbols those files need from the HIP objects (hrt::device_upload returning HRT_OK, hrt::device_release
a no-op), so no HIP object is linked, no Python process loads the result and nothing is preloaded.

It builds and commits random, two_spheres, two_perlin_spheres, simple_light, cornell, cornell_smoke, final, features and
motion (random and final twice) serially, keeps every hrt_debug_scene_blob, builds all of them again on one thread each and
compares the blobs byte for byte, while two more threads make argument errors of different kinds and each checks that
hrt_last_error() is its own text.  What this does NOT cover: the .hip translation units (render.hip's slots, lists and
caches), which TSan cannot see; tests/test_gpu_threads.py holds their results, not their races."""
import os
import subprocess

from conftest import tool_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hyper-ray-tracer_amd", "csrc")
HOST_SOURCES = ("scene.cpp", "presets.cpp", "knobs.cpp", "image_io.cpp")
PRESETS = ("random", "two_spheres", "two_perlin_spheres", "simple_light", "cornell", "cornell_smoke", "final", "features",
           "motion", "random (second)", "final (second)")


def test_scene_host_is_race_free_and_deterministic_across_threads(tmp_path):
    exe = str(tmp_path / "scene_threads_tsan")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-fsanitize=thread", "-g", "-O1", "-ffp-contract=off", "-fno-fast-math",
                    "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
                   + [os.path.join(CSRC, f) for f in HOST_SOURCES]
                   + [os.path.join(HERE, "native", "scene_threads_tsan.cpp"), "-o", exe],
                   check=True, env=tool_env())
    r = subprocess.run([exe], capture_output=True, text=True, env=tool_env(), timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "WARNING: ThreadSanitizer" not in out, out
    lines = r.stdout.splitlines()
    for name in PRESETS:
        assert any(ln.startswith(name + " ") and ln.endswith("threaded vs serial identical") for ln in lines), (name, out)
    assert sum("0 of 200 calls read another text" in ln for ln in lines) == 2, out
    assert "scene_threads_tsan: ok" in r.stdout
