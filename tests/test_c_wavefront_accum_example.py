"""examples/render_accum_wavefront.c: a wavefront loop on the C ABI whose passes end in an accumulator through
hrt_accum_add_paths.  It builds warning-free, is in the examples' Makefile and fails loudly without a device; on the GPU
it exits 0 only if its accumulator equals one fed the same passes by hrt_accum_add, and the filtered frame it writes is
the one an hrt.Accumulator given those passes resolves to, bit for bit."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NAME = "render_accum_wavefront"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("caccumwavefront") / NAME)
    lib = os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROCM, "include"),
                    os.path.join(ROOT, "examples", NAME + ".c"), "-o", out, "-L" + lib, "-lhrt",
                    "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, env=tool_env())
    return out


def test_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count(NAME) == 2   # built by `all`, removed by `clean`
    all_line = [ln for ln in text.splitlines() if ln.startswith("all:")][0]
    assert NAME in all_line and NAME in text.split("clean:")[1]
    assert "examples/" + NAME + "\n" in open(os.path.join(ROOT, ".gitignore")).read()


def _has_gpu():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_example_fails_loudly_without_a_device(exe, tmp_path):
    path = str(tmp_path / "frame.pfm")
    r = subprocess.run([exe, "16", "9", "2", path], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not os.path.exists(path)


@pytest.mark.gpu
def test_example_writes_the_accumulators_filtered_frame(exe, tmp_path):
    """`random` at 64x36, three passes of 4 spp: exit status 0 (the example's own comparison of the two routes), the PFM
    equals the filtered resolve of an accumulator fed the three passes by `add`, and the rays are those passes' segments."""
    import numpy as np

    import hrt

    w, h, passes = 64, 36, 3
    path = tmp_path / "frame.pfm"
    r = subprocess.run([exe, str(w), str(h), str(passes), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    words = r.stdout.split()
    s = hrt.preset("random", 1)
    s.commit()
    cam = hrt.preset_camera(s.info, w, h)
    acc = hrt.Accumulator(s, w, h, noise=True)
    segments = 0
    for k in range(passes):
        st = acc.add(cam, hrt.params(w, h, 4, 50, 1, tuple(s.info.background), sample_offset=4 * k), stats=True)
        segments += int(st.segments)
    frame = acc.resolve("f32", denoise=dict(iterations=3, sigma=4.0))
    img = hrt.read_pfm(str(path))
    assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    assert words[0] == "rays" and int(words[1]) == segments and words[2] == "rendered" and int(words[3]) == segments
    assert "agree" in words
    acc.close()
    s.close()
