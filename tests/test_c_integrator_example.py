"""examples/render_integrator.c: a frame rendered through the query calls of the C ABI alone (hrt_camera_paths_host,
hrt_scene_intersect_host, hrt_scene_scatter_host) builds warning-free, fails loudly without a device, and on a GPU
writes the frame an hrt.Accumulator fed the same one-sample passes resolves to."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cintegrator") / "render_integrator")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_integrator.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt", "-lm",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_integrator_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count("render_integrator") == 2   # built by `all`, removed by `clean`


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_integrator_example_fails_loudly_without_a_device(exe, tmp_path):
    path = str(tmp_path / "integrator.pfm")
    r = subprocess.run([exe, "16", "9", "2", path], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not os.path.exists(path)


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_integrator_example_writes_the_accumulators_frame(exe, tmp_path):
    """`random` at 64x36, 4 spp: the PFM equals an accumulator fed the four one-sample passes (sample_offset 0 .. 3) and
    resolved, bit for bit, and the printed ray count is the sum of those passes' segments."""
    import numpy as np

    import hrt

    w, h, spp = 64, 36, 4
    path = tmp_path / "integrator.pfm"
    r = subprocess.run([exe, str(w), str(h), str(spp), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    words = r.stdout.split()
    s = hrt.preset("random", 1)
    s.commit()
    cam = hrt.preset_camera(s.info, w, h)
    acc = hrt.Accumulator(s, w, h)
    segments = 0
    for k in range(spp):
        st = acc.add(cam, hrt.params(w, h, 1, 50, 1, tuple(s.info.background), sample_offset=k), stats=True)
        segments += int(st.segments)
    frame = acc.resolve("f32")
    img = hrt.read_pfm(str(path))
    assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    assert words[0] == "rays" and int(words[1]) == segments
    acc.close()
    s.close()
