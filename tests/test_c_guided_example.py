"""examples/render_guided.c: the plain, the variance-only and the feature-guided frame of an accumulator through the C
ABI alone (hrt_accum_add_features, hrt_accum_resolve_guided_host) builds warning-free, fails loudly without a device,
and on a GPU writes the frames the Python binding gives, bit for bit."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cguided") / "render_guided")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_guided.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_guided_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count("render_guided") == 2   # built by `all`, removed by `clean`


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_guided_example_fails_loudly_without_a_device(exe, tmp_path):
    paths = [str(tmp_path / n) for n in ("a.pfm", "b.pfm", "c.pfm")]
    r = subprocess.run([exe, "8", "8", "4", "2", "4", *paths], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not any(os.path.exists(p) for p in paths)


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_guided_example_writes_the_library_frames(exe, tmp_path):
    """The Cornell box at 48x40, two passes of 50 spp and a 16-sample feature pass: the three PFMs are the Python
    binding's."""
    import numpy as np

    import hrt

    paths = [tmp_path / n for n in ("plain.pfm", "filtered.pfm", "guided.pfm")]
    r = subprocess.run([exe, "48", "40", "50", "2", "16", *[str(p) for p in paths]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "100 spp and 16 feature samples" in r.stdout
    s = hrt.preset("cornell", 1)
    s.commit()
    w, h = 48, 40
    a = hrt.Accumulator(s, w, h, noise=True, features=True)
    cam = hrt.preset_camera(s.info, w, h)
    for k in range(2):
        a.add(cam, hrt.params(w, h, 50, 50, 1, tuple(s.info.background), sample_offset=50 * k))
    a.add_features(cam, hrt.params(w, h, 16, 50, 1, tuple(s.info.background)))
    want = a.resolve(), a.resolve(denoise=True), a.resolve_guided(guide=dict(normal=0.1, albedo=0.1, depth=0.1))
    assert not np.array_equal(want[1], want[2]) and not np.array_equal(want[0], want[2])
    for path, frame in zip(paths, want):
        img = hrt.read_pfm(str(path))
        assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    a.close()
    s.close()
