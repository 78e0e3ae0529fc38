"""examples/render_denoise.c: the plain and the filtered frame of an accumulator through the C ABI alone
(hrt_accum_resolve_filtered_host) builds warning-free, fails loudly without a device, and on a GPU writes the frames
hrt.Accumulator.resolve() and resolve(denoise=...) give, bit for bit."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cdenoise") / "render_denoise")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_denoise.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_denoise_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count("render_denoise") == 2   # built by `all`, removed by `clean`


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_denoise_example_fails_loudly_without_a_device(exe, tmp_path):
    r = subprocess.run([exe, "8", "8", "4", "2", "3", "4.0", str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")],
                       capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not (tmp_path / "a.pfm").exists() and not (tmp_path / "b.pfm").exists()


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_denoise_example_writes_the_library_frames(exe, tmp_path):
    """The Cornell box at 48x40, 3 passes of 16 spp, 2 iterations at sigma 3: both PFMs are the Python binding's."""
    import numpy as np

    import hrt

    plain, filtered = tmp_path / "plain.pfm", tmp_path / "filtered.pfm"
    r = subprocess.run([exe, "48", "40", "16", "3", "2", "3.0", str(plain), str(filtered)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "48 spp" in r.stdout and "2 iterations at sigma 3" in r.stdout
    s = hrt.preset("cornell", 1)
    s.commit()
    w, h = 48, 40
    a = hrt.Accumulator(s, w, h, noise=True)
    cam = hrt.preset_camera(s.info, w, h)
    for k in range(3):
        a.add(cam, hrt.params(w, h, 16, 50, 1, tuple(s.info.background), sample_offset=16 * k))
    want_plain, want_filtered = a.resolve(), a.resolve(denoise=dict(iterations=2, sigma=3.0))
    assert not np.array_equal(want_plain, want_filtered)
    for path, want in ((plain, want_plain), (filtered, want_filtered)):
        img = hrt.read_pfm(str(path))
        assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))
    a.close()
    s.close()
