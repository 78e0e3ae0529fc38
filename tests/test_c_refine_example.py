"""examples/render_refine.c: a frame refined pass by pass through hrt_accum_* on the C ABI alone (no Python, no
PyTorch) builds warning-free, fails loudly without a device, and on a GPU its passes add up to the oracle's frame."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cref") / "render_refine")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_refine.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_refine_example_fails_loudly_without_a_device(exe, tmp_path):
    r = subprocess.run([exe, "8", "8", "1", "2", str(tmp_path / "p.ppm"), str(tmp_path / "x.pfm")], capture_output=True,
                       text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not (tmp_path / "p.ppm").exists() and not (tmp_path / "x.pfm").exists()


def _read_pfm(path):
    import numpy as np

    data = open(path, "rb").read()
    head, rest = data.split(b"\n", 1)
    size, rest = rest.split(b"\n", 1)
    scale, rest = rest.split(b"\n", 1)
    assert head == b"PF" and float(scale) < 0  # RGB, little-endian
    w, h = map(int, size.split())
    return np.frombuffer(rest, "<f4", count=w * h * 3).reshape(h, w, 3)  # scanlines bottom to top = y up


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_refine_example_passes_add_up_to_the_oracle(exe, tmp_path, earth):
    """64x36 in 3 passes of 4 spp: the PFM is the oracle's 12-spp frame (the project's bar), the preview exists."""
    import numpy as np

    import hrt
    from oracle import oracle as O

    pre, out = tmp_path / "pre.ppm", tmp_path / "fin.pfm"
    r = subprocess.run([exe, "64", "36", "4", "3", str(pre), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "3 passes of 4 spp = 12 spp" in r.stdout and "rays" in r.stdout
    assert pre.read_bytes().startswith(b"P6\n64 36\n255\n")
    assert len(pre.read_bytes()) == len(b"P6\n64 36\n255\n") + 64 * 36 * 3
    img = _read_pfm(out)
    ref, cnt = O.OracleScene(hrt.PRESETS["random"], 1, earth).render(64, 36, 12, 50, seed=1)
    assert float(np.abs(img - ref[..., :3]).max()) <= 1e-3
    assert f" {cnt['segments']} rays" in r.stdout   # the passes' rays sum to the oracle's count exactly
