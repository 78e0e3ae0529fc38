"""examples/render_adaptive_filtered.c: refinement driven by hrt_accum_noise_filtered on the C ABI alone builds
warning-free, fails loudly without a device, and on a GPU runs the policies of hrt.Accumulator.refine and
refine_filtered to the same tiles, and writes the filtered frame of the second, bit for bit."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cadaptf") / "render_adaptive_filtered")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_adaptive_filtered.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_adaptive_filtered_example_fails_loudly_without_a_device(exe, tmp_path):
    r = subprocess.run([exe, "8", "8", "4", "1", "0.05", "4", str(tmp_path / "x.pfm")], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not (tmp_path / "x.pfm").exists()


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_adaptive_filtered_example_runs_both_policies(exe, tmp_path):
    """64x36 in 16-px tiles, passes of 40 spp to a mean error of 0.05, at most 400 spp: the tiles' sample counts are those
    of hrt.Accumulator.refine and refine_filtered with the same arguments, and the PFM is resolve(denoise=True) of the
    second."""
    import numpy as np

    import hrt

    out = tmp_path / "adaptive_filtered.pfm"
    r = subprocess.run([exe, "64", "36", "16", "40", "0.05", "400", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert "(raw error)" in lines[0] and "(filtered estimate)" in lines[1]
    held = [[int(v) for v in line.split(":")[1].split()] for line in lines[:2]]
    s = hrt.preset("random", 1)
    s.commit()
    w, h = 64, 36
    args = (hrt.preset_camera(s.info, w, h), hrt.params(w, h, 1, 50, 1, tuple(s.info.background)), 0.05, 40, 400)
    a = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16), noise=True)
    a.refine(*args)
    b = hrt.Accumulator(s, w, h, hrt.tile_grid(w, h, 16), noise=True)
    b.refine_filtered(*args)
    assert held[0] == a.tile_samples and held[1] == b.tile_samples
    totals = [sum(n * tw * th for n, (_, _, tw, th) in zip(x.tile_samples, x.tiles)) for x in (a, b)]
    assert f"raw error {totals[0]} samples" in lines[2] and f"filtered estimate {totals[1]} samples" in lines[2]
    px, off = b.resolve(denoise=True), 0
    frame = np.zeros((h, w, 4), np.float32)
    for x, y, tw, th in b.tiles:
        frame[y:y + th, x:x + tw] = px[off:off + tw * th].reshape(th, tw, 4)
        off += tw * th
    img = hrt.read_pfm(str(out))
    assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    for x in (a, b):
        x.close()
    s.close()
