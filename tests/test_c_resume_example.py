"""examples/render_resume.c: checkpoint and resume of a noise-driven refinement through hrt_accum_snapshot /
hrt_accum_snapshot_info / hrt_accum_restore on the C ABI alone builds warning-free, fails loudly without a device, and
on a GPU the resumed run gives the uninterrupted run's frame and per-tile samples, which are those of
hrt.Accumulator.refine with the same arguments."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cresume") / "render_resume")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_resume.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_resume_example_fails_loudly_without_a_device(exe, tmp_path):
    r = subprocess.run([exe, "8", "8", "4", "1", "0.05", "4", str(tmp_path / "x.hrts")], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not (tmp_path / "x.hrts").exists()


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_resume_example_resumes_to_the_uninterrupted_frame(exe, tmp_path):
    """64x36 in 16-px tiles, passes of 40 spp to a mean error of 0.05, at most 400 spp, stopped after two rounds."""
    import hrt

    ckpt = tmp_path / "resume.hrts"
    r = subprocess.run([exe, "64", "36", "16", "40", "0.05", "400", str(ckpt)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "frame: identical, samples per tile: identical"
    assert "tiles differ" in lines[1]       # the checkpoint was taken while the tiles held different passes
    held = [int(v) for v in lines[0].split(":")[1].split()]
    blob = ckpt.read_bytes()
    info, tiles = hrt.snapshot_info(blob)
    assert (info.width, info.height, info.n_tiles, info.flags, info.uniform, info.bytes) == (64, 36, 12, hrt.ACCUM_NOISE, 0, len(blob))
    # the Python policy from the same checkpoint ends at the same tiles
    s = hrt.preset("random", 1)
    s.commit()
    a = hrt.Accumulator.load(s, ckpt)
    assert sorted(set(a.tile_samples)) == [40, 80]     # two rounds: the tiles that stopped after the first, and the rest
    a.refine(hrt.preset_camera(s.info, 64, 36), hrt.params(64, 36, 1, 50, 1, tuple(s.info.background)), 0.05, 40, 400, resume=True)
    assert a.tile_samples == held and len(set(held)) > 1
    a.close()
    s.close()
