"""examples/render_autofocus.c: picking and autofocus through the C ABI alone (hrt_camera_rays_host,
hrt_scene_intersect_host) builds warning-free, fails loudly without a device, and on a GPU reports the primitive and the
depth Scene.intersect gives and the frame the Python binding renders at that focus distance."""
import os
import subprocess

import pytest
from conftest import tool_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cautofocus") / "render_autofocus")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "render_autofocus.c"), "-o", out,
                    "-L" + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib"), "-lhrt", "-lm",
                    "-Wl,-rpath," + os.path.join(ROOT, "hyper-ray-tracer_amd", "lib")], check=True, env=tool_env())
    return out


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def test_autofocus_example_is_in_the_examples_makefile(exe):
    text = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert text.count("render_autofocus") == 2   # built by `all`, removed by `clean`


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device path")
def test_autofocus_example_fails_loudly_without_a_device(exe, tmp_path):
    path = str(tmp_path / "focus.pfm")
    r = subprocess.run([exe, "16", "9", "2", path], capture_output=True, text=True)
    assert r.returncode == 1
    assert "status 6" in r.stderr          # HRT_ERR_HIP from the scene upload
    assert not os.path.exists(path)


@pytest.mark.gpu
@pytest.mark.skipif(not _has_gpu(), reason="needs a GPU")
def test_autofocus_example_reports_the_librarys_depth(exe, tmp_path):
    """`random` at 64x36, 4 spp: the printed primitive, material and depth are Scene.intersect's for the centre pixel's
    pinhole ray, and the PFM is the Python binding's render with focus_dist = that depth."""
    import numpy as np

    import hrt

    w, h, spp = 64, 36, 4
    path = tmp_path / "focus.pfm"
    r = subprocess.run([exe, str(w), str(h), str(spp), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    words = r.stdout.split()
    s = hrt.preset("random", 1)
    s.commit()
    i = s.info
    pinhole = hrt.camera(i.look_from, i.look_at, i.fov, 0.0, i.focus_dist, i.time0, i.time1, w, h)
    bg = tuple(i.background)
    ray = hrt.camera_rays(s, pinhole, hrt.params(w, h, 1, 50, 1, bg), tiles=[(w // 2, h // 2, 1, 1)])
    hit = s.intersect(ray, seed=1, shutter=(pinhole.time0, pinhole.time1))[0]
    assert hit["flags"] & hrt.HIT_HIT
    d = ray[0]["direction"]
    depth = hit["t"] * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=np.float32)
    assert words[0:4] == ["prim", str(hit["prim"]), "material", str(hit["material"])]
    assert np.float32(float(words[5])) == depth and 1.0 < depth < 30.0
    cam = hrt.camera(i.look_from, i.look_at, i.fov, i.aperture, float(depth), i.time0, i.time1, w, h)
    frame = hrt.render(s, cam, hrt.params(w, h, spp, 50, 1, bg))
    img = hrt.read_pfm(str(path))
    assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32))
    s.close()
