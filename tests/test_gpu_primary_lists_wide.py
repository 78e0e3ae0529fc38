"""The camera segment's 16-entry leaf lists and their reuse across launches (csrc/primary_list.h, render_sphere.hip,
render.hip) on the GPU.

As tests/test_gpu_primary_lists.py, whose helpers this reuses: every case renders with HRT_PRIMARY_LISTS=0 (every
ray walks the stream) and with the named capacity (None: the default, 16), and requires the same pixel bits and
equal segments, samples, pixels and tex_evals.  tests/test_primary_lists_wide.py checks the lists themselves
against the walk on the host.

Reuse: the lists are built once per view and kept by the scene (render.hip ViewLists).  Launches from camera A, B
and A again, on one stream and on two streams with both launches in flight, and launches around a re-commit, must
each give the frame of a freshly committed scene rendered without lists.
"""
import numpy as np
import pytest

import cameras as C
import hrt
from test_gpu_primary_lists import SEED, _both, _render, _same

# tiles of the 1920x1080 `random` frame: cells 186..189 x 87..92 (the frame's 16-, 17- and 18-leaf cells among them),
# cells of 12..16 leaves, and sky
LONG_TILES = [(1488, 696, 32, 48), (800, 704, 64, 32), (37, 5, 24, 8)]


@pytest.fixture(scope="module")
def scenes(earth):
    out = {}

    def get(name):
        if name not in out:
            s = hrt.preset(name, 1, earth)
            s.commit()
            out[name] = s
        return out[name]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("lists", [None, 16, 12, 9])
def test_small_frame_at_each_capacity(monkeypatch, scenes, lists):
    """64x36: cells of at most 8 leaves, of 9 .. 16 and of more (overflow) in one frame."""
    W, H, spp = 64, 36, 8
    off, st_off, on, st_on = _both(monkeypatch, scenes("random"), W, H, spp, lists=lists)
    assert st_on.pixels == W * H and st_on.samples == W * H * spp
    _same(off, st_off, on, st_on)


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,spp", [
    ("random", 40, 24, 100),     # head and tail chunks; every cell has 9 .. 61 leaves
    ("random", 37, 23, 8),       # partial cells on both axes
    ("motion", 48, 27, 8),       # per-sphere shutters
    ("random_10k", 32, 18, 2),   # a hybrid stream: no lists, the same instantiation
])
def test_frame_is_the_walks_frame(monkeypatch, scenes, name, W, H, spp):
    off, st_off, on, st_on = _both(monkeypatch, scenes(name), W, H, spp)
    assert st_on.pixels == W * H and st_on.samples == W * H * spp
    _same(off, st_off, on, st_on)


@pytest.mark.gpu
def test_long_cells_of_the_headline_frame(monkeypatch, scenes):
    """The tiles with the frame's longest lists, counted: the default capacity replaces more node steps than
    capacity 8, which replaces more than no lists."""
    s = scenes("random")
    off, st_off, on16, st16 = _both(monkeypatch, s, 1920, 1080, 8, tiles=LONG_TILES, flags=hrt.RENDER_COUNT_WORK)
    _same(off, st_off, on16, st16)
    off2, st_off2, on8, st8 = _both(monkeypatch, s, 1920, 1080, 8, tiles=LONG_TILES, lists=8, flags=hrt.RENDER_COUNT_WORK)
    _same(off2, st_off2, on8, st8)
    assert np.array_equal(off, off2)
    print(f"node visits: lists off {st_off.node_visits}, capacity 8 {st8.node_visits}, default {st16.node_visits}")
    assert st16.node_visits < st8.node_visits < st_off.node_visits, (st16.node_visits, st8.node_visits, st_off.node_visits)


def _specs(s):
    return C.spec("random", None, s.info), C.spec("random", "wide", s.info)


@pytest.fixture(scope="module")
def walked(earth):
    """The frames of a freshly committed `random` rendered without lists: {(camera index, case): pixels}, computed
    once."""
    import os

    s = hrt.preset("random", 1, earth)
    s.commit()
    old = os.environ.get("HRT_PRIMARY_LISTS")
    os.environ["HRT_PRIMARY_LISTS"] = "0"
    try:
        out = {}
        for i, cam in enumerate(_specs(s)):
            out[i, "small"] = _render(s, 64, 36, 8, camera=cam)[0]
            out[i, "tiles"] = _render(s, 1920, 1080, 8, tiles=LONG_TILES, camera=cam)[0]
    finally:
        if old is None:
            del os.environ["HRT_PRIMARY_LISTS"]
        else:
            os.environ["HRT_PRIMARY_LISTS"] = old
    return out


CASES = {"small": (64, 36, 8, None), "tiles": (1920, 1080, 8, LONG_TILES)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small", "tiles"])
def test_lists_follow_the_camera(monkeypatch, earth, walked, case):
    """Camera A, B, A again (the second A reuses nothing stale), then A once more (reuses A's lists)."""
    monkeypatch.delenv("HRT_PRIMARY_LISTS", raising=False)
    W, H, spp, tiles = CASES[case]
    s = hrt.preset("random", 1, earth)
    s.commit()
    cams = _specs(s)
    for i in (0, 1, 0, 0, 1):
        got, _ = _render(s, W, H, spp, tiles=tiles, camera=cams[i])
        assert np.array_equal(got, walked[i, case]), (case, i)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small", "tiles"])
def test_two_cameras_in_flight_on_two_streams(monkeypatch, earth, walked, case):
    """A and B alternate over two streams, nothing waited for between the launches: a launch whose key differs
    from the lists a launch in flight reads builds its own, and a launch on the other stream than the builder's
    waits for the build."""
    import torch

    monkeypatch.delenv("HRT_PRIMARY_LISTS", raising=False)
    W, H, spp, tiles = CASES[case]
    tiles = tiles if tiles is not None else [(0, 0, W, H)]
    s = hrt.preset("random", 1, earth)
    s.commit()
    cams = [hrt.camera(*sp, W, H) for sp in _specs(s)]
    p = hrt.params(W, H, spp, 50, SEED, tuple(s.info.background))
    n = sum(t[2] * t[3] for t in tiles)
    order = [(0, 0), (1, 1), (0, 1), (1, 0), (0, 0), (1, 1)]  # (camera, stream)
    bufs = [torch.zeros(n * 4, device="cuda") for _ in order]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for (ci, si), d in zip(order, bufs):
        hrt.render_tiles_device(s, cams[ci], p, tiles, d.data_ptr(), streams[si].cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    for (ci, si), d in zip(order, bufs):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), walked[ci, case]), (case, ci, si)


@pytest.mark.gpu
def test_another_camera_leaves_the_lists_of_a_launch_in_flight(monkeypatch, earth):
    """The two-stream cases above are short launches, which may never overlap.  Here camera A renders the whole
    1920x1080 frame (milliseconds on the GPU) and camera B's small launches are enqueued behind it on another stream
    at once (tens of microseconds each on the host), so they find A in flight: they must build into their slots'
    buffers.  Were A's lists rebuilt in place for B's camera, A's cells would read lists of another view, and its
    frame would lose hits against the frame rendered without lists.

    This tests the effect, not the path taken (the library reports no count of builds): an in-place rebuild is caught
    only where A's kernel has not yet passed the cells that B's build overwrites, which holds for nearly all of a
    frame that renders for milliseconds behind builds enqueued within its first fraction of one."""
    import torch

    W, H, spp = 1920, 1080, 8
    s = hrt.preset("random", 1, earth)
    s.commit()
    spec_a, spec_b = _specs(s)
    monkeypatch.setenv("HRT_PRIMARY_LISTS", "0")
    want_a = _render(s, W, H, spp, camera=spec_a)[0]
    want_b = _render(s, W, H, spp, tiles=LONG_TILES, camera=spec_b)[0]
    monkeypatch.delenv("HRT_PRIMARY_LISTS")
    cam_a, cam_b = hrt.camera(*spec_a, W, H), hrt.camera(*spec_b, W, H)
    p = hrt.params(W, H, spp, 50, SEED, tuple(s.info.background))
    n_b = sum(t[2] * t[3] for t in LONG_TILES)
    full = torch.zeros(W * H * 4, device="cuda")
    small = [torch.zeros(n_b * 4, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    hrt.render_tiles_device(s, cam_a, p, [(0, 0, W, H)], full.data_ptr(), streams[0].cuda_stream)
    for d in small:
        hrt.render_tiles_device(s, cam_b, p, LONG_TILES, d.data_ptr(), streams[1].cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(full.cpu().numpy().view(np.uint32), want_a)
    for d in small:
        assert np.array_equal(d.cpu().numpy().view(np.uint32), want_b)


@pytest.mark.gpu
def test_commit_between_two_launches(monkeypatch, earth, walked):
    """The lists live and die with a commit's device state.  A committed scene is immutable (a second
    hrt_scene_commit is refused and must leave the scene and its lists usable), so the scene is committed anew the
    only way the ABI allows: the first is destroyed and the preset built and committed again between the launches."""
    monkeypatch.delenv("HRT_PRIMARY_LISTS", raising=False)
    s = hrt.preset("random", 1, earth)
    s.commit()
    cam = _specs(s)[0]
    first, _ = _render(s, 64, 36, 8, camera=cam)
    with pytest.raises(hrt.HrtError):
        s.commit()
    again, _ = _render(s, 64, 36, 8, camera=cam)
    del s
    s = hrt.preset("random", 1, earth)
    s.commit()
    second, _ = _render(s, 64, 36, 8, camera=cam)
    for got in (first, again, second):
        assert np.array_equal(got, walked[0, "small"])
