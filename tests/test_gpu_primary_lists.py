"""The camera segment's per-cell leaf lists (csrc/primary_list.h, render_sphere.hip) on the GPU.

Every case renders twice, with HRT_PRIMARY_LISTS=0 (every ray walks the stream, as before the lists) and with the
default (or the capacity the case names), and requires the same bits: np.array_equal on the uint32 view of the
pixels, and equal segments, samples, pixels and tex_evals.  tests/test_primary_lists.py checks the lists
themselves against the walk on the host.
"""
import numpy as np
import pytest

import hrt
from hrt.tiling import split_tiles

SEED = 5


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


def _render(s, W, H, spp, depth=50, tiles=None, flags=0, camera=None):
    """The call's pixels as uint32 (packed tile after tile) and its stats.  camera: a tests/cameras.py spec in place
    of the preset's own."""
    import torch

    cam = hrt.preset_camera(s.info, W, H) if camera is None else hrt.camera(*camera, W, H)
    p = hrt.params(W, H, spp, depth, SEED, tuple(s.info.background), flags=flags)
    tiles = tiles if tiles is not None else [(0, 0, W, H)]
    n = sum(t[2] * t[3] for t in tiles)
    d = torch.zeros(n * 4, device="cuda")
    st = hrt.render_tiles_device(s, cam, p, tiles, d.data_ptr(), 0, want_stats=True)
    return d.cpu().numpy().view(np.uint32), st


def _both(monkeypatch, s, *a, lists=None, **k):
    monkeypatch.setenv("HRT_PRIMARY_LISTS", "0")
    off, st_off = _render(s, *a, **k)
    name_off = hrt.last_launch()["kernel"]
    if lists is None:
        monkeypatch.delenv("HRT_PRIMARY_LISTS")
    else:
        monkeypatch.setenv("HRT_PRIMARY_LISTS", str(lists))
    on, st_on = _render(s, *a, **k)
    assert hrt.last_launch()["kernel"] == name_off  # one instantiation, with and without lists
    return off, st_off, on, st_on


def _same(off, st_off, on, st_on):
    assert np.array_equal(off, on)
    for f in ("segments", "samples", "pixels", "tex_evals"):
        assert getattr(st_off, f) == getattr(st_on, f), f


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H,spp", [
    ("random", 64, 36, 8),        # one chunk
    ("random", 40, 24, 100),      # head and tail chunks
    ("random", 37, 23, 8),        # partial cells on both axes
    ("motion", 48, 27, 8),        # per-sphere shutters
    ("two_spheres", 48, 27, 8),   # lens radius 0 (the packet walk: no lists)
])
def test_frame_is_the_walks_frame(monkeypatch, scenes, name, W, H, spp):
    off, st_off, on, st_on = _both(monkeypatch, scenes(name), W, H, spp)
    assert st_on.pixels == W * H and st_on.samples == W * H * spp
    _same(off, st_off, on, st_on)


@pytest.mark.gpu
def test_lists_replace_node_steps(monkeypatch, scenes):
    """The COUNT build: same frame, and fewer node visits with the lists (the phase runs by default and its steps
    are counted as node visits and walk steps)."""
    off, st_off, on, st_on = _both(monkeypatch, scenes("random"), 64, 36, 8, flags=hrt.RENDER_COUNT_WORK)
    _same(off, st_off, on, st_on)
    assert 0 < st_on.node_visits < st_off.node_visits, (st_on.node_visits, st_off.node_visits)
    assert 0 < st_on.walk_steps < st_off.walk_steps


@pytest.mark.gpu
@pytest.mark.parametrize("lists", [None, 3])
def test_region_of_the_headline_frame(monkeypatch, scenes, lists):
    """Tiles of the 1920x1080 frame, where a cell's beam is thin and most lists are usable (on the small frames
    above a cell spans a fifth of the view and nearly every random cell overflows): small spheres and ground, the
    horizon, the sky; at capacity 8 (default) and 3 (a mix of listed and overflow cells in one wave's reach)."""
    W, H, spp = 1920, 1080, 8
    tiles = [(800, 600, 64, 16), (1000, 300, 40, 24), (37, 5, 24, 8)]
    off, st_off, on, st_on = _both(monkeypatch, scenes("random"), W, H, spp, tiles=tiles, lists=lists,
                                   flags=hrt.RENDER_COUNT_WORK)
    _same(off, st_off, on, st_on)
    assert st_on.node_visits < st_off.node_visits, (st_on.node_visits, st_off.node_visits)


@pytest.mark.gpu
def test_single_row_tiles(monkeypatch, scenes):
    """Bands one pixel row high: the cells are the frame's, not the call's tiles'."""
    W, H, spp = 64, 36, 8
    s = scenes("random")
    for y in (0, 7, 8, 21, 35):
        _same(*_both(monkeypatch, s, W, H, spp, tiles=[(0, y, W, 1)]))


@pytest.mark.gpu
def test_rank_share_of_split(monkeypatch, scenes):
    """Rank 3 of an 8-way 16-px split."""
    W, H, spp = 64, 36, 8
    tiles = split_tiles(W, H, 8, 3)
    assert tiles
    _same(*_both(monkeypatch, scenes("random"), W, H, spp, tiles=tiles))


@pytest.mark.gpu
def test_capacity_one_overflows_nearly_everywhere(monkeypatch, scenes):
    _same(*_both(monkeypatch, scenes("random"), 64, 36, 8, lists=1))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1])
def test_depth_caps(monkeypatch, scenes, depth):
    off, st_off, on, st_on = _both(monkeypatch, scenes("random"), 64, 36, 8, depth=depth)
    _same(off, st_off, on, st_on)
    assert st_on.segments == (0 if depth == 0 else 64 * 36 * 8)


@pytest.mark.gpu
def test_hybrid_stream_builds_no_lists(monkeypatch, scenes):
    """random_10k's stream exceeds the LDS budget: the same instantiation as without the knob (checked by _both), the
    same frame."""
    _same(*_both(monkeypatch, scenes("random_10k"), 32, 18, 2))
