"""The sphere kernel's block claim (kernel_common.h claim_blocks) on the GPU.

The wave decodes a claimed 64-item block once and its lanes finish their items from that descriptor.  Small frames
whose tiles have partial 8x8 blocks on both axes, with one chunk and with head + tail chunks, against the CPU
oracle, and every rank's share of a 16-px split (several tiles per call: the stride and the search lookups)
against the same pixels of the one-tile frame.  tests/test_claim_decode.py checks the decode itself for every
item on the host.
"""
import numpy as np
import pytest

import hrt
from hrt.tiling import split_tiles
from oracle import oracle as O

TOL = 1e-3
DEPTH, SEED = 8, 5


@pytest.fixture(scope="module")
def scene(earth):
    s = hrt.preset("random", 1, earth)
    s.commit()
    return s


def _frame(s, W, H, spp):
    cam = hrt.preset_camera(s.info, W, H)
    p = hrt.params(W, H, spp, DEPTH, SEED, tuple(s.info.background))
    img, st = hrt.render(s, cam, p, stats=True)
    return img, st, cam, p


@pytest.fixture(scope="module")
def frames(scene):
    """The one-tile frames the tests share: (W, H, spp) -> (image, stats)."""
    out = {}
    for W, H, spp in ((37, 19, 48), (37, 19, 1), (48, 32, 48)):
        img, st, _, _ = _frame(scene, W, H, spp)
        out[(W, H, spp)] = (img, st)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [48, 1])
def test_partial_blocks_match_oracle(frames, earth, spp):
    """37x19: partial blocks on both axes; 48 spp is 2 head + 8 tail chunks, 1 spp one chunk written straight out."""
    W, H = 37, 19
    img, st = frames[(W, H, spp)]
    ref, cnt = O.OracleScene(hrt.PRESETS["random"], 1, earth).render(W, H, spp, DEPTH, seed=SEED)
    assert st.samples == W * H * spp and st.pixels == W * H, (st.samples, st.pixels)
    assert st.segments == cnt["segments"], (st.segments, cnt["segments"])
    assert (img[..., 3] == 1.0).all()
    linf = float(np.abs(img - ref).max())
    assert linf <= TOL, linf
    assert "launch_basic" in hrt.last_launch()["kernel"]  # the sphere kernel's launcher


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(37, 19), (48, 32)])
def test_split_shares_equal_one_tile_frame(scene, frames, W, H):
    """Each rank's packed share of a 3-way 16-px split, bit for bit the same pixels of the one-tile frame."""
    import torch

    spp = 48
    full, _ = frames[(W, H, spp)]
    cam = hrt.preset_camera(scene.info, W, H)
    p = hrt.params(W, H, spp, DEPTH, SEED, tuple(scene.info.background))
    covered = np.zeros((H, W), bool)
    for rank in range(3):
        tiles = split_tiles(W, H, 3, rank)
        n = sum(t[2] * t[3] for t in tiles)
        d = torch.zeros(n * 4, device="cuda")
        st = hrt.render_tiles_device(scene, cam, p, tiles, d.data_ptr(), 0, want_stats=True)
        assert st.pixels == n and st.samples == n * spp
        flat = d.cpu().numpy()
        off = 0
        for x, y, w, h in tiles:
            blk = flat[off * 4:(off + w * h) * 4].reshape(h, w, 4)
            assert np.array_equal(blk, full[y:y + h, x:x + w]), (rank, x, y)
            covered[y:y + h, x:x + w] = True
            off += w * h
    assert covered.all()


@pytest.mark.gpu
def test_claim_fine_knob_leaves_block_claims_whole(scene, frames, monkeypatch):
    """The sphere kernel claims whole 64-aligned blocks to the end of the frame: HRT_CLAIM_FINE does not apply to
    it (the counter must stay a multiple of 64 for the block decode).  With the knob set to half the items the
    frame is the default frame, and the launch reports the knob."""
    W, H, spp = 37, 19, 48
    full, st0 = frames[(W, H, spp)]
    items = 5 * 3 * 64 * 10  # 5x3 blocks of 64 padded pixels, 10 chunks
    monkeypatch.setenv("HRT_CLAIM_FINE", str(items // 2))
    img, st, _, _ = _frame(scene, W, H, spp)
    assert "HRT_CLAIM_FINE" in hrt.last_launch()["knobs"]
    assert np.array_equal(img, full)
    assert (st.segments, st.samples, st.pixels) == (st0.segments, st0.samples, st0.pixels)
