"""build_walk.hip split_level against the host build and against the restated cut rule (tests/hierarchy.py), and
every builder's hierarchy rendered on the GPU.  tests/test_hierarchy.py is the host half.

- Every row of the input table through hrt_debug_walk_regroup: the device build equals the host's greedy build and
  the restated greedy cuts node for node and box bit for box bit, and is a valid tree.  The rows are chosen for what
  generic scenes never reach: exact cost ties decided by the distance to the middle and by the smaller cut, costs
  that differ by f64 rounding only (a contracted or re-associated sum moves the cut), range lengths at the edges of
  the 256-thread chunks, chains that run one level per leaf, zero-area boxes, and one input above the size from
  which commit uses the device build by default.
- The commit path on scenes of 2, 3, 256, 257 and 513 spheres on a lattice: host and device builds give the same
  stream bytes, and a frame that is the same bits and the oracle's.
- `random` under HRT_WALK_DP = 0, 1, 2, 3 and `random_10k` under 0 and 3 with the default plan: the oracle's frame,
  the same bits whatever the mode, and node visits that differ (different trees were walked).
"""
import hashlib

import numpy as np
import pytest

import hierarchy as Hy
import hrt
import scene_desc
from oracle import oracle as O

TOL = 1e-3  # the project's bar (tests/test_gpu_parity.py)
SEED = 3


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", Hy.ROWS)
def test_device_build_equals_host_build_and_restatement(name, n):
    boxes = Hy.boxes_of(name, n)
    dev = hrt.walk_regroup(boxes, hrt.WALK_DEVICE)
    host = hrt.walk_regroup(boxes, hrt.WALK_GREEDY)
    ref = Hy.greedy_of(name, n)
    Hy.check_tree(boxes, dev)
    diff = np.flatnonzero((dev[0] != host[0]) | (dev[1] != host[1]) | (dev[2] != host[2]))
    assert diff.size == 0, f"first differing node {diff[0]}: device {[int(a[diff[0]]) for a in dev[:3]]}, " \
                           f"host {[int(a[diff[0]]) for a in host[:3]]}"
    assert Hy.same_tree(dev, host)
    assert Hy.same_tree(dev, ref)


# ------------------------------------------------------------------------------------------------ commit path
def _lattice_scene(n):
    """n unit-spaced spheres of radius 0.5 on a lattice (equal boxes at equal spacings: cost ties) under one BvhNode."""
    s = max(1, int(np.ceil(round(n ** (1 / 3), 9))))
    pos = [(float(i % s), float((i // s) % s), float(i // (s * s))) for i in range(n)]
    at = tuple(float(c) for c in (np.max(pos, axis=0) / 2))
    frm = tuple(a + c * (3.0 + 2.0 * s) for a, c in zip(at, (0.55, 0.35, 0.75)))  # the lattice fills the frame
    d = scene_desc.Desc(camera=(frm, at, 40.0, 0.0, 10.0, 0.0, 1.0))
    mats = [d.lambertian(d.solid(0.8, 0.3, 0.3)), d.metal((0.8, 0.8, 0.9), 0.1), d.dielectric(1.5),
            d.lambertian(d.solid(0.2, 0.4, 0.8))]
    objs = [d.sphere(p, 0.5, mats[i % len(mats)]) for i, p in enumerate(pos)]
    d.set_root(d.bvh(objs, 0.0, 1.0))
    return d


def _walk(s):
    buf, info = hrt.scene_blob(s)
    return hashlib.sha256(buf.raw[info.off_walk:info.off_walk + info.walk_bytes]).hexdigest(), info


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 256, 257, 513])
def test_commit_with_the_device_build_on_small_scenes(monkeypatch, n):
    d = _lattice_scene(n)
    w, h, spp = 48, 27, 4
    frames = {}
    for build in ("host", "device"):
        monkeypatch.setenv("HRT_WALK_BUILD", build)
        monkeypatch.setenv("HRT_WALK_DP", "0")  # the host's greedy split, which the device build mirrors
        s = d.to_hrt()
        s.commit()
        monkeypatch.delenv("HRT_WALK_BUILD")
        monkeypatch.delenv("HRT_WALK_DP")
        si = s.scene_info()
        assert si.walk_device_built == (1 if build == "device" else 0) and si.walk_regrouped == 1
        img, st = hrt.render(s, d.hrt_camera(w, h), d.params(w, h, spp, SEED), stats=True)
        frames[build] = (img, int(st.segments), *_walk(s))
        s.close()
    (a, sa, wa, ia), (b, sb, wb, ib) = frames["host"], frames["device"]
    assert ia.walk_bytes == ib.walk_bytes > 0 and wa == wb
    assert ia.walk_hot == ib.walk_hot and ia.walk_c16 == ib.walk_c16 and ia.walk_regrouped == ib.walk_regrouped == 1
    assert sa == sb and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ref, cnt = d.to_oracle().render(w, h, spp, 50, seed=SEED, camera=d.spec())
    linf = float(np.abs(b - ref).max())
    print(f"{n} spheres: segments {sb} (oracle {cnt['segments']}), L-inf {linf:.3g}")
    assert sb == cnt["segments"]
    assert np.isfinite(b).all()
    assert linf <= TOL


# ------------------------------------------------------------------------------------------------ every mode rendered
RENDER = {"random": ("0", "1", "2", "3"), "random_10k": ("0", "3")}
W, H, SPP = 64, 36, 8


@pytest.fixture(scope="module")
def rendered(earth):
    """(scene, HRT_WALK_DP) -> (default-plan frame, its stats, node visits per ray of the counting build's frame),
    (scene, "oracle") -> the oracle's (frame, counters); each rendered once."""
    cache = {}

    def get(name, mode):
        if (name, mode) in cache:
            return cache[(name, mode)]
        if mode == "oracle":
            out = O.OracleScene(hrt.PRESETS[name], 1, earth).render(W, H, SPP, 50, seed=SEED)
        else:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("HRT_WALK_DP", mode)
                mp.setenv("HRT_WALK_DP_SUB", "16")
                s = hrt.preset(name, 1, earth)
                s.commit()
            assert s.scene_info().walk_regrouped == 1 and s.scene_info().walk_device_built == 0
            cam = hrt.preset_camera(s.info, W, H)
            bg = tuple(s.info.background)
            img, st = hrt.render(s, cam, hrt.params(W, H, SPP, 50, SEED, bg), stats=True)
            cimg, cst = hrt.render(s, cam, hrt.params(W, H, SPP, 50, SEED, bg, flags=hrt.RENDER_COUNT_WORK), stats=True)
            assert np.array_equal(img.view(np.uint32), cimg.view(np.uint32)) and cst.segments == st.segments
            s.close()
            out = (img, int(st.segments), cst.node_visits / cst.segments)
        cache[(name, mode)] = out
        return out

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(name, m) for name, modes in RENDER.items() for m in modes])
def test_every_host_builders_hierarchy_renders_the_oracles_frame(rendered, name, mode):
    ref, cnt = rendered(name, "oracle")
    img, seg, visits = rendered(name, mode)
    linf = float(np.abs(img - ref).max())
    print(f"{name} HRT_WALK_DP={mode}: segments {seg} (oracle {cnt['segments']}), L-inf {linf:.3g}, "
          f"node visits per ray {visits:.2f}")
    assert seg == cnt["segments"]
    assert np.isfinite(img).all()
    assert linf <= TOL
    first = rendered(name, RENDER[name][0])
    assert seg == first[1] and np.array_equal(img.view(np.uint32), first[0].view(np.uint32))


@pytest.mark.gpu
def test_walk_dp_modes_walk_different_trees(rendered):
    """Node visits per ray differ between the modes: the knob selected builders, and their trees were walked."""
    r = {m: rendered("random", m)[2] for m in ("0", "1", "2")}
    print("random node visits per ray:", {m: round(v, 3) for m, v in r.items()})
    assert len(set(r.values())) == 3
    assert rendered("random_10k", "0")[2] != rendered("random_10k", "3")[2]
