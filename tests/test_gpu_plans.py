"""Every row of tests/plans.py on the GPU: one parametrised test per row (-m gpu).

Every row: the launch record holds the row's substrings, pixel and sample counts are exact, every pixel is finite; and
the row rendered once more with HRT_RENDER_COUNT_WORK gives the same bits and segment / sample / pixel counts through
the COUNT = true instantiation, with node visits and primitive tests counted.
- "exact" rows: the oracle's segment count, L-inf <= 1e-3, and the bits of the default plan's frame (the scene
  committed and rendered with no knob and no flag, same camera and parameters).
- "slab" rows (HRT_RENDER_FAST_CULL): CULL = 1 in the record; bits and segments of the default plan's frame, on the
  inputs tests/test_plans.py qualified on the host lanes.
- "sah" rows (HRT_RENDER_FAST_CULL | HRT_RENDER_SAH): FAST = true, sah_stream_len > 0, the slab frame's bits on
  every unambiguous pixel (the oracle's BvhNode frame equal to its brute-force List frame), L-inf <= 1e-3 against the
  oracle over the whole frame.  No tolerance on the unambiguous pixels.
Each scene and set of commit knobs is committed once, each default frame and oracle frame rendered once.
"""
import contextlib
import os

import numpy as np
import pytest

import hrt
import plans as P
from test_plans import unambiguous_mask

TOL = 1e-3
LINF = {}  # family -> the largest L-inf against the oracle seen (printed when the module's scenes are closed)


@contextlib.contextmanager
def knobs(pairs):
    old = {k: os.environ.get(k) for k, _ in pairs}
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Bench:
    """The module's caches: scene sources, committed scenes, default frames, oracle frames, slab frames, masks."""

    def __init__(self, earth):
        self.earth = earth
        self.src, self.scenes, self.defaults, self.oracles, self.slabs, self.masks = {}, {}, {}, {}, {}, {}

    def source(self, name):
        if name not in self.src:
            self.src[name] = P.Source(name, self.earth)
        return self.src[name]

    def committed(self, name, commit=()):
        key = (name, tuple(commit))
        if key not in self.scenes:
            with knobs(commit):
                s = self.source(name).build()
                s.commit()
            self.scenes[key] = s
        return self.scenes[key]

    def render(self, name, size, seed, shutter=None, flags=0, commit=(), launch=()):
        w, h, spp = size
        src, s = self.source(name), self.committed(name, commit)
        cam = hrt.camera(*src.spec(s, shutter), w, h)
        p = hrt.params(w, h, spp, 50, seed, src.background(s), flags=flags)
        with knobs(launch):
            try:
                img, st = hrt.render(s, cam, p, stats=True)
            except hrt.HrtError as e:
                if e.status == hrt.ERR_HIP:  # a device error: nothing more is launched on this GPU by this session
                    pytest.exit(f"{name} flags {flags} commit {commit} launch {launch}: {e}", returncode=3)
                raise
            rec = hrt.last_launch()
        return img, st, rec

    def default(self, name, size, seed, shutter):
        key = (name, size, seed, shutter)
        if key not in self.defaults:
            img, st, rec = self.render(name, size, seed, shutter)
            assert rec["knobs"] == "", rec["knobs"]  # the default plan: no knob in the environment
            self.defaults[key] = (img, st)
        return self.defaults[key]

    def oracle(self, name, size, seed, shutter):
        key = (name, size, seed, shutter)
        if key not in self.oracles:
            w, h, spp = size
            src = self.source(name)
            self.oracles[key] = src.oracle().render(w, h, spp, 50, seed=seed, threads=16,
                                                    camera=src.spec(self.committed(name), shutter))
        return self.oracles[key]

    def slab(self, name, size, seed):
        key = (name, size, seed)
        if key not in self.slabs:
            img, st, rec = self.render(name, size, seed, flags=hrt.RENDER_FAST_CULL)
            assert "CULL = 1" in rec["kernel"], rec["kernel"]
            self.slabs[key] = (img, st)
        return self.slabs[key]

    def mask(self, name, size, seed):
        key = (name, size, seed)
        if key not in self.masks:
            self.masks[key] = unambiguous_mask(self.source(name), size, seed)
        return self.masks[key]

    def close(self):
        print("largest L-inf against the oracle per family:", {f: f"{v:.3g}" for f, v in LINF.items()})
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def bench(earth):
    b = Bench(earth)
    yield b
    b.close()


def _bits(a):
    return a.view(np.uint32)


def _counts(st):
    return int(st.segments), int(st.samples), int(st.pixels)


def _check_record(row, kernel, count):
    for sub in P.expected(row) + [f"COUNT = {'true' if count else 'false'}"]:
        if sub.startswith("!"):
            assert sub[1:] not in kernel, (row.id, sub, kernel)
        elif sub.endswith("["):
            assert kernel.startswith(sub), (row.id, sub, kernel)
        else:
            assert sub in kernel, (row.id, sub, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("row", P.ROWS, ids=[r.id for r in P.ROWS])
def test_row(bench, row):
    w, h, spp = row.size
    args = dict(shutter=row.shutter, commit=row.commit, launch=row.launch)
    img, st, rec = bench.render(row.scene, row.size, row.seed, flags=row.flags, **args)
    _check_record(row, rec["kernel"], False)
    assert st.pixels == w * h and st.samples == w * h * spp
    assert np.isfinite(img).all()

    # the instrumented build of the same instantiation renders the same frame
    cimg, cst, crec = bench.render(row.scene, row.size, row.seed, flags=row.flags | hrt.RENDER_COUNT_WORK, **args)
    _check_record(row, crec["kernel"], True)
    assert _counts(cst) == _counts(st), (row.id, _counts(cst), _counts(st))
    assert np.array_equal(_bits(cimg), _bits(img)), row.id
    assert cst.node_visits > 0 and cst.prim_tests > 0, (row.id, cst.node_visits, cst.prim_tests)

    ref, cnt = bench.oracle(row.scene, row.size, row.seed, row.shutter)
    linf = float(np.abs(img - ref).max())
    fam = P.family(row)
    LINF[fam] = max(LINF.get(fam, 0.0), linf)
    print(f"{row.id}: {rec['kernel']}; segments {st.segments} (oracle {cnt['segments']}), L-inf {linf:.3g}")
    dimg, dst = bench.default(row.scene, row.size, row.seed, row.shutter)
    if row.kind == "exact":
        assert st.segments == cnt["segments"], (row.id, st.segments, cnt["segments"])
        assert linf <= TOL, (row.id, linf)
        assert _counts(st) == _counts(dst), row.id
        assert np.array_equal(_bits(img), _bits(dimg)), row.id
    elif row.kind == "slab":
        assert "CULL = 1" in rec["kernel"], rec["kernel"]
        assert _counts(st) == _counts(dst), (row.id, _counts(st), _counts(dst))
        assert np.array_equal(_bits(img), _bits(dimg)), row.id
    else:
        assert "FAST = true" in rec["kernel"], rec["kernel"]
        assert bench.committed(row.scene, row.commit).scene_info().sah_stream_len > 0
        mask = bench.mask(row.scene, row.size, row.seed)
        assert int(mask.sum()) == row.unambiguous
        simg, _ = bench.slab(row.scene, row.size, row.seed)
        differ = mask & np.any(_bits(img) != _bits(simg), axis=2)
        assert not differ.any(), (row.id, np.argwhere(differ)[:8].tolist())  # (y, x) of unambiguous pixels that differ
        assert linf <= TOL, (row.id, linf)
