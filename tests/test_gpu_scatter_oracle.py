"""hrt_scene_scatter and hrt_scene_step on the GPU against the oracle's Material::scatter and world->hit: the batches and
the expected records of tests/test_scatter_oracle.py (tests/oracle_queries.py), computed by the oracle here and compared
with the device directly, word for word."""
import numpy as np
import pytest

import hrt
import oracle_queries as OQ
from test_gpu_step import counter, fresh_hits, list_of, new_list, to_device, to_host

_scenes = {}


@pytest.fixture(scope="module")
def scene():
    """One commit per scene for the whole module."""
    def get(c, key):
        if key not in _scenes:
            s = c.to_hrt()
            s.commit()
            _scenes[key] = s
        return _scenes[key]

    yield get
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def assert_words(got, want, what):
    bad = np.flatnonzero((got != OQ.words(want)).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d records differ, first %s" % (what, len(bad), len(want), bad[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OQ.SCATTER_SCENES))
def test_device_scatter_equals_the_oracle(scene, monkeypatch, name):
    """Scene.scatter with the Perlin tables in LDS (HRT_SCATTER_PERLIN_LDS unset) and in global memory (= 0): all 24 words
    of every ray and path are the oracle's, misses and the rule-2 refusals included."""
    c = OQ.scatter_case(name)
    rays, hits, paths = OQ.scatter_batch(c)
    want_rays, want_paths = OQ.expected_scatter(c, rays, hits, paths, c.background)
    s = scene(c, "scatter:" + name)
    assert s.scene_info().materials == c.n_mats
    d_hits = to_device(hits)
    for knob in (None, "0"):
        if knob is None:
            monkeypatch.delenv("HRT_SCATTER_PERLIN_LDS", raising=False)
        else:
            monkeypatch.setenv("HRT_SCATTER_PERLIN_LDS", knob)
        d_rays, d_paths = to_device(rays), to_device(paths)
        s.scatter(d_rays, d_hits, d_paths, c.background)
        assert_words(to_host(d_rays), want_rays, "%s rays, knob %s" % (name, knob))
        assert_words(to_host(d_paths), want_paths, "%s paths, knob %s" % (name, knob))
        assert np.array_equal(to_host(d_hits), OQ.words(hits))  # read only


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_smoke", "materials_spheres"])
@pytest.mark.parametrize("steps", [1, 2])
def test_device_steps_equal_the_chained_oracle(scene, name, steps):
    """Scene.step with steps = 1 and 2, without and with an out list, against `steps` rounds of oracle hit and oracle
    scatter on family A: rays, paths, the hit of each path's last intersect, the count of valid rays walked, and an out
    list that holds exactly the indices of the expected live paths, as a set."""
    c = OQ.case(name)
    rays0, paths0, want_rays, want_paths, last, last_nan, stepped, walked = OQ.chained(c, steps)
    n = len(rays0)
    want_live = np.flatnonzero((want_paths["flags"] & OQ.DONE) == 0)
    assert len(want_live) >= 20
    s = scene(c, name)
    kw = dict(steps=steps, seed=OQ.SEED, shutter=c.shutter, background=c.background)
    for with_list in (False, True):
        d_rays, d_paths, d_hits, d_walked = to_device(rays0), to_device(paths0), fresh_hits(n), counter()
        out = new_list(n) if with_list else None
        s.step(d_rays, d_paths, hits=d_hits, live_out=out, n_rays=d_walked, **kw)
        what = "%s steps %d list %s" % (name, steps, with_list)
        assert len(OQ.nan_equal(to_host(d_rays), want_rays)) == 0, what
        assert len(OQ.nan_equal(to_host(d_paths), want_paths)) == 0, what
        assert len(OQ.differing(to_host(d_hits)[stepped], last[stepped], last_nan[stepped])) == 0, what
        assert int(d_walked.item()) == walked, what
        if with_list:
            index, count = list_of(out)
            assert count == len(want_live) and np.array_equal(index, want_live), what
