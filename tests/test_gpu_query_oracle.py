"""hrt_scene_intersect on the GPU against the oracle's recursive world->hit, record by record: the batches and the expected
records of tests/test_query_oracle.py (tests/oracle_queries.py, tests/ray_families.py), computed by the oracle here, and
compared with the device directly - not with the host simulator - word for word.  The one exemption is a float word that
is NaN in the oracle's record, which must be NaN in the device's."""
import numpy as np
import pytest

import hrt
import oracle_queries as OQ
from test_gpu_query import VARIANTS, to_device, to_host

_scenes = {}


@pytest.fixture(scope="module")
def scene(earth):
    """One commit per scene for the whole module."""
    def get(name):
        if name not in _scenes:
            s = OQ.case(name).to_hrt(earth)
            s.commit()
            _scenes[name] = s
        return _scenes[name]

    yield get
    for s in _scenes.values():
        s.close()
    _scenes.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OQ.SCENES))
def test_device_hits_equal_the_oracle(scene, name):
    """Families A to G in one batch (a 64-lane wave holds hits, misses and invalid rays) with the scene in LDS, in global
    memory and under the reference box test: every record is the oracle's."""
    c = OQ.case(name)
    rays, parts = OQ.batch(c)
    want, nan = OQ.expected_hits(c, rays, raw=OQ.raw_batch(c))
    hit = (want["flags"] & hrt.HIT_HIT) != 0
    assert 0.1 < hit.mean() < 0.9 and ((want["flags"] & hrt.HIT_INVALID) != 0).sum() >= 300
    s = scene(name)
    d = to_device(rays)
    for flags in VARIANTS:
        got = to_host(s.intersect(d, flags=flags, seed=OQ.SEED, shutter=c.shutter))
        OQ.report(c, rays, got, want, nan, "%s flags %d" % (name, flags), ids=c.has_ids)
    assert "CULL = 0" in hrt.last_launch()["kernel"]  # the last variant ran the reference test


@pytest.mark.gpu
@pytest.mark.parametrize("name", OQ.MEDIA_SCENES)
def test_device_skip_media_equals_the_oracle_without_media(scene, name):
    c = OQ.case(name)
    rays, _ = OQ.batch(c)
    want, nan = OQ.expected_hits(c, rays, clear=True)
    assert not (want["flags"] & hrt.HIT_MEDIUM).any()
    s = scene(name)
    d = to_device(rays)
    for flags in VARIANTS:
        got = to_host(s.intersect(d, flags=flags | hrt.QUERY_SKIP_MEDIA, seed=OQ.SEED, shutter=c.shutter))
        OQ.report(c, rays, got, want, nan, "%s flags %d" % (name, flags | hrt.QUERY_SKIP_MEDIA))
