"""hrt_scene_intersect on the host (tests/native/query_sim.hip over csrc/query.h) against the oracle's recursive
world->hit (oracle.cpp oracle_scene_hit), record by record, for the rays a render never produces (tests/ray_families.py)
on description scenes both sides build from the same words (tests/oracle_queries.py).  All twelve words of every record
are compared; the one exemption is a float word that is NaN in the oracle's record, which must be NaN in the library's.
No GPU."""
import numpy as np
import pytest

import hrt
import oracle_queries as OQ
import query_sim as QS

F = np.float32
U = np.uint32


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return QS.build(tmp_path_factory)


def counts(c):
    """What the conditions below are asserted on: the oracle's records alone."""
    f = c.families()
    out = {}
    for k in OQ.FAMILIES:
        rays, raw = f["rays"][k], f["hits"][k]
        ok = OQ.valid(rays, c.shutter)
        hit = ok & (raw["hit"] != 0)
        _, nan = OQ.expected_hits(c, rays, raw=raw)
        out[k] = dict(n=len(rays), invalid=int((~ok).sum()), hit=int(hit.sum()), miss=int((ok & ~hit).sum()),
                      medium=int((hit & (raw["medium"] != 0)).sum()), nan=int(nan.any(axis=1).sum()),
                      nan_t=int((hit & np.isnan(raw["t"])).sum()))
    return out


def interval_outcomes(c):
    """Family F's four copies against the oracle, over the surface hits of family A they were made from: (sources, copies
    1 and 3 that hit at the source's t, copies 2 that miss, copies 4 that miss or hit at a larger t)."""
    f = c.families()
    raw, src = f["hits"]["F"], f["hits"]["A"][f["f_src"]]
    surface = src["medium"] == 0
    t = src["t"]
    hit = raw["hit"] != 0
    at_max = hit[0::4] & (raw["t"][0::4].view(U) == t.view(U))
    below = ~hit[1::4]
    at_min = hit[2::4] & (raw["t"][2::4].view(U) == t.view(U))
    above = ~hit[3::4] | (raw["t"][3::4] > t)
    return int(surface.sum()), int((at_max & surface).sum()), int((below & surface).sum()), int((at_min & surface).sum()), \
        int((above & surface).sum())


@pytest.mark.parametrize("name", list(OQ.SCENES))
def test_hits_equal_the_oracle(sim, name):
    """Every record of families A to G under flags 0 and HRT_QUERY_REFERENCE_CULL is the oracle's.  Conditions, asserted on
    the oracle's records alone: families A, D and E each have at least a tenth hits and a tenth misses; the media scenes
    have at least 20 MEDIUM records in A and in D; NaN records are at most 2% of a family; every invalid ray of family G
    is answered as one.  Measured (hits, misses, invalid, MEDIUM, NaN records) per family, three of the 20 scenes:
      materials_spheres  A 595 1405 0 0 0    B 312 688 0 0 0    C 233 767 0 0 0   D 796 204 0 0 0    E 601 399 0 0 5
                         F 1653 727 0 0 0    G 232 434 334 0 0
      instances_90       A 388 1612 0 0 0    B 206 794 0 0 2    C 147 853 0 0 0   D 685 315 0 0 0    E 448 552 0 0 20
      cornell_smoke      A 1209 791 0 100 0  B 580 420 0 61 15  C 401 599 0 18 0  D 787 213 0 220 0  E 155 845 0 80 0
                         F 2709 2127 0 235 0 G 423 243 334 43 0
    cornell's family B holds 17 NaN records, all NaN-t hits of rays in a wall's plane.  The whole table is in DESIGN.md
    ("Queries against the oracle")."""
    c = OQ.case(name)
    n = counts(c)
    print(name, {k: (v["hit"], v["miss"], v["invalid"], v["medium"], v["nan"]) for k, v in n.items()})
    for k in "ADE":
        assert n[k]["hit"] >= n[k]["n"] // 10 and n[k]["miss"] >= n[k]["n"] // 10, (k, n[k])
    for k in OQ.FAMILIES:
        assert n[k]["nan"] <= n[k]["n"] // 50, (k, n[k])
    if name in OQ.MEDIA_SCENES:
        assert n["A"]["medium"] >= 20 and n["D"]["medium"] >= 20, n
    if name == "cornell":
        assert n["B"]["nan_t"] >= 1, n["B"]
    assert n["G"]["invalid"] == len(c.families()["g_bad"]) and n["F"]["n"] >= 4 * 50
    rays, _ = OQ.batch(c)
    want, nan = OQ.expected_hits(c, rays, raw=OQ.raw_batch(c))
    s = c.to_hrt()
    blob = hrt.scene_blob(s)
    for flags in (0, hrt.QUERY_REFERENCE_CULL):
        got = QS.intersect(sim, s, rays, flags=flags, seed=OQ.SEED, shutter=c.shutter, blob=blob)
        OQ.report(c, rays, got, want, nan, "%s flags %d" % (name, flags), ids=c.has_ids)
    s.close()


@pytest.mark.parametrize("name", list(OQ.SCENES))
def test_interval_ends_against_the_oracle(name):
    """Family F against the oracle alone: of the surface hits of family A at t, t_max = t hits at t, t_max just below t
    misses, t_min = t hits at t, and t_min = nextafter(t, inf) gives a hit at a larger t or a miss (hrt.h "the interval is
    the reference's at both ends").  The two hits hold for every sphere.  A rect lies in the face of its own box - its
    0.0002-thick slab, or a Cuboid's box - whose entry or exit time (aabb.rs: (bound - o) * (1 / d)) can round onto t, and
    aabb.rs's `t_max <= t_min` then culls the box before rect.rs is asked: the reference's own miss, which hrt.h names.
    Measured: all four outcomes on every source in the scenes without rects (materials_spheres 595 of 595, motion 578 of
    578); with rects up to 4% of the t_max = t copies and 1% of the t_min = t copies miss (instances_0: 14 and 2 of 455,
    cornell: 22 and 8 of 1216, media_nested: none of 461).  The bound below is a tenth: the rect must be met within an ulp
    of its box face, which a random ray does rarely."""
    c = OQ.case(name)
    n, at_max, below, at_min, above = interval_outcomes(c)
    print(name, n, at_max, below, at_min, above)
    rects = (c.prims["kind"] == 2).any()
    slack = n // 10 if rects else 0
    assert n >= 50 and below == n and above == n and n - slack <= at_max <= n and n - slack <= at_min <= n


@pytest.mark.parametrize("name", OQ.MEDIA_SCENES)
def test_skip_media_equals_the_oracle_without_media(sim, name):
    """HRT_QUERY_SKIP_MEDIA against an oracle scene built from the same description with its media removed."""
    c = OQ.case(name)
    rays, _ = OQ.batch(c)
    want, nan = OQ.expected_hits(c, rays, clear=True)
    assert not (want["flags"] & hrt.HIT_MEDIUM).any() and ((want["flags"] & hrt.HIT_HIT) != 0).sum() > len(rays) // 10
    s = c.to_hrt()
    for flags in (hrt.QUERY_SKIP_MEDIA, hrt.QUERY_SKIP_MEDIA | hrt.QUERY_REFERENCE_CULL):
        got = QS.intersect(sim, s, rays, flags=flags, seed=OQ.SEED, shutter=c.shutter)
        OQ.report(c, rays, got, want, nan, "%s flags %d" % (name, flags))
    s.close()


@pytest.mark.parametrize("name", ["materials_spheres", "cornell_smoke"])
def test_prim_names_the_descriptions_primitive(name):
    """One scene of each plan: hrt.prim_record(s, prim)[:4] of the index the contract gives a primitive holds that
    primitive's own parameters (a sphere's centre and radius, a moving sphere's first centre and radius, a rect's four
    extents), from the oracle's table of the description's leaves."""
    c = OQ.case(name)
    s = c.to_hrt()
    hrt.scene_blob(s)  # flattens the scene
    for i, p in enumerate(c.prims):
        rec = hrt.prim_record(s, int(c.prim_of[i]))
        k, q = int(p["kind"]), p["p"]
        own = q[:4] if k == 0 else (np.array([q[0], q[1], q[2], q[8]], F) if k == 1 else q[1:5])
        assert np.array_equal(rec[:4].view(U), np.ascontiguousarray(own, F).view(U)), (i, rec[:4], own)
    s.close()
