"""Path stepping on the GPU: step.hip through Scene.step and hrt.trace_paths_fused, the contract of include/hrt/hrt.h
"path stepping".  The device is held to code that is already held to the oracle: the host simulators of
hrt_scene_intersect and hrt_scene_scatter (tests/query_sim.py, tests/scatter_sim.py), whose rounds the fused call must
reproduce word for word - rays, paths, the hits it keeps, the live lists and the ray count - whatever the domain, the
number of steps per call and the A/B knobs.  Every comparison is equality of words."""
import ctypes

import numpy as np
import pytest

import hrt
import query_sim as QS
import scatter_sim as SS

F = np.float32
SEED = 7
SENTINEL = 0x5A5A5A5A  # what an unwritten hit word or list entry holds
# name: (width, height, samples)
SHAPES = {"random": (64, 36, 2), "cornell": (32, 32, 1), "cornell_smoke": (32, 32, 1), "earth": (32, 32, 1),
          "two_perlin_spheres": (50, 37, 2), "smoke72": (72, 72, 1)}
PRESET = {"smoke72": "cornell_smoke"}
DONE = hrt.PATH_DONE

_scenes, _refs = {}, {}


@pytest.fixture(scope="module")
def scene(earth):
    def get(name):
        if name not in _scenes:
            s = hrt.preset(name, 1, earth)
            s.commit()
            _scenes[name] = (s, hrt.scene_blob(s))
        return _scenes[name]

    yield get
    for s, _ in _scenes.values():
        s.close()
    _scenes.clear()
    _refs.clear()


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    return SS.build(tmp_path_factory, lane=False)


class Ref:
    """One input's rounds on the host, computed once per module and never written again: start = the camera paths,
    rounds[i] = (rays, hits, paths) after round i, walked[i] = the valid rays walked up to and including round i."""

    def __init__(self, sims, s, blob, shape, flags=0, max_rounds=None):
        w, h, spp = shape
        self.s, self.blob, self.w, self.h, self.spp = s, blob, w, h, spp
        self.cam = hrt.preset_camera(s.info, w, h)
        self.p = hrt.params(w, h, spp, 50, SEED, tuple(s.info.background))
        self.n_mats = s.scene_info().materials
        self.kw = dict(seed=SEED, shutter=(self.cam.time0, self.cam.time1), background=tuple(self.p.background))
        self.rounds, self.walked = [], []

        def on_round(i, rays, hits, paths):
            for a in (rays, hits, paths):
                a.flags.writeable = False
            self.rounds.append((rays, hits, paths))
            self.walked.append((self.walked[-1] if self.walked else 0) + int(((hits["flags"] & hrt.HIT_INVALID) == 0).sum()))

        self.start = SS.camera_paths(sims, self.cam, self.p)
        if flags == 0 and max_rounds is None:
            _, self.n_rays, _ = SS.loop(sims, s, self.cam, self.p, blob=blob, on_round=on_round, n_mats=self.n_mats)
        else:  # SS.loop's rounds with the query's flags, or only the first few of them
            rays, paths = self.start
            for i in range(max_rounds or 50):
                if (paths["flags"] & DONE).all():
                    break
                hits = QS.intersect(sims.Q, s, rays, flags=flags, seed=SEED, shutter=self.kw["shutter"], blob=blob)
                rays, paths = SS.scatter(sims, blob, rays, hits, paths, self.kw["background"], self.n_mats)
                on_round(i, rays, hits, paths)
            self.n_rays = self.walked[-1]
        for a in self.start:
            a.flags.writeable = False
        self.n = len(self.start[0])

    def paths_before(self, i):
        return self.start[1] if i == 0 else self.rounds[i - 1][2]

    def state(self, k):
        """(rays, paths, walked) after k rounds, k capped at the last round."""
        k = min(k, len(self.rounds))
        return (self.start[0], self.start[1], 0) if k == 0 else (self.rounds[k - 1][0], self.rounds[k - 1][2], self.walked[k - 1])

    def last_hits(self, k0, k1):
        """Word rows of the hit of the last intersect made for each path in rounds [k0, k1), and which paths had one."""
        out = np.full((self.n, 12), SENTINEL, np.uint32)
        k1 = min(k1, len(self.rounds))
        for i in range(k0, k1):
            live = (self.paths_before(i)["flags"] & DONE) == 0
            out[live] = SS.words(self.rounds[i][1])[live]
        return out, ((self.paths_before(k0)["flags"] & DONE) == 0) if k0 < len(self.rounds) else np.zeros(self.n, bool)


def ref_of(sims, scene, name, flags=0, max_rounds=None):
    key = (name, flags, max_rounds)
    if key not in _refs:
        s, blob = scene(PRESET.get(name, name))
        _refs[key] = Ref(sims, s, blob, SHAPES[name], flags, max_rounds)
    return _refs[key]


def to_device(records):
    import torch

    return torch.from_numpy(QS.words(records).view(np.int32).copy()).cuda()


def to_host(tensor):
    import torch

    return tensor.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 12)


def new_list(capacity, entries=None, count=None):
    """An (index, count) pair on the device: `capacity` entries holding SENTINEL, or the given entries and count."""
    import torch

    index = torch.full((capacity,), SENTINEL, dtype=torch.int32, device="cuda")
    if entries is not None:
        index[:len(entries)] = torch.from_numpy(np.asarray(entries, np.uint32).view(np.int32)).cuda()
    n = len(entries) if count is None and entries is not None else (count or 0)
    return index, torch.tensor([n], dtype=torch.int32, device="cuda")


def list_of(pair):
    count = int(pair[1].item())
    return np.sort(pair[0][:count].cpu().numpy().view(np.uint32)), count


def fresh_hits(n):
    import torch

    return torch.full((n, 12), SENTINEL, dtype=torch.int32, device="cuda")


def counter():
    import torch

    return torch.zeros(1, dtype=torch.int64, device="cuda")


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} records differ, first {bad[:8].tolist()}")


# ------------------------------------------------------------------------------------------ 1. round by round
def run_round_by_round(ref):
    s = ref.s
    d_rays, d_paths = hrt.camera_paths(s, ref.cam, ref.p, device=True)
    assert_words(to_host(d_rays), SS.words(ref.start[0]), "camera rays")
    lists = [new_list(ref.n), new_list(ref.n)]
    d_walked = counter()
    live = None
    for i, (rays, hits, paths) in enumerate(ref.rounds):
        d_hits = fresh_hits(ref.n)
        out = lists[i & 1]
        got = s.step(d_rays, d_paths, steps=1, hits=d_hits, live=live, live_out=out, n_rays=d_walked, **ref.kw)
        assert got[0] is d_rays and got[1] is d_paths  # in place
        assert_words(to_host(d_rays), SS.words(rays), f"rays after round {i}")
        assert_words(to_host(d_paths), SS.words(paths), f"paths after round {i}")
        want_hits, _ = ref.last_hits(i, i + 1)
        assert_words(to_host(d_hits), want_hits, f"hits of round {i}")  # the simulator's where live on entry, untouched elsewhere
        index, count = list_of(out)
        want_live = np.flatnonzero((paths["flags"] & DONE) == 0)
        assert count == len(want_live) and np.array_equal(index, want_live), (i, count, len(want_live))
        assert int(d_walked.item()) == ref.walked[i], (i, int(d_walked.item()), ref.walked[i])
        live = out
    final = to_host(d_paths)[:, 11]
    assert (final & DONE).all() and not (final & hrt.PATH_INVALID).any()
    assert int(d_walked.item()) == ref.n_rays and list_of(live)[1] == 0
    assert len(ref.rounds) >= 2 and ref.n_rays > ref.n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "cornell", "cornell_smoke", "earth"])
def test_steps_equal_the_simulator_round_by_round(scene, sims, name):
    """steps = 1 over ping-pong lists: after every round all 48 bytes of every ray and path, the hits of the paths live
    on entry, the out list as a set, its count and the running ray count are the simulator's."""
    run_round_by_round(ref_of(sims, scene, name))
    assert "step_kernel" in hrt.last_launch()["kernel"]


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "0"])
def test_perlin_tables_in_lds_and_in_global_memory_give_the_same_records(scene, sims, monkeypatch, knob):
    if knob is not None:
        monkeypatch.setenv("HRT_SCATTER_PERLIN_LDS", knob)
    run_round_by_round(ref_of(sims, scene, "two_perlin_spheres"))
    info = hrt.last_launch()
    assert "step_kernel" in info["kernel"]
    assert (info["lds_bytes"] >= 12288) == (knob is None)  # the tables are 12 KB each; the two spheres themselves are not


# ------------------------------------------------------------------------------------------ 2. several steps per call
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "cornell_smoke"])
def test_several_steps_per_call(scene, sims, name):
    ref = ref_of(sims, scene, name)
    s = ref.s
    assert len(ref.rounds) > 4
    finished = None
    for steps in (2, 3, 50):
        d_rays, d_paths, d_hits, d_walked = to_device(ref.start[0]), to_device(ref.start[1]), fresh_hits(ref.n), counter()
        out = new_list(ref.n)
        s.step(d_rays, d_paths, steps=steps, hits=d_hits, live_out=out, n_rays=d_walked, **ref.kw)
        rays, paths, walked = ref.state(steps)
        assert_words(to_host(d_rays), SS.words(rays), f"rays after {steps} steps")
        assert_words(to_host(d_paths), SS.words(paths), f"paths after {steps} steps")
        assert_words(to_host(d_hits), ref.last_hits(0, steps)[0], f"last hits of {steps} steps")
        assert int(d_walked.item()) == walked
        index, count = list_of(out)
        assert np.array_equal(index, np.flatnonzero((paths["flags"] & DONE) == 0)) and count == len(index)
        finished = to_host(d_paths)
    assert (finished[:, 11] & DONE).all()
    assert_words(finished, SS.words(ref.rounds[-1][2]), "a finished batch")
    # a mixed schedule over the lists: 1, then 3, then 50
    d_rays, d_paths, d_walked = to_device(ref.start[0]), to_device(ref.start[1]), counter()
    lists, live, done_rounds = [new_list(ref.n), new_list(ref.n)], None, 0
    for call, steps in enumerate((1, 3, 50)):
        d_hits = fresh_hits(ref.n)
        s.step(d_rays, d_paths, steps=steps, hits=d_hits, live=live, live_out=lists[call & 1], n_rays=d_walked, **ref.kw)
        live = lists[call & 1]
        rays, paths, walked = ref.state(done_rounds + steps)
        assert_words(to_host(d_rays), SS.words(rays), f"rays after call {call}")
        assert_words(to_host(d_paths), SS.words(paths), f"paths after call {call}")
        assert_words(to_host(d_hits), ref.last_hits(done_rounds, done_rounds + steps)[0], f"hits of call {call}")
        assert int(d_walked.item()) == walked
        index, count = list_of(live)
        assert np.array_equal(index, np.flatnonzero((paths["flags"] & DONE) == 0)) and count == len(index)
        done_rounds += steps
    assert_words(to_host(d_paths), finished, "the mixed schedule's finished batch")
    assert int(d_walked.item()) == ref.n_rays


# ------------------------------------------------------------------------------------------ 3. against the render
@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 4])
@pytest.mark.parametrize("check_every", [1, 4])
def test_trace_paths_fused_equals_trace_paths_and_the_render(scene, steps, check_every):
    s, _ = scene("random")
    w, h = 64, 36
    cam = hrt.preset_camera(s.info, w, h)
    p = hrt.params(w, h, 2, 50, SEED, tuple(s.info.background))
    radiance, n_rays = hrt.trace_paths_fused(s, cam, p, steps=steps, check_every=check_every)
    want, want_rays = hrt.trace_paths(s, cam, p)
    assert np.array_equal(radiance.view(np.uint32), want.view(np.uint32)) and n_rays == want_rays
    _, st2 = hrt.render(s, cam, p, stats=True)
    assert n_rays == int(st2.segments)
    for k in (0, 1):
        p1 = hrt.params(w, h, 1, 50, SEED, tuple(s.info.background), sample_offset=k)
        rad1, rays1 = hrt.trace_paths_fused(s, cam, p1, steps=steps, check_every=check_every)
        frame, st = hrt.render(s, cam, p1, stats=True)
        got = np.sqrt(rad1.astype(F) * F(1.0)).reshape(h, w, 3)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(frame[..., :3]).view(np.uint32)), k
        assert rays1 == int(st.segments)
        assert np.array_equal(rad1.view(np.uint32), radiance.reshape(h * w, 2, 3)[:, k].view(np.uint32))


# ------------------------------------------------------------------------------------------ 4. domains and guards
def mid_state(ref, k=2):
    """The batch after k rounds: live and finished paths side by side."""
    rays, paths, _ = ref.state(k)
    live = (paths["flags"] & DONE) == 0
    assert 100 < live.sum() < ref.n - 100
    return rays, paths, live


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_tails_and_guard_records(scene, sims, n):
    """n records of a larger batch, without a list and without hits: records [0, n) are the simulator's next round, the
    guard records behind them are untouched."""
    ref = ref_of(sims, scene, "smoke72", max_rounds=3)
    rays, paths, _ = mid_state(ref)
    d_rays, d_paths, d_walked = to_device(rays), to_device(paths), counter()
    out = new_list(ref.n)
    ref.s.step(d_rays[:n], d_paths[:n], steps=1, live_out=(out[0][:n], out[1]), n_rays=d_walked, **ref.kw)
    got_r, got_p = to_host(d_rays), to_host(d_paths)
    want_r, want_h, want_p = ref.rounds[2]
    assert_words(got_r[:n], SS.words(want_r)[:n], "rays [0, n)")
    assert_words(got_p[:n], SS.words(want_p)[:n], "paths [0, n)")
    assert_words(got_r[n:], SS.words(rays)[n:], "guard rays")
    assert_words(got_p[n:], SS.words(paths)[n:], "guard paths")
    index, count = list_of(out)
    assert np.array_equal(index, np.flatnonzero((want_p["flags"][:n] & DONE) == 0)) and count == len(index)
    assert (out[0][count:].cpu().numpy().view(np.uint32) == SENTINEL).all()
    live_in = (paths["flags"][:n] & DONE) == 0
    assert int(d_walked.item()) == int(((want_h["flags"][:n] & hrt.HIT_INVALID) == 0)[live_in].sum())


@pytest.mark.gpu
def test_lists_select_the_domain(scene, sims):
    import torch

    ref = ref_of(sims, scene, "smoke72", max_rounds=3)
    s = ref.s
    rays, paths, live = mid_state(ref)
    want_r, want_h, want_p = (SS.words(a) for a in ref.rounds[2])
    before_r, before_p = SS.words(rays), SS.words(paths)
    live_at, done_at = np.flatnonzero(live), np.flatnonzero(~live)

    def run(entries, n=ref.n, count=None, capacity=None, spare=0):
        d_rays, d_paths, d_hits = to_device(rays), to_device(paths), fresh_hits(ref.n)
        lin = new_list(len(entries) + spare, entries, count)
        if capacity is not None:
            lin = (lin[0][:capacity], lin[1])
        out = new_list(ref.n)
        L = hrt.load()
        sp = hrt.step_params(1, **ref.kw)
        a, b = hrt.PathList(lin[0].data_ptr(), lin[1].data_ptr(), lin[0].numel(), 0), hrt.PathList(out[0].data_ptr(), out[1].data_ptr(), ref.n, 0)
        assert L.hrt_scene_step(s.h, ctypes.byref(sp), d_rays.data_ptr(), d_paths.data_ptr(), n, d_hits.data_ptr(), ctypes.byref(a),
                                ctypes.byref(b), None, None) == hrt.OK
        torch.cuda.synchronize()
        return to_host(d_rays), to_host(d_paths), to_host(d_hits), list_of(out)

    def check(result, stepped, what):
        got_r, got_p, got_h, (index, count) = result
        mask = np.zeros(ref.n, bool)
        mask[stepped] = True
        assert_words(got_r[mask], want_r[mask], what + ": stepped rays")
        assert_words(got_p[mask], want_p[mask], what + ": stepped paths")
        assert_words(got_h[mask], want_h[mask], what + ": stepped hits")
        assert_words(got_r[~mask], before_r[~mask], what + ": other rays")  # all 48 bytes, although many are live
        assert_words(got_p[~mask], before_p[~mask], what + ": other paths")
        assert (got_h[~mask] == SENTINEL).all(), what
        still = np.sort(np.asarray(stepped)[(want_p[stepped, 11] & DONE) == 0]) if len(stepped) else np.zeros(0, np.uint32)
        assert count == len(still) and np.array_equal(index, still), what

    third = live_at[::3]
    check(run(third), third, "every third live index")
    shuffled = np.random.default_rng(5).permutation(live_at)
    check(run(shuffled), live_at, "the live indices in another order")
    # entries past n and entries that are DONE are skipped and absent from out
    n = 4097
    mixed = np.concatenate([live_at[:700], [n, n + 1, ref.n - 1, ref.n + 7, 0xFFFFFFFF], done_at[:300], live_at[700:900]])
    check(run(mixed, n=n), [i for i in np.concatenate([live_at[:700], live_at[700:900]]) if i < n], "entries past n and DONE entries")
    # *d_count beyond the capacity is clamped: the entries behind the capacity are in memory and live, and stay untouched
    check(run(live_at[:500], count=400 + 10**6, capacity=400), live_at[:400], "a count beyond the capacity")
    check(run(live_at[:500], count=77), live_at[:77], "a count below the capacity")
    # an empty list: count 0, no change
    check(run(live_at[:500], count=0), [], "an empty list")
    check(run(np.zeros(0, np.uint32), spare=4), [], "an empty list of capacity 4")


# ------------------------------------------------------------------------------------------ 5. knobs
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["no_lds", "reference_cull", "claim3"])
@pytest.mark.parametrize("name", ["random", "cornell_smoke"])
def test_knobs_give_identical_records(scene, sims, monkeypatch, name, how):
    ref = ref_of(sims, scene, name)
    flags = {"no_lds": hrt.STEP_NO_LDS, "reference_cull": hrt.STEP_REFERENCE_CULL, "claim3": 0}[how]
    if how == "claim3":
        monkeypatch.setenv("HRT_QUERY_CLAIM", "3")
    d_rays, d_paths, d_hits, d_walked = to_device(ref.start[0]), to_device(ref.start[1]), fresh_hits(ref.n), counter()
    out = new_list(ref.n)
    ref.s.step(d_rays, d_paths, steps=3, flags=flags, hits=d_hits, live_out=out, n_rays=d_walked, **ref.kw)
    rays, paths, walked = ref.state(3)
    assert_words(to_host(d_rays), SS.words(rays), how + ": rays")
    assert_words(to_host(d_paths), SS.words(paths), how + ": paths")
    assert_words(to_host(d_hits), ref.last_hits(0, 3)[0], how + ": hits")
    assert int(d_walked.item()) == walked and list_of(out)[1] == int(((paths["flags"] & DONE) == 0).sum())
    info = hrt.last_launch()
    assert "step_kernel" in info["kernel"]
    if how == "no_lds":
        assert info["lds_bytes"] == 0 and info["block"] == 256
    elif how == "reference_cull":
        assert "CULL = 0" in info["kernel"]
    else:
        assert "HRT_QUERY_CLAIM=3" in info["knobs"]


@pytest.mark.gpu
def test_skip_media_equals_the_simulator_with_skip_media(scene, sims):
    ref = ref_of(sims, scene, "cornell_smoke", flags=hrt.QUERY_SKIP_MEDIA, max_rounds=3)
    plain = ref_of(sims, scene, "cornell_smoke")
    assert not np.array_equal(SS.words(ref.rounds[2][2]), SS.words(plain.rounds[2][2]))  # the media matter
    d_rays, d_paths, d_hits = to_device(ref.start[0]), to_device(ref.start[1]), fresh_hits(ref.n)
    ref.s.step(d_rays, d_paths, steps=3, flags=hrt.STEP_SKIP_MEDIA, hits=d_hits, **ref.kw)
    assert_words(to_host(d_rays), SS.words(ref.rounds[2][0]), "rays")
    assert_words(to_host(d_paths), SS.words(ref.rounds[2][2]), "paths")
    assert_words(to_host(d_hits), ref.last_hits(0, 3)[0], "hits")
    assert not (to_host(d_hits)[:, 3] & hrt.HIT_MEDIUM).any()


# ------------------------------------------------------------------------------------------ 6. malformed live records
@pytest.mark.gpu
def test_malformed_live_records(scene, sims):
    ref = ref_of(sims, scene, "random")
    s, blob = ref.s, ref.blob
    rays, paths = ref.start[0].copy(), ref.start[1].copy()
    zero_rng, no_depth, nan_ray = 100, 1001, 2500
    paths["rng"][zero_rng] = 0
    paths["depth_left"][no_depth] = 0
    rays["origin"][nan_ray, 1] = np.nan
    hits = QS.intersect(sims.Q, s, rays, seed=SEED, shutter=ref.kw["shutter"], blob=blob)
    want_r, want_p = SS.scatter(sims, blob, rays, hits, paths, ref.kw["background"], ref.n_mats)
    assert want_p["flags"][zero_rng] == hrt.PATH_INVALID | DONE and want_p["flags"][no_depth] == hrt.PATH_DEPTH | DONE
    assert hits["flags"][nan_ray] == hrt.HIT_INVALID and want_p["flags"][nan_ray] == hrt.PATH_INVALID | DONE
    d_rays, d_paths, d_hits, d_walked = to_device(rays), to_device(paths), fresh_hits(ref.n), counter()
    out = new_list(ref.n)
    s.step(d_rays, d_paths, steps=1, hits=d_hits, live_out=out, n_rays=d_walked, **ref.kw)
    got_p = to_host(d_paths)
    assert got_p[zero_rng, 11] == hrt.PATH_INVALID | DONE and got_p[no_depth, 11] == hrt.PATH_DEPTH | DONE
    assert got_p[nan_ray, 11] == hrt.PATH_INVALID | DONE
    assert_words(to_host(d_rays), SS.words(want_r), "rays")  # the three records and every neighbour
    assert_words(got_p, SS.words(want_p), "paths")
    assert_words(to_host(d_hits), SS.words(hits), "hits")
    assert int(d_walked.item()) == int(((hits["flags"] & hrt.HIT_INVALID) == 0).sum()) == ref.n - 1
    index, count = list_of(out)
    assert np.array_equal(index, np.flatnonzero((want_p["flags"] & DONE) == 0)) and not {zero_rng, no_depth, nan_ray} & set(index.tolist())
    # a second call of many steps ends: the refused records are DONE and stay as they are
    s.step(d_rays, d_paths, steps=50, **ref.kw)
    after = to_host(d_paths)
    assert (after[:, 11] & DONE).all()
    for i in (zero_rng, no_depth, nan_ray):
        assert np.array_equal(after[i], got_p[i])


# ------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.gpu
def test_refusals_change_nothing(scene, sims):
    import torch

    L = hrt.load()
    ref = ref_of(sims, scene, "random")
    s, n = ref.s, ref.n
    d_rays, d_paths, d_hits = to_device(ref.start[0]), to_device(ref.start[1]), fresh_hits(n)
    r, q, hh = d_rays.data_ptr(), d_paths.data_ptr(), d_hits.data_ptr()
    a, b = new_list(n, np.arange(n)), new_list(n)
    d_walked = counter()
    sp = hrt.step_params(1, **ref.kw)
    lin = hrt.PathList(a[0].data_ptr(), a[1].data_ptr(), n, 0)
    lout = hrt.PathList(b[0].data_ptr(), b[1].data_ptr(), n, 0)
    never = hrt.preset("two_spheres", 1)  # not committed
    ref_ = ctypes.byref

    def call(scene_h=s.h, rr=r, pp=q, nn=n, hits=hh, i=lin, o=lout, nr=d_walked.data_ptr()):
        return L.hrt_scene_step(scene_h, ref_(sp), rr, pp, nn, hits, None if i is None else ref_(i), None if o is None else ref_(o), nr, None)

    small = hrt.PathList(b[0].data_ptr(), b[1].data_ptr(), n - 1, 0)
    cases = [(dict(o=small), hrt.ERR_INVALID_ARG, b"smaller"),
             (dict(i=None, o=small), hrt.ERR_INVALID_ARG, b"smaller"),
             (dict(o=hrt.PathList(a[0].data_ptr(), b[1].data_ptr(), n, 0)), hrt.ERR_INVALID_ARG, b"shares a pointer"),
             (dict(o=hrt.PathList(b[0].data_ptr(), a[1].data_ptr(), n, 0)), hrt.ERR_INVALID_ARG, b"shares a pointer"),
             (dict(o=lin), hrt.ERR_INVALID_ARG, b"shares a pointer"),
             (dict(rr=r + 4, nn=n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             (dict(pp=q + 8, nn=n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             (dict(hits=hh + 12, nn=n - 1), hrt.ERR_INVALID_ARG, b"16-byte aligned"),
             (dict(nr=d_walked.data_ptr() + 4), hrt.ERR_INVALID_ARG, b"8-byte aligned"),
             (dict(i=hrt.PathList(a[0].data_ptr() + 2, a[1].data_ptr(), n - 1, 0)), hrt.ERR_INVALID_ARG, b"path list"),
             (dict(scene_h=never.h), hrt.ERR_STATE, b"not committed")]
    for kw, status, text in cases:
        assert call(**kw) == status, text
        assert text in L.hrt_last_error(), (text, L.hrt_last_error())
    torch.cuda.synchronize()
    assert_words(to_host(d_rays), SS.words(ref.start[0]), "rays")
    assert_words(to_host(d_paths), SS.words(ref.start[1]), "paths")
    assert (to_host(d_hits) == SENTINEL).all() and int(d_walked.item()) == 0
    assert list_of(a)[1] == n and (b[0].cpu().numpy().view(np.uint32) == SENTINEL).all()
    # n == 0 is HRT_OK, launches nothing and still zeroes the out count
    b[1].fill_(123)
    assert call(rr=None, pp=None, nn=0, hits=None, i=None) == hrt.OK
    torch.cuda.synchronize()
    assert int(b[1].item()) == 0
    never.close()


# ------------------------------------------------------------------------------------------ 8. the host variant
@pytest.mark.gpu
def test_host_variant_gives_the_device_variants_records(scene, sims):
    ref = ref_of(sims, scene, "cornell_smoke")
    rays, paths = ref.start[0].copy(), ref.start[1].copy()
    hits = np.zeros(ref.n, hrt.HIT_DTYPE)
    walked = np.array([5], np.uint64)
    r1, p1 = ref.s.step(rays, paths, steps=1, hits=hits, n_rays=walked, **ref.kw)
    assert r1 is not rays and p1 is not paths  # new arrays come back, the inputs stay
    assert_words(SS.words(rays), SS.words(ref.start[0]), "input rays")
    assert_words(SS.words(paths), SS.words(ref.start[1]), "input paths")
    assert_words(SS.words(r1), SS.words(ref.rounds[0][0]), "rays")
    assert_words(SS.words(p1), SS.words(ref.rounds[0][2]), "paths")
    assert_words(SS.words(hits), SS.words(ref.rounds[0][1]), "hits")
    assert int(walked[0]) == 5 + ref.walked[0]  # added to
    r2, p2 = ref.s.step(r1, p1, steps=50, **ref.kw)  # ... and without hits or a count, to the end
    assert_words(SS.words(r2), SS.words(ref.rounds[-1][0]), "finished rays")
    assert_words(SS.words(p2), SS.words(ref.rounds[-1][2]), "finished paths")
    d_rays, d_paths = to_device(ref.start[0]), to_device(ref.start[1])
    ref.s.step(d_rays, d_paths, steps=50, **ref.kw)
    assert_words(to_host(d_paths), SS.words(p2), "the device variant's paths")
