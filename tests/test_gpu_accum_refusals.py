"""Every refusal of the accumulator's entry points as ONE table: how the accumulator is set up, the call, the status
(include/hrt/hrt.h).  Argument errors win over state errors, so each argument row is made on a full accumulator and on
an empty one; after every call, refused or not, the accumulators it named hold what they held: tile_samples,
feature_samples where kept, and the bytes of resolve("f32") wherever a plain resolve is possible at all.

Shapes: `two_spheres` at 16x16 in four 8x8 tiles, max_depth 4, passes of 2 spp.  A 2-spp pass is one chunk, so two
passes are the two chunks a variance estimate needs (test_setups_hold_what_the_rows_assume)."""
import ctypes

import numpy as np
import pytest

import hrt

W = H = 16
DEPTH, SPP, SEED = 4, 2, 7
FLOOR = 0.05
TILES = hrt.tile_grid(W, H, 8)
OVERLAP = [(0, 0, 12, 16), (8, 0, 8, 16)]
WHOLE = [(0, 0, W, H)]
NAN = float("nan")
OK, ARG, STATE, UNSUP = hrt.OK, hrt.ERR_INVALID_ARG, hrt.ERR_STATE, hrt.ERR_UNSUPPORTED

# name -> (tiles, noise, features, passes, the tiles of every pass (None: all), feature samples, seed, first sample)
SETUPS = {
    "empty": (TILES, False, False, 0, None, False, SEED, 0),
    "empty_nf": (TILES, True, True, 0, None, False, SEED, 0),
    "plain2": (TILES, False, False, 2, None, False, SEED, 0),
    "plain2b": (TILES, False, False, 2, None, False, SEED, 0),       # plain2's samples again
    "seed9": (TILES, False, False, 1, None, False, 9, 100),          # another frame identity, disjoint samples
    "whole": (WHOLE, False, False, 2, None, False, SEED, 100),       # another tile list
    "nonuni": (TILES, False, False, 1, [0], False, SEED, 0),         # tile 0 alone holds samples
    "noise2": (TILES, True, False, 2, None, False, SEED, 0),
    "full": (TILES, True, True, 2, None, True, SEED, 0),
    "no_fsamples": (TILES, True, True, 2, None, False, SEED, 0),
    "one_pass": (TILES, True, True, 1, None, True, SEED, 0),         # one chunk per tile
    "tile0": (TILES, True, True, 2, [0], True, SEED, 0),             # two chunks in tile 0, the others empty
    "overlap": (OVERLAP, True, False, 2, None, False, SEED, 0),
    "overlap_nf": (OVERLAP, True, False, 2, None, False, SEED, 0),   # its first filtered call is noise_filtered
}


class Ctx:
    """The scene, its accumulators, and the buffers the calls write to (no refused call reaches them)."""

    def __init__(self):
        import torch

        self.L = hrt.load()
        self.scene = hrt.preset("two_spheres", 1)
        self.scene.commit()
        self.cam = hrt.preset_camera(self.scene.info, W, H)
        self.d_out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        self.out = np.zeros(W * H * 4, np.float32)
        self.rec = (hrt.TileNoise * 4)()
        self.acc = {}
        for name, (tiles, noise, features, passes, only, fsamples, seed, first) in SETUPS.items():
            a = hrt.Accumulator(self.scene, W, H, tiles, noise=noise, features=features)
            for k in range(passes):
                a.add(self.cam, self.params(first + SPP * k, seed), tiles=only)
            if fsamples:
                a.add_features(self.cam, self.params(0, seed))
            self.acc[name] = a
        self.held = {name: self.fingerprint(a) for name, a in self.acc.items()}

    def params(self, offset=0, seed=SEED, samples=SPP):
        return hrt.params(W, H, samples, DEPTH, seed, tuple(self.scene.info.background), sample_offset=offset)

    @staticmethod
    def fingerprint(a):
        held = a.tile_samples
        return (held, a.feature_samples if a.has_features else None, a.resolve("f32").tobytes() if all(held) else None)

    def close(self):
        for a in self.acc.values():
            a.close()
        self.scene.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def vp(x):
    return ctypes.c_void_p(x.data_ptr())


def fparams(it=3, sigma=4.0):
    return ctypes.byref(hrt.FilterParams(it, sigma))


def gparams(it=3, sigma=4.0, n=0.1, al=0.1, d=0.1):
    return ctypes.byref(hrt.GuidedParams(it, sigma, n, al, d))


def xparams(it=3, sigma=4.0, n=0.1, al=0.1, d=0.1, flags=0, afloor=0.0, reserved=0):
    return ctypes.byref(hrt.GuidedExParams(it, sigma, n, al, d, flags, afloor, reserved))


# the seven filtered entry points as (name, parameter struct, call(ctx, accumulator, params, format))
FILTERED = [
    ("resolve_filtered", fparams, lambda c, a, p, f: c.L.hrt_accum_resolve_filtered(a.h, p, f, vp(c.d_out), None)),
    ("resolve_filtered_host", fparams, lambda c, a, p, f: c.L.hrt_accum_resolve_filtered_host(a.h, p, f, c.out.ctypes.data)),
    ("resolve_guided", gparams, lambda c, a, p, f: c.L.hrt_accum_resolve_guided(a.h, p, f, vp(c.d_out), None)),
    ("resolve_guided_host", gparams, lambda c, a, p, f: c.L.hrt_accum_resolve_guided_host(a.h, p, f, c.out.ctypes.data)),
    ("resolve_guided_ex", xparams, lambda c, a, p, f: c.L.hrt_accum_resolve_guided_ex(a.h, p, f, vp(c.d_out), None)),
    ("resolve_guided_ex_host", xparams, lambda c, a, p, f: c.L.hrt_accum_resolve_guided_ex_host(a.h, p, f, c.out.ctypes.data)),
    ("noise_filtered", xparams,
     lambda c, a, p, f: c.L.hrt_accum_noise_filtered(a.h, p, FLOOR, None, None, ctypes.cast(c.rec, ctypes.c_void_p))),
]
RESOLVES = FILTERED[:6]


def noise_filtered(c, a, p, floor=FLOOR):
    return c.L.hrt_accum_noise_filtered(a.h, p, floor, None, None, ctypes.cast(c.rec, ctypes.c_void_p))


def add_tiles(c, a, idx, offset):
    arr = np.array(idx, np.uint32)
    return c.L.hrt_accum_add_tiles(a.h, ctypes.byref(c.cam), ctypes.byref(c.params(offset)), arr.ctypes.data, arr.size, None, None)


def upload(c, a):
    rng = np.array([200, 202], np.uint32)
    return c.L.hrt_accum_upload(a.h, ctypes.byref(c.cam), ctypes.byref(c.params()), c.out.ctypes.data, rng.ctypes.data, 1)


def download(c, a):
    n = ctypes.c_uint32()
    return c.L.hrt_accum_download(a.h, None, None, 0, ctypes.byref(n))


def restore_own_snapshot(c, a):
    blob = np.frombuffer(a.snapshot(), np.uint8)
    return c.L.hrt_accum_restore(a.h, blob.ctypes.data, blob.size)


ROWS = []   # (id, the accumulators named, call(ctx, *accumulators) -> status, the status)


def row(rid, names, call, status):
    ROWS.append(pytest.param(names.split(), call, status, id=rid))


# ---- formats and parameters: HRT_ERR_INVALID_ARG, on a full accumulator and on an empty one
for acc in ("full", "empty_nf"):
    row(f"format2-resolve-{acc}", acc, lambda c, a: c.L.hrt_accum_resolve(a.h, 2, vp(c.d_out), None), ARG)
    row(f"format2-resolve_host-{acc}", acc, lambda c, a: c.L.hrt_accum_resolve_host(a.h, 2, c.out.ctypes.data), ARG)
    row(f"format2-add_resolve-{acc}", acc,
        lambda c, a: c.L.hrt_accum_add_resolve(a.h, ctypes.byref(c.cam), ctypes.byref(c.params(100)), 2, vp(c.d_out), None, None), ARG)
    for name, mk, call in RESOLVES:
        row(f"format2-{name}-{acc}", acc, lambda c, a, mk=mk, call=call: call(c, a, mk(), 2), ARG)
    for name, mk, call in FILTERED:
        for it in (0, 6):
            row(f"iterations{it}-{name}-{acc}", acc, lambda c, a, mk=mk, call=call, it=it: call(c, a, mk(it=it), 0), ARG)
        for sigma in (0.0, NAN):
            row(f"sigma{sigma}-{name}-{acc}", acc, lambda c, a, mk=mk, call=call, s=sigma: call(c, a, mk(sigma=s), 0), ARG)
    for name, mk, call in FILTERED[2:]:
        for tol in (-1.0, NAN):
            for term in ("n", "al", "d"):
                row(f"tolerance-{term}{tol}-{name}-{acc}", acc,
                    lambda c, a, mk=mk, call=call, kw={term: tol}: call(c, a, mk(**kw), 0), ARG)
    for name, mk, call in FILTERED[4:]:
        row(f"reserved1-{name}-{acc}", acc, lambda c, a, call=call: call(c, a, xparams(reserved=1), 0), ARG)
        row(f"flagbit2-{name}-{acc}", acc, lambda c, a, call=call: call(c, a, xparams(flags=2, afloor=0.01), 0), ARG)
        for afloor in (0.0, NAN):
            row(f"demodulate-floor{afloor}-{name}-{acc}", acc,
                lambda c, a, call=call, fl=afloor: call(c, a, xparams(flags=hrt.GUIDED_DEMODULATE, afloor=fl), 0), ARG)
    row(f"floor0-noise-{acc}", acc, lambda c, a: c.L.hrt_accum_noise(a.h, 0.0, None, None, ctypes.cast(c.rec, ctypes.c_void_p)), ARG)
    row(f"floor0-noise_filtered-{acc}", acc, lambda c, a: noise_filtered(c, a, xparams(), 0.0), ARG)
# the counter-row: without the flag the albedo floor is not read
for name, mk, call in FILTERED[4:]:
    row(f"accepted-floor0-without-the-flag-{name}", "full", lambda c, a, call=call: call(c, a, xparams(afloor=0.0), 0), OK)

# ---- state: HRT_ERR_STATE
row("no-noise-plane-resolve_filtered", "plain2", lambda c, a: FILTERED[1][2](c, a, fparams(), 0), STATE)
row("no-noise-plane-noise", "plain2", lambda c, a: c.L.hrt_accum_noise(a.h, FLOOR, None, None, ctypes.cast(c.rec, ctypes.c_void_p)), STATE)
row("no-noise-plane-noise_filtered", "plain2", lambda c, a: noise_filtered(c, a, xparams(n=0.0, al=0.0, d=0.0)), STATE)
row("no-noise-plane-noise_filtered-guided", "plain2", lambda c, a: noise_filtered(c, a, xparams()), STATE)
for name, mk, call in FILTERED[2:]:
    row(f"no-feature-planes-{name}", "noise2", lambda c, a, mk=mk, call=call: call(c, a, mk(), 0), STATE)
row("no-feature-planes-add_features", "noise2",
    lambda c, a: c.L.hrt_accum_add_features(a.h, ctypes.byref(c.cam), ctypes.byref(c.params()), None), STATE)
row("no-feature-planes-features", "noise2", lambda c, a: c.L.hrt_accum_features(a.h, vp(c.d_out), None, None), STATE)
row("no-feature-planes-features_host", "noise2", lambda c, a: c.L.hrt_accum_features_host(a.h, c.out.ctypes.data, None), STATE)
row("no-feature-planes-feature_samples", "noise2", lambda c, a: c.L.hrt_accum_feature_samples(a.h, ctypes.byref(ctypes.c_uint64())), STATE)
row("no-samples-resolve", "empty", lambda c, a: c.L.hrt_accum_resolve(a.h, 0, vp(c.d_out), None), STATE)
row("no-samples-resolve_host", "empty", lambda c, a: c.L.hrt_accum_resolve_host(a.h, 0, c.out.ctypes.data), STATE)
for name, mk, call in FILTERED:
    row(f"no-samples-{name}", "empty_nf", lambda c, a, mk=mk, call=call: call(c, a, mk(), 0), STATE)
    row(f"one-chunk-{name}", "one_pass", lambda c, a, mk=mk, call=call: call(c, a, mk(), 0), STATE)
    row(f"other-tiles-empty-{name}", "tile0", lambda c, a, mk=mk, call=call: call(c, a, mk(), 0), STATE)
for name, mk, call in FILTERED[2:]:
    row(f"no-feature-samples-{name}", "no_fsamples", lambda c, a, mk=mk, call=call: call(c, a, mk(), 0), STATE)
row("non-uniform-samples", "nonuni", lambda c, a: c.L.hrt_accum_samples(a.h, ctypes.byref(ctypes.c_uint64())), STATE)
row("empty-tile-resolve", "nonuni", lambda c, a: c.L.hrt_accum_resolve(a.h, 0, vp(c.d_out), None), STATE)
row("empty-tile-resolve_host", "nonuni", lambda c, a: c.L.hrt_accum_resolve_host(a.h, 0, c.out.ctypes.data), STATE)
row("restore-into-held-samples", "plain2", restore_own_snapshot, STATE)
# the counter-row: every term off and no flag is the variance-only filter, which asks for no feature planes
row("accepted-noise_filtered-all-terms-off-without-feature-planes", "noise2",
    lambda c, a: noise_filtered(c, a, xparams(n=0.0, al=0.0, d=0.0)), OK)

# ---- unsupported: HRT_ERR_UNSUPPORTED
row("overlap-noise_filtered-before-any-plane", "overlap_nf", lambda c, a: noise_filtered(c, a, xparams(n=0.0, al=0.0, d=0.0)), UNSUP)
row("overlap-noise_filtered-cached", "overlap_nf", lambda c, a: noise_filtered(c, a, xparams(n=0.0, al=0.0, d=0.0)), UNSUP)
row("overlap-resolve_filtered-first", "overlap", lambda c, a: FILTERED[0][2](c, a, fparams(), 0), UNSUP)
row("overlap-resolve_filtered-cached", "overlap", lambda c, a: FILTERED[0][2](c, a, fparams(), 0), UNSUP)
row("overlap-resolve_filtered_host-cached", "overlap", lambda c, a: FILTERED[1][2](c, a, fparams(), 0), UNSUP)
row("non-uniform-add_resolve", "nonuni",
    lambda c, a: c.L.hrt_accum_add_resolve(a.h, ctypes.byref(c.cam), ctypes.byref(c.params(100)), 0, vp(c.d_out), None, None), UNSUP)
row("non-uniform-merge-dst", "nonuni plain2", lambda c, a, b: c.L.hrt_accum_merge(a.h, b.h, None), UNSUP)
row("non-uniform-merge-src", "plain2 nonuni", lambda c, a, b: c.L.hrt_accum_merge(a.h, b.h, None), UNSUP)
row("non-uniform-download", "nonuni", download, UNSUP)
row("non-uniform-upload", "nonuni", upload, UNSUP)
row("noise-plane-upload", "full", upload, UNSUP)
# two faults at once: the non-uniform destination is reported, not the other tile list
row("non-uniform-dst-and-other-tiles-merge", "nonuni whole", lambda c, a, b: c.L.hrt_accum_merge(a.h, b.h, None), UNSUP)

# ---- merges and tile passes: HRT_ERR_INVALID_ARG
for fn in ("hrt_accum_merge", "hrt_accum_merge_tiles"):
    def merge(c, a, b, fn=fn):
        return getattr(c.L, fn)(a.h, b.h, None)

    row(f"{fn}-into-itself", "plain2", lambda c, a, fn=fn: getattr(c.L, fn)(a.h, a.h, None), ARG)
    row(f"{fn}-noise-dst-only", "noise2 plain2", merge, ARG)
    row(f"{fn}-noise-src-only", "plain2 noise2", merge, ARG)
    row(f"{fn}-features-dst-only", "full noise2", merge, ARG)
    row(f"{fn}-features-src-only", "noise2 full", merge, ARG)
    row(f"{fn}-other-tiles", "plain2 whole", merge, ARG)
    row(f"{fn}-overlapping-samples", "plain2 plain2b", merge, ARG)
    row(f"{fn}-another-seed", "plain2 seed9", merge, ARG)
row("hrt_accum_merge_tiles-non-uniform-dst-and-other-tiles", "nonuni whole", lambda c, a, b: c.L.hrt_accum_merge_tiles(a.h, b.h, None), ARG)
row("add_tiles-index-out-of-range", "plain2", lambda c, a: add_tiles(c, a, [4], 100), ARG)
row("add_tiles-index-twice", "plain2", lambda c, a: add_tiles(c, a, [0, 0], 100), ARG)
row("add-overlapping-samples", "plain2", lambda c, a: c.L.hrt_accum_add(a.h, ctypes.byref(c.cam), ctypes.byref(c.params(1)), None, None), ARG)
row("add_tiles-overlapping-samples", "nonuni", lambda c, a: add_tiles(c, a, [0, 1], 1), ARG)


@pytest.mark.gpu
def test_setups_hold_what_the_rows_assume(ctx):
    def chunks(name):
        return [(r.samples, r.chunks) for r in ctx.acc[name].noise(FLOOR)]

    assert chunks("full") == chunks("noise2") == chunks("no_fsamples") == [(2 * SPP, 2)] * 4
    assert chunks("overlap") == chunks("overlap_nf") == [(2 * SPP, 2)] * 2
    assert chunks("one_pass") == [(SPP, 1)] * 4
    assert chunks("tile0") == [(2 * SPP, 2)] + [(0, 0)] * 3
    assert ctx.acc["nonuni"].tile_samples == [SPP, 0, 0, 0] and ctx.acc["plain2"].samples == ctx.acc["plain2b"].samples == 2 * SPP
    assert ctx.acc["full"].feature_samples == ctx.acc["one_pass"].feature_samples == ctx.acc["tile0"].feature_samples == SPP
    assert ctx.acc["no_fsamples"].feature_samples == ctx.acc["empty_nf"].feature_samples == 0
    assert not any(ctx.acc["empty"].tile_samples) and not any(ctx.acc["empty_nf"].tile_samples)
    assert sum(v[2] is not None for v in ctx.held.values()) == len(SETUPS) - 4    # both empty ones, nonuni and tile0 cannot resolve


@pytest.mark.gpu
@pytest.mark.parametrize("names, call, status", ROWS)
def test_refusal(ctx, names, call, status):
    got = call(ctx, *[ctx.acc[n] for n in names])
    assert got == status, (got, ctx.L.hrt_last_error())
    for n in names:
        assert Ctx.fingerprint(ctx.acc[n]) == ctx.held[n], n
