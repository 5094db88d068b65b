"""The traversal at the limits its own comments state, against the CPU restatement walking the
exported BVH2, on device 0: scenes scaled across the lean test's 2^40 gate, origins and directions
across lean_ok's bounds, waves that hold lean and exact lanes together, intervals that end on a hit,
non-finite rays, and a render whose camera rays all take the persistent kernels' inline exact walk.

Bar: bit-exact, as in test_gpu_parity.py (whose _check_trace / _check_render do the comparing).
Which path a ray took is read from option ray_steps (0xFFFFFFFF: the exact BVH2 walk) and predicted
by helpers.lean_expected, a restatement of lean_ok.  Every share a test relies on (oracle hits,
continuing pixels) is asserted on the oracle's output, and test_host.py checks the same conditions
without a GPU.
"""
import numpy as np
import pytest

from akari_amd import capi
from helpers import (FAR_CAMERA_SCALE, LEAN_REFUSALS, RAY_STEPS_EXACT, cornell, far_camera_soup, far_origin_rays,
                     interval_variants, lean_expected, near_axis_rays, nonfinite_rays, random_rays, refusal_mask,
                     refuse_lean, scaled_rays, scaled_soup, slot_pixels)
from test_gpu_parity import _check_render, _check_trace, _setup

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
GATE_K = 39           # the largest k whose wide view passes the 2^40 gate (frame origins up to 1.197 * 2^k)


def _hit_share(oh):
    return float((oh["gid"] != MISS).mean())


def _check_routed(ctx, orc, cs, rays, any_hit, exact_walk):
    """Parity with the counting build, and the routing it reports: exactly the rays of the boolean
    array `exact_walk` went through the exact BVH2 walk (exact_cull 0, option ray_steps on)."""
    _, oh = _check_trace(ctx, orc, cs, rays, any_hit, False)
    got = ctx.ray_steps(len(rays)) == RAY_STEPS_EXACT
    bad = np.flatnonzero(got != exact_walk)
    assert len(bad) == 0, f"{len(bad)} rays took the other path, first {bad[:5]} (exact walk: {got[bad[:5]]})"
    return oh


@pytest.mark.parametrize("k", [0, 20, 38, 39, 40])
def test_trace_scaled_scene_across_the_gate(hip_ctx_factory, k):
    """The soup and its rays scaled by 2^k (exact): the oracle's hits are the k = 0 hits scaled, the
    device's must equal them in the product build and in the counting build, closest and any-hit,
    both culls; up to k = 39 every ray stays in the lean loop, at k = 40 (frame origins above 2^40)
    every ray takes the exact walk."""
    rays = scaled_rays(random_rays(1 << 14, 2, -1.2, 1.2), k)
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, scaled_soup(k))
        for steps in (0, 1):
            ctx.set_option("ray_steps", steps)
            for any_hit in (False, True):
                for exact in (False, True):
                    _, oh = _check_trace(ctx, orc, cs, rays, any_hit, exact)
                    assert _hit_share(oh) >= 0.5
                if steps:
                    assert lean_expected(rays).all()
                    _check_routed(ctx, orc, cs, rays, any_hit, np.full(len(rays), k > GATE_K))


@pytest.mark.parametrize("k", [0, 38])
def test_trace_far_origins(hip_ctx_factory, k):
    """Rays aimed at the scene from 2^59 (inside lean_ok's origin bound: the lean loop, its terms near
    2^59 / d) and from 2^61 (past it: the exact walk)."""
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, scaled_soup(k))
        for log2_dist, lean in ((59, True), (61, False)):
            rays = far_origin_rays(k, log2_dist)
            assert lean_expected(rays).all() == lean and lean_expected(rays).any() == lean
            for steps in (0, 1):
                ctx.set_option("ray_steps", steps)
                for any_hit in (False, True):
                    for exact in (False, True):
                        _, oh = _check_trace(ctx, orc, cs, rays, any_hit, exact)
                        assert _hit_share(oh) >= 0.2
                    if steps:
                        _check_routed(ctx, orc, cs, rays, any_hit, np.full(len(rays), not lean))


@pytest.mark.parametrize("e", [-62, -63, -64, -65, -66])
def test_trace_near_axis_directions(hip_ctx_factory, e):
    """One direction component per ray at +-2^e: |1 / d| = 2^-e stays lean up to 2^64 and takes the
    exact walk above it."""
    rays = near_axis_rays(e)
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, scaled_soup(0))
        for steps in (0, 1):
            ctx.set_option("ray_steps", steps)
            for any_hit in (False, True):
                for exact in (False, True):
                    _, oh = _check_trace(ctx, orc, cs, rays, any_hit, exact)
                    assert _hit_share(oh) >= 0.5
                if steps:
                    assert np.array_equal(lean_expected(rays), np.full(len(rays), e >= -64))
                    _check_routed(ctx, orc, cs, rays, any_hit, np.full(len(rays), e < -64))


@pytest.mark.parametrize("config", ["default", "wide0", "lean0"])
@pytest.mark.parametrize("reason", LEAN_REFUSALS)
def test_trace_lean_and_exact_lanes_in_one_wave(hip_ctx_factory, reason, config):
    """Waves that hold lean rays and rays lean_ok refuses (for each of its reasons) together: one
    refused lane in 64, every other lane, all but one, the second half; batches of 1, 63, 64, 65 and
    4096 + 17 rays.  Parity in the product build and the counting build; the counting build marks
    exactly the refused rays and traces every ray once.  With option wide 0 the BVH2 kernel takes all of
    them itself (one ray that could make NaN slabs switches its wave to the reference's ternaries),
    with lean 0 every ray takes the exact walk."""
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, scaled_soup(0))
        if config != "default":
            ctx.set_option("wide" if config == "wide0" else "lean", 0)
        for n in (1, 63, 64, 65, 4096 + 17):
            base = random_rays(n, 7 + n, -1.2, 1.2)
            for pattern in ("1in64", "alternate", "63in64", "half"):
                refused = refusal_mask(n, pattern)
                rays = refuse_lean(base, refused, reason)
                assert np.array_equal(lean_expected(rays), ~refused)
                walk = {"default": refused, "wide0": np.zeros(n, bool), "lean0": np.ones(n, bool)}[config]
                for any_hit in (False, True):
                    ctx.set_option("ray_steps", 0)
                    ctx.set_option("count_tests", 0)
                    _check_trace(ctx, orc, cs, rays, any_hit, False)
                    ctx.set_option("ray_steps", 1)
                    ctx.set_option("count_tests", 1)
                    ctx.reset_stats()
                    _check_routed(ctx, orc, cs, rays, any_hit, walk)
                    assert ctx.trace_counts()["per_mode"]["any" if any_hit else "closest"]["rays"] == n


def _scene_and_rays(name):
    if name == "soup":
        return scaled_soup(0), random_rays(1 << 12, 6, -1.2, 1.2), (0.0, 0.0, 0.0)
    rays = random_rays(1 << 12, 6, -0.9, 0.9)
    rays["o"][:, 1] += 1.0          # the box spans y in [0, 2]
    return cornell((24, 24)), rays, (0.0, 1.0, 0.0)


# the variant on the other side of each interval edge: an end one float inside the hit keeps the answer,
# so what it must differ from is the variant with the end on the hit
_ACROSS = {"tmax=t+": "tmax=t", "tmin=t-": "tmin=t"}


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", ["soup", "cornell"])
def test_trace_intervals_that_end_on_a_hit(hip_ctx_factory, name, exact):
    """The hitting rays of a batch re-traced with tmax and tmin on the oracle's closest hit t* and one
    float to either side of it (t < tmax is carried as t <= float_below(tmax) through the lean test,
    the pop site and the any-hit cull), with tmax at +-0, 2^-149 and 2^-126, and with tmin -0.  The
    oracle defines the answers.  Each edge is crossed: a variant's oracle answers differ for some rays
    from those of the unchanged batch or, for the two variants that keep the hit inside the interval
    (tmax just above t*, tmin just below), from those of the variant with the end on t*."""
    sc, rays, _ = _scene_and_rays(name)
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, sc)
        oh, _, _ = orc.trace(rays, exact_cull=exact)
        hit = oh["gid"] != MISS
        assert hit.mean() >= 0.5
        rays, t_hit = rays[hit], oh["t"][hit]
        variants = interval_variants(rays, t_hit)
        for any_hit in (False, True):
            _, base = _check_trace(ctx, orc, cs, rays, any_hit, exact)
            answers = {}
            for vname, vrays in variants.items():
                _, answers[vname] = _check_trace(ctx, orc, cs, vrays, any_hit, exact)
            for vname, a in answers.items():
                other = answers[_ACROSS[vname]] if vname in _ACROSS else base
                changed = (a["gid"] != other["gid"]) | (a["t"] != other["t"])
                assert changed.any(), f"{vname} (any_hit {any_hit}) changes no answer of the oracle"


@pytest.mark.parametrize("config", ["default", "wide0", "lean0"])
@pytest.mark.parametrize("name", ["soup", "cornell"])
def test_trace_nonfinite_rays(hip_ctx_factory, name, config):
    """Infinite and NaN origins, NaN and infinite interval ends, zero, NaN and infinite directions:
    the library takes them (each goes through a depth-first walk of the finite tree, which visits a
    node at most once whatever its box tests answer), and the reference's algorithm defines the
    result: the oracle's, bit for bit."""
    sc, _, center = _scene_and_rays(name)
    rays = nonfinite_rays(center)
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, sc)
        if config != "default":
            ctx.set_option("wide" if config == "wide0" else "lean", 0)
        for steps in (0, 1):
            ctx.set_option("ray_steps", steps)
            for any_hit in (False, True):
                for exact in (False, True):
                    _, oh = _check_trace(ctx, orc, cs, rays, any_hit, exact)
                    assert (oh["gid"][12:] != MISS).all() and (oh["gid"][:12] == MISS).all()
            if steps and config == "default":
                ctx.set_option("exact_cull", 0)
                ctx.trace(rays)
                assert np.array_equal(ctx.ray_steps(len(rays)) == RAY_STEPS_EXACT, ~lean_expected(rays))


FORMS = {"wavefront": dict(path=0, path_defer=0, path_spec=0), "k_path": dict(path=1, path_defer=0, path_spec=0),
         "k_path_defer": dict(path=1, path_defer=1, path_spec=0), "k_path_spec": dict(path=1, path_defer=0, path_spec=1)}


@pytest.mark.parametrize("form", list(FORMS))
def test_render_camera_rays_take_the_inline_exact_walk(hip_ctx_factory, form):
    """The soup scaled by 2^30 seen from z = 2^61: every camera ray fails lean_ok (the persistent
    kernels' path_begin then runs trace_exact_core inline; the wavefront's k_trace its exact lane)
    while bounce and shadow rays start on the scene and pass it.  Film, weights, final sampler states
    and per-pixel ray counts (counting build) equal the oracle's; a render continued 2 + 2 spp equals
    the 4-spp one."""
    W = H = 24
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, far_camera_soup((W, H)))
        assert abs(cs.camera.position[2]) > 2.0 ** 60 and np.abs(cs.vertices).max() < 2.0 ** (FAR_CAMERA_SCALE + 2)
        for key, v in FORMS[form].items():
            ctx.set_option(key, v)
        ctx.set_option("count_tests", 1)
        rad, w, rays = _check_render(ctx, orc, 4, 5, tiles, W, H, probe=True)
        assert rays and ctx.render_form()["form"] == form
        assert np.isfinite(rad).all() and rad.mean() > 0
        probe = orc.render(4, 5, tiles=tiles, probe=True)[3]
        assert (probe["closest_rays"] > 4).mean() >= 0.4      # the paths go on past their camera rays
        ctx.set_option("count_tests", 0)
        _check_render(ctx, orc, 4, 5, tiles, W, H, probe=True)   # the product build
        ctx.render(2, 5, tiles, W, H)
        rad2, w2 = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == form
        assert np.array_equal(w2, w) and np.array_equal(rad2, rad)
        ys, xs = slot_pixels(tiles, W, H)
        assert np.array_equal(ctx.render_state_export()[0], probe["seed"][ys, xs])
