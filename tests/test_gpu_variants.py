"""Every kernel variant an option selects gives the reference's bits, on device 0.

options.h says of its A/B knobs that they change the schedule, the grid or the kernel build and never
a result; bench.py exposes some of them.  Traces under each traversal variant are compared with the
oracle (test_gpu_parity._check_trace); renders are compared with the oracle once, at the defaults, and
then byte for byte (film, weights, pixel probe) with that render, one knob changed at a time, in the
wavefront form and in each persistent form.  A knob value its table row allows must be accepted, and a
hang-guard report fails the test like any other error of the render.
"""
import numpy as np
import pytest

from akari_amd import capi
from helpers import (chain_axis_rays, chain_rays, chain_scene, cornell, edge_rays, random_rays, scaled_soup, slot_pixels,
                     small_soup)
from test_gpu_parity import _check_render, _check_trace, _setup

pytestmark = pytest.mark.gpu

# (options set before the tree is built, options set after): the selectable traversal kernels and grids
TRACE_VARIANTS = {
    "wide0": ({}, {"wide": 0}),
    "lean0": ({}, {"lean": 0}),
    "rays_per_lane7": ({}, {"rays_per_lane": 7}),
    "rays_per_lane64": ({}, {"rays_per_lane": 64}),
    "leaf_align8_wide0": ({"leaf_align": 8}, {"wide": 0}),
}


def _trace_inputs(name):
    """(scene, build options, ray batches)"""
    if name == "soup":
        return scaled_soup(0), {}, [random_rays(1 << 14, 2, -1.2, 1.2), edge_rays()]
    if name == "cornell":
        rays = random_rays(1 << 12, 1, -0.9, 0.9)
        rays["o"][:, 1] += 1.0          # the box spans y in [0, 2]
        return cornell((24, 24)), {}, [rays, edge_rays((0.0, 1.0, 0.0))]
    return chain_scene(65), dict(builder=capi.BUILDER_LBVH), [chain_rays(), chain_axis_rays(), edge_rays()]   # the deep stack


@pytest.mark.parametrize("variant", list(TRACE_VARIANTS))
@pytest.mark.parametrize("name", ["soup", "cornell", "chain"])
def test_trace_variants(hip_ctx_factory, name, variant):
    """Closest-hit and any-hit traces, both culls, under each traversal variant: the BVH2 kernels
    (wide 0, with packed and with 128-B-aligned leaf records), the tight wide kernel with every ray on
    the exact walk (lean 0), and grids of 7 and 64 queued rays per lane."""
    sc, build_kw, batches = _trace_inputs(name)
    before, after = TRACE_VARIANTS[variant]
    with hip_ctx_factory(0) as ctx:
        for key, v in before.items():
            ctx.set_option(key, v)
        cs, orc = _setup(ctx, sc, **build_kw)
        for key, v in after.items():
            ctx.set_option(key, v)
        hits = 0
        for rays in batches:
            for any_hit in (False, True):
                for exact in (False, True):
                    _, oh = _check_trace(ctx, orc, cs, rays, any_hit, exact)
                    hits += int(np.count_nonzero(oh["gid"] != 0xFFFFFFFF))
        assert hits > 0


FORMS = {"wavefront": dict(path=0, path_defer=0, path_spec=0), "k_path": dict(path=1, path_defer=0, path_spec=0),
         "k_path_defer": dict(path=1, path_defer=1, path_spec=0), "k_path_spec": dict(path=1, path_defer=0, path_spec=1)}
PERSISTENT = ("k_path", "k_path_defer", "k_path_spec")

# option -> (default, values): one knob changed at a time
WAVEFRONT_KNOBS = {"any_far_first": (0, [1]), "shadow_grid_pct": (75, [1, 50]), "rays_per_lane": (1, [64]),
                   "serial_shadow": (0, [1])}
PERSISTENT_KNOBS = {"any_far_first": (0, [1]), "path_min_wait": (0, [1, 64]), "path_grid_pct": (100, [1]),
                    "path_prio": (0, [128, 256])}
ORDER_KNOBS = {"path_order_sub": (0, [3, 5]), "path_order_classes": (16, [1, 32]), "path_order_cap": (64, [0, 1]),
               "path_order_shift": (2, [0, 31])}

SPP, DEPTH = 4, 5


def _render_scene(name):
    return (cornell((32, 32)), 32, 32) if name == "cornell" else (small_soup(20_000, (96, 54)), 96, 54)


def _render(ctx, tiles, W, H):
    """(film, weights, probe bytes) of a render with the probe on; any error of the render, a
    hang-guard report included, raises."""
    ctx.set_option("pixel_probe", 1)
    rad, w = ctx.render(SPP, DEPTH, tiles, W, H)
    ctx.set_option("pixel_probe", 0)
    return rad, w, ctx.pixel_probe(len(slot_pixels(tiles, W, H)[0]))


def _same(got, want, what):
    for a, b, part in zip(got, want, ("film", "weights", "probe")):
        assert a.tobytes() == b.tobytes(), f"{what}: the {part} differs from the default render's"


@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_render_variants_wavefront(hip_ctx_factory, name):
    """The wavefront form: the default render equals the oracle (film, weights, sampler states, ray
    counts); with wide 0 or lean 0 the library's own choice of form is the wavefront and the bytes are
    the same; so are they under any_far_first, the shadow grid's size, rays_per_lane, serial_shadow, and
    the camera-ray queue's cost order on and off."""
    sc, W, H = _render_scene(name)
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, sc)
        ctx.set_option("path", 0)
        *_, rays = _check_render(ctx, orc, SPP, DEPTH, tiles, W, H, probe=True)
        assert rays and ctx.render_form()["form"] == "wavefront"
        base = _render(ctx, tiles, W, H)
        ctx.set_option("path", 2)
        for key in ("wide", "lean"):
            ctx.set_option(key, 0)
            _same(_render(ctx, tiles, W, H), base, f"{key} 0")
            assert ctx.render_form()["form"] == "wavefront"
            ctx.set_option(key, 1)
        ctx.set_option("path", 0)
        for key, (default, values) in WAVEFRONT_KNOBS.items():
            for v in values:
                ctx.set_option(key, v)
                _same(_render(ctx, tiles, W, H), base, f"{key} {v}")
            ctx.set_option(key, default)
        ctx.set_option("path_order_min_spp", 0)       # the cost order at every spp
        ctx.set_option("path_order_share_min_spp", 0)
        for v in (1, 0):
            ctx.set_option("wave_order", v)
            _same(_render(ctx, tiles, W, H), base, f"wave_order {v}")
            assert ctx.render_form() == {"form": "wavefront", "ordered": bool(v)}


@pytest.mark.parametrize("form", PERSISTENT)
@pytest.mark.parametrize("name", ["cornell", "soup"])
def test_render_variants_persistent(hip_ctx_factory, name, form):
    """Each persistent form: the default render equals the oracle, and the bytes stay the same under
    any_far_first, the ends of path_min_wait, path_grid_pct and path_prio, the speculation depth, and
    the ends of the cost order's sub-sampling, class count, step cap and class shift (the order forced
    on at every spp, and seen to be on)."""
    sc, W, H = _render_scene(name)
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        cs, orc = _setup(ctx, sc)
        for key, v in FORMS[form].items():
            ctx.set_option(key, v)
        _check_render(ctx, orc, SPP, DEPTH, tiles, W, H, probe=True)
        assert ctx.render_form() == {"form": form, "ordered": False}
        base = _render(ctx, tiles, W, H)
        knobs = dict(PERSISTENT_KNOBS)
        if form == "k_path_spec":
            knobs["path_spec_depth"] = (3, [1, 2])
        for key, (default, values) in knobs.items():
            for v in values:
                ctx.set_option(key, v)
                _same(_render(ctx, tiles, W, H), base, f"{form} {key} {v}")
                assert ctx.render_form()["form"] == form
            ctx.set_option(key, default)
        ctx.set_option("path_order_min_spp", 0)
        ctx.set_option("path_order_share_min_spp", 0)
        for key, (default, values) in ORDER_KNOBS.items():
            for v in values:
                ctx.set_option(key, v)
                _same(_render(ctx, tiles, W, H), base, f"{form} {key} {v}")
                assert ctx.render_form() == {"form": form, "ordered": True}
            ctx.set_option(key, default)
