"""k_path's bounded pop and fit-tested push ("bounded pop") against the oracle.

Bar: bit-exact.  A lane whose pop is cut short pops the same stack entries in the same order one
iteration later, against a best that can only have shrunk, and the push writes the same entries to
the same rows whichever of its two forms an iteration takes: radiance, weights and the per-pixel
probe (final sampler state, and the ray counts in the counting build) must equal the oracle's for
every setting of path_pop_rounds / path_pop_keep.

Scenes (96x54, 4 spp, max_depth 5, SBVH, leaf size 1, forced to k_path):
  deep  the soup of helpers.small_soup, a deep tree of small triangles, at 200,000 triangles.  Chosen
        size: at 20,000 and 60,000 triangles no or two iterations of the 4-spp render push with a lane at
        sp >= 12 (push_slow 0 and 2), at 200,000 triangles 22 do, and all of them fit in LDS.
  thick the 20,000-triangle soup with ten times the triangle radius (0.1): the same count, but boxes that
        overlap, so 1.4 % of the push iterations have a lane at sp >= 12 and a few rays overflow.
  wide  4,000 triangles of radius 0.5 in the same cube: every node overlaps most others, a ray enters
        nearly every slot it tests and its stack runs past the 15 LDS rows into the global overflow
        area (deep_rays > 0 below), the path of test_gpu_c3.test_c3_deep_stack_overflow_path at a
        size the oracle renders in seconds.
"""
import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from helpers import check_probe, small_soup

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 96, 54, 4, 5
TILES = [(0, 0, W, H)]
# (path_pop_rounds, path_pop_keep): stack_pop's behaviour, one round for everyone, one round with every
# straggler deferred (the hardest case), and a mixed setting
SETTINGS = [(255, 1), (1, 1), (1, 64), (2, 4)]
K_PATH = dict(path=1, path_defer=0, path_spec=0, path_order=0)


def _make(hip_ctx_factory, sc):
    ctx = hip_ctx_factory(0)
    cs = scene.compile_scene(sc)
    scene.upload_scene(ctx, cs, builder=capi.BUILDER_SBVH, max_leaf_size=1, n_threads=16)
    nodes, tris = ctx.accel_export()
    orc = py_oracle.OracleScene(cs, nodes, tris, capi)
    orad, ow, _, oprobe = orc.render(SPP, DEPTH, tiles=TILES, n_threads=16, probe=True)
    for k, v in K_PATH.items():
        ctx.set_option(k, v)
    ctx.set_option("pixel_probe", 1)
    return ctx, (orad, ow, oprobe)


@pytest.fixture(scope="module", params=["deep", "thick"])
def deep(hip_ctx_factory, request):
    sc = small_soup(200_000, (W, H)) if request.param == "deep" else small_soup(20_000, (W, H), r=0.1)
    ctx, ref = _make(hip_ctx_factory, sc)
    yield ctx, ref
    ctx.close()


@pytest.fixture(scope="module")
def wide(hip_ctx_factory):
    ctx, ref = _make(hip_ctx_factory, small_soup(4_000, (W, H), r=0.5))
    yield ctx, ref
    ctx.close()


def _render_check(ctx, ref, rounds, keep, count=0):
    orad, ow, oprobe = ref
    what = f"pop_rounds {rounds} pop_keep {keep}{' (counting build)' if count else ''}"
    ctx.set_option("path_pop_rounds", rounds)
    ctx.set_option("path_pop_keep", keep)
    ctx.set_option("count_tests", count)
    ctx.reset_stats()
    try:
        rad, w = ctx.render(SPP, DEPTH, TILES, W, H)
        assert ctx.render_form()["form"] == "k_path"
        assert np.array_equal(w, ow), f"{what}: weights differ"
        assert np.array_equal(rad, orad), f"{what}: radiance differs (max abs diff {np.abs(rad - orad).max()})"
        counted = check_probe(ctx.pixel_probe(W * H), oprobe, TILES, W, H, what)
        assert counted == bool(count)
        return rad, w, ctx.path_profile(), ctx.trace_counts()
    finally:
        ctx.set_option("count_tests", 0)


def test_render_equal_among_pop_settings(deep):
    """Radiance, weights and probe: bit for bit the oracle's, so equal among the four settings."""
    ctx, ref = deep
    out = [_render_check(ctx, ref, r, k)[:2] for r, k in SETTINGS]
    for rad, w in out[1:]:
        assert rad.tobytes() == out[0][0].tobytes() and w.tobytes() == out[0][1].tobytes()
    assert out[0][0].mean() > 0


def test_stack_depth_exercises_pop_and_push(deep):
    """The counting build on the same scene: the pop site really runs more rounds than iterations, some
    pushes happen with fewer than four free LDS rows, and some of those fit all the same (they take the
    straight-line push now); with every straggler deferred the wave runs one round per pop iteration."""
    ctx, ref = deep
    _, _, pp, _ = _render_check(ctx, ref, 255, 1, count=1)
    print({k: pp[k] for k in ("trav_iters", "pop_iters", "pop_rounds", "pop_lane_rounds", "pop_lanes", "push_iters",
                              "push_slow", "push_would_fit")})
    assert pp["push_slow"] > 0 and pp["push_would_fit"] > 0
    assert pp["pop_lane_rounds"] > pp["pop_iters"]
    assert pp["pop_rounds"] > pp["pop_iters"] > 0
    assert pp["push_iters"] >= pp["push_slow"] >= pp["push_would_fit"]
    _, _, pd, _ = _render_check(ctx, ref, 1, 64, count=1)
    assert pd["pop_rounds"] == pd["pop_iters"] > 0            # one round per iteration with a pop
    # (the entries popped are not compared: when a wave's leaf phases fall changes with the setting, and with
    # it how far every lane of the wave walks on an older best; the hits do not depend on that)
    assert pd["pop_lane_rounds"] > 0


@pytest.mark.parametrize("rounds,keep", [(1, 64), (2, 4)])
def test_overflow_stack_with_deferred_pop(wide, rounds, keep):
    """Stacks past the LDS rows (the global overflow area) with the deferred pop on: bit-exact."""
    ctx, ref = wide
    _, _, pp, counts = _render_check(ctx, ref, rounds, keep, count=1)
    deep_rays = sum(counts["per_mode"][m]["deep_rays"] for m in ("closest", "shadow"))
    print(f"deep-stack rays {deep_rays}, push_slow {pp['push_slow']}, would fit {pp['push_would_fit']}")
    assert deep_rays > 0, "no ray reached the overflow stack"
    assert pp["push_slow"] > pp["push_would_fit"]   # some pushes really left LDS
    _render_check(ctx, ref, rounds, keep)
