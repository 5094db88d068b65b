"""The HIP path tracer against the independent restatement's goldens, directly (no oracle).

tests/golden/path_golden_<scene>.npz come from tests/golden/ref_restate.py, a second reading of
the reference source in numpy f32 with a brute-force intersection (no BVH).  Outside the stored
ambiguity mask the device has to give the same bits in radiance and weight, the same final sampler
state per pixel, and (counting build) the same closest-hit and shadow ray counts, in every render
form and under every BVH builder.  NaNs compare equal to NaNs; everything else as u32 patterns.
"""
import numpy as np
import pytest

from akari_amd import capi, scene
from conftest import GOLDEN
from helpers import hits_to_gid
from test_path_kat_host import M, check, check_hits, compare_with_golden, golden

pytestmark = pytest.mark.gpu

# option sets of the render forms
ORDERED = {"path_order": 2, "path_order_min_spp": 0, "path_order_share_min_spp": 0, "path_order_pilot_spp": 2}
FORMS = {
    "wavefront": {"path": 0},
    "k_path_tab0": {"path": 1, "path_defer": 0, "path_spec": 0, "path_tab": 0},
    "k_path_tab1": {"path": 1, "path_defer": 0, "path_spec": 0, "path_tab": 1},
    "k_path_defer": {"path": 1, "path_defer": 1, "path_spec": 0},
    "k_path_spec": {"path": 1, "path_defer": 0, "path_spec": 1},
    "k_path_ordered": {"path": 1, "path_defer": 0, "path_spec": 0, **ORDERED},
}
# what ctx.render_form() must report after a render with those options
FORM_RAN = {"wavefront": "wavefront", "k_path_tab0": "k_path", "k_path_tab1": "k_path", "k_path_defer": "k_path_defer",
            "k_path_spec": "k_path_spec", "k_path_ordered": "k_path"}


def upload(ctx, name, resolution=None, **build_kw):
    sc = M.build_scene(name, resolution)
    cs = scene.compile_scene(sc)
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def probe_frame(ctx, W, H):
    """The last render's per-slot probe of a whole-frame tile as a [H, W] array."""
    return ctx.pixel_probe(W * H).reshape(H, W)


def render_and_compare(ctx, name, form, counting):
    g = golden(name)
    H, W = g["mask"].shape
    ctx.set_option("pixel_probe", 1)
    ctx.set_option("count_tests", int(counting))
    try:
        for depth, clamp in M.CONFIGS[name]:
            rad, w = ctx.render(M.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
            rays = compare_with_golden(g, M.cfg_key(depth, clamp), g["mask"], rad, w, probe_frame(ctx, W, H),
                                       f"{name} depth {depth} clamp {clamp} {form}")
            if counting and form != "wavefront":
                assert rays, f"{form}: the counting build recorded no ray counts"
    finally:
        ctx.set_option("count_tests", 0)
        ctx.set_option("pixel_probe", 0)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_render_forms_equal_golden(hip_ctx_factory, name, form):
    """Every depth and clamp of the scene in one render form: film, weights and sampler states from
    the product kernels, then again with the counting build for the per-pixel ray counts."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        for k, v in FORMS[form].items():
            ctx.set_option(k, v)
        render_and_compare(ctx, name, form, counting=False)
        ran = ctx.render_form()
        assert ran["form"] == FORM_RAN[form] and ran["ordered"] == (form == "k_path_ordered"), ran
        render_and_compare(ctx, name, form, counting=True)


BUILDERS = {
    "sah_leaf1": dict(max_leaf_size=1), "sah_leaf8": dict(max_leaf_size=8),
    "sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH),
}


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_builders_equal_golden(hip_ctx_factory, name, builder):
    """The golden is builder-free (brute-force intersection): every builder's tree gives its bits."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, **BUILDERS[builder])
        render_and_compare(ctx, name, builder, counting=False)


@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_trace_of_stored_camera_rays(hip_ctx_factory, name):
    g = golden(name)
    H, W = g["mask"].shape
    rays = np.zeros(H * W, capi.RAY_DTYPE)
    rays["o"], rays["d"] = g["ray_o"].reshape(-1, 3), g["ray_d"].reshape(-1, 3)
    rays["tmin"], rays["tmax"] = np.float32(0.001), np.inf
    with hip_ctx_factory(0) as ctx:
        cs = upload(ctx, name)
        hits = ctx.trace(rays)
        check_hits(hits_to_gid(hits, cs.mesh_base), hits["t"], hits["u"], hits["v"], g, ~g["mask"].reshape(-1))


def test_sampler_extreme_pixels(hip_ctx_factory):
    """Pixels of a 65535 x 65535 camera whose sampler seed x + y * W makes one draw exactly 0.0 or
    1.0 in a chosen role (light selection, light sample, GGX u.x), or lands the Mix draw exactly on
    the fraction; each as a one-pixel tile into packed device buffers (nothing is sized by the
    frame).  Film, weight, final sampler state and, with the counting build, ray counts."""
    torch = pytest.importorskip("torch")
    e = np.load(GOLDEN / "path_golden_edges.npz")
    W, spp, depth = (int(v) for v in e["params"])
    for name in sorted(set(e["scene"].tolist())):
        idx = np.nonzero(e["scene"] == name)[0]
        tiles = [(int(x), int(y), int(x) + 1, int(y) + 1) for x, y in e["xy"][idx]]
        with hip_ctx_factory(0) as ctx:
            upload(ctx, name, (W, W))
            ctx.set_option("pixel_probe", 1)
            for counting in (0, 1):
                ctx.set_option("count_tests", counting)
                rad = torch.zeros(len(idx) * 3, device="cuda:0")
                wt = torch.zeros(len(idx), device="cuda:0")
                n = ctx.render_device(spp, depth, tiles, rad.data_ptr(), wt.data_ptr())
                ctx.synchronize()
                assert n == len(idx)
                what = f"{name} pixels {e['role'][idx].tolist()}"
                check(rad.cpu().numpy().reshape(-1, 3), e["radiance"][idx], what + " radiance")
                check(wt.cpu().numpy(), e["weight"][idx], what + " weight")
                pr = ctx.pixel_probe(len(idx))
                assert np.array_equal(pr["seed"], e["seed"][idx]), what + " final sampler state"
                if counting:
                    assert np.all(pr["flags"] & capi.PROBE_RAYS)
                    assert np.array_equal(pr["closest_rays"], e["closest"][idx]), what
                    assert np.array_equal(pr["shadow_rays"], e["shadow"][idx]), what
            ctx.set_option("count_tests", 0)
