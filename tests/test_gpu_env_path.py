"""k_path's environment build (option "env_path") against the environment's restatement.

With the option on an environment no longer forces the wavefront form: where `path` takes the persistent
kernel, k_path_env / k_path_env_general render the scene.  Bar: bit-exact, as tests/test_gpu_environment.py
holds the wavefront to: film, weight, final sampler state and (counting build) closest-hit and shadow ray counts
equal tests/golden/env_golden_<scene>.npz, whatever table placement, builder, leaf size, fetch order, session
split or context split is used; and with the option off, or without an environment, every render is the one
it was.  Every case is the 24 x 24, 4-spp goldens or smaller.
"""
import subprocess
import sys

import numpy as np
import pytest

from akari_amd import capi, film, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from test_gpu_leaf_one import leaf_counts
from test_gpu_path_kat import probe_frame
from test_path_kat_host import M, check, compare_with_golden, golden

sys.path.insert(0, str(GOLDEN))
import make_env_golden as ME  # noqa: E402
import make_mis_golden as MM  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = list(ME.CONFIGS)
ON = {"env_path": 1, "path": 1}
BUILDERS = {"sah": {}, "sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH)}


def env_golden(name):
    return np.load(GOLDEN / f"env_golden_{name}.npz")


def set_options(ctx, options):
    for k, v in options.items():
        ctx.set_option(k, v)


def upload(ctx, name, select_prob=0.5, **build_kw):
    cs = scene.compile_scene(ME.build_scene(name, select_prob=select_prob))
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def expected_shading(name, counting):
    """cornell's tables are constant Diffuse / Emissive; sky has a Glossy box, mixed Mix and Glossy; the
    counting build shades with the general build everywhere."""
    return "simple" if name == "cornell" and not counting else "general"


def render_and_compare(ctx, name, what, counting=False, form="k_path", exact_cull=False, configs=None):
    """Every configuration of the scene (or `configs` of them); a configuration's select_prob is part of the
    upload.  `form`: what akr_hip_render_form has to report."""
    g = env_golden(name)
    H, W = g["mask"].shape
    assert not g["mask"].any()
    ctx.set_option("pixel_probe", 1)
    ctx.set_option("count_tests", int(counting))
    try:
        sp_now = None
        for key, sp, depth, clamp in (configs or ME.CONFIGS[name]):
            if sp != sp_now:
                scene.upload_environment(ctx, scene.compile_scene(ME.build_scene(name, select_prob=sp)).environment)
                sp_now = sp
            rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp, exact_cull=exact_cull)
            rays = compare_with_golden(g, key, g["mask"], rad, w, probe_frame(ctx, W, H), f"{name} {key} {what}")
            assert ctx.render_form()["form"] == form, (what, key, ctx.render_form())
            if form == "k_path":
                assert ctx.render_info()["shading"] == expected_shading(name, counting), (what, key, ctx.render_info())
                assert ctx.render_info()["passes"] == 1
            if counting:
                assert rays, f"{what}: the counting build recorded no ray counts"
    finally:
        ctx.set_option("count_tests", 0)
        ctx.set_option("pixel_probe", 0)


# ---- 1. the goldens
@pytest.mark.parametrize("tab", [1, 0])
@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden(hip_ctx_factory, name, tab):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, {**ON, "path_tab": tab})
        render_and_compare(ctx, name, f"path_tab {tab}")
        render_and_compare(ctx, name, f"path_tab {tab}, counting build", counting=True)


def test_other_persistent_forms_are_not_consulted(hip_ctx_factory):
    """Only k_path has an environment build: forced k_path_defer / k_path_spec run it all the same."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "cornell")
        for extra in ({"path_defer": 1}, {"path_defer": 0, "path_spec": 1}):
            set_options(ctx, {**ON, **extra})
            render_and_compare(ctx, "cornell", str(extra), configs=ME.CONFIGS["cornell"][2:3])


# ---- 2. both leaf phases, every builder
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SCENES)
def test_builders_and_leaf_sizes_equal_golden(hip_ctx_factory, name, builder, max_leaf):
    """max_leaf_size 1: every leaf holds one triangle, so cornell's product build is k_path_env (simple shading,
    the one-triangle leaf phase); 4: fewer than 97 % do (leaf_layout.h leaf_one_pays), so it is
    k_path_env_general<TAB, true>.  sky and mixed shade with the general build: k_path_env_general<TAB, false>.
    The LBVH builder makes one-triangle leaves whatever max_leaf_size says (lbvh.hip), so both of its trees
    are of the first kind."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, max_leaf_size=max_leaf, n_threads=16, **BUILDERS[builder])
        counts = leaf_counts(ctx.accel_export()[0])
        if max_leaf == 1 or builder == "lbvh":
            assert np.all(counts == 1)
        else:
            assert counts.max() > 1 and np.mean(counts == 1) < 0.97, np.bincount(counts)
        set_options(ctx, ON)
        render_and_compare(ctx, name, f"{builder} max_leaf {max_leaf}")


def test_one_triangle_leaves_with_the_tables_in_memory(hip_ctx_factory):
    """cornell, max_leaf_size 1, path_tab 0: k_path_env<false, false>.  The tests above render that tree with the
    tables in LDS only, and the tables in memory on the default tree (k_path_env_general) only."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "cornell", max_leaf_size=1, n_threads=16)
        assert np.all(leaf_counts(ctx.accel_export()[0]) == 1)
        set_options(ctx, {**ON, "path_tab": 0})
        render_and_compare(ctx, "cornell", "max_leaf 1, path_tab 0", configs=ME.CONFIGS["cornell"][2:3])


# ---- 3. the auto rule
@pytest.mark.parametrize("name", SCENES)
def test_auto_rule(hip_ctx_factory, name):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, {"env_path": 1, "path": 2})
        render_and_compare(ctx, name, "auto, env_path 1", form="k_path" if name == "cornell" else "wavefront")
        ctx.set_option("env_path", 0)
        render_and_compare(ctx, name, "auto, env_path 0", form="wavefront")
        ctx.set_option("path", 1)
        render_and_compare(ctx, name, "path 1, env_path 0", form="wavefront", configs=ME.CONFIGS[name][-1:])


# ---- 4. what still takes the wavefront
@pytest.mark.parametrize("name", SCENES)
def test_exact_cull_keeps_the_wavefront(hip_ctx_factory, name):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, ON)
        render_and_compare(ctx, name, "exact_cull", form="wavefront", exact_cull=True)
        ctx.set_option("wide", 0)
        render_and_compare(ctx, name, "wide 0", form="wavefront", configs=ME.CONFIGS[name][-1:])


def test_mis_keeps_the_wavefront(hip_ctx_factory):
    g = np.load(GOLDEN / "mis_golden_cornell.npz")
    entries = [c for c in MM.CONFIGS["cornell"] if c[1]]
    assert len(entries) >= 3
    for key, _, sp, depth, clamp in entries:
        with hip_ctx_factory(0) as ctx:
            set_options(ctx, {**ON, "mis": 1, "pixel_probe": 1})
            scene.upload_scene(ctx, scene.compile_scene(MM.build_scene("cornell", key, sp)))
            mask = g[key + "_mask"]
            H, W = mask.shape
            rad, w = ctx.render(MM.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
            compare_with_golden(g, key, mask, rad, w, probe_frame(ctx, W, H), f"mis, env_path 1, {key}")
            assert ctx.render_form()["form"] == "wavefront", ctx.render_form()


# ---- 5. the ordered fetch at golden size
@pytest.mark.parametrize("pilot_spp", [0, 2])
@pytest.mark.parametrize("name", SCENES)
def test_ordered_fetch(hip_ctx_factory, name, pilot_spp):
    """4 spp is ranked: by the camera-ray pilot, and by the path pilot, whose counting render is the
    environment kernel's."""
    g = env_golden(name)
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, {**ON, "path_order_min_spp": 1, "path_order_pilot_spp": pilot_spp, "pixel_probe": 1})
        for counting in (0, 1):
            ctx.set_option("count_tests", counting)
            for key, sp, depth, clamp in ME.CONFIGS[name]:
                if sp != 0.5:
                    continue
                rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
                assert ctx.render_form() == {"form": "k_path", "ordered": True}, ctx.render_form()
                rays = compare_with_golden(g, key, g["mask"], rad, w, probe_frame(ctx, W, H),
                                           f"{name} {key} ordered, pilot_spp {pilot_spp}, count {counting}")
                assert bool(rays) == bool(counting)


# ---- 6. waves that are not full, and waves that only miss
def test_sampler_edge_pixels(hip_ctx_factory):
    """env_golden_edges.npz's one-pixel tiles of the 65535 x 65535 camera (su.x exactly select_prob, lu.x or
    lu.y exactly 0): a handful of lanes of one wave, in both builds."""
    torch = pytest.importorskip("torch")
    e = np.load(GOLDEN / "env_golden_edges.npz")
    assert set(e["role"].tolist()) == {"light_select", "env_ux", "env_uy"}
    W, spp, depth = (int(v) for v in e["params"])
    for name in sorted(set(e["scene"].tolist())):
        idx = np.nonzero(e["scene"] == name)[0]
        tiles = [(int(x), int(y), int(x) + 1, int(y) + 1) for x, y in e["xy"][idx]]
        with hip_ctx_factory(0) as ctx:
            scene.upload_scene(ctx, scene.compile_scene(ME.build_scene(name, (W, W))))
            set_options(ctx, {**ON, "pixel_probe": 1})
            for counting in (0, 1):
                ctx.set_option("count_tests", counting)
                rad = torch.zeros(len(idx) * 3, device="cuda:0")
                wt = torch.zeros(len(idx), device="cuda:0")
                assert ctx.render_device(spp, depth, tiles, rad.data_ptr(), wt.data_ptr()) == len(idx)
                ctx.synchronize()
                assert ctx.render_form()["form"] == "k_path", ctx.render_form()
                what = f"{name} pixels {e['role'][idx].tolist()} count {counting}"
                check(rad.cpu().numpy().reshape(-1, 3), e["radiance"][idx], what + " radiance")
                check(wt.cpu().numpy(), e["weight"][idx], what + " weight")
                pr = ctx.pixel_probe(len(idx))
                assert np.array_equal(pr["seed"], e["seed"][idx]), what + " final sampler state"
                if counting:
                    assert np.all(pr["flags"] & capi.PROBE_RAYS)
                    assert np.array_equal(pr["closest_rays"], e["closest"][idx]), what
                    assert np.array_equal(pr["shadow_rays"], e["shadow"][idx]), what


def check_tiles(ctx, g, key, depth, clamp, tiles, what, counting):
    """A tile list of disjoint tiles against the golden's pixels, slot by slot."""
    H, W = g["mask"].shape
    ys = np.concatenate([np.repeat(np.arange(y0, y1), x1 - x0) for x0, y0, x1, y1 in tiles])
    xs = np.concatenate([np.tile(np.arange(x0, x1), y1 - y0) for x0, y0, x1, y1 in tiles])
    ctx.set_option("count_tests", int(counting))
    rad, w = ctx.render(ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
    assert ctx.render_form()["form"] == "k_path", ctx.render_form()
    erad, ew = np.zeros_like(rad), np.zeros_like(w)
    erad[ys, xs], ew[ys, xs] = g[key + "_radiance"][ys, xs], g[key + "_weight"][ys, xs]
    check(rad, erad, what + " radiance")
    check(w, ew, what + " weight")
    pr = ctx.pixel_probe(len(ys))
    assert np.array_equal(pr["seed"], g[key + "_seed"][ys, xs]), what + " final sampler states"
    if counting:
        assert np.all(pr["flags"] & capi.PROBE_RAYS)
        assert np.array_equal(pr["closest_rays"], g[key + "_closest"][ys, xs]), what
        assert np.array_equal(pr["shadow_rays"], g[key + "_shadow"][ys, xs]), what


@pytest.mark.parametrize("name", SCENES)
def test_ragged_tile(hip_ctx_factory, name):
    g = env_golden(name)
    key, sp, depth, clamp = ME.CONFIGS[name][-1]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {**ON, "pixel_probe": 1})
        for counting in (0, 1):
            check_tiles(ctx, g, key, depth, clamp, [(7, 9, 12, 12)], f"{name} {key} 5 x 3 tile count {counting}", counting)


def test_waves_that_only_miss(hip_ctx_factory):
    """One-pixel tiles of sky pixels whose samples are one camera ray each and no shadow ray: every lane's
    every sample ends in the depth-0 miss term, and no lane ever shades."""
    g = env_golden("sky")
    key, sp, depth, clamp = ME.CONFIGS["sky"][1]
    only = (g[key + "_closest"] == ME.SPP) & (g[key + "_shadow"] == 0)
    ys, xs = np.nonzero(only)
    assert len(ys) >= 32, "the sky golden has too few pixels that only see the sky"
    assert np.any(g[key + "_radiance"][ys, xs] > 0), "the map is black where the camera sees it"
    tiles = [(int(x), int(y), int(x) + 1, int(y) + 1) for y, x in zip(ys[:100], xs[:100])]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "sky", sp)
        set_options(ctx, {**ON, "pixel_probe": 1})
        for counting in (0, 1):
            check_tiles(ctx, g, key, depth, clamp, tiles, f"sky {key} miss-only tiles count {counting}", counting)


# ---- 7. sessions
@pytest.mark.parametrize("first", [0, 1])
def test_continue_changes_form_between_segments(hip_ctx_factory, first):
    name, (key, sp, depth, clamp) = "cornell", ME.CONFIGS["cornell"][2]
    g = env_golden(name)
    H, W = g["mask"].shape
    forms = {0: "wavefront", 1: "k_path"}
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {"path": 1, "pixel_probe": 1, "env_path": first})
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        assert ctx.render_form()["form"] == forms[first]
        ctx.set_option("env_path", 1 - first)        # read at every render and continue
        rad, w = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == forms[1 - first]
        check(rad, g[key + "_radiance"], "2 + 2 spp: radiance")
        check(w, g[key + "_weight"], "2 + 2 spp: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g[key + "_seed"]), "2 + 2 spp: final sampler states"


def session_calls(ctx, depth, clamp, W, H, threshold):
    """A masked continue that gives slots different counts, a uniform continue from them, and the stepwise
    adaptive render; what each leaves (film, weight, exported sampler states and film sums, the slots' count
    range), and the form each ran, to be compared between the two forms."""
    n = W * H
    tiles = [(0, 0, W, H)]
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    out, forms = [], []

    def state(rad, w, extra):
        sampler, sfilm = ctx.render_state_export()
        out.append((rad, w, sampler, sfilm, np.array(ctx.render_state_spp_range()), extra))

    def drew():   # the form of the call that just drew samples
        forms.append(ctx.render_form()["form"])

    ctx.render(3, depth, tiles, W, H, ray_clamp=clamp)
    rad, w = ctx.render_continue_masked(5, mask, W, H)
    drew()
    state(rad, w, ctx.pixel_probe(n)["seed"])
    rad, w = ctx.render_continue(2, W, H)
    drew()
    state(rad, w, ctx.pixel_probe(n)["seed"])
    info, more = ctx.adaptive_begin(16, depth, tiles, threshold, min_spp=4, ray_clamp=clamp)
    drew()
    while more:
        err, act = ctx.adaptive_error()
        state(*ctx.render_continue(0, W, H), np.concatenate([err, act.astype(np.float32)]))
        info, more = ctx.adaptive_step()
        drew()
    state(*ctx.render_continue(0, W, H), np.array([info["passes"], info["samples"], info["spp_min"], info["spp_max"]]))
    return out, forms, info


@pytest.mark.parametrize("name", ["cornell", "sky"])
def test_masked_continue_and_adaptive_equal_the_wavefront(hip_ctx_factory, name):
    key, sp, depth, clamp = ME.CONFIGS[name][-1]
    H, W = env_golden(name)["mask"].shape
    got = {}
    threshold = None
    for on in (0, 1):
        with hip_ctx_factory(0) as ctx:
            upload(ctx, name, sp)
            set_options(ctx, {"path": 1, "pixel_probe": 1, "env_path": on})
            if threshold is None:   # the median strip error of the first test (after 4 + 4 samples): about half the strips go on
                ctx.adaptive_begin(16, depth, [(0, 0, W, H)], 0.0, min_spp=4, ray_clamp=clamp)
                ctx.adaptive_step()
                threshold = float(np.median(ctx.adaptive_error()[0]))
                assert threshold > 0
            got[on] = session_calls(ctx, depth, clamp, W, H, threshold)
    assert set(got[0][1]) == {"wavefront"} and set(got[1][1]) == {"k_path"}, (got[0][1], got[1][1])
    info = got[1][2]
    assert info["passes"] >= 2 and info["spp_min"] < info["spp_max"], f"the adaptive case masks nothing: {info}"
    assert len(got[0][0]) == len(got[1][0]) >= 4
    for step, (a, b) in enumerate(zip(got[0][0], got[1][0])):
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"{name}: call {step}, result {k} differs between the forms"


def test_film_variance_changes_no_bit(hip_ctx_factory):
    name = "cornell"
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, {**ON, "film_variance": 1})
        render_and_compare(ctx, name, "film_variance 1", configs=ME.CONFIGS[name][2:])
        assert ctx.render_variance(24, 24).shape == (24, 24, 4)


# ---- 8. two contexts
def test_two_context_split_equals_golden(hip_ctx_factory):
    name, (key, sp, depth, clamp) = "sky", ME.CONFIGS["sky"][1]
    g = env_golden(name)
    H, W = g["mask"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        for c in (a, b):
            upload(c, name, sp)
            set_options(c, ON)
        rad, w = capi.render_node([a, b], ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
        check(rad, g[key + "_radiance"], "two-context render_node radiance")
        check(w, g[key + "_weight"], "two-context render_node weight")
        assert a.render_form()["form"] == "k_path" and b.render_form()["form"] == "k_path"


# ---- 9. clearing
def test_clear_gives_todays_kernel_and_bits(hip_ctx_factory):
    """With the switch still on and the environment removed, the Cornell goldens of the path loop's restatement
    come out of k_path as they always did; a new upload brings the environment kernel back."""
    gp, ge = golden("cornell"), env_golden("cornell")
    H, W = gp["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "cornell")
        set_options(ctx, {**ON, "path_defer": 0, "path_spec": 0})
        render_and_compare(ctx, "cornell", "before the clear", configs=ME.CONFIGS["cornell"][2:3])
        ctx.upload_environment(None)
        ctx.set_option("pixel_probe", 1)
        for counting in (0, 1):
            ctx.set_option("count_tests", counting)
            for depth, clamp in M.CONFIGS["cornell"]:
                rad, w = ctx.render(M.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
                compare_with_golden(gp, M.cfg_key(depth, clamp), gp["mask"], rad, w, probe_frame(ctx, W, H),
                                    f"cornell depth {depth} after the environment was removed, count {counting}")
                assert ctx.render_form()["form"] == "k_path"
                assert ctx.render_info()["shading"] == ("general" if counting else "simple")
        ctx.set_option("count_tests", 0)
        render_and_compare(ctx, "cornell", "after a new upload")
        render_and_compare(ctx, "cornell", "after a new upload, counting build", counting=True,
                           configs=ME.CONFIGS["cornell"][2:3])


# ---- 10. the command line and the adapter
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 4, max_depth: 3, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey, {last}] }} ]
}}
"""


def test_cli_env_path_writes_the_same_file(tmp_path):
    """The CLI has no --path: the scene's shading is constant Diffuse, so the default rule takes k_path with
    --env-path and the wavefront without it (test_auto_rule pins both through the library)."""
    sky = np.zeros((8, 16, 3), np.float32)
    sky[:4] = [0.4, 0.6, 1.0]
    sky[4:] = [0.1, 0.1, 0.1]
    sky[1, 3] = [300.0, 280.0, 250.0]
    film.write_pfm(tmp_path / "sky.pfm", sky, np.ones(sky.shape[:2], np.float32))
    outs = []
    for flags in ([], ["--env-path"], ["--env-path", "--gpus", "2"]):
        out = tmp_path / f"o{len(outs)}.pfm"
        (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH, last="$grey"))
        argv = [str(tmp_path / "s.akari"), "--env", str(tmp_path / "sky.pfm"), "--env-res", "16", *flags]
        if "--gpus" in flags and capi.device_count() < 2:
            continue
        assert render.main(argv) == 0
        outs.append(out.read_bytes())
    assert len(outs) >= 2 and all(o == outs[0] for o in outs[1:])
    from akari_amd import envmap
    img = envmap.read_pfm(tmp_path / "o1.pfm")
    assert img.shape == (24, 40, 3) and np.all(np.isfinite(img)) and img.mean() > 0
    # without an environment the flag is accepted and changes nothing
    plain = []
    for flags in ([], ["--env-path"]):
        out = tmp_path / f"p{len(plain)}.pfm"
        (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH, last="EmissiveMaterial { color: [17, 12, 4] }"))
        assert render.main([str(tmp_path / "s.akari"), *flags]) == 0
        plain.append(out.read_bytes())
    assert plain[0] == plain[1]


def test_adapter_set_env_path(tmp_path):
    exe, lib = tmp_path / "env_path_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "env_path_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "on_k_path=1" in r.stdout and "same=1" in r.stdout
