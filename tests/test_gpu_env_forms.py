"""k_path_defer's and k_path_spec's environment builds (option "env_forms") against the
environment's restatement.

With an environment set, "env_path" 1 and "env_forms" 1 the render form rule decides as it does without an
environment, and k_path_defer_env / k_path_spec_env carry its choice out.  Bar: the one tests/test_gpu_env_path.py
holds k_path_env to.  Film, weight and final sampler state equal tests/golden/env_golden_<scene>.npz bit for bit,
and with the counting build the closest-hit and shadow ray counts per pixel too, whatever table placement, builder,
leaf size, tile list, session split or context split is used; with the option off, or "env_path" off, or without
an environment, every render is the one it was.  Every case is the 24 x 24, 4-spp goldens or smaller.
"""
import subprocess
import sys

import numpy as np
import pytest

from akari_amd import capi, scene
from conftest import GOLDEN, ROOT
from test_path_kat_host import M, check, compare_with_golden, golden

sys.path.insert(0, str(GOLDEN))
import make_env_golden as ME  # noqa: E402
import ref_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = list(ME.CONFIGS)
ON = {"env_path": 1, "env_forms": 1, "path": 1}
FORCE = {"k_path_defer": {"path_defer": 1}, "k_path_spec": {"path_defer": 0, "path_spec": 1}}
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


def planned_form(options, depth):
    """What plan_path() (csrc/path_plan.h) returns for a forced form: k_path_spec when path_spec is 1, else
    k_path_defer when path_defer is 1 and the depth fits its eight shadow slots, else k_path."""
    if options.get("path_spec", 2) == 1:
        return "k_path_spec"
    if options.get("path_defer", 2) == 1 and depth <= 8:
        return "k_path_defer"
    return "k_path"


def expected_shading(name, counting):
    """cornell's tables are constant Diffuse / Emissive; sky and mixed hold Glossy or Mix; the counting builds
    shade with the general build everywhere."""
    return "simple" if name == "cornell" and not counting else "general"


def frame_probe(ctx, W, H):
    return ctx.pixel_probe(W * H).reshape(H, W)


def render_configs(ctx, name, options, what, counting=False, configs=None, form=None):
    """Every configuration of the scene (or `configs` of them) under `options`, which are set here; a
    configuration's select_prob is part of the upload.  `form`: what akr_hip_render_form has to report (default:
    what the plan says for the forced form and the configuration's depth)."""
    g = env_golden(name)
    H, W = g["mask"].shape
    assert not g["mask"].any()
    set_options(ctx, {**options, "pixel_probe": 1, "count_tests": int(counting)})
    try:
        sp_now = None
        for key, sp, depth, clamp in (configs or ME.CONFIGS[name]):
            if sp != sp_now:
                scene.upload_environment(ctx, scene.compile_scene(ME.build_scene(name, select_prob=sp)).environment)
                sp_now = sp
            rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
            rays = compare_with_golden(g, key, g["mask"], rad, w, frame_probe(ctx, W, H), f"{name} {key} {what}")
            want = form or planned_form(options, depth)
            assert ctx.render_form()["form"] == want, (what, key, ctx.render_form())
            if want != "wavefront":
                info = ctx.render_info()
                assert info["shading"] == expected_shading(name, counting), (what, key, info)
                assert info["passes"] == 1
            if counting:
                assert rays, f"{what}: the counting build recorded no ray counts"
            elif want != "wavefront":   # the wavefront's probe counts rays in every build
                assert not rays, f"{what}: the product build recorded ray counts"
    finally:
        set_options(ctx, {"count_tests": 0, "pixel_probe": 0})


# ---- 1. the goldens
@pytest.mark.parametrize("tab", [1, 0])
@pytest.mark.parametrize("form", list(FORCE))
@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden(hip_ctx_factory, name, form, tab):
    options = {**ON, **FORCE[form], "path_tab": tab}
    assert {planned_form(options, c[2]) for c in ME.CONFIGS[name]} == {form}   # no golden depth is above 8 today
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        render_configs(ctx, name, options, f"{form} path_tab {tab}")
        render_configs(ctx, name, options, f"{form} path_tab {tab}, counting build", counting=True)


@pytest.mark.parametrize("form", list(FORCE))
def test_depth_above_eight_takes_the_planned_form(hip_ctx_factory, form):
    """k_path_defer holds eight shadow slots per sample, so at max_depth 9 the plan's forced form is k_path (its
    environment build); k_path_spec has no such limit.  The film has to be the wavefront's at that depth."""
    name = "cornell"
    H, W = env_golden(name)["mask"].shape
    options = {**ON, **FORCE[form]}
    want = planned_form(options, 9)
    assert want == ("k_path" if form == "k_path_defer" else form)
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        set_options(ctx, {"path": 0, "pixel_probe": 1})
        ref = ctx.render(ME.SPP, 9, [(0, 0, W, H)], W, H)
        assert ctx.render_form()["form"] == "wavefront"
        ref_seed = frame_probe(ctx, W, H)["seed"].copy()
        set_options(ctx, options)
        rad, w = ctx.render(ME.SPP, 9, [(0, 0, W, H)], W, H)
        assert ctx.render_form()["form"] == want, ctx.render_form()
        check(rad, ref[0], f"{form} at max_depth 9: radiance")
        check(w, ref[1], f"{form} at max_depth 9: weight")
        assert np.array_equal(frame_probe(ctx, W, H)["seed"], ref_seed)


@pytest.mark.parametrize("name", SCENES)
def test_control_env_forms_off_keeps_k_path(hip_ctx_factory, name):
    """The same options with env_forms 0: only k_path's environment build is taken, as before."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        for form in FORCE:
            render_configs(ctx, name, {**ON, **FORCE[form], "env_forms": 0}, f"{form} forced, env_forms 0", form="k_path",
                           configs=ME.CONFIGS[name][-1:])


# ---- 2. every builder, both leaf sizes
@pytest.mark.parametrize("max_leaf", [1, 4])
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("form", list(FORCE))
@pytest.mark.parametrize("name", SCENES)
def test_builders_and_leaf_sizes_equal_golden(hip_ctx_factory, name, form, builder, max_leaf):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, max_leaf_size=max_leaf, n_threads=16, **BUILDERS[builder])
        render_configs(ctx, name, {**ON, **FORCE[form]}, f"{form} {builder} max_leaf {max_leaf}", configs=ME.CONFIGS[name][-1:])


# ---- 3. small and ragged work: helpers from the first fetch (k_path_spec), idle lanes to hand rays to (k_path_defer)
def check_tiles(ctx, g, key, depth, clamp, tiles, what, counting, form):
    """A tile list of disjoint tiles against the golden's pixels, slot by slot."""
    H, W = g["mask"].shape
    ys = np.concatenate([np.repeat(np.arange(y0, y1), x1 - x0) for x0, y0, x1, y1 in tiles])
    xs = np.concatenate([np.tile(np.arange(x0, x1), y1 - y0) for x0, y0, x1, y1 in tiles])
    ctx.set_option("count_tests", int(counting))
    rad, w = ctx.render(ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
    assert ctx.render_form()["form"] == form, ctx.render_form()
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


@pytest.mark.parametrize("form", list(FORCE))
@pytest.mark.parametrize("name", SCENES)
def test_ragged_and_single_pixel_tiles(hip_ctx_factory, name, form):
    g = env_golden(name)
    key, sp, depth, clamp = ME.CONFIGS[name][-1]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {**ON, **FORCE[form], "pixel_probe": 1})
        for tiles, label in (([(7, 9, 12, 12)], "5 x 3 tile"), ([(11, 13, 12, 14)], "1 x 1 tile")):
            for counting in (0, 1):
                check_tiles(ctx, g, key, depth, clamp, tiles, f"{name} {key} {form} {label} count {counting}", counting, form)


@pytest.mark.parametrize("form", list(FORCE))
def test_waves_that_only_miss(hip_ctx_factory, form):
    """One-pixel tiles of sky pixels whose samples are one camera ray each and no shadow ray: every sample ends
    in the depth-0 miss term after four draws (neither of k_path_spec's guessed lengths), and no lane shades."""
    g = env_golden("sky")
    key, sp, depth, clamp = ME.CONFIGS["sky"][1]
    only = (g[key + "_closest"] == ME.SPP) & (g[key + "_shadow"] == 0)
    ys, xs = np.nonzero(only)
    assert len(ys) >= 32, "the sky golden has too few pixels that only see the sky"
    assert np.any(g[key + "_radiance"][ys, xs] > 0), "the map is black where the camera sees it"
    tiles = [(int(x), int(y), int(x) + 1, int(y) + 1) for y, x in zip(ys[:100], xs[:100])]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "sky", sp)
        set_options(ctx, {**ON, **FORCE[form], "pixel_probe": 1})
        for counting in (0, 1):
            check_tiles(ctx, g, key, depth, clamp, tiles, f"sky {key} {form} miss-only tiles count {counting}", counting, form)


# ---- 4. sessions
SEGMENT = {"k_path_defer": {**ON, **FORCE["k_path_defer"]}, "k_path_spec": {**ON, **FORCE["k_path_spec"]},
           "wavefront": {"env_path": 0, "env_forms": 1, "path": 1, "path_defer": 2, "path_spec": 2},
           "k_path": {"env_path": 1, "env_forms": 0, "path": 1, "path_defer": 2, "path_spec": 2}}
CHAIN = ["k_path_defer", "k_path_spec", "wavefront", "k_path"]


@pytest.mark.parametrize("first,second", list(zip(CHAIN, CHAIN[1:] + CHAIN[:1])))
def test_continue_changes_form_between_segments(hip_ctx_factory, first, second):
    """2 + 2 spp, the form changed between the segments (the options are read at every render and continue)."""
    name, (key, sp, depth, clamp) = "cornell", ME.CONFIGS["cornell"][2]
    g = env_golden(name)
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {**SEGMENT[first], "pixel_probe": 1})
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        assert ctx.render_form()["form"] == first
        set_options(ctx, SEGMENT[second])
        rad, w = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == second
        check(rad, g[key + "_radiance"], f"2 + 2 spp {first} -> {second}: radiance")
        check(w, g[key + "_weight"], f"2 + 2 spp {first} -> {second}: weight")
        assert np.array_equal(frame_probe(ctx, W, H)["seed"], g[key + "_seed"]), "2 + 2 spp: final sampler states"


def test_continue_through_every_form(hip_ctx_factory):
    """1 + 1 + 1 + 1 spp: k_path_defer -> k_path_spec -> wavefront -> k_path, one session."""
    name, (key, sp, depth, clamp) = "sky", ME.CONFIGS["sky"][1]
    g = env_golden(name)
    H, W = g["mask"].shape
    assert ME.SPP == len(CHAIN)
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        ctx.set_option("pixel_probe", 1)
        for k, form in enumerate(CHAIN):
            set_options(ctx, SEGMENT[form])
            rad, w = ctx.render(1, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp) if k == 0 else ctx.render_continue(1, W, H)
            assert ctx.render_form()["form"] == form
        check(rad, g[key + "_radiance"], "1 + 1 + 1 + 1 spp: radiance")
        check(w, g[key + "_weight"], "1 + 1 + 1 + 1 spp: weight")
        assert np.array_equal(frame_probe(ctx, W, H)["seed"], g[key + "_seed"]), "1 + 1 + 1 + 1 spp: final sampler states"


_TWO = {}


def restated_two_spp(name):
    """The restatement's film sums and sampler states after 2 samples of every pixel of the scene's last
    configuration, run once per scene and shared: a slot's samples are one chain, so a slot that holds 2 samples
    equals this whatever its neighbours hold (4 samples: the golden)."""
    if name not in _TWO:
        key, sp, depth, clamp = ME.CONFIGS[name][-1]
        sc = R.RefScene(ME.build_scene(name, select_prob=sp))
        W, H = sc.camera.res
        out, _ = ME.render_pixels(sc, ME.restated_env(name, sp), [(x, y) for y in range(H) for x in range(W)], 2, depth, clamp,
                                  parallel=False)
        assert not out["ambiguous"].any()
        rad, seed = out["radiance"].reshape(H, W, 3), out["seed"].reshape(H, W)
        rad.setflags(write=False)
        seed.setflags(write=False)
        _TWO[name] = (rad, seed)
    return _TWO[name]


@pytest.mark.parametrize("form", list(FORCE))
@pytest.mark.parametrize("name", ["cornell", "sky"])
def test_masked_continue_equals_restatement_per_slot(hip_ctx_factory, name, form):
    """2 spp, then 2 more over every third slot: a subset list fetched by the environment kernel.  Each slot has
    to equal the restatement's render of its own count (2: run here, 4: the golden)."""
    key, sp, depth, clamp = ME.CONFIGS[name][-1]
    g = env_golden(name)
    H, W = g["mask"].shape
    rad2, seed2 = restated_two_spp(name)
    mask = (np.arange(W * H) % 3 == 0).astype(np.uint8)
    four = mask.reshape(H, W) != 0
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {**ON, **FORCE[form], "pixel_probe": 1})
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        assert ctx.render_form()["form"] == form
        rad, w = ctx.render_continue_masked(2, mask, W, H)
        assert ctx.render_form()["form"] == form, ctx.render_form()
        assert np.array_equal(w, np.where(four, 4.0, 2.0).astype(np.float32))
        check(rad, np.where(four[..., None], g[key + "_radiance"], rad2), f"{name} {form} masked continue: radiance per slot count")
        sampler, sfilm = ctx.render_state_export()
        assert np.array_equal(sampler.reshape(H, W), np.where(four, g[key + "_seed"], seed2)), "sampler states per slot count"
        assert np.array_equal(sfilm[:, 3].reshape(H, W), w)
        assert np.array_equal(frame_probe(ctx, W, H)["seed"], sampler.reshape(H, W))
        rad, w = ctx.render_continue_masked(2, 1 - mask, W, H)   # the other slots catch up: the golden everywhere
        assert ctx.render_form()["form"] == form
        check(rad, g[key + "_radiance"], f"{name} {form} second masked continue: radiance")
        assert np.array_equal(frame_probe(ctx, W, H)["seed"], g[key + "_seed"])


@pytest.mark.parametrize("form", list(FORCE))
def test_film_variance_changes_no_bit(hip_ctx_factory, form):
    name = "cornell"
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        ctx.set_option("film_variance", 1)
        render_configs(ctx, name, {**ON, **FORCE[form]}, f"{form} film_variance 1", configs=ME.CONFIGS[name][2:])
        assert ctx.render_variance(24, 24).shape == (24, 24, 4)


# ---- 5. the rule's gated launch of two candidates under an environment
@pytest.mark.parametrize("name", ["cornell", "sky"])
def test_gated_launch(hip_ctx_factory, name):
    """`path` 2 with the pilot on from 4 spp, the order for every form and a tail bar every camera ray clears
    (path_tail_steps 1), as tests/test_gpu_parity.py reaches the rule without an environment: the plan launches
    k_path_env and the tail form's environment kernel behind the device's gate word.  A tree this small is
    cache-resident (tail form k_path_defer); with path_cache_mb 0 it is not (k_path_spec); a bar no ray clears
    leaves k_path."""
    g = env_golden(name)
    H, W = g["mask"].shape
    key, sp, depth, clamp = ME.CONFIGS[name][-1]
    assert depth <= 8
    options = {"env_path": 1, "env_forms": 1, "path": 2, "path_auto_complex": 1, "path_order": 2,
               "path_order_min_spp": ME.SPP, "path_tail_steps": 1, "pixel_probe": 1}
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, options)
        for extra, gate_forms, want in (({}, ("k_path", "k_path_defer"), "k_path_defer"),
                                        ({"path_cache_mb": 0}, ("k_path", "k_path_spec"), "k_path_spec"),
                                        ({"path_tail_steps": 4096}, ("k_path", "k_path_spec"), "k_path")):
            set_options(ctx, extra)
            for counting in (0, 1):
                ctx.set_option("count_tests", counting)
                rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
                what = f"{name} {key} gated {extra} count {counting}"
                rays = compare_with_golden(g, key, g["mask"], rad, w, frame_probe(ctx, W, H), what)
                assert bool(rays) == bool(counting)
                inp = ctx.render_form_inputs()
                # gated: the camera-ray pilot summed its steps for the rule (want_steps) and the tail form is not k_path
                assert inp["pilot_rays"] == W * H and inp["pilot_mean_steps"] is not None, (what, inp)
                form = ctx.render_form()
                assert form["form"] in gate_forms and form["ordered"], (what, form)
                assert form["form"] == want, (what, form, inp)
        ctx.set_option("count_tests", 0)
        ctx.set_option("env_forms", 0)   # the same knobs without the option: one ungated k_path_env launch
        rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        compare_with_golden(g, key, g["mask"], rad, w, frame_probe(ctx, W, H), f"{name} {key} env_forms 0")
        assert ctx.render_form() == {"form": "k_path", "ordered": True}
        assert ctx.render_form_inputs()["pilot_rays"] == -1


# ---- 6. two contexts
def test_two_context_split_with_k_path_spec(hip_ctx_factory):
    name, (key, sp, depth, clamp) = "sky", ME.CONFIGS["sky"][1]
    g = env_golden(name)
    H, W = g["mask"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        for c in (a, b):
            upload(c, name, sp)
            set_options(c, {**ON, **FORCE["k_path_spec"]})
        rad, w = capi.render_node([a, b], ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
        check(rad, g[key + "_radiance"], "two-context render_node radiance")
        check(w, g[key + "_weight"], "two-context render_node weight")
        assert a.render_form()["form"] == "k_path_spec" and b.render_form()["form"] == "k_path_spec"


@pytest.mark.parametrize("form", list(FORCE))
def test_two_contexts_with_different_maps_do_not_cross_talk(hip_ctx_factory, form):
    """Each context's kernel reads its own context's environment record: two scenes with different maps,
    rendered in turn, each equal to its own golden every time."""
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        upload(a, "sky")
        upload(b, "cornell")
        for turn in range(2):
            render_configs(a, "sky", {**ON, **FORCE[form]}, f"{form} sky beside cornell, turn {turn}", configs=ME.CONFIGS["sky"][1:])
            render_configs(b, "cornell", {**ON, **FORCE[form]}, f"{form} cornell beside sky, turn {turn}",
                           configs=ME.CONFIGS["cornell"][2:3])


# ---- 7. off means off
@pytest.mark.parametrize("extra,form", [({}, "k_path"), (FORCE["k_path_defer"], "k_path_defer"), (FORCE["k_path_spec"], "k_path_spec")])
def test_without_an_environment_nothing_changes(hip_ctx_factory, extra, form):
    """env_forms 1 and no environment: the Cornell box of the path loop's restatement, in the form it takes
    without the option."""
    g = golden("cornell")
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, scene.compile_scene(M.build_scene("cornell")))
        set_options(ctx, {**ON, **extra, "pixel_probe": 1})
        for counting in (0, 1):
            ctx.set_option("count_tests", counting)
            for depth, clamp in M.CONFIGS["cornell"]:
                rad, w = ctx.render(M.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
                compare_with_golden(g, M.cfg_key(depth, clamp), g["mask"], rad, w, frame_probe(ctx, W, H),
                                    f"cornell depth {depth} without an environment, env_forms 1, {form}, count {counting}")
                assert ctx.render_form()["form"] == (form if depth <= 8 or form != "k_path_defer" else "k_path")
                assert ctx.render_info()["shading"] == ("general" if counting else "simple")


@pytest.mark.parametrize("name", SCENES)
def test_env_path_off_keeps_the_wavefront(hip_ctx_factory, name):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        for form in FORCE:
            render_configs(ctx, name, {**ON, **FORCE[form], "env_path": 0}, f"env_forms 1, env_path 0, {form} forced",
                           form="wavefront", configs=ME.CONFIGS[name][-1:])


# ---- 8. refusals
def test_refusals_leave_the_context_usable(hip_ctx_factory):
    name, (key, sp, depth, clamp) = "cornell", ME.CONFIGS["cornell"][2]
    g = env_golden(name)
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        set_options(ctx, {**ON, **FORCE["k_path_defer"], "pixel_probe": 1})
        for bad in (2, -1):
            with pytest.raises(capi.AkrError, match=r"env_forms must be in \[0, 1\]"):
                ctx.set_option("env_forms", bad)
            rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)   # still 1: the forced form runs
            assert ctx.render_form()["form"] == "k_path_defer"
            compare_with_golden(g, key, g["mask"], rad, w, frame_probe(ctx, W, H), f"after env_forms {bad} was refused")
        ctx.set_option("env_forms", 0)
        for bad in (2, -1):
            with pytest.raises(capi.AkrError, match=r"env_forms must be in \[0, 1\]"):
                ctx.set_option("env_forms", bad)
            ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)                # still 0
            assert ctx.render_form()["form"] == "k_path"


# ---- 9. the adapter
def test_adapter_set_env_forms(tmp_path):
    exe, lib = tmp_path / "env_forms_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "env_forms_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "on_k_path_defer=1" in r.stdout and "on_k_path_spec=1" in r.stdout and "same=1" in r.stdout
