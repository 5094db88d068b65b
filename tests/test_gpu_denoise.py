"""Feature buffers and the a-trous filter of the film on device 0.

The feature pass is compared with feature_reference (py_oracle.camera_ray + OracleScene.trace + f32
NumPy) and the filter with denoise_reference, both restated in test_denoise_host.py; every comparison is
array_equal.  A slot's record depends on its pixel alone (its chain is seeded x + y * width), so the
reference is computed once per (scene, cull, spp) over the whole frame and gathered for any tile list."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, denoise, film as film_io, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell, mixed_scene, slot_pixels, small_soup, textured_scene
from test_denoise_host import SDL, denoise_reference, feature_reference, frame_features

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 70, 45      # neither a multiple of 64 nor of 4; the stride-16 taps are partly inside, partly clipped
FULL = [(0, 0, W, H)]
RAGGED = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 64, 64), (5, 5, 5, 9), (60, 30, 100, 100)]   # overlapping, clipped, empty
DEPTH = 5
SCENES = {
    "cornell": lambda: cornell((W, H)),
    "mixed_scene": lambda: mixed_scene((W, H)),
    "textured_scene": lambda: textured_scene((W, H)),
    "small_soup": lambda: small_soup(resolution=(W, H)),
}
_REF = {}   # (scene, exact_cull, spp) -> whole-frame packed records [H * W, 12], read-only


def _upload(ctx, name):
    cs = scene.compile_scene(SCENES[name]())
    scene.upload_scene(ctx, cs)
    return cs


def _reference(ctx, cs, name, exact_cull, spp):
    key = (name, exact_cull, spp)
    if key not in _REF:
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        rec = feature_reference(cs, orc, FULL, spp, exact_cull=exact_cull)
        rec.setflags(write=False)
        _REF[key] = rec
    return _REF[key].reshape(H, W, 12)


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("name", list(SCENES))
def test_features_bit_exact(hip_ctx_factory, name):
    torch = _torch()
    with hip_ctx_factory(0) as ctx:
        cs = _upload(ctx, name)
        full3 = _reference(ctx, cs, name, False, 3)
        hits = full3[..., 3]
        # the frame holds all three classes of pixel: no hit, partly covered, fully covered
        assert np.count_nonzero(hits == 0) > 0 and np.count_nonzero((hits > 0) & (hits < 3)) > 0
        assert np.count_nonzero(hits == 3) > 0
        for exact_cull in (False, True):
            for spp in (1, 3):
                ref = _reference(ctx, cs, name, exact_cull, spp)
                for tiles in (FULL, RAGGED):
                    what = f"{name} cull={exact_cull} spp={spp} tiles={len(tiles)}"
                    ys, xs = slot_pixels(tiles, W, H)
                    packed = ref[ys, xs]
                    got = ctx.render_features(spp, tiles, W, H, exact_cull=exact_cull)
                    want = frame_features(packed, tiles, W, H)
                    assert got.shape == (H, W, 12) and got.dtype == f32
                    assert np.array_equal(got, want), f"{what}: {np.count_nonzero(got != want)} host values differ"
                    d = torch.full((len(ys) * 12 + 12,), float("nan"), dtype=torch.float32, device="cuda")
                    assert ctx.render_features_device(spp, tiles, d.data_ptr(), exact_cull=exact_cull) == len(ys)
                    ctx.synchronize()
                    dev = d.cpu().numpy()
                    assert np.all(np.isnan(dev[len(ys) * 12:])), f"{what}: wrote past the packed records"
                    assert np.array_equal(dev[:len(ys) * 12].reshape(-1, 12), packed), f"{what}: device form differs"
        # the host form ADDS into the caller's buffer
        twice = ctx.render_features(1, RAGGED, W, H, features=ctx.render_features(1, RAGGED, W, H))
        once = ctx.render_features(1, RAGGED, W, H)
        assert np.array_equal(twice, once + once)


def test_feature_reference_gathers_per_pixel(hip_ctx_factory):
    """The shortcut above: the reference run directly on the ragged list equals the gathered one."""
    with hip_ctx_factory(0) as ctx:
        cs = _upload(ctx, "textured_scene")
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        ys, xs = slot_pixels(RAGGED, W, H)
        assert np.array_equal(feature_reference(cs, orc, RAGGED, 3), _reference(ctx, cs, "textured_scene", False, 3)[ys, xs])


def _both_forms(ctx, rad, wt, ft, what, **kw):
    """The host and the device form against the restatement; returns the filtered image."""
    torch = _torch()
    want = denoise_reference(rad, wt, ft, **dict(denoise.DEFAULTS, **kw))
    got = ctx.denoise(rad, wt, ft, **kw)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert got.dtype == f32 and got.shape == want.shape and same.all(), f"{what}: {np.count_nonzero(~same)} host values differ"
    h, w = wt.shape
    d_in = [torch.from_numpy(np.ascontiguousarray(a, f32)).cuda() for a in (rad, wt, ft)]
    d_out = torch.full((h * w * 3 + 3,), -7.0, dtype=torch.float32, device="cuda")
    ctx.denoise_device(w, h, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), d_out.data_ptr(), **kw)
    ctx.synchronize()
    dev = d_out.cpu().numpy()
    assert np.all(dev[h * w * 3:] == -7.0), f"{what}: wrote past the output"
    dev = dev[:h * w * 3].reshape(h, w, 3)
    assert np.array_equal(dev, got, equal_nan=True), f"{what}: the device form differs from the host form"
    return got


SETTINGS = {
    "defaults": dict(),
    "one_iteration": dict(iterations=1),
    "eight_iterations": dict(iterations=8),
    "no_squarings": dict(normal_squarings=0),
    "no_colour_stop": dict(sigma_color=0.0),
    "negative_sigma_color": dict(sigma_color=-2.0),
    "tight_sigmas": dict(sigma_depth=0.005, sigma_albedo=0.05, sigma_color=0.1, normal_squarings=8),
}


def test_filter_bit_exact_on_rendered_films(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _upload(ctx, "textured_scene")
        ft = ctx.render_features(2, FULL, W, H)
        hits = ft[..., 3]
        assert np.count_nonzero(hits == 0) and np.count_nonzero(hits == 1) and np.count_nonzero(hits == 2)
        rad, wt = ctx.render(4, DEPTH, FULL, W, H)
        plain = None
        for name, kw in SETTINGS.items():
            out = _both_forms(ctx, rad, wt, ft, name, **kw)
            plain = out if name == "defaults" else plain
        assert not np.array_equal(plain, rad / wt[..., None])      # the filter did something
        # a film from a ragged tile list: weight-0 holes, and doubled weights where tiles overlap
        rrad, rwt = ctx.render(4, DEPTH, RAGGED, W, H)
        assert np.count_nonzero(rwt == 0) and set(np.unique(rwt)) == {0.0, 4.0, 8.0}
        out = _both_forms(ctx, rrad, rwt, ft, "ragged")
        assert not out[rwt == 0].any()
        _both_forms(ctx, rrad, rwt, ctx.render_features(2, RAGGED, W, H), "ragged film, ragged features")
        # an adaptive film: mixed weights
        # (strip errors of this frame after the first test run from 0.07 to 0.2: a threshold of 0.1 stops some)
        arad, awt, info = ctx.render_adaptive(16, DEPTH, FULL, W, H, 0.1, min_spp=2)
        assert info["spp_min"] < info["spp_max"] and len(np.unique(awt)) > 1
        _both_forms(ctx, arad, awt, ft, "adaptive")
        # one NaN and one +inf pixel planted by the test: neither spreads nor changes
        prad = rad.copy()
        prad[20, 33, 1] = np.nan
        prad[7, 50] = np.inf
        out = _both_forms(ctx, prad, wt, ft, "planted")
        assert np.isnan(out[20, 33, 1]) and np.all(np.isinf(out[7, 50]))
        rest = np.ones((H, W), bool)
        rest[20, 33] = rest[7, 50] = False
        assert np.all(np.isfinite(out[rest]))
        # an AO film is not albedo times lighting: NO_DEMODULATE
        orad, owt = ctx.render_ao(4, FULL, W, H)
        _both_forms(ctx, orad, owt, ft, "ao", demodulate=False)


def test_filter_on_a_frame_smaller_than_a_workgroup(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        cs = scene.compile_scene(cornell((9, 3)))
        scene.upload_scene(ctx, cs)
        tiles = [(0, 0, 9, 3)]
        rad, wt = ctx.render(4, DEPTH, tiles, 9, 3)
        ft = ctx.render_features(2, tiles, 9, 3)
        for name, kw in (("9x3", dict()), ("9x3 no colour stop", dict(sigma_color=0.0, iterations=8))):
            _both_forms(ctx, rad, wt, ft, name, **kw)


FORMS = {"wavefront": dict(path=0, path_defer=0, path_spec=0), "k_path": dict(path=1, path_defer=0, path_spec=0)}


@pytest.mark.parametrize("form", list(FORMS))
def test_features_and_filter_keep_the_session(hip_ctx_factory, form):
    with hip_ctx_factory(0) as ctx:
        for k, v in FORMS[form].items():
            ctx.set_option(k, v)
        ctx.set_option("pixel_probe", 1)
        cs = _upload(ctx, "cornell")
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        ys, xs = slot_pixels(RAGGED, W, H)
        rad4, wt4 = ctx.render(4, DEPTH, RAGGED, W, H)
        before = ctx.render_state_export()
        ft = ctx.render_features(3, FULL, W, H)          # another tile list, larger than the session's
        out = ctx.denoise(rad4, wt4, ft)
        assert np.isfinite(out).all()
        info = ctx.render_state_info()
        assert info["spp_done"] == 4 and info["n_pixels"] == len(ys)
        after = ctx.render_state_export()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        rad, wt = ctx.render_continue(4, W, H)
        assert ctx.render_form()["form"] == form
        orad, owt, _, oprobe = orc.render(8, DEPTH, tiles=RAGGED, probe=True)
        assert np.array_equal(wt, owt) and np.array_equal(rad, orad), "the continued film differs from the oracle's 8 spp"
        sampler, sfilm = ctx.render_state_export()
        assert np.array_equal(sampler, oprobe["seed"][ys, xs]), "sampler states differ from the oracle's"
        p = ctx.pixel_probe(len(ys))
        assert np.all(p["flags"] & capi.PROBE_SEED) and np.array_equal(p["seed"], oprobe["seed"][ys, xs])
        assert ctx.render_state_info()["spp_done"] == 8


def test_stats_names(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _upload(ctx, "cornell")
        ctx.set_option("stats", 1)
        ctx.reset_stats()
        ft = ctx.render_features(3, FULL, W, H)
        rad, wt = ctx.render(1, DEPTH, FULL, W, H)
        ctx.denoise(rad, wt, ft, iterations=4)
        st = ctx.kernel_stats()
        assert st["features"]["launches"] == 3 and st["feature_rays"]["launches"] == 3
        assert st["denoise"]["launches"] == 4 and st["denoise_prep"]["launches"] == 1 and st["denoise_finish"]["launches"] == 1


def test_refusals_leave_the_context_usable(hip_ctx_factory):
    lib = capi.load_library()
    with hip_ctx_factory(0) as ctx:
        feat = np.zeros((H, W, 12), f32)
        with pytest.raises(capi.AkrError, match="acceleration structure not built"):
            ctx.render_features(1, FULL, W, H)
        _upload(ctx, "cornell")
        rad, wt = ctx.render(2, DEPTH, FULL, W, H)
        with pytest.raises(capi.AkrError, match="spp must be >= 1"):
            ctx.render_features(0, FULL, W, H)
        fp = capi.FeatureParams(1, 2)
        assert lib.akr_hip_render_features(ctx.h, C.byref(fp), None, 0, feat.ctypes.data_as(C.c_void_p)) != 0
        assert b"flags" in lib.akr_hip_last_error(ctx.h)
        fp = capi.FeatureParams(1, 0)
        assert lib.akr_hip_render_features(ctx.h, C.byref(fp), None, 0, None) != 0
        assert lib.akr_hip_render_features(ctx.h, None, None, 0, feat.ctypes.data_as(C.c_void_p)) != 0
        assert lib.akr_hip_render_features(ctx.h, C.byref(fp), None, 3, feat.ctypes.data_as(C.c_void_p)) != 0
        # an empty tile list is a pass over nothing
        assert not ctx.render_features(1, [(5, 5, 5, 9)], W, H).any()
        ft = ctx.render_features(2, FULL, W, H)
        out = np.zeros((H, W, 3), f32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)

        def refused(p, w, h, r, wgt, f, o, message):
            assert lib.akr_hip_denoise(ctx.h, C.byref(p) if p is not None else None, w, h, r, wgt, f, o) != 0
            assert message in lib.akr_hip_last_error(ctx.h), lib.akr_hip_last_error(ctx.h)
            assert lib.akr_hip_denoise_device(ctx.h, C.byref(p) if p is not None else None, w, h, r, wgt, f, o, None) != 0
            assert message in lib.akr_hip_last_error(ctx.h), lib.akr_hip_last_error(ctx.h)

        good = denoise.params()
        args = (ptr(rad), ptr(wt), ptr(ft), ptr(out))
        refused(None, W, H, *args, b"null parameters")
        for k in range(4):
            a = list(args)
            a[k] = None
            refused(good, W, H, *a, b"null argument")
        refused(good, 0, H, *args, b"W * H == 0")
        refused(good, W, 0, *args, b"W * H == 0")
        refused(good, -3, H, *args, b"W * H == 0")
        for fields, message in (((0, 5, 0.02, 0.3, 0.5, 0), b"iterations"), ((9, 5, 0.02, 0.3, 0.5, 0), b"iterations"),
                                ((5, -1, 0.02, 0.3, 0.5, 0), b"normal_squarings"), ((5, 9, 0.02, 0.3, 0.5, 0), b"normal_squarings"),
                                ((5, 5, 0.0, 0.3, 0.5, 0), b"sigma_depth"), ((5, 5, float("nan"), 0.3, 0.5, 0), b"sigma_depth"),
                                ((5, 5, 0.02, -1.0, 0.5, 0), b"sigma_albedo"), ((5, 5, 0.02, 0.3, float("nan"), 0), b"sigma_color"),
                                ((5, 5, 0.02, 0.3, 0.5, 2), b"flags")):
            refused(capi.DenoiseParams(*fields), W, H, *args, message)
        assert not out.any()
        # the context is as usable as before, and its session is still there
        _both_forms(ctx, rad, wt, ft, "after the refusals")
        assert ctx.render_state_info()["spp_done"] == 2


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0     # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1].copy()


def test_cli_denoise_and_aov(tmp_path):
    path = tmp_path / "s.akari"
    out, aov = tmp_path / "o.pfm", tmp_path / "aov"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3, tile_size: 16 }", out=out, mesh=CORNELL_MESH))
    assert render.main([str(path), "--denoise", "--aov", str(aov), "--feature-spp", "3", "--denoise-iters", "4"]) == 0
    sc = scene.load_scene_file(str(path))
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    tiles = render._tiles(sc, 16)
    with capi.HipContext(0) as ctx:
        scene.upload_scene(ctx, cs)
        rad, wt = ctx.render(4, 3, tiles, w, h, ray_clamp=sc.integrator.ray_clamp)
        ft = ctx.render_features(3, tiles, w, h)
        img = ctx.denoise(rad, wt, ft, iterations=4)
    albedo, normal, depth, _ = denoise.split_features(ft)
    assert np.array_equal(_read_pfm(out), img)
    assert np.array_equal(_read_pfm(str(aov) + ".albedo.pfm"), albedo)
    assert np.array_equal(_read_pfm(str(aov) + ".normal.pfm"), normal)
    assert np.array_equal(_read_pfm(str(aov) + ".depth.pfm"), np.repeat(depth[..., None], 3, axis=-1))
    # previews are filtered too, the features are rendered once, and --aov works without --denoise
    out2 = tmp_path / "p.pfm"
    assert render.main([str(path), "--out", str(out2), "--preview", "--denoise", "--feature-spp", "3",
                        "--denoise-iters", "4"]) == 0
    assert np.array_equal(_read_pfm(out2), img)
    out3 = tmp_path / "q.pfm"
    assert render.main([str(path), "--out", str(out3), "--aov", str(tmp_path / "b"), "--feature-spp", "3"]) == 0
    assert np.array_equal(_read_pfm(out3), film_io.resolve(rad, wt))
    assert np.array_equal(_read_pfm(str(tmp_path / "b") + ".albedo.pfm"), albedo)


def test_cpp_adapter_denoise(tmp_path):
    exe = tmp_path / "denoise_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "denoise_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "continued_equals_fresh=1" in r.stdout and "spp_done=8" in r.stdout and "bad=0" in r.stdout
