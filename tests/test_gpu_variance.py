"""The film variance tracker and the variance-guided a-trous filter on device 0.

The tracker is compared with variance_reference fed with the films the device held after each pass
(render_state_export: the packed film), the filter with denoise_guided_reference, both restated in
test_variance_host.py; every comparison is array_equal."""
import subprocess

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, denoise, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell, slot_pixels
from test_denoise_host import SDL, denoise_reference
from test_variance_host import denoise_guided_reference, variance_reference

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 70, 45
FULL = [(0, 0, W, H)]
RAGGED = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 64, 64), (5, 5, 5, 9), (60, 30, 100, 100)]   # overlapping, clipped, empty
DEPTH = 5
FORMS = {"wavefront": dict(path=0, path_defer=0, path_spec=0), "k_path": dict(path=1, path_defer=0, path_spec=0)}


def _ctx_with_cornell(ctx, res=(W, H), track=True, **options):
    for k, v in options.items():
        ctx.set_option(k, v)
    if track:
        ctx.set_option("film_variance", 1)
    cs = scene.compile_scene(cornell(res))
    scene.upload_scene(ctx, cs)
    return cs


def _frame(packed, tiles, w=W, h=H):
    """Packed (vr, vg, vb, K) records added into a full frame, as the host form does."""
    ys, xs = slot_pixels(tiles, w, h)
    out = np.zeros((h, w, 4), f32)
    np.add.at(out, (ys, xs), packed)
    return out


def _check_tracker(ctx, films, tiles, what, w=W, h=H, device=True):
    """Both export forms against the restatement fed with `films`; returns the packed records."""
    want = variance_reference(films)
    n = len(want)
    got = ctx.render_variance(w, h)
    assert got.dtype == f32 and got.shape == (h, w, 4)
    frame = _frame(want, tiles, w, h)
    assert np.array_equal(got, frame), f"{what}: {np.count_nonzero(got != frame)} host values differ"
    if device:
        import torch
        d = torch.full((n * 4 + 4,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()      # torch filled the buffer on its own stream; the export runs on the context's
        assert ctx.render_variance_device(d.data_ptr()) == n
        ctx.synchronize()
        dev = d.cpu().numpy()
        assert np.all(np.isnan(dev[n * 4:])), f"{what}: wrote past the packed records"
        assert np.array_equal(dev[:n * 4].reshape(-1, 4), want), f"{what}: the device form differs"
    return want


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tiles", [FULL, RAGGED], ids=["full", "ragged"])
def test_tracker_over_passes(hip_ctx_factory, form, tiles):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx, **FORMS[form])
        films = []
        for k, n in enumerate((1, 1, 2, 4)):
            if k == 0:
                ctx.render(n, DEPTH, tiles, W, H)
            else:
                ctx.render_continue(n, W, H)
            assert ctx.render_form()["form"] == form
            films.append(ctx.render_state_export()[1])
            rec = _check_tracker(ctx, films, tiles, f"{form} after pass {k}", device=k == 3)
            assert np.all(rec[:, 3] == k + 1)
            assert not rec[:, :3].any() if k == 0 else np.count_nonzero(rec[:, :3]) > len(rec)   # noise from the second batch on
        assert np.all(np.isfinite(rec)) and np.all(rec[:, :3] >= 0)
        # the host form ADDS into the caller's buffer; a continue of no samples is no batch
        once = ctx.render_variance(W, H)
        assert np.array_equal(ctx.render_variance(W, H, variance=once.copy()), once + once)
        ctx.render_continue(0, W, H)
        assert np.array_equal(ctx.render_variance(W, H), once)


def test_tracker_masked_continues_give_mixed_batch_counts(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx)
        ys, xs = slot_pixels(FULL, W, H)
        ctx.render(2, DEPTH, FULL, W, H)
        films = [ctx.render_state_export()[1]]
        for mask, n in (((xs < 40), 2), ((ys < 20), 3)):
            ctx.render_continue_masked(n, mask.astype(np.uint8), W, H)
            films.append(ctx.render_state_export()[1])
        rec = _check_tracker(ctx, films, FULL, "masked")
        assert set(np.unique(rec[:, 3])) == {1.0, 2.0, 3.0}
        assert np.array_equal(rec[:, 3], 1 + (xs < 40).astype(f32) + (ys < 20).astype(f32))
        assert not rec[rec[:, 3] == 1, :3].any()
        # a later uniform continue is one more batch for every slot, from each slot's own count
        ctx.render_continue(1, W, H)
        films.append(ctx.render_state_export()[1])
        rec = _check_tracker(ctx, films, FULL, "masked, then uniform")
        assert set(np.unique(rec[:, 3])) == {2.0, 3.0, 4.0}


def test_tracker_adaptive_begin_and_steps(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx)
        info, more = ctx.adaptive_begin(16, DEPTH, FULL, 0.1, min_spp=2)
        rad, wt = ctx.render_continue(0, W, H)           # the film read between steps (a whole-frame tile: slot order)
        films = [np.concatenate([rad, wt[..., None]], axis=-1).reshape(-1, 4)]
        assert np.array_equal(films[0], ctx.render_state_export()[1])
        while more:
            info, more = ctx.adaptive_step()
            films.append(ctx.render_state_export()[1])
        assert info["spp_min"] < info["spp_max"] and len(films) == info["passes"]
        rec = _check_tracker(ctx, films, FULL, "adaptive steps")
        assert len(np.unique(rec[:, 3])) > 1 and rec[:, 3].max() == info["passes"]
        # the one-call form runs the same passes
        rad, wt, info2 = ctx.render_adaptive(16, DEPTH, FULL, W, H, 0.1, min_spp=2)
        assert info2 == info
        _check_tracker(ctx, films, FULL, "render_adaptive")


def test_tracker_import_is_one_batch_and_zero_spp_is_none(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx)
        ctx.render(0, DEPTH, RAGGED, W, H)
        rec = _check_tracker(ctx, [ctx.render_state_export()[1]], RAGGED, "0 spp")
        assert not rec.any()
        ctx.render_continue(4, W, H)
        sampler, film4 = ctx.render_state_export()
        rec = _check_tracker(ctx, [film4], RAGGED, "0 + 4 spp")
        assert np.all(rec[:, 3] == 1)
        ctx.render_continue(2, W, H)          # K = 2 now; the import below starts again from one batch
        ctx.render_state_import(4, DEPTH, RAGGED, sampler, film4)
        rec = _check_tracker(ctx, [film4], RAGGED, "import")
        assert np.all(rec[:, 3] == 1) and not rec[:, :3].any()
        ctx.render_continue(4, W, H)
        rec = _check_tracker(ctx, [film4, ctx.render_state_export()[1]], RAGGED, "import + 4")
        assert np.all(rec[:, 3] == 2) and rec[:, :3].any()
        ctx.render_state_import(0, DEPTH, FULL, np.arange(W * H, dtype=np.uint32), np.zeros((W * H, 4), f32))
        assert not ctx.render_variance(W, H).any()       # an imported film of weight 0 is no batch


@pytest.mark.parametrize("form", list(FORMS))
def test_tracker_leaves_the_render_alone(hip_ctx_factory, form):
    with hip_ctx_factory(0) as ctx:
        cs = _ctx_with_cornell(ctx, track=False, pixel_probe=1, **FORMS[form])
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        ys, xs = slot_pixels(RAGGED, W, H)
        orad, owt, _, oprobe = orc.render(8, DEPTH, tiles=RAGGED, probe=True)
        got = {}
        for on in (0, 1):
            ctx.set_option("film_variance", on)
            ctx.render(4, DEPTH, RAGGED, W, H)
            rad, wt = ctx.render_continue(4, W, H)
            assert ctx.render_form()["form"] == form
            sampler, film = ctx.render_state_export()
            probe = ctx.pixel_probe(len(ys))
            assert np.array_equal(rad, orad) and np.array_equal(wt, owt), f"film_variance {on}: the film differs from the oracle's"
            assert np.array_equal(sampler, oprobe["seed"][ys, xs]) and np.array_equal(probe["seed"], oprobe["seed"][ys, xs])
            got[on] = (rad, wt, sampler, film, probe)
        for a, b in zip(got[0], got[1]):
            assert np.array_equal(a, b)
        assert np.all(ctx.render_variance(W, H)[ys, xs, 3] >= 2)
        # option off: the export is refused with its message, both forms, and the context stays usable
        ctx.set_option("film_variance", 0)
        ctx.render(2, DEPTH, FULL, W, H)
        import torch
        d = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for call in (lambda: ctx.render_variance(W, H), lambda: ctx.render_variance_device(d.data_ptr())):
            with pytest.raises(capi.AkrError, match="started without option film_variance"):
                call()
        assert not d.cpu().numpy().any()
        ctx.set_option("film_variance", 1)                # read when a session starts: this one started without
        with pytest.raises(capi.AkrError, match="started without option film_variance"):
            ctx.render_variance(W, H)
        rad, wt = ctx.render_continue(2, W, H)
        o4 = orc.render(4, DEPTH)
        assert np.array_equal(rad, o4[0]) and np.array_equal(wt, o4[1])
        ctx.set_camera(cs.camera.position, cs.camera.rotation, cs.camera.fov, cs.camera.resolution)   # ends the session
        with pytest.raises(capi.AkrError, match="no render session"):
            ctx.render_variance(W, H)
        with pytest.raises(capi.AkrError, match="must be in"):
            ctx.set_option("film_variance", 2)


def test_update_is_launched_once_per_call_that_draws_samples(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx, track=False, stats=1)
        ctx.render(2, DEPTH, FULL, W, H)
        ctx.render_continue(2, W, H)
        assert "variance_update" not in ctx.kernel_stats()        # off: nothing is launched
        ctx.set_option("film_variance", 1)
        ctx.reset_stats()
        ctx.render(2, DEPTH, FULL, W, H)
        ctx.render_continue(0, W, H)
        ctx.render_continue(2, W, H)
        ctx.render_continue_masked(2, np.zeros(W * H, np.uint8), W, H)    # an all-zero mask draws nothing
        var = ctx.render_variance(W, H)
        ft = ctx.render_features(2, FULL, W, H)
        rad, wt = ctx.render_continue(0, W, H)
        ctx.denoise_guided(rad, wt, ft, var, iterations=4)
        st = ctx.kernel_stats()
        assert st["variance_update"]["launches"] == 2 and st["variance_resolve"]["launches"] == 1
        assert st["denoise_guided"]["launches"] == 4 and st["denoise_prep_variance"]["launches"] == 1
        assert "denoise" not in st and st["denoise_prep"]["launches"] == 1 and st["denoise_finish"]["launches"] == 1


# ----------------------------------------------------------------------------------- the guided filter
def _both_forms(ctx, rad, wt, ft, var, what, **kw):
    """The host and the device form against the restatement; returns the filtered image."""
    import torch
    ref_kw = dict(denoise.DEFAULTS, sigma_variance=denoise.DEFAULT_SIGMA_VARIANCE)
    want = denoise_guided_reference(rad, wt, ft, var, **dict(ref_kw, **kw))
    got = ctx.denoise_guided(rad, wt, ft, var, **kw)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert got.dtype == f32 and got.shape == want.shape and same.all(), f"{what}: {np.count_nonzero(~same)} host values differ"
    h, w = wt.shape
    d_in = [torch.from_numpy(np.ascontiguousarray(a, f32)).cuda() for a in (rad, wt, ft, var)]
    d_out = torch.full((h * w * 3 + 3,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()          # torch's uploads and fill ran on its own stream; the filter runs on the context's
    ctx.denoise_guided_device(w, h, *[d.data_ptr() for d in d_in], d_out.data_ptr(), **kw)
    ctx.synchronize()
    dev = d_out.cpu().numpy()
    assert np.all(dev[h * w * 3:] == -7.0), f"{what}: wrote past the output"
    assert np.array_equal(dev[:h * w * 3].reshape(h, w, 3), got, equal_nan=True), f"{what}: the device form differs"
    return got


SETTINGS = {
    "defaults": dict(),
    "one_iteration": dict(iterations=1),
    "eight_iterations": dict(iterations=8),
    "narrow": dict(sigma_variance=0.5, normal_squarings=0),
    "wide_no_shipped_stop": dict(sigma_variance=8.0, sigma_color=0.0),
    "no_demodulation": dict(demodulate=False),
}


def test_guided_filter_bit_exact_on_rendered_films(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx)
        ft = ctx.render_features(2, FULL, W, H)
        ys, xs = slot_pixels(FULL, W, H)
        ctx.render(1, DEPTH, FULL, W, H)
        ctx.render_continue(1, W, H)
        rad, wt = ctx.render_continue(2, W, H)
        var = ctx.render_variance(W, H)
        assert np.all(var[..., 3] == 3) and np.count_nonzero(var[..., :3]) > W * H
        plain = None
        for name, kw in SETTINGS.items():
            out = _both_forms(ctx, rad, wt, ft, var, name, **kw)
            plain = out if name == "defaults" else plain
        assert not np.array_equal(plain, rad / wt[..., None]) and not np.array_equal(plain, ctx.denoise(rad, wt, ft))
        # every K < 2: the shipped filter, bit for bit
        single = var.copy()
        single[..., 3] = 1
        for kw in (dict(), dict(iterations=8), dict(sigma_color=0.0)):
            assert np.array_equal(ctx.denoise_guided(rad, wt, ft, single, **kw), ctx.denoise(rad, wt, ft, **kw))
            assert np.array_equal(ctx.denoise_guided(rad, wt, ft, np.zeros_like(var), **kw), ctx.denoise(rad, wt, ft, **kw))
        # a film that mixes pixels with and without hv: a masked continue leaves the others at one batch
        ctx.render(2, DEPTH, FULL, W, H)
        mrad, mwt = ctx.render_continue_masked(2, ((xs + ys) % 7 < 4).astype(np.uint8), W, H)
        mvar = ctx.render_variance(W, H)
        assert set(np.unique(mvar[..., 3])) == {1.0, 2.0} and len(np.unique(mwt)) == 2
        for name, kw in (("mixed hv", dict()), ("mixed hv, 8 iterations", dict(iterations=8)),
                         ("mixed hv, no shipped stop", dict(sigma_color=-1.0))):
            _both_forms(ctx, mrad, mwt, ft, mvar, name, **kw)
        # a film from a ragged tile list: weight-0 holes, doubled weights and batch counts where tiles overlap
        ctx.render(2, DEPTH, RAGGED, W, H)
        rrad, rwt = ctx.render_continue(2, W, H)
        rvar = ctx.render_variance(W, H)
        assert np.count_nonzero(rwt == 0) and set(np.unique(rvar[..., 3])) == {0.0, 2.0, 4.0}
        out = _both_forms(ctx, rrad, rwt, ft, rvar, "ragged")
        assert not out[rwt == 0].any()
        garbage = rvar.copy()
        garbage[rwt == 0] = [1e30, np.nan, 5.0, 7.0]          # what lies under weight 0 is never read as a variance
        assert np.array_equal(ctx.denoise_guided(rrad, rwt, ft, garbage), out)
        # NaN and +inf planted in the film and in the variance: neither spreads nor changes
        prad, pvar = rad.copy(), var.copy()
        prad[20, 33, 1] = np.nan
        prad[7, 50] = np.inf
        pvar[30, 10, 2] = np.nan
        pvar[12, 60, :3] = np.inf
        pvar[40, 40, 3] = np.nan
        for name, kw in (("planted", dict()), ("planted, one iteration", dict(iterations=1))):
            out = _both_forms(ctx, prad, wt, ft, pvar, name, **kw)
            assert np.isnan(out[20, 33, 1]) and np.all(np.isinf(out[7, 50]))
            rest = np.ones((H, W), bool)
            rest[20, 33] = rest[7, 50] = False
            assert np.all(np.isfinite(out[rest]))


def test_guided_filter_on_a_frame_smaller_than_a_workgroup(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx, res=(9, 3))
        tiles = [(0, 0, 9, 3)]
        ctx.render(2, DEPTH, tiles, 9, 3)
        ctx.render_continue(2, 9, 3)
        rad, wt = ctx.render_continue(4, 9, 3)
        var = ctx.render_variance(9, 3)
        assert var.shape == (3, 9, 4) and np.all(var[..., 3] == 3)
        ft = ctx.render_features(2, tiles, 9, 3)
        for name, kw in (("9x3", dict()), ("9x3, 8 iterations", dict(iterations=8, sigma_variance=1.0)),
                         ("9x3, 1 iteration", dict(iterations=1))):
            _both_forms(ctx, rad, wt, ft, var, name, **kw)


@pytest.mark.parametrize("form", list(FORMS))
def test_variance_and_guided_filter_keep_the_session(hip_ctx_factory, form):
    with hip_ctx_factory(0) as ctx:
        cs = _ctx_with_cornell(ctx, pixel_probe=1, **FORMS[form])
        nodes, tris = ctx.accel_export()
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        ys, xs = slot_pixels(RAGGED, W, H)
        ctx.render(2, DEPTH, RAGGED, W, H)
        rad4, wt4 = ctx.render_continue(2, W, H)
        before = ctx.render_state_export()
        var = ctx.render_variance(W, H)
        ft = ctx.render_features(2, FULL, W, H)
        out = ctx.denoise_guided(rad4, wt4, ft, var)
        assert np.isfinite(out).all() and not out[wt4 == 0].any()
        after = ctx.render_state_export()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.array_equal(ctx.render_variance(W, H), var)          # the tracker was kept too
        rad, wt = ctx.render_continue(4, W, H)
        assert ctx.render_form()["form"] == form
        orad, owt, _, oprobe = orc.render(8, DEPTH, tiles=RAGGED, probe=True)
        assert np.array_equal(wt, owt) and np.array_equal(rad, orad), "the continued film differs from the oracle's 8 spp"
        sampler, film8 = ctx.render_state_export()
        assert np.array_equal(sampler, oprobe["seed"][ys, xs]), "sampler states differ from the oracle's"
        assert ctx.render_state_info()["spp_done"] == 8
        assert np.all(ctx.render_variance(W, H)[ys, xs, 3] >= 3)


def test_guided_refusals_leave_the_context_usable(hip_ctx_factory):
    import ctypes as C
    lib = capi.load_library()
    with hip_ctx_factory(0) as ctx:
        _ctx_with_cornell(ctx)
        ctx.render(2, DEPTH, FULL, W, H)
        rad, wt = ctx.render_continue(2, W, H)
        ft, var = ctx.render_features(2, FULL, W, H), ctx.render_variance(W, H)
        out = np.zeros((H, W, 3), f32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        args = (ptr(rad), ptr(wt), ptr(ft), ptr(var), ptr(out))

        def refused(p, w, h, a, message):
            assert lib.akr_hip_denoise_guided(ctx.h, C.byref(p) if p is not None else None, w, h, *a) != 0
            assert message in lib.akr_hip_last_error(ctx.h), lib.akr_hip_last_error(ctx.h)
            assert lib.akr_hip_denoise_guided_device(ctx.h, C.byref(p) if p is not None else None, w, h, *a, None) != 0
            assert message in lib.akr_hip_last_error(ctx.h), lib.akr_hip_last_error(ctx.h)

        good = denoise.guided_params()
        refused(None, W, H, args, b"null parameters")
        for k in range(5):
            a = list(args)
            a[k] = None
            refused(good, W, H, a, b"null argument")
        refused(good, 0, H, args, b"W * H == 0")
        for sv in (0.0, -1.0, float("nan"), float("inf")):
            refused(capi.DenoiseGuidedParams(denoise.params(), sv), W, H, args, b"sigma_variance")
        refused(capi.DenoiseGuidedParams(capi.DenoiseParams(0, 5, 0.02, 0.3, 0.5, 0), 2.0), W, H, args, b"iterations")
        assert lib.akr_hip_render_variance(ctx.h, None) != 0 and b"null argument" in lib.akr_hip_last_error(ctx.h)
        assert not out.any()
        _both_forms(ctx, rad, wt, ft, var, "after the refusals")
        assert ctx.render_state_info()["spp_done"] == 4


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0     # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)[::-1].copy()


def test_cli_denoise_variance_and_aov(tmp_path):
    path = tmp_path / "s.akari"
    out, aov = tmp_path / "o.pfm", tmp_path / "aov"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3, tile_size: 16 }", out=out, mesh=CORNELL_MESH))
    assert render.main([str(path), "--pass-spp", "2", "--spp", "8", "--denoise", "--denoise-variance", "--aov", str(aov)]) == 0
    sc = scene.load_scene_file(str(path))
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    tiles = render._tiles(sc, 16)
    with capi.HipContext(0) as ctx:
        ctx.set_option("film_variance", 1)
        scene.upload_scene(ctx, cs)
        ctx.render(2, 3, tiles, w, h, ray_clamp=sc.integrator.ray_clamp)
        for _ in range(3):
            rad, wt = ctx.render_continue(2, w, h)
        var = ctx.render_variance(w, h)
        ft = ctx.render_features(denoise.DEFAULT_FEATURE_SPP, tiles, w, h)
        img = ctx.denoise_guided(rad, wt, ft, var)
        shipped = ctx.denoise(rad, wt, ft)
    assert np.all(var[..., 3] == 4) and np.all(wt == 8)
    assert np.array_equal(_read_pfm(out), img) and not np.array_equal(img, shipped)
    assert np.array_equal(_read_pfm(str(aov) + ".variance.pfm"), var[..., :3])
    albedo, _, _, _ = denoise.split_features(ft)
    assert np.array_equal(_read_pfm(str(aov) + ".albedo.pfm"), albedo)
    # previews are filtered with the variance of their own film
    out2 = tmp_path / "p.pfm"
    assert render.main([str(path), "--out", str(out2), "--spp", "8", "--pass-spp", "2", "--preview", "--denoise",
                        "--denoise-variance"]) == 0
    assert np.array_equal(_read_pfm(out2), img)
    # without --denoise-variance nothing changes: the shipped filter, no variance image
    out3 = tmp_path / "q.pfm"
    assert render.main([str(path), "--out", str(out3), "--spp", "8", "--pass-spp", "2", "--denoise", "--aov", str(tmp_path / "b")]) == 0
    assert np.array_equal(_read_pfm(out3), shipped) and not (tmp_path / "b.variance.pfm").exists()


def test_cpp_adapter_variance(tmp_path):
    exe = tmp_path / "variance_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "variance_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "continued_equals_fresh=1" in r.stdout and "refused=1" in r.stdout and "bad=0" in r.stdout
