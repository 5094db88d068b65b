"""Host side of the film variance tracker and the variance-guided a-trous filter: the
NumPy f32 restatements that the GPU tests compare against (variance_reference, denoise_guided_reference),
the tracker against an f64 two-pass variance, the filter's invariants on hand-made films, the parameter
and CLI refusals, and the quality condition of the specification on the oracle's Cornell box.  No GPU
needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, denoise, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell
from test_denoise_host import (SDL, _dot, _flat_features, _rmax, denoise_reference, feature_reference, frame_features,
                               relmse)

f32 = np.float32


# ------------------------------------------------------------------------------------ the two definitions
class VarianceTracker:
    """k_variance_update of include/akr_hip.h restated: West's weighted incremental update on the batch
    means, one call of update() per film the session held after a call that drew samples.  Films are
    [n, 4] (sum r, g, b, weight); f32, unfused, left to right."""

    def __init__(self, n):
        self.P = np.zeros((n, 4), f32)
        self.M2 = np.zeros((n, 3), f32)
        self.K = np.zeros(n, f32)

    def update(self, film):
        F = np.asarray(film, f32).reshape(-1, 4)
        P = self.P
        with np.errstate(all="ignore"):
            n = F[:, 3] - P[:, 3]
            upd = n > 0
            has = upd & (P[:, 3] > 0)
            d = (F[:, :3] - P[:, :3]) / n[:, None] - P[:, :3] / P[:, 3:4]
            add = (d * d) * ((P[:, 3] * n) / F[:, 3])[:, None]
            assert add.dtype == f32
            self.M2 = np.where(has[:, None], self.M2 + add, self.M2)
        self.K = np.where(upd, self.K + f32(1), self.K)
        self.P = np.where(upd[:, None], F, P)

    def resolve(self, film=None):
        """k_variance_resolve: per slot (vr, vg, vb, K), the variance of the mean for K >= 2, else 0."""
        F = self.P if film is None else np.asarray(film, f32).reshape(-1, 4)
        out = np.zeros((len(self.K), 4), f32)
        with np.errstate(all="ignore"):
            v = (self.M2 / (self.K - f32(1))[:, None]) / F[:, 3:4]
        out[:, :3] = np.where((self.K >= 2)[:, None], v, f32(0))
        out[:, 3] = self.K
        return out


def variance_reference(films):
    """The tracker's export after a session whose film was `films[i]` ([n, 4]) after its i-th call that drew
    samples (an imported film counts as the first): [n, 4] = (vr, vg, vb, K)."""
    films = [np.asarray(f, f32).reshape(-1, 4) for f in films]
    t = VarianceTracker(len(films[0]) if films else 0)
    for f in films:
        t.update(f)
    return t.resolve()


def denoise_guided_reference(radiance, weight, features, variance, iterations=5, normal_squarings=5, sigma_depth=0.02,
                             sigma_albedo=0.3, sigma_color=0.5, demodulate=True, sigma_variance=2.0):
    """The guided filter of include/akr_hip.h restated: denoise_reference with the variance record, its 3x3
    prefilter, the variance colour stop of pixels with hv and the propagation; f32, left to right."""
    rad, wt, ft, var = (np.asarray(a, f32) for a in (radiance, weight, features, variance))
    H, W = wt.shape
    assert var.shape == (H, W, 4)
    sd, sa, scol, sv = f32(sigma_depth), f32(sigma_albedo), f32(sigma_color), f32(sigma_variance)
    zero, one = f32(0), f32(1)
    with np.errstate(all="ignore"):
        valid = wt > 0
        c = np.where(valid[..., None], rad / wt[..., None], zero)
        h = ft[..., 3]
        some = h > 0
        hd = h[..., None]
        a = np.where(some[..., None], ft[..., 0:3] / hd, zero)
        nn = np.where(some[..., None], ft[..., 4:7] / hd, zero)
        t = np.where(some, ft[..., 7] / h, zero)
        x = np.where(some[..., None], ft[..., 8:11] / hd, zero)
        l = np.sqrt(_dot(nn, nn))
        nh = np.where((l > 0)[..., None], nn / l[..., None], zero)
        m = np.where((a > f32(1e-3)) & bool(demodulate), a, one)
        I = (c / m).astype(f32)
        hv = valid & (var[..., 3] >= 2) & np.isfinite(var[..., 0:3]).all(axis=-1)
        V = np.where(hv[..., None], var[..., 0:3] / (m * m), zero).astype(f32)
        sv3 = (f32(3.0) * sv) * sv
        Y, X = np.mgrid[0:H, 0:W]
        hk = [f32(1) / f32(16), f32(1) / f32(4), f32(3) / f32(8), f32(1) / f32(4), f32(1) / f32(16)]
        gk = [f32(1) / f32(4), f32(1) / f32(2), f32(1) / f32(4)]
        zden = sd * t
        for i in range(int(iterations)):
            s = 1 << i
            sc = scol * (one / f32(1 << i))
            sc2 = sc * sc
            fin = np.isfinite(I).all(axis=-1)
            gn = np.zeros((H, W, 3), f32)
            gd = np.zeros((H, W), f32)
            for j in range(3):
                for k in range(3):
                    qy, qx = Y + (j - 1), X + (k - 1)
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    acc = inside & hv[qy, qx]
                    gw = gk[j] * gk[k]
                    gn = np.where(acc[..., None], gn + gw * V[qy, qx], gn)
                    gd = np.where(acc, gd + gw, gd)
            G = np.where((gd > 0)[..., None], gn / gd[..., None], V)
            assert G.dtype == f32
            num = np.zeros((H, W, 3), f32)
            vnum = np.zeros((H, W, 3), f32)
            den = np.zeros((H, W), f32)
            for j in range(5):
                for k in range(5):
                    qy, qx = Y + (j - 2) * s, X + (k - 2) * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    Iq = I[qy, qx]
                    Vq = np.where(hv[qy, qx][..., None], V[qy, qx], zero)
                    accept = inside & valid[qy, qx] & fin[qy, qx]
                    if j == 2 and k == 2:
                        g = wc = np.ones((H, W), f32)
                    else:
                        wn = _rmax(_dot(nh, nh[qy, qx]), zero)
                        for _ in range(int(normal_squarings)):
                            wn = wn * wn
                        wz = _rmax(one - np.abs(_dot(nh, x[qy, qx] - x)) / zden, zero)
                        da = a[qy, qx] - a
                        dsum = np.abs(da[..., 0]) + np.abs(da[..., 1])
                        dsum = dsum + np.abs(da[..., 2])
                        wa = _rmax(one - dsum / sa, zero)
                        sq = some[qy, qx]
                        g = np.where(some & sq, wn * wz * wa, np.where(some | sq, zero, one)).astype(f32)
                        d = Iq - I
                        if scol > 0:
                            wc = one / (one + _dot(d, d) / sc2)
                        else:
                            wc = np.ones((H, W), f32)
                        e = (d * d) / (G + f32(1e-8))
                        r = ((e[..., 0] + e[..., 1]) + e[..., 2]) / sv3
                        wc = np.where(hv, one / (one + r), wc)
                    w = ((hk[j] * hk[k]) * g) * wc
                    assert w.dtype == f32
                    num = np.where(accept[..., None], num + w[..., None] * Iq, num)
                    vnum = np.where(accept[..., None], vnum + (w * w)[..., None] * Vq, vnum)
                    den = np.where(accept, den + w, den)
            res = np.where((den > 0)[..., None], num / den[..., None], I)
            res = np.where(fin[..., None], res, I)
            Vres = np.where((den > 0)[..., None], vnum / (den * den)[..., None], V)
            V = np.where((fin & valid)[..., None], Vres, V).astype(f32)
            I = np.where(valid[..., None], res, zero).astype(f32)
        out = np.where(valid[..., None], I * m, zero).astype(f32)
    return out


def frame_film(rad, wt):
    """A full-frame film as the [n, 4] slot records of a whole-frame tile."""
    return np.concatenate([np.asarray(rad, f32), np.asarray(wt, f32)[..., None]], axis=-1).reshape(-1, 4)


# ------------------------------------------------------------------------------------------- the tracker
def test_tracker_against_f64_two_pass_variance():
    """Batches of one sample, K = 16, values in [0, 1) on a 2^-10 grid (so the f32 film sums are exact): the
    tracker's variance of the mean equals the f64 two-pass sample variance divided by the count to rtol 1e-4
    (the f32 round-off of 16 terms is about 1e-6: a margin of 100)."""
    rng = np.random.default_rng(3)
    n, k = 500, 16
    y = rng.integers(0, 1024, (k, n, 3)).astype(np.float64) / 1024.0
    tr = VarianceTracker(n)
    film = np.zeros((n, 4), f32)
    for b in range(k):
        film = film.copy()
        film[:, :3] += y[b].astype(f32)
        film[:, 3] += 1
        tr.update(film)
    assert np.array_equal(film[:, :3].astype(np.float64), y.sum(axis=0))   # the sums were exact
    out = tr.resolve()
    assert out.dtype == f32 and np.all(out[:, 3] == k)
    want = y.var(axis=0, ddof=1) / k
    np.testing.assert_allclose(out[:, :3], want, rtol=1e-4)
    assert np.array_equal(out, variance_reference([f for f in _cumulative(y)]))


def _cumulative(y):
    film = np.zeros((y.shape[1], 4), f32)
    for b in range(y.shape[0]):
        film = film.copy()
        film[:, :3] += y[b].astype(f32)
        film[:, 3] += 1
        yield film


def test_tracker_first_batch_zero_weight_and_unchanged_slots():
    film1 = np.array([[1.0, 2.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0], [4.0, 4.0, 4.0, 4.0]], f32)
    out = variance_reference([film1])
    assert np.array_equal(out, f32([[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 1]]))   # one batch: no variance yet
    film2 = film1.copy()
    film2[0] = [3.0, 2.0, 5.0, 4.0]    # 2 more samples with batch mean (1, 0, 1) against (0.5, 1, 1.5)
    film2[1] = [1.0, 1.0, 1.0, 1.0]    # this slot's first batch
    out = variance_reference([film1, film2])   # slot 2 did not change: K stays 1
    assert np.array_equal(out[:, 3], f32([2, 1, 1])) and not out[1:, :3].any()
    # M2 = d^2 * (2 * 2 / 4) with d = (0.5, -1, -0.5); v = M2 / (K - 1) / 4
    assert np.array_equal(out[0, :3], f32([0.25, 1.0, 0.25]) / f32(4))
    assert np.array_equal(variance_reference([np.zeros((5, 4), f32)]), np.zeros((5, 4), f32))   # a 0-spp session


def test_tracker_unequal_batches_same_expectation():
    """Per-sample variance s2 = 1/12 (uniform samples), 16 samples per slot split 1, 1, 2, 4, 8 and 4, 4, 4, 4:
    M2 / (K - 1) has expectation s2 for both.  Its relative standard deviation per slot is sqrt(2 / (K - 1))
    plus the uniform's kurtosis term, below 0.9; the mean over 40 000 slot-channels has 0.9 / 200 = 0.0045, so
    3 % is more than six of them."""
    rng = np.random.default_rng(17)
    n = 40000 // 3 + 1
    y = rng.random((16, n, 3))
    for sizes in ((1, 1, 2, 4, 8), (4, 4, 4, 4), (8, 4, 2, 1, 1)):
        tr = VarianceTracker(n)
        film = np.zeros((n, 4), np.float64)
        at = 0
        for b in sizes:
            film[:, :3] += y[at:at + b].sum(axis=0)
            film[:, 3] += b
            at += b
            tr.update(film.astype(f32))
        out = tr.resolve()
        assert np.all(out[:, 3] == len(sizes))
        s2 = (out[:, :3].astype(np.float64) * 16).mean()    # variance of the mean times the count
        print(f"batches {sizes}: mean per-sample variance {s2:.5f} (1/12 = {1 / 12:.5f})")
        assert abs(s2 * 12 - 1) < 0.03, (sizes, s2)


# ------------------------------------------------------------------------------------- the guided filter
def _noisy_film(H, W, spp=4, seed=9):
    rng = np.random.default_rng(seed)
    wt = np.full((H, W), spp, f32)
    rad = (rng.uniform(0.5, 1.5, (H, W, 3)) * spp).astype(f32)
    var = np.empty((H, W, 4), f32)
    var[..., :3] = rng.uniform(0.01, 0.05, (H, W, 3)).astype(f32)
    var[..., 3] = 3
    return rad, wt, var


def test_guided_with_no_variance_is_the_shipped_filter():
    H, W = 21, 34
    ft = _flat_features(H, W)
    ft[:, :6] = 0
    rad, wt, var = _noisy_film(H, W)
    wt[4:7, 20:25] = 0
    rad[10, 10, 2] = np.nan
    for K in (0, 1):
        var[..., 3] = K
        for kw in (dict(), dict(iterations=8), dict(sigma_color=0.0, demodulate=False), dict(iterations=1, normal_squarings=0)):
            want = denoise_reference(rad, wt, ft, **kw)
            got = denoise_guided_reference(rad, wt, ft, var, sigma_variance=0.5, **kw)
            assert got.dtype == f32 and np.array_equal(got, want, equal_nan=True), (K, kw)
    # ... and so is a film whose variances are all non-finite
    var[..., 3] = 5
    var[..., 1] = np.inf
    assert np.array_equal(denoise_guided_reference(rad, wt, ft, var), denoise_reference(rad, wt, ft), equal_nan=True)


def test_guided_constant_film_with_zero_variance_is_unchanged():
    H, W = 19, 33
    ft = _flat_features(H, W, albedo=(0.5, 0.25, 0.125))
    wt = np.full((H, W), 4, f32)
    rad = np.tile(f32([1.0, 0.5, 0.75]) * f32(4), (H, W, 1))
    var = np.zeros((H, W, 4), f32)
    var[..., 3] = 3
    for kw in (dict(), dict(demodulate=False), dict(sigma_variance=0.25), dict(iterations=8, normal_squarings=0)):
        out = denoise_guided_reference(rad, wt, ft, var, **kw)
        assert out.dtype == f32 and np.array_equal(out, rad / wt[..., None]), kw


def test_guided_albedo_step_is_kept():
    H, W = 16, 40
    ft = _flat_features(H, W)
    ft[:, 20:, 0:3] = f32([0.9, 0.1, 0.1]) * f32(2)
    rad, wt, var = _noisy_film(H, W, spp=2, seed=5)
    base = np.empty((H, W, 3), f32)
    base[:, :20] = f32([1.0, 0.8, 0.6])
    base[:, 20:] = f32([3.6, 0.4, 0.4])
    zero_var = var.copy()
    zero_var[..., :3] = 0
    assert np.array_equal(denoise_guided_reference(base, wt, ft, zero_var), base / wt[..., None])
    out = denoise_guided_reference(base, wt, ft, var)
    noisy = base.copy()
    noisy[:, :20] *= np.random.default_rng(6).uniform(0.5, 1.5, (H, 20, 1)).astype(f32)
    out2 = denoise_guided_reference(noisy, wt, ft, var)
    assert np.array_equal(out2[:, 20:], out[:, 20:])       # noise on one side stays on its side
    assert not np.array_equal(out2[:, :20], noisy[:, :20] / f32(2))


def test_guided_holes_and_non_finite_values_neither_spread_nor_change():
    H, W = 24, 31
    ft = _flat_features(H, W)
    rad, wt, var = _noisy_film(H, W)
    base = denoise_guided_reference(rad, wt, ft, var)
    assert np.all(np.isfinite(base))
    rad2, wt2, var2 = rad.copy(), wt.copy(), var.copy()
    wt2[5:9, 7:12] = 0                       # a hole whose radiance and variance are garbage
    rad2[5:9, 7:12] = 1e30
    var2[5:9, 7:12, :3] = 1e30
    rad2[15, 20, 1] = np.nan
    rad2[3, 28] = np.inf
    var2[12, 5, 0] = np.nan                  # a pixel without hv: it keeps the shipped colour stop ...
    var2[20, 15, :3] = np.inf
    var2[18, 3, 3] = 1                       # ... as does one with a single batch
    out = denoise_guided_reference(rad2, wt2, ft, var2)
    assert np.all(out[5:9, 7:12] == 0)
    alb = f32([0.5, 0.4, 0.3])
    assert np.isnan(out[15, 20, 1]) and np.array_equal(out[15, 20, [0, 2]], (rad2[15, 20] / f32(4) / alb * alb)[[0, 2]])
    assert np.all(np.isinf(out[3, 28]))
    rest = np.ones((H, W), bool)
    rest[5:9, 7:12] = rest[15, 20] = rest[3, 28] = False
    assert np.all(np.isfinite(out[rest])) and np.all(out[rest] < 3.0)    # nothing of the 1e30, the NaN or the inf leaked
    assert not np.array_equal(out[rest], base[rest])                     # the taps were dropped
    for y, x in ((12, 5), (20, 15), (18, 3)):
        assert np.isfinite(out[y, x]).all() and not np.array_equal(out[y, x], base[y, x])
    # a pixel far from every planted value is untouched by them at one iteration (the stencil is 5 x 5)
    one = denoise_guided_reference(rad2, wt2, ft, var2, iterations=1)
    assert np.array_equal(one[22, 29], denoise_guided_reference(rad, wt, ft, var, iterations=1)[22, 29])
    assert np.all(denoise_guided_reference(rad, np.zeros((H, W), f32), ft, var) == 0)


def test_guided_variance_opens_and_closes_the_colour_stop():
    """More variance, more smoothing: the same noisy film comes out flatter when its variance record is
    larger, and a variance of 0 leaves a noisy film's hv pixels almost alone."""
    H, W = 20, 20
    ft = _flat_features(H, W)
    rad, wt, var = _noisy_film(H, W)
    lo, hi = var.copy(), var.copy()
    lo[..., :3] = 1e-6
    hi[..., :3] = 1.0
    spread = [float(denoise_guided_reference(rad, wt, ft, v).std()) for v in (lo, var, hi)]
    assert spread[0] > spread[1] > spread[2], spread


# --------------------------------------------------------------------------------------------- refusals
def test_guided_parameter_validation():
    p = denoise.guided_params()
    assert isinstance(p, capi.DenoiseGuidedParams) and C.sizeof(capi.DenoiseGuidedParams) == 48
    assert (p.base.iterations, p.base.normal_squarings, p.base.flags) == (5, 5, 0)
    assert f32(p.base.sigma_color) == f32(0.5) and f32(p.sigma_variance) == f32(denoise.DEFAULT_SIGMA_VARIANCE)
    assert 1.0 <= denoise.DEFAULT_SIGMA_VARIANCE <= 4.0
    assert "sigma_variance" not in denoise.DEFAULTS           # the shipped filter's parameters are unchanged
    assert denoise.guided_params(sigma_variance=0.5, iterations=3).base.iterations == 3
    for bad, msg in ((dict(sigma_variance=0.0), "sigma_variance"), (dict(sigma_variance=-1.0), "sigma_variance"),
                     (dict(sigma_variance=float("nan")), "sigma_variance"), (dict(sigma_variance=float("inf")), "sigma_variance"),
                     (dict(iterations=0), "iterations"), (dict(sigma_depth=0.0), "sigma_depth"), (dict(sigma=1.0), "unknown")):
        with pytest.raises(ValueError, match=msg):
            denoise.guided_params(**bad)
    with pytest.raises(ValueError, match="unknown"):
        denoise.params(sigma_variance=2.0)
    z = np.zeros((4, 4, 3), f32)
    ft, var = np.zeros((4, 4, 12), f32), np.zeros((4, 4, 4), f32)
    with pytest.raises(ValueError, match="sigma_variance"):
        capi.HipContext.denoise_guided(None, z, z[..., 0], ft, var, sigma_variance=0)
    with pytest.raises(ValueError, match="variance has shape"):
        capi.HipContext.denoise_guided(None, z, z[..., 0], ft, var[..., :3])
    with pytest.raises(ValueError, match="variance has shape"):
        capi.HipContext.denoise_guided(None, z, z[..., 0], ft, var[:3])
    with pytest.raises(ValueError, match="features have shape"):
        capi.HipContext.denoise_guided(None, z, z[..., 0], ft[..., :11], var)
    for name in ("akr_hip_render_variance", "akr_hip_render_variance_device", "akr_hip_denoise_guided",
                 "akr_hip_denoise_guided_device"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load_library(), name), f"{name} is not exported by the library"


def test_cli_denoise_variance_flag_validation_needs_no_gpu(tmp_path, capsys, monkeypatch):
    path = tmp_path / "s.akari"
    path.write_text(SDL.format(integrator="Path { spp: 8, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    ao = tmp_path / "ao.akari"
    ao.write_text(SDL.format(integrator="AO { spp: 8 }", out=tmp_path / "ao.pfm", mesh=CORNELL_MESH))

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(capi, "HipContext", no_device)

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            render.main([str(a) for a in argv])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err, err

    refused([ao, "--denoise", "--denoise-variance", "--pass-spp", "2"], "need the Path integrator")   # the scene is read for this one
    monkeypatch.setattr(scene, "load_scene_file", no_device)   # the others are refused before the scene is read
    refused([path, "--denoise-variance", "--pass-spp", "2"], "--denoise-variance needs --denoise")
    refused([path, "--denoise", "--denoise-variance"], "--denoise-variance needs one of --pass-spp, --preview, --adaptive")
    refused([path, "--denoise", "--denoise-variance", "--time-budget", "5"], "--denoise-variance needs one of")
    refused([path, "--denoise", "--denoise-variance", "--pass-spp", "2", "--gpus", "2"], "one GPU")
    refused([path, "--denoise", "--denoise-variance", "--preview", "--denoise-iters", "9"], "--denoise-iters needs 1..8")
    assert not (tmp_path / "o.pfm").exists()


def test_adapter_variance_calls_compile(tmp_path):
    exe = tmp_path / "variance_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "variance_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # no argument: nothing touches a device


# ------------------------------------------------------------------------------- the quality condition
def test_quality_condition_on_the_oracle_cornell():
    """relMSE against the oracle's 1024-spp render, Cornell 128 x 128, 2 feature samples, the doubling schedule
    1, 1, 2, 4, 8, ... (the oracle's renders of 1, 2, 4, ... spp are that session's films bit for bit), library
    defaults.  At 16 and 64 spp the guided result is below HALF the shipped filter's and below the raw
    film's; at 4 spp it is no worse than the shipped filter's.  (The specification's prototype: 0.00205 against
    0.00936 and 0.00884 at 16 spp, 0.00084 against 0.00920 and 0.00215 at 64, 0.00462 against 0.01013 at 4.)"""
    cs = scene.compile_scene(cornell((128, 128)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = py_oracle.OracleScene(cs, nodes, tris, capi)
    tiles = [(0, 0, 128, 128)]
    ft = frame_features(feature_reference(cs, orc, tiles, 2), tiles, 128, 128)
    ref_rad, ref_w, _ = orc.render(1024, 5)
    ref = ref_rad / ref_w[..., None]
    shipped_kw = dict(denoise.DEFAULTS)
    guided_kw = dict(denoise.DEFAULTS, sigma_variance=denoise.DEFAULT_SIGMA_VARIANCE)
    tr = VarianceTracker(128 * 128)
    seen = {}
    for spp in (1, 2, 4, 8, 16, 32, 64):
        rad, w, _ = orc.render(spp, 5)
        tr.update(frame_film(rad, w))
        if spp not in (4, 16, 64):
            continue
        var = tr.resolve().reshape(128, 128, 4)
        raw = relmse(rad / w[..., None], ref)
        shipped = relmse(denoise_reference(rad, w, ft, **shipped_kw), ref)
        guided = relmse(denoise_guided_reference(rad, w, ft, var, **guided_kw), ref)
        seen[spp] = (raw, shipped, guided)
        print(f"{spp} spp ({int(var[0, 0, 3])} batches): raw relMSE {raw:.5f}, shipped filter {shipped:.5f}, "
              f"guided {guided:.5f} ({guided / shipped:.3f} of shipped, {guided / raw:.3f} of raw)")
    for spp in (16, 64):
        raw, shipped, guided = seen[spp]
        assert guided < 0.5 * shipped and guided < raw, (spp, seen[spp])
    raw, shipped, guided = seen[4]
    assert guided <= shipped, (4, seen[4])
