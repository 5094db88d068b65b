"""Host side of the feature buffers and the a-trous filter of the film: the NumPy f32
restatements that the GPU tests compare against (feature_reference, denoise_reference), the filter's
invariants on hand-made films, the parameter and CLI refusals, and the quality condition of the
specification on the oracle's Cornell box.  No GPU needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, denoise, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell, slot_pixels

f32 = np.float32
NO_HIT = 0xFFFFFFFF


# ----------------------------------------------------------------------------- akr_math.h in NumPy f32
def _dot(a, b):
    s = a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    s = s + a[..., 2] * b[..., 2]
    return s


def _cross(a, b):
    return np.stack([(a[..., 1] * b[..., 2]) - (a[..., 2] * b[..., 1]), (a[..., 2] * b[..., 0]) - (a[..., 0] * b[..., 2]),
                     (a[..., 0] * b[..., 1]) - (a[..., 1] * b[..., 0])], axis=-1)


def _rmax(a, b):
    return np.where(a < b, b, a)


def _lerp3(a, b, c, u, v):
    w = f32(1.0) - u - v
    return (a * w[..., None] + b * u[..., None]) + c * v[..., None]


def _lcg_next(s):
    """LCGSampler::next1d on one uint32 state: (new state, draw)."""
    s = (1103515245 * int(s) + 12345) & 0xFFFFFFFF
    return s, f32(np.uint32(s)) / f32(0xFFFFFFFF)


def _tex_eval(cs, ti, tc):
    """Texture::evaluate (kernels.hip tex_eval): a constant, or the texel with fmod wrap and clamp."""
    t = cs.textures[ti]
    if t.type == capi.TEX_CONSTANT:
        return np.array(list(t.value), f32)
    img = cs.images[t.image]
    h, w = img.shape[:2]
    x = np.fmod(f32(tc[0]), f32(1.0))
    y = f32(1.0) - np.fmod(f32(tc[1]), f32(1.0))
    ix, iy = int(f32(x * f32(w))), int(f32(y * f32(h)))
    ix, iy = min(max(ix, 0), w - 1), min(max(iy, 0), h - 1)
    return np.asarray(img[iy, ix, :3], f32)


def _albedo(cs, mid, tc, seed):
    """The colour of the material the path tracer would shade: Material::select_material's Mix walk
    (shade_hit_tab) with the next draw of a copy of the chain as the selector."""
    if mid < 0:
        return np.zeros(3, f32)
    mat = cs.materials[mid]
    _, sel_u = _lcg_next(seed)
    while mat.type == capi.MAT_MIX:
        frac = _tex_eval(cs, mat.fraction, tc)[0]
        with np.errstate(all="ignore"):
            if sel_u < frac:
                sel_u = sel_u / frac
                mat = cs.materials[mat.second]
            else:
                sel_u = (sel_u - frac) / (f32(1.0) - frac)
                mat = cs.materials[mat.first]
    if mat.type in (capi.MAT_DIFFUSE, capi.MAT_GLOSSY, capi.MAT_EMISSIVE):
        return _tex_eval(cs, mat.color, tc)
    return np.zeros(3, f32)


def feature_reference(cs, orc, tiles, spp, exact_cull=False):
    """The feature pass of include/akr_hip.h restated: packed records [n, 12] in tile order, from
    py_oracle.camera_ray (four draws per sample of the slot's own chain), OracleScene.trace and f32 NumPy
    in the operation order of akr_math.h."""
    W, H = (int(v) for v in cs.camera.resolution)
    ys, xs = slot_pixels(tiles, W, H)
    n = len(ys)
    rec = np.zeros((n, 12), f32)
    seed = [(int(x) + int(y) * W) & 0xFFFFFFFF for x, y in zip(xs, ys)]
    verts = np.asarray(cs.vertices, f32)
    idx = np.asarray(cs.indices)
    tcs = np.asarray(cs.texcoords, f32).reshape(-1, 3, 2)
    for _ in range(spp):
        rays = np.zeros(n, capi.RAY_DTYPE)
        for i in range(n):
            rays[i], seed[i] = py_oracle.camera_ray(cs.camera, capi, int(xs[i]), int(ys[i]), seed[i])
        hits, _, _ = orc.trace(rays, exact_cull=exact_cull)
        hit = np.nonzero(hits["gid"] != NO_HIT)[0]
        if not len(hit):
            continue
        gid = hits["gid"][hit].astype(np.int64)
        u, v, t = hits["u"][hit], hits["v"][hit], hits["t"][hit]
        v0, v1, v2 = (verts[idx[gid, k]] for k in range(3))
        with np.errstate(all="ignore"):
            p = _lerp3(v0, v1, v2, u, v)
            c = _cross(v1 - v0, v2 - v0)
            ng = c / np.sqrt(_dot(c, c))[:, None]
            ng = np.where((_dot(ng, rays["d"][hit]) > 0)[:, None], -ng, ng)
            w = f32(1.0) - u - v
            tc = np.stack([(tcs[gid, 0, k] * w + tcs[gid, 1, k] * u) + tcs[gid, 2, k] * v for k in range(2)], axis=-1)
        alb = np.stack([_albedo(cs, int(cs.matid[g]), tc[j], seed[i]) for j, (g, i) in enumerate(zip(gid, hit))])
        add = np.zeros((len(hit), 12), f32)
        add[:, 0:3], add[:, 3] = alb, 1
        add[:, 4:7], add[:, 7] = ng, t
        add[:, 8:11] = p
        assert p.dtype == ng.dtype == tc.dtype == f32
        rec[hit] = rec[hit] + add
    return rec


def frame_features(rec, tiles, W, H):
    """Packed records added into a full frame [H, W, 12], as the host form does."""
    ys, xs = slot_pixels(tiles, W, H)
    out = np.zeros((H, W, 12), f32)
    np.add.at(out, (ys, xs), rec)
    return out


def denoise_reference(radiance, weight, features, iterations=5, normal_squarings=5, sigma_depth=0.02, sigma_albedo=0.3,
                      sigma_color=0.5, demodulate=True):
    """The filter of include/akr_hip.h restated: 25 shifted arrays per iteration, accumulated in tap
    order (j outer, k inner) with np.where; f32, left to right."""
    rad, wt, ft = (np.asarray(a, f32) for a in (radiance, weight, features))
    H, W = wt.shape
    sd, sa, scol = f32(sigma_depth), f32(sigma_albedo), f32(sigma_color)
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
        Y, X = np.mgrid[0:H, 0:W]
        hk = [f32(1) / f32(16), f32(1) / f32(4), f32(3) / f32(8), f32(1) / f32(4), f32(1) / f32(16)]
        zden = sd * t
        for i in range(int(iterations)):
            s = 1 << i
            sc = scol * (one / f32(1 << i))
            sc2 = sc * sc
            fin = np.isfinite(I).all(axis=-1)
            num = np.zeros((H, W, 3), f32)
            den = np.zeros((H, W), f32)
            for j in range(5):
                for k in range(5):
                    qy, qx = Y + (j - 2) * s, X + (k - 2) * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    Iq = I[qy, qx]
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
                        if scol > 0:
                            d = Iq - I
                            wc = one / (one + _dot(d, d) / sc2)
                        else:
                            wc = np.ones((H, W), f32)
                    w = ((hk[j] * hk[k]) * g) * wc
                    assert w.dtype == f32
                    num = np.where(accept[..., None], num + w[..., None] * Iq, num)
                    den = np.where(accept, den + w, den)
            res = np.where((den > 0)[..., None], num / den[..., None], I)
            res = np.where(fin[..., None], res, I)
            I = np.where(valid[..., None], res, zero).astype(f32)
        out = np.where(valid[..., None], I * m, zero).astype(f32)
    return out


def relmse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


# ----------------------------------------------------------------------------------------- filter tests
def _flat_features(H, W, albedo=(0.5, 0.4, 0.3), spp=2):
    """A fronto-parallel plane at depth 5 seen through every pixel: `spp` hits per pixel."""
    ft = np.zeros((H, W, 12), f32)
    ft[..., 0:3] = f32(albedo) * f32(spp)
    ft[..., 3] = spp
    ft[..., 6] = spp                       # normal (0, 0, 1)
    ft[..., 7] = f32(5.0) * f32(spp)
    Y, X = np.mgrid[0:H, 0:W]
    ft[..., 8], ft[..., 9], ft[..., 10] = X * f32(0.01 * spp), Y * f32(0.01 * spp), f32(-5.0 * spp)
    return ft


def test_constant_film_over_constant_features_is_unchanged():
    H, W = 19, 33
    ft = _flat_features(H, W, albedo=(0.5, 0.25, 0.125))
    wt = np.full((H, W), 4, f32)
    rad = np.tile(f32([1.0, 0.5, 0.75]) * f32(4), (H, W, 1))   # mean (1, 0.5, 0.75): I = (2, 2, 6), exact
    for kw in (dict(), dict(demodulate=False), dict(sigma_color=0.0), dict(iterations=8, normal_squarings=0)):
        out = denoise_reference(rad, wt, ft, **kw)
        assert out.dtype == f32 and np.array_equal(out, rad / wt[..., None]), kw


def test_albedo_step_is_kept_exactly():
    H, W = 16, 40
    ft = _flat_features(H, W)
    ft[:, 20:, 0:3] = f32([0.9, 0.1, 0.1]) * f32(2)            # |da| = 0.9 > sigma_albedo: wa = 0 across the step
    wt = np.full((H, W), 2, f32)
    rng = np.random.default_rng(5)
    rad = np.empty((H, W, 3), f32)
    rad[:, :20] = f32([1.0, 0.8, 0.6])                          # constant lighting 1 on each side ...
    rad[:, 20:] = f32([3.6, 0.4, 0.4])                          # ... and 2 on the other: I is 1 | 2 after demodulation
    out = denoise_reference(rad, wt, ft, sigma_color=0.0)
    assert np.array_equal(out, rad / wt[..., None])
    # noise on one side stays on its side: the other side's pixels do not change at all
    noisy = rad.copy()
    noisy[:, :20] *= rng.uniform(0.5, 1.5, (H, 20, 1)).astype(f32)
    out2 = denoise_reference(noisy, wt, ft, sigma_color=0.0)
    assert np.array_equal(out2[:, 20:], out[:, 20:])
    assert not np.array_equal(out2[:, :20], noisy[:, :20] / f32(2))


def test_holes_and_non_finite_pixels_neither_spread_nor_change():
    H, W = 24, 31
    ft = _flat_features(H, W)
    rng = np.random.default_rng(9)
    wt = np.full((H, W), 4, f32)
    rad = (rng.uniform(0.5, 1.5, (H, W, 3)) * 4).astype(f32)
    base = denoise_reference(rad, wt, ft)
    rad2, wt2 = rad.copy(), wt.copy()
    wt2[5:9, 7:12] = 0                      # a hole whose radiance is garbage
    rad2[5:9, 7:12] = 1e30
    rad2[15, 20, 1] = np.nan
    rad2[3, 28] = np.inf
    out = denoise_reference(rad2, wt2, ft)
    assert np.all(out[5:9, 7:12] == 0)
    assert np.isnan(out[15, 20, 1]) and np.array_equal(out[15, 20, [0, 2]], (rad2[15, 20] / f32(4) / f32([0.5, 0.4, 0.3])
                                                                             * f32([0.5, 0.4, 0.3]))[[0, 2]])
    assert np.all(np.isinf(out[3, 28]))
    rest = np.ones((H, W), bool)
    rest[5:9, 7:12] = rest[15, 20] = rest[3, 28] = False
    assert np.all(np.isfinite(out[rest]))
    assert np.all(out[rest] < 3.0)          # nothing of the 1e30 or the inf leaked
    assert np.all(np.isfinite(base)) and not np.array_equal(out[rest], base[rest])   # the taps were dropped
    # a film with no valid pixel at all
    assert np.all(denoise_reference(rad, np.zeros((H, W), f32), ft) == 0)
    # pixels without hits filter among themselves (g = 1) and never with pixels that have hits (g = 0)
    ft3 = ft.copy()
    ft3[:, :10] = 0
    out3 = denoise_reference(rad, wt, ft3, sigma_color=0.0, demodulate=False)
    rad4 = rad.copy()
    rad4[:, 10:] *= f32(3)
    out4 = denoise_reference(rad4, wt, ft3, sigma_color=0.0, demodulate=False)
    assert np.array_equal(out3[:, :10], out4[:, :10])


def test_parameter_validation():
    p = denoise.params()
    assert (p.iterations, p.normal_squarings, p.flags) == (5, 5, 0)
    assert f32(p.sigma_depth) == f32(0.02) and f32(p.sigma_albedo) == f32(0.3) and f32(p.sigma_color) == f32(0.5)
    assert denoise.params(demodulate=False).flags == capi.DENOISE_NO_DEMODULATE
    assert denoise.params(sigma_color=-1.0, iterations=8, normal_squarings=0).iterations == 8
    for bad, msg in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
                     (dict(iterations=2.5), "iterations"), (dict(normal_squarings=-1), "normal_squarings"),
                     (dict(normal_squarings=9), "normal_squarings"), (dict(sigma_depth=0.0), "sigma_depth"),
                     (dict(sigma_depth=float("nan")), "sigma_depth"), (dict(sigma_albedo=-0.1), "sigma_albedo"),
                     (dict(sigma_color=float("nan")), "sigma_color"), (dict(sigma=1.0), "unknown")):
        with pytest.raises(ValueError, match=msg):
            denoise.params(**bad)
    # HipContext.denoise refuses them before it touches the context (self is never used)
    z = np.zeros((4, 4, 3), f32)
    with pytest.raises(ValueError, match="iterations"):
        capi.HipContext.denoise(None, z, z[..., 0], np.zeros((4, 4, 12), f32), iterations=0)
    with pytest.raises(ValueError, match="features have shape"):
        capi.HipContext.denoise(None, z, z[..., 0], np.zeros((4, 4, 11), f32))
    with pytest.raises(ValueError, match="radiance has shape"):
        capi.HipContext.denoise(None, z[:3], z[..., 0], np.zeros((4, 4, 12), f32))
    with pytest.raises(ValueError, match="non-empty"):
        capi.HipContext.denoise(None, np.zeros((0, 4, 3), f32), np.zeros((0, 4), f32), np.zeros((0, 4, 12), f32))
    # the structs the bindings pass match the header's layout, and the library exports the calls
    assert C.sizeof(capi.FeatureParams) == 8 and C.sizeof(capi.DenoiseParams) == 32
    for name in ("akr_hip_render_features", "akr_hip_render_features_device", "akr_hip_denoise", "akr_hip_denoise_device"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load_library(), name), f"{name} is not exported by the library"


def test_split_features():
    ft = np.zeros((2, 3, 12), f32)
    ft[0, 0] = [1.0, 2.0, 3.0, 2.0, 0.0, 0.0, -2.0, 10.0, 1.0, 1.0, 1.0, 0.0]
    albedo, normal, depth, cov = denoise.split_features(ft)
    assert albedo.shape == normal.shape == (2, 3, 3) and depth.shape == cov.shape == (2, 3)
    assert np.array_equal(albedo[0, 0], f32([0.5, 1.0, 1.5])) and np.array_equal(normal[0, 0], f32([0, 0, -1]))
    assert depth[0, 0] == 5 and cov[0, 0] == 2
    assert not albedo[1].any() and not normal[0, 1:].any() and not depth[1].any() and cov.sum() == 2
    with pytest.raises(ValueError):
        denoise.split_features(np.zeros((2, 3, 11), f32))


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: {integrator},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def test_cli_denoise_flag_validation_needs_no_gpu(tmp_path, capsys, monkeypatch):
    path = tmp_path / "s.akari"
    path.write_text(SDL.format(integrator="Path { spp: 8, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(capi, "HipContext", no_device)
    monkeypatch.setattr(scene, "load_scene_file", no_device)   # refused before the scene is read

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            render.main([str(a) for a in argv])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err, err

    refused([path, "--denoise", "--denoise-iters", "0"], "--denoise-iters needs 1..8")
    refused([path, "--denoise", "--denoise-iters", "9"], "--denoise-iters needs 1..8")
    refused([path, "--denoise-iters", "3"], "--denoise-iters needs --denoise")
    refused([path, "--denoise", "--feature-spp", "0"], "--feature-spp needs at least one sample")
    refused([path, "--feature-spp", "2"], "--feature-spp needs --denoise or --aov")
    refused([path, "--aov", ""], "--aov needs a file prefix")
    assert not (tmp_path / "o.pfm").exists()


def test_adapter_denoise_calls_compile(tmp_path):
    exe = tmp_path / "denoise_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "denoise_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # no argument: nothing touches a device


# ------------------------------------------------------------------------------- the quality condition
@pytest.fixture(scope="module")
def cornell128():
    """Oracle Cornell 128x128, default camera: the scene, its oracle and the 2-sample feature frame."""
    cs = scene.compile_scene(cornell((128, 128)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = py_oracle.OracleScene(cs, nodes, tris, capi)
    tiles = [(0, 0, 128, 128)]
    ft = frame_features(feature_reference(cs, orc, tiles, 2), tiles, 128, 128)
    ft.setflags(write=False)
    return cs, orc, ft


def test_feature_reference_classes_of_pixel(cornell128):
    """The default Cornell camera sees past the box: the frame holds pixels without a hit, partly
    covered and fully covered ones, and the records are what split_features expects."""
    _, _, ft = cornell128
    hits = ft[..., 3]
    assert set(np.unique(hits)) == {0.0, 1.0, 2.0}
    assert np.count_nonzero(hits == 0) == 1169 and np.count_nonzero(hits == 1) == 203   # the specification's counts
    assert not ft[hits == 0].any() and not ft[..., 11].any()
    albedo, normal, depth, cov = denoise.split_features(ft)
    full = hits == 2
    norm = np.linalg.norm(normal[full], axis=-1)   # a mean of unit normals: 1 unless the two samples hit two faces
    assert np.all(depth[full] > 0) and np.all(norm < 1 + 1e-5) and np.count_nonzero(np.abs(norm - 1) < 1e-5) > 14000
    assert np.all((albedo >= 0) & (albedo <= 17.0))
    # the lamp's albedo is its emission colour, whichever way it faces
    assert np.any(np.all(albedo == f32([17.0, 12.0, 4.0]), axis=-1))


def test_quality_condition_on_the_oracle_cornell(cornell128):
    """relMSE = mean (x - ref)^2 / (ref^2 + 0.01) against the oracle's 1024-spp render: the 4-spp film
    filtered with the library's default parameters is below HALF the raw film's (the specification's
    prototype: ratio 0.28 at 4 spp, 0.11 at 1 spp)."""
    cs, orc, ft = cornell128
    ref_rad, ref_w, _ = orc.render(1024, 5)
    ref = ref_rad / ref_w[..., None]
    kw = {k: v for k, v in denoise.DEFAULTS.items()}
    for spp, prototype in ((4, 0.28), (1, 0.11)):
        rad, w, _ = orc.render(spp, 5)
        raw = relmse(rad / w[..., None], ref)
        out = denoise_reference(rad, w, ft, **kw)
        filt = relmse(out, ref)
        print(f"{spp} spp: raw relMSE {raw:.4f}, filtered {filt:.4f}, ratio {filt / raw:.3f} (prototype {prototype})")
        assert filt < 0.5 * raw, (spp, raw, filt)
