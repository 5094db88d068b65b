"""The environment light's definition on the host: the restatement
tests/golden/env_restate.py against its committed vectors and against the mathematics it claims
(the solid-angle measure, an unbiased estimator, importance sampling that pays), the image readers,
the lat-long resampling, and the scene layers that carry an EnvironmentLight to the upload.
"""
import json
import struct
import sys

import numpy as np
import pytest

from akari_amd import envmap, film, scene
from conftest import CORNELL_MESH, GOLDEN

sys.path.insert(0, str(GOLDEN))
import env_restate as E  # noqa: E402
import make_env_golden as ME  # noqa: E402
import ref_restate as R  # noqa: E402

F = np.float32
KAT = json.loads((GOLDEN / "env_kat.json").read_text())


def f32(bits, k=None):
    a = np.array(bits, np.uint32).view(np.float32)
    return a if k is None else a.reshape(-1, k)


def same(got, want, what):
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    nan = np.isnan(got) & np.isnan(want)
    bad = np.count_nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad == 0, f"{what}: {bad} of {got.size} values differ from the committed vectors"


# ----------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_committed_vectors():
    k = KAT["decode"]
    same([E.decode(x, y)[0] + (E.decode(x, y)[1],) for x, y in f32(k["xy"], 2)], f32(k["out"]), "decode")
    for tag in ME.KAT_MAPS:
        k, env = KAT[tag], ME.kat_environment(tag)
        ev = [env.eval(R.vec(d)) for d in f32(k["dirs"], 3)]
        same([e[0] for e in ev], f32(k["eval_rgb"]), f"{tag} eval texel")
        same([e[1] for e in ev], f32(k["eval_pdf"]), f"{tag} eval pdf")
        assert [list(e[2]) for e in ev] == k["eval_ij"]
        sm = [env.sample(R.vec(u)) for u in f32(k["u"], 2)]
        same([s[0] for s in sm], f32(k["sample_dir"]), f"{tag} sample direction")
        same([s[1] for s in sm], f32(k["sample_rgb"]), f"{tag} sampled texel")
        same([s[2] for s in sm], f32(k["sample_pdf"]), f"{tag} sample pdf")
        assert [list(s[3]) for s in sm] == k["sample_ij"]
        same(env.marginal.cdf, f32(k["marginal_cdf"]), f"{tag} marginal CDF")


def test_decode_and_encode_at_axes_fold_line_and_corners():
    v = lambda *a: tuple(float(x) for x in a)
    axes = {(1, 0): (1, 0, 0), (-1, 0): (-1, 0, 0), (0, 1): (0, 1, 0), (0, -1): (0, -1, 0), (0, 0): (0, 0, 1)}
    for (x, y), d in axes.items():
        got, ln = E.decode(F(x), F(y))
        assert v(*got) == v(*d) and ln == 1
    for x, y in ((1, 1), (-1, 1), (1, -1), (-1, -1)):            # the four corners are the -z pole
        got, ln = E.decode(F(x), F(y))
        assert v(*got) == (0.0, 0.0, -1.0) and ln == 1
    for x, y in ((0.5, 0.5), (-0.25, 0.75), (0.75, -0.25), (-0.5, -0.5)):   # the fold line is the equator z = 0
        got, _ = E.decode(F(x), F(y))
        assert got[2] == 0 and np.sign(got[0]) == np.sign(x) and np.sign(got[1]) == np.sign(y)
    # encode: +z is the centre, -z a corner (sgn 0 = +1: the (+, +) one), the other axes the edge midpoints
    for n in (1, 2, 5, 8):
        assert E.encode(R.vec((0, 0, 1)), n)[:2] == (n // 2, n // 2)
        assert E.encode(R.vec((0, 0, -1)), n)[:2] == (n - 1, n - 1)
        assert E.encode(R.vec((1, 0, 0)), n)[:2] == (n - 1, n // 2)
        assert E.encode(R.vec((-1, 0, 0)), n)[:2] == (0, n // 2)
        assert E.encode(R.vec((0, 1, 0)), n)[:2] == (n // 2, n - 1)
        assert E.encode(R.vec((0, -1, 0)), n)[:2] == (n // 2, 0)
    # the fold's signs: a direction below the equator lands in its own quadrant's corner region
    i, j, _ = E.encode(R.normalize(R.vec((-0.2, 0.3, -0.9))), 8)
    assert i < 4 <= j and (i < 2 or j >= 6)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_encode_of_every_texel_centre_is_that_texel(n):
    for j in range(n):
        for i in range(n):
            d, ln = E.decode(E.texel_point(i, 0.5, n), E.texel_point(j, 0.5, n))
            ti, tj, ln2 = E.encode(d, n)
            assert (ti, tj) == (i, j)
            assert abs(float(ln2) - float(ln)) <= 4 * np.finfo(np.float32).eps * float(ln)


def test_solid_angle_measure_integrates_to_four_pi():
    """d omega = dx dy / |q|^3: a midpoint quadrature over the square, in double (the exact measure)."""
    m = 2000
    t = (np.arange(m) + 0.5) / m * 2 - 1
    x, y = np.meshgrid(t, t)
    z = 1 - np.abs(x) - np.abs(y)
    fx, fy = np.where(z < 0, 1 - np.abs(y), np.abs(x)), np.where(z < 0, 1 - np.abs(x), np.abs(y))
    total = ((fx * fx + fy * fy + z * z) ** -1.5).sum() * (2.0 / m) ** 2
    assert abs(total - 4 * np.pi) < 1e-5 * 4 * np.pi, total


def _draws(n, seed):
    return np.random.default_rng(seed).random((n, 2)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_furnace_constant_map(n):
    """A constant map over a diffuse point: the mean of cos+ / pi / p_omega is 1, within 5 standard errors
    taken from the same samples."""
    env = E.Environment(np.full((n, n, 3), 0.7, np.float32))
    up = R.vec((0.3, 0.9, -0.2))
    up = R.normalize(up)
    est = []
    for u in _draws(3000, 100 + n):
        wi, _, pdf, _ = env.sample(R.vec(u))
        assert pdf > 0
        est.append(max(0.0, float(R.dot(wi, up))) / np.pi / float(pdf))
    est = np.array(est)
    se = est.std(ddof=1) / np.sqrt(len(est))
    assert abs(est.mean() - 1.0) <= 5 * se, (est.mean(), se)


def test_importance_sampling_beats_uniform_on_the_bright_texel_map():
    spec = ME.env_spec("sky")
    env = E.Environment(spec["map"])
    up = R.vec((0.0, 1.0, 0.0))
    lum = lambda c: float(R.dot(c, E.LUMA))
    imp, uni = [], []
    for u in _draws(3000, 7):
        wi, Le, pdf, _ = env.sample(R.vec(u))
        imp.append(lum(Le) * max(0.0, float(R.dot(wi, up))) / np.pi / float(pdf))
        z = 1 - 2 * float(u[0])
        r, ph = np.sqrt(max(0.0, 1 - z * z)), 2 * np.pi * float(u[1])
        d = R.vec((r * np.cos(ph), z, r * np.sin(ph)))
        uni.append(lum(env.eval(d)[0]) * max(0.0, float(R.dot(d, up))) / np.pi * 4 * np.pi)
    imp, uni = np.array(imp), np.array(uni)
    se = np.hypot(imp.std(ddof=1), uni.std(ddof=1)) / np.sqrt(len(imp))
    assert abs(imp.mean() - uni.mean()) <= 5 * se            # the same integral
    assert imp.var(ddof=1) < uni.var(ddof=1), (imp.var(ddof=1), uni.var(ddof=1))


def test_zero_rows_and_columns_are_never_sampled_and_have_pdf_zero():
    env = ME.kat_environment("n8")          # row 2 and column 7 are black
    for u in _draws(400, 3):
        _, _, pdf, (i, j) = env.sample(R.vec(u))
        assert j != 2 and i != 7 and pdf > 0
    assert env.pdf(3, 2, F(1.0)) == 0 and env.pdf(7, 4, F(1.0)) == 0
    # u = 1.0 clamps into the black last column: the sample is refused by its pdf, not by a NaN
    _, _, pdf, (i, _) = env.sample((F(1.0), F(0.5)))
    assert i == 7 and pdf == 0


# ----------------------------------------------------------------------------- readers, layouts
def test_pfm_round_trip_with_the_film_writer(tmp_path):
    img = np.random.default_rng(1).random((5, 7, 3)).astype(np.float32)
    film.write_pfm(tmp_path / "a.pfm", img, np.ones((5, 7), np.float32))
    assert np.array_equal(envmap.read_pfm(tmp_path / "a.pfm"), img)
    assert np.array_equal(envmap.read_map(tmp_path / "a.pfm"), img)
    # big endian, and grey
    (tmp_path / "b.pfm").write_bytes(b"PF\n7 5\n1.0\n" + np.ascontiguousarray(img[::-1], ">f4").tobytes())
    assert np.array_equal(envmap.read_pfm(tmp_path / "b.pfm"), img)
    (tmp_path / "g.pfm").write_bytes(b"Pf\n7 5\n-1.0\n" + np.ascontiguousarray(img[::-1, :, 0], "<f4").tobytes())
    assert np.array_equal(envmap.read_pfm(tmp_path / "g.pfm"), np.repeat(img[..., :1], 3, axis=2))
    with pytest.raises(envmap.EnvMapError):
        (tmp_path / "c.pfm").write_bytes(b"PF\n7 5\n-1.0\n" + b"\0" * 10)
        envmap.read_pfm(tmp_path / "c.pfm")
    np.save(tmp_path / "n.npy", img)
    assert np.array_equal(envmap.read_map(tmp_path / "n.npy"), img)
    with pytest.raises(envmap.EnvMapError, match="unsupported"):
        envmap.read_map(tmp_path / "x.exr")


def test_hdr_flat_and_run_length_rows():
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    # flat: 2 x 2 pixels; (128, 64, 32, 129) is (1, 0.5, 0.25)
    px = bytes([128, 64, 32, 129, 0, 0, 0, 0, 255, 255, 255, 128, 128, 0, 0, 136])
    img = envmap.decode_hdr(head + b"-Y 2 +X 2\n" + px)
    assert img.shape == (2, 2, 3)
    assert np.array_equal(img[0, 0], F([1.0, 0.5, 0.25])) and not img[0, 1].any()
    assert np.array_equal(img[1, 0], F([255 / 256] * 3)) and np.array_equal(img[1, 1], F([128.0, 0, 0]))
    # new-style RLE, one row of 8: r = run of 8 x 128; g = literal 8; b = run 5 x 0 + literal 3; e = run 8 x 129
    row = bytes([2, 2, 0, 8]) + bytes([128 + 8, 128]) + bytes([8, 0, 32, 64, 96, 128, 160, 192, 224]) \
        + bytes([128 + 5, 0, 3, 64, 128, 192]) + bytes([128 + 8, 129])
    img = envmap.decode_hdr(head + b"-Y 1 +X 8\n" + row)
    assert img.shape == (1, 8, 3)
    assert np.array_equal(img[0, :, 0], np.ones(8, np.float32))
    assert np.array_equal(img[0, :, 1], np.arange(8, dtype=np.float32) * 32 / 128)
    assert np.array_equal(img[0, :, 2], F([0, 0, 0, 0, 0, 0.5, 1.0, 1.5]))
    with pytest.raises(envmap.EnvMapError):
        envmap.decode_hdr(head + b"-Y 1 +X 8\n" + row[:-1])
    with pytest.raises(envmap.EnvMapError):
        envmap.decode_hdr(b"P6\n")


def test_latlong_to_octahedral():
    const = np.full((16, 32, 3), [0.25, 0.5, 2.0], np.float32)
    out = envmap.latlong_to_octahedral(const, 5)
    assert out.shape == (5, 5, 3) and np.array_equal(out, np.broadcast_to(F([0.25, 0.5, 2.0]), (5, 5, 3)))
    # up is +y: a bright top row of the lat-long image is the texels around (x, y) = (0, 1) ... the +y axis
    img = np.zeros((16, 32, 3), np.float32)
    img[:2] = 1.0
    out = envmap.latlong_to_octahedral(img, 8)
    i, j, _ = E.encode(R.vec((0.01, 1.0, 0.01)), 8)
    assert out[j, i, 0] > 0.5 and out[0, 4, 0] == 0           # and -y stays dark
    # a one-texel sun is not missed by a coarse map (area average, not a point lookup)
    img = np.zeros((64, 128, 3), np.float32)
    img[20, 37] = 1000.0
    assert envmap.latlong_to_octahedral(img, 4, supersample=32).max() > 0
    sky = envmap.procedural_sky(8)
    assert sky.shape == (8, 8, 3) and np.all(np.isfinite(sky)) and np.all(sky >= 0) and sky.max() > 10 * np.median(sky)


def test_rotation_matrix():
    assert np.array_equal(envmap.rotation_matrix((0, 0, 0)), np.eye(3))
    r = envmap.rotation_matrix((0, 90, 0))            # d_world = M d_env turns +z to +x; R = M^T
    assert np.allclose(r.T @ [0, 0, 1], [1, 0, 0]) and np.allclose(r @ r.T, np.eye(3))
    m = ME.rotation((1, 2, 3), 40)
    assert np.array_equal(envmap.rotation_matrix(m), m.T)
    with pytest.raises(envmap.EnvMapError):
        envmap.rotation_matrix((1, 2))


# ----------------------------------------------------------------------------- scene layers
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    environment: EnvironmentLight {{ image: "sky.npy", layout: "{layout}", scale: [1, 2, 3], rotation: [0, 90, 0],
                                    select_prob: 0.25, resolution: 6 }},
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def test_parser_and_compile_scene_carry_the_node(tmp_path):
    img = np.random.default_rng(2).random((8, 16, 3)).astype(np.float32)
    np.save(tmp_path / "sky.npy", img)
    (tmp_path / "s.akari").write_text(SDL.format(layout="latlong", mesh=CORNELL_MESH))
    sc = scene.load_scene_file(tmp_path / "s.akari")
    env = sc.environment
    assert isinstance(env, scene.EnvironmentLight) and env.layout == "latlong" and np.array_equal(env.image, img)
    assert tuple(env.scale) == (1.0, 2.0, 3.0) and env.select_prob == 0.25 and env.resolution == 6
    cs = scene.compile_scene(sc)
    ce = cs.environment
    assert ce.map.shape == (6, 6, 3) and ce.map.dtype == np.float32
    assert np.array_equal(ce.map, envmap.latlong_to_octahedral(img, 6))
    assert np.array_equal(ce.scale, F([1, 2, 3])) and ce.select_prob == 0.25
    assert np.array_equal(ce.world_to_env, envmap.rotation_matrix((0, 90, 0)).astype(np.float32))
    # the octahedral layout is taken as it is; a scene without the node compiles to none, as before
    np.save(tmp_path / "sky.npy", img[:, :8])
    (tmp_path / "o.akari").write_text(SDL.format(layout="octahedral", mesh=CORNELL_MESH))
    assert np.array_equal(scene.compile_scene(scene.load_scene_file(tmp_path / "o.akari")).environment.map, img[:, :8])
    sc.environment = None
    assert scene.compile_scene(sc).environment is None
    (tmp_path / "bad.akari").write_text(SDL.format(layout="latlong", mesh=CORNELL_MESH).replace("sky.npy", "none.npy"))
    with pytest.raises(scene.SdlError):
        scene.load_scene_file(tmp_path / "bad.akari")


def test_fingerprint_follows_the_environment():
    from akari_amd import progressive
    sc = scene.cornell_scene(CORNELL_MESH, resolution=(8, 8))
    plain = progressive.scene_fingerprint(scene.compile_scene(sc))
    sc.environment = scene.EnvironmentLight(np.ones((2, 2, 3), np.float32))
    a = progressive.scene_fingerprint(scene.compile_scene(sc))
    sc.environment.scale = (2.0, 2.0, 2.0)
    b = progressive.scene_fingerprint(scene.compile_scene(sc))
    assert len({plain, a, b}) == 3


def test_refusals():
    sc = scene.cornell_scene(CORNELL_MESH, resolution=(8, 8))      # has area lights
    good = np.ones((4, 4, 3), np.float32)

    def refused(match, image=good, **kw):
        sc.environment = scene.EnvironmentLight(image, **kw)
        with pytest.raises(ValueError, match=match):
            scene.compile_scene(sc)

    refused("N x N", np.zeros((0, 0, 3), np.float32))                       # N = 0
    refused("N x N", np.ones((4, 5, 3), np.float32))
    refused("resolution", np.ones((4, 8, 3), np.float32), layout="latlong", resolution=4096)
    neg = good.copy()
    neg[1, 2, 0] = -0.5
    refused("negative", neg)
    nan = good.copy()
    nan[0, 0, 1] = np.nan
    refused("non-finite", nan)
    refused("black", np.zeros((4, 4, 3), np.float32))
    refused("black", good, scale=(0.0, 0.0, 0.0))
    refused("select_prob", good, select_prob=0.0)
    refused("select_prob", good, select_prob=1.0)
    refused("layout", good, layout="cube")
    sc.environment = scene.EnvironmentLight(good)
    assert scene.compile_scene(sc).environment.select_prob == 0.5
