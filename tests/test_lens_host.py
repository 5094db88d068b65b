"""The thin-lens camera's definition, on the host.

tests/golden/lens_restate.py restates the lens branch of the reference's kernel camera (kernel/camera.h:67-86)
and the AO integrator's pixel loop; tests/golden/make_lens_golden.py ran it into lens_golden_<scene>.npz and
lens_kat.json.  Here: the committed files are what the restatement gives, the lens switched off is
ref_restate.Camera bit for bit, the rays of one film point meet on the plane of focus, a plane in focus renders
as through a pinhole and one out of focus does not, the AO restatement equals the oracle's with the lens off,
and the host side (parser, compiler, fingerprint, command line, autofocus arithmetic) carries the two values.
"""
import json
import sys

import numpy as np
import pytest

from akari_amd import lens, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN
from test_path_kat_host import check, oracle_scene

sys.path.insert(0, str(GOLDEN))
import lens_restate as L  # noqa: E402
import make_lens_golden as ML  # noqa: E402
import ref_restate as R  # noqa: E402
import helpers  # noqa: E402
import lens_scenes  # noqa: E402

F = np.float32
KAT = json.loads((GOLDEN / "lens_kat.json").read_text())
# the pinhole Cornell fixture at 16 x 8 as progressive.scene_fingerprint gave it before the camera had a lens
PINHOLE_FINGERPRINT = "75f586e80c166758100c19c06261a5dc3f28a31c5a0e90c028307af52c2c94d2"


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def kat_camera(name):
    c = KAT["cameras"][name]
    return L.LensCamera(c["position"], c["rotation"], c["fov"], c["resolution"], f32([c["lens_radius"]])[0],
                        f32([c["focal_distance"]])[0])


# ----------------------------------------------------------------------------- goldens and KATs
def test_kat_is_the_restatements():
    assert set(KAT["cameras"]) == set(ML.KAT_CAMERAS)
    cams = {k: kat_camera(k) for k in KAT["cameras"]}
    assert len(KAT["generate_ray"]) == len(cams) * 3 * len(ML.KAT_U1) * len(ML.KAT_U2)
    for v in KAT["generate_ray"]:
        o, d = cams[v["camera"]].generate_ray(tuple(f32(v["u1"])), tuple(f32(v["u2"])), tuple(v["raster"]))
        assert [ML.b32(x) for x in o] == v["o"] and [ML.b32(x) for x in d] == v["d"], v
    # the cases the vectors are there for
    u1s = {tuple(v["u1"]) for v in KAT["generate_ray"]}
    assert (ML.b32(F(0.5)),) * 2 in u1s and (0, 0) in u1s and (ML.b32(ML.BELOW_ONE),) * 2 in u1s
    assert any(tuple(v["u2"]) == (0, 0) for v in KAT["generate_ray"])
    got = {(float(c.lens_radius), float(c.focal_distance)) for c in cams.values()}
    assert {(float(F(1e-30)), 8.0), (1e3, 8.0), (float(F(0.3)), float(F(1e-3))), (float(F(0.3)), 1e6)} <= got


def test_kat_centre_of_the_lens_is_the_pinhole_origin_and_inactive_lenses_are_pinholes():
    """u1 = (0.5, 0.5): the disk gives exactly (0, 0), so the origin is the pinhole's; the direction went through
    one more normalize.  A radius or a focal distance alone changes no bit."""
    pin = R.Camera(*ML.KAT_CAMERAS["box"][:4])
    half = [ML.b32(F(0.5))] * 2
    n = 0
    for v in KAT["generate_ray"]:
        o, d = pin.generate_ray(None, tuple(f32(v["u2"])), tuple(v["raster"]))
        if v["camera"] == "box" and v["u1"] == half:
            assert [ML.b32(x) for x in o] == v["o"]
            n += 1
        if v["camera"] in ("radius_only", "focal_only"):
            assert [ML.b32(x) for x in o] == v["o"] and [ML.b32(x) for x in d] == v["d"], v
            n += 1
    assert n > 50


@pytest.mark.parametrize("name", list(ML.CONFIGS))
def test_golden_block_is_the_restatements(name):
    """A 3 x 3 block of every configuration regenerated: the committed golden is this restatement's."""
    g = np.load(GOLDEN / f"lens_golden_{name}.npz")
    _, kind, configs = ML.CONFIGS[name]
    assert json.loads(str(g["configs"])) == [list(c) for c in configs]
    sc, env = ML.restate_scene(name)
    W, H = sc.camera.res
    px = [(x, y) for y in range(H // 2 - 1, H // 2 + 2) for x in range(W // 2 - 1, W // 2 + 2)]
    ys, xs = [p[1] for p in px], [p[0] for p in px]
    for key, depth, clamp, mis in configs:
        out, _ = ML.render_pixels(sc, env, kind, px, ML.SPP, depth, clamp, mis, parallel=False)
        check(out["radiance"], g[key + "_radiance"][ys, xs], f"{name} {key} radiance")
        check(out["weight"], g[key + "_weight"][ys, xs], f"{name} {key} weight")
        assert np.array_equal(out["seed"], g[key + "_seed"][ys, xs])
        assert np.array_equal(out["closest"], g[key + "_closest"][ys, xs])
        assert np.array_equal(out["shadow"], g[key + "_shadow"][ys, xs])
        assert float(g[key + "_differs"]) >= 0.5
    counts = json.loads(str(g["counts"]))
    assert counts["disk.x_arm"] > 0 and counts["disk.y_arm"] > 0


# ----------------------------------------------------------------------------- lens off
@pytest.mark.parametrize("radius,focal", [(0.0, 0.0), (0.3, 0.0), (0.0, 8.0)])
def test_lens_off_is_ref_restate_camera_bit_for_bit(radius, focal):
    rng = np.random.default_rng(7)
    for pos, rot, fov, res in (((0.3, 1.2, 9.0), (3.0, -2.0, 5.0), 15.0, (24, 24)), ((0, 1, 3), (0, 0, 0), 80.0, (24, 16)),
                               ((-3.1, 1.3, 0.07), (-90.0, 4.0, 0.0), 80.0, (16, 24))):
        a, b = R.Camera(pos, rot, fov, res), L.LensCamera(pos, rot, fov, res, radius, focal)
        assert not b.active
        for _ in range(100):
            u = [F(v) for v in rng.random(4, dtype=np.float32)]
            raster = (int(rng.integers(res[0])), int(rng.integers(res[1])))
            ra, rb = a.generate_ray((u[0], u[1]), (u[2], u[3]), raster), b.generate_ray((u[0], u[1]), (u[2], u[3]), raster)
            assert R.bits(ra[0]).tolist() == R.bits(rb[0]).tolist() and R.bits(ra[1]).tolist() == R.bits(rb[1]).tolist()


# ----------------------------------------------------------------------------- the focus property
FOCUS_CAMERAS = [(15.0, 8.0, (24, 24), 0.3), (80.0, 0.5, (24, 16), 0.2), (60.0, 1000.0, (16, 24), 25.0), (120.0, 3.0, (7, 5), 0.5)]


@pytest.mark.parametrize("fov,focal,res,radius", FOCUS_CAMERAS)
def test_rays_of_one_film_point_meet_on_the_plane_of_focus(fov, focal, res, radius):
    """Fix u2 and the pixel, draw eight u1: the rays meet the camera-space plane z = -focal_distance in one
    point.  The worst spread measured on this restatement was 1.3e-7 of the focal distance; 2e-6 is about 32
    f32 ulps.  Every origin lies on the lens."""
    cam = L.LensCamera((0.3, 1.2, 9.0), (3.0, -2.0, 5.0), fov, res, radius, focal)
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(200):
        u2 = tuple(F(v) for v in rng.random(2, dtype=np.float32))
        raster = (int(rng.integers(res[0])), int(rng.integers(res[1])))
        pts = []
        for _ in range(8):
            u1 = tuple(F(v) for v in rng.random(2, dtype=np.float32))
            o, d = cam.camera_space_ray(u1, u2, raster)
            o, d = np.array(o, np.float64), np.array(d, np.float64)
            assert o[2] == 0 and np.hypot(o[0], o[1]) <= float(cam.lens_radius) * (1 + 1e-6)
            s = (-float(cam.focal_distance) - o[2]) / d[2]
            pts.append(o + s * d)
        pts = np.array(pts)
        worst = max(worst, float(np.max(np.linalg.norm(pts - pts.mean(axis=0), axis=1))) / float(cam.focal_distance))
    print(f"fov {fov} focal {focal} {res}: worst spread {worst:.3g} of the focal distance")
    assert worst <= 2e-6


# ----------------------------------------------------------------------------- a plane in and out of focus
_CHECKER = {}


def checker_films(focal=8.0, radius=0.3, res=(4, 4), spp=4096, cell=0.4):
    """A camera at the origin looking down -z at a plane z = -dist that carries a checker of `cell` world units
    (0 or 1, emitted): per pixel the mean and the variance of what `spp` samples see, through the lens and
    through the pinhole, at dist = focal and dist = 2 focal.  The samples are the renderer's: the pixel's chain
    from x + y * width, u1 ahead of u2.  -> {(lens, dist factor): (mean [H, W], variance [H, W])}."""
    if not _CHECKER:
        W, H = res
        cams = {True: L.LensCamera((0, 0, 0), (0, 0, 0), 4.0, res, radius, focal),
                False: L.LensCamera((0, 0, 0), (0, 0, 0), 4.0, res, 0.0, 0.0)}
        for on, cam in cams.items():
            o = np.zeros((H, W, spp, 3))
            d = np.zeros((H, W, spp, 3))
            for y in range(H):
                for x in range(W):
                    s = R.LCG(x + y * W)
                    for k in range(spp):
                        u1, u2 = s.next2d(), s.next2d()
                        o[y, x, k], d[y, x, k] = cam.generate_ray(u1, u2, (x, y))
            for factor in (1, 2):
                t = (-focal * factor - o[..., 2]) / d[..., 2]
                p = o + t[..., None] * d
                v = ((np.floor(p[..., 0] / cell + 0.37) + np.floor(p[..., 1] / cell + 0.37)) % 2).astype(np.float64)
                _CHECKER[(on, factor)] = (v.mean(axis=2), v.var(axis=2, ddof=1))
        _CHECKER["spp"] = spp
    return _CHECKER


def test_plane_at_the_focal_distance_renders_as_through_a_pinhole_and_twice_as_far_does_not():
    f = checker_films()
    n = f["spp"]

    def beyond(factor):
        (ml, vl), (mp, vp) = f[(True, factor)], f[(False, factor)]
        se = np.sqrt((vl + vp) / n)
        return np.abs(ml - mp) > 5 * se, ml, mp

    bad, ml, mp = beyond(1)
    assert not bad.any(), f"in focus: {int(bad.sum())} of {bad.size} pixels differ by more than 5 standard errors"
    assert 0.05 < mp.mean() < 0.95 and mp.std() > 0.1     # the checker shows: the pixels are not all alike
    bad2, ml2, mp2 = beyond(2)
    assert bad2.sum() > bad2.size // 2, f"out of focus: only {int(bad2.sum())} of {bad2.size} pixels differ"
    assert ml2.std() < mp2.std()                          # and what differs is a blur


# ----------------------------------------------------------------------------- AO restatement
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_ao_restatement_with_the_lens_off_equals_the_oracle(name):
    """The new restatement of the AO pixel loop, pinned before the lens uses it: bit-equal to orc_render_ao."""
    desc, cs, orc = oracle_scene(name)
    sc = R.RefScene(desc)
    cam = L.lens_camera_of(desc.camera)
    assert not cam.active
    W, H = cam.res
    x0, y0, x1, y1 = W // 2 - 6, H // 2 - 6, W // 2 + 6, H // 2 + 6
    orad, ow, stats = orc.render_ao(3, [(x0, y0, x1, y1)], n_threads=2)
    rad, wt, closest, shadow = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), 0, 0
    for y in range(y0, y1):
        for x in range(x0, x1):
            r = L.ao_pixel(sc, cam, x, y, 3)
            assert not r["ambiguous"]
            rad[y, x], wt[y, x] = r["radiance"], r["weight"]
            closest, shadow = closest + r["closest"], shadow + r["shadow"]
    check(rad, orad, f"{name}: AO radiance")
    check(wt, ow, f"{name}: AO weight")
    assert (closest, shadow) == (stats["camera_rays"], stats["shadow_rays"])
    assert 0 < rad[y0:y1, x0:x1].mean() < 3


# ----------------------------------------------------------------------------- parser, compiler, fingerprint
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
let lamp = EmissiveMaterial {{ color: [17, 12, 4] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24]{lens} }},
    integrator: Path {{ spp: 4, max_depth: 5, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey, $lamp] }} ]
}}
"""


def write_sdl(tmp_path, lens_fields="", out=None):
    p = tmp_path / "s.akari"
    p.write_text(SDL.format(lens=lens_fields, out=out or tmp_path / "o.pfm", mesh=CORNELL_MESH))
    return p


def test_parser_reads_the_lens(tmp_path):
    cam = scene.load_scene_file(write_sdl(tmp_path)).camera
    assert (cam.lens_radius, cam.focal_distance) == (0.0, 0.0)
    cam = scene.load_scene_file(write_sdl(tmp_path, ", lens_radius: 0.3, focal_distance: 8")).camera
    assert (cam.lens_radius, cam.focal_distance) == (float(F(0.3)), 8.0)
    cam = scene.load_scene_file(write_sdl(tmp_path, ", focal_distance: 8")).camera      # a focus without a lens: a pinhole
    assert (cam.lens_radius, cam.focal_distance) == (0.0, 8.0)
    assert scene.PerspectiveCamera.__dataclass_fields__.keys() >= {"lens_radius", "focal_distance"}
    assert list(scene.PerspectiveCamera.__dataclass_fields__)[-2:] == ["lens_radius", "focal_distance"]   # trailing


@pytest.mark.parametrize("fields,word", [(", lens_radius: -0.1, focal_distance: 8", "lens_radius"),
                                         (", lens_radius: 0.3, focal_distance: -8", "focal_distance"),
                                         (", lens_radius: 4" + "0" * 40 + ", focal_distance: 8", "lens_radius"),   # inf in f32
                                         (", lens_radius: 0.3", "focal_distance"),
                                         (", lens_radius: 0.3, focal_distance: 0", "focal_distance"),
                                         (', lens_radius: "wide", focal_distance: 8', "lens_radius")])
def test_parser_refuses(tmp_path, fields, word):
    with pytest.raises(scene.SdlError, match=word):
        scene.load_scene_file(write_sdl(tmp_path, fields))


def test_compiler_carries_the_lens_and_the_fingerprint_tells_lenses_apart():
    plain = scene.compile_scene(helpers.cornell((16, 8)))
    assert progressive.scene_fingerprint(plain) == PINHOLE_FINGERPRINT        # a pinhole keeps what it always had
    prints = {PINHOLE_FINGERPRINT}
    for r, f in ((0.3, 8.0), (0.31, 8.0), (0.3, 8.5)):
        sc = helpers.cornell((16, 8))
        sc.camera.lens_radius, sc.camera.focal_distance = r, f
        cs = scene.compile_scene(sc)
        assert (cs.camera.lens_radius, cs.camera.focal_distance) == (r, f)
        prints.add(progressive.scene_fingerprint(cs))
    assert len(prints) == 4
    for r, f in ((0.3, 0.0), (0.0, 8.0)):                                    # inactive: the pinhole's film, its fingerprint
        sc = helpers.cornell((16, 8))
        sc.camera.lens_radius, sc.camera.focal_distance = r, f
        assert progressive.scene_fingerprint(scene.compile_scene(sc)) == PINHOLE_FINGERPRINT


class _Recorder:
    """What upload_lens needs of a context."""

    def __init__(self, has_entry):
        self.lib = type("Lib", (), {"akr_hip_set_lens": None} if has_entry else {})()
        self.calls = []

    def set_lens(self, r, f):
        self.calls.append((r, f))


def test_upload_lens_sends_zeros_for_a_pinhole_and_guards_older_libraries():
    cam = scene.PerspectiveCamera(lens_radius=0.3, focal_distance=8.0)
    ctx = _Recorder(True)
    scene.upload_lens(ctx, cam)
    scene.upload_lens(ctx, scene.PerspectiveCamera())
    assert ctx.calls == [(0.3, 8.0), (0.0, 0.0)]
    old = _Recorder(False)
    scene.upload_lens(old, scene.PerspectiveCamera())          # a pinhole needs nothing of it
    assert old.calls == []
    with pytest.raises(RuntimeError, match="akr_hip_set_lens"):
        scene.upload_lens(old, cam)                            # a lens is not dropped silently


# ----------------------------------------------------------------------------- command line, autofocus
@pytest.mark.parametrize("argv,word", [(["--lens-radius", "-1"], "--lens-radius"), (["--lens-radius", "nan"], "--lens-radius"),
                                       (["--focal-distance", "inf"], "--focal-distance"),
                                       (["--focus-at", "3", "4", "--focal-distance", "8"], "cannot be combined"),
                                       (["--lens-radius", "0.3"], "focal distance")])
def test_cli_refusals_need_no_device(tmp_path, capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        render.main([str(write_sdl(tmp_path))] + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_autofocus_arithmetic():
    """A made-up hit: t along the unit camera-space direction d puts the plane of focus at t |d.z|, in f32, and
    the lens then aims at that hit: ft = focal_distance / |d.z| gives t back."""
    assert lens.focal_distance_from_hit(10.0, np.array([0.6, 0.0, -0.8], np.float32)) == float(F(F(10.0) * F(0.8)))
    cam = scene.PerspectiveCamera(position=(0.3, 1.2, 9.0), rotation=(3.0, -2.0, 5.0), fov=15.0, resolution=(24, 24))
    rc = R.Camera(cam.position, cam.rotation, cam.fov, cam.resolution)
    for x, y in ((0, 0), (23, 23), (12, 7)):
        o, d, dc = lens.pinhole_ray(cam, x, y)
        ro, rd = rc.generate_ray(None, (F(0.5), F(0.5)), (x, y))
        assert np.allclose(o, ro, rtol=0, atol=1e-6) and np.allclose(d, rd, rtol=0, atol=2e-6)
        assert abs(float(np.linalg.norm(dc)) - 1) < 1e-6 and dc[2] < 0
        t = F(7.25)
        fd = lens.focal_distance_from_hit(t, dc)
        assert fd == float(F(t * F(abs(dc[2]))))
        assert abs(F(fd) / F(abs(dc[2])) - t) <= 2 * np.spacing(t)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            lens.focal_distance_from_hit(bad, np.array([0, 0, -1], np.float32))
