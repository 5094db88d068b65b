"""Render sessions on device 0: a render of a spp continued by b spp is the oracle's
render of a + b spp, bit for bit, in radiance, weight and every slot's final sampler state, whichever
form runs each segment; the session's export / import, its rules, the checkpoint CLI and the C++ adapter.

The oracle (oracle/, unchanged) only renders whole films, so every expectation here is one
`orc.render(total, ..., probe=True)`, computed once per (scene, total, depth, tiles, clamp) and shared."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, progressive, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell, mixed_scene, slot_pixels, small_soup, textured_scene

pytestmark = pytest.mark.gpu

RAGGED = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 64, 64), (5, 5, 5, 9)]   # ragged, clipped, empty
NO_SESSION = "no render session to continue"

_ORACLES = {}   # scene name -> [nodes, tris, OracleScene, {key: (radiance, weight, probe)}]


def _setup(ctx, name, make):
    """Upload scene `name`; returns (cs, expect) where expect(total, depth, tiles, clamp) is the
    oracle's (radiance, weight, probe), shared by every test that renders this scene."""
    cs = scene.compile_scene(make())
    scene.upload_scene(ctx, cs)
    nodes, tris = ctx.accel_export()
    ent = _ORACLES.get(name)
    if ent is None or not (np.array_equal(ent[0], nodes) and np.array_equal(ent[1], tris)):
        ent = _ORACLES[name] = [nodes, tris, py_oracle.OracleScene(cs, nodes, tris, capi), {}]

    def expect(total, depth, tiles, clamp=0.0):
        key = (total, depth, tuple(tiles), clamp)
        if key not in ent[3]:
            out = ent[2].render(total, depth, tiles=tiles, ray_clamp=clamp, probe=True)
            for a in (out[0], out[1], out[3]):
                a.setflags(write=False)
            ent[3][key] = (out[0], out[1], out[3])
        return ent[3][key]
    return cs, expect


FORMS = {
    "wavefront": dict(path=0, path_defer=0, path_spec=0),
    "k_path": dict(path=1, path_defer=0, path_spec=0),
    "k_path_defer": dict(path=1, path_defer=1, path_spec=0),
    "k_path_spec": dict(path=1, path_defer=0, path_spec=1),
}


def _set_form(ctx, form, order):
    """Force one render form, with the cost-ordered fetch off (order 0) or forced on at every spp, as
    test_render_path_kernel_and_wavefront_bit_exact sets them."""
    for k, v in FORMS[form].items():
        ctx.set_option(k, v)
    ctx.set_option("path_order", (1 if form == "wavefront" else 2) if order else 0)
    ctx.set_option("path_order_pair", ((1 if form in ("k_path_defer", "k_path_spec") else 3) if order else 0))
    ctx.set_option("path_order_min_spp", 0 if order else 64)
    ctx.set_option("path_order_shift", 0)


def _ran(ctx, form, depth):
    want = "k_path" if form == "k_path_defer" and depth > 8 else form   # above depth 8 k_path_defer falls back
    got = ctx.render_form()["form"]
    assert got == want, f"segment ran {got}, not {want}"


def _check_total(ctx, expect_out, rad, w, tiles, W, H, probe=True):
    """The film, the pixel probe's sampler states and the exported session state against the oracle."""
    orad, ow, oprobe = expect_out
    assert np.array_equal(w, ow), f"{np.count_nonzero(w != ow)} weights differ"
    bad = rad != orad
    assert not bad.any(), f"{bad.sum()} radiance values differ, max {np.abs(rad - orad).max()}"
    ys, xs = slot_pixels(tiles, W, H)
    sampler, film = ctx.render_state_export()
    assert len(sampler) == len(ys)
    assert np.array_equal(sampler, oprobe["seed"][ys, xs]), "exported sampler states differ from the oracle"
    if probe:
        p = ctx.pixel_probe(len(ys))
        assert np.all(p["flags"] & capi.PROBE_SEED)
        assert np.array_equal(p["seed"], oprobe["seed"][ys, xs]), "probe sampler states differ from the oracle"
    return sampler, film


def _run_split(ctx, expect, split, depth, tiles, W, H, clamp=0.0, form=None):
    rad, w = ctx.render(split[0], depth, tiles, W, H, ray_clamp=clamp)
    if form and split[0]:
        _ran(ctx, form, depth)
    done = split[0]
    for n in split[1:]:
        rad, w = ctx.render_continue(n, W, H)
        done += n
        if form and n:
            _ran(ctx, form, depth)
        assert ctx.render_state_info()["spp_done"] == done
    return _check_total(ctx, expect(sum(split), depth, tiles, clamp), rad, w, tiles, W, H)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("form", list(FORMS))
def test_continue_forms_and_splits(hip_ctx_factory, form, order):
    with hip_ctx_factory(0) as ctx:
        _set_form(ctx, form, order)
        ctx.set_option("pixel_probe", 1)
        cs, expect = _setup(ctx, "cornell40x24", lambda: cornell((40, 24)))
        for split in ((2, 3), (1, 1, 1, 4), (5, 0)):
            _run_split(ctx, expect, split, 5, RAGGED, 40, 24, form=form)
        for depth in (0, 9):
            _run_split(ctx, expect, (2, 2), depth, RAGGED, 40, 24, form=form)
        _run_split(ctx, expect, (2, 2), 5, RAGGED, 40, 24, clamp=10.0, form=form)
        info = ctx.render_state_info()
        assert info == dict(n_pixels=len(slot_pixels(RAGGED, 40, 24)[0]), spp_done=4, max_depth=5, ray_clamp=10.0,
                            flags=0, width=40, height=24, n_tiles=3)


def test_continue_switches_form_between_segments(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        cs, expect = _setup(ctx, "cornell40x24", lambda: cornell((40, 24)))
        rad = w = None
        for k, (form, n) in enumerate((("wavefront", 2), ("k_path_spec", 1), ("k_path_defer", 3), ("k_path", 2))):
            _set_form(ctx, form, k & 1)
            rad, w = ctx.render(n, 5, RAGGED, 40, 24) if k == 0 else ctx.render_continue(n, 40, 24)
            _ran(ctx, form, 5)
        _check_total(ctx, expect(8, 5, RAGGED), rad, w, RAGGED, 40, 24)


def test_continue_mid_kernel_fetch_and_small_tile(hip_ctx_factory):
    """A grid shrunk to 1 % of the resident one: every lane fetches several pixels, so the state is
    loaded at the mid-kernel fetch (the deep-stack soup); and a tile list smaller than a workgroup."""
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("path_grid_pct", 1)
        cs, expect = _setup(ctx, "soup100k", lambda: small_soup(100_000, (64, 36)))
        for form in FORMS:
            _set_form(ctx, form, 0)
            for tiles in ([(0, 0, 64, 36)], [(3, 3, 10, 8)]):
                _run_split(ctx, expect, (3, 4), 5, tiles, 64, 36, form=form)


@pytest.mark.parametrize("name,make", [("mixed48", lambda: mixed_scene((48, 48))),
                                       ("textured40", lambda: textured_scene((40, 40)))])
def test_continue_shading_variety_and_ray_counts(hip_ctx_factory, name, make):
    """Glossy / Mix / two-sided emitter and image textures, split 2 + 3 with the counting build: the
    probe of a continue holds the state after the total and the rays of its segment alone, so the
    segments' ray counts sum to the oracle's per pixel."""
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("count_tests", 1)
        cs, expect = _setup(ctx, name, make)
        W, H = cs.camera.resolution
        tiles = [(0, 0, W, H)]
        ys, xs = slot_pixels(tiles, W, H)
        for form in FORMS:
            _set_form(ctx, form, 0)
            ctx.render(2, 5, tiles, W, H)
            p0 = ctx.pixel_probe(len(ys))
            rad, w = ctx.render_continue(3, W, H)
            p1 = ctx.pixel_probe(len(ys))
            out = expect(5, 5, tiles)
            _check_total(ctx, out, rad, w, tiles, W, H)
            assert np.all(p0["flags"] & p1["flags"] & capi.PROBE_RAYS), f"{form}: ray counts not recorded"
            for k in ("closest_rays", "shadow_rays"):
                assert np.array_equal(p0[k] + p1[k], out[2][k][ys, xs]), f"{form}: per-pixel {k} of 2 + 3 differ"


class _DeviceFloats:
    """n floats of device memory through the HIP runtime the library already loaded."""

    def __init__(self, n):
        self.hip, self.n, self.p = C.CDLL("libamdhip64.so"), n, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(4 * n)) == 0

    def poison(self):   # every float a NaN; done before the context's stream is given the buffer
        assert self.hip.hipMemset(self.p, 0xFF, C.c_size_t(4 * self.n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def host(self):
        out = np.empty(self.n, np.float32)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(4 * self.n), 2) == 0   # device to host
        return out

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def test_state_export_import_and_device_form(hip_ctx_factory):
    tiles, W, H = RAGGED, 40, 24
    ys, xs = slot_pixels(tiles, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        cs, expect = _setup(a, "cornell40x24", lambda: cornell((40, 24)))
        _setup(b, "cornell40x24", lambda: cornell((40, 24)))
        a.render(3, 5, tiles, W, H)
        sampler, film = a.render_state_export()
        assert sampler.shape == (n,) and film.shape == (n, 4) and np.all(film[:, 3] == 3)
        b.render_state_import(3, 5, tiles, sampler, film)
        assert b.render_state_info()["spp_done"] == 3
        rad, w = b.render_continue(2, W, H)
        out5 = expect(5, 5, tiles)
        _check_total(b, out5, rad, w, tiles, W, H, probe=False)
        # a session that has drawn nothing: the start states, a zero film, spp 0
        seeds = (xs + ys * W).astype(np.uint32)
        b.render_state_import(0, 5, tiles, seeds, np.zeros((n, 4), np.float32))
        s0, f0 = b.render_state_export()
        assert np.array_equal(s0, seeds) and not f0.any()
        rad, w = b.render_continue(4, W, H)
        _check_total(b, expect(4, 5, tiles), rad, w, tiles, W, H, probe=False)
        # and after a render of 0 spp the export gives those start states
        b.render(0, 5, tiles, W, H)
        s0, f0 = b.render_state_export()
        assert np.array_equal(s0, seeds) and not f0.any()
        rad, w = b.render_continue(4, W, H)
        _check_total(b, expect(4, 5, tiles), rad, w, tiles, W, H, probe=False)
        # the device form: each slot's totals, packed; merged into a frame (the ragged tiles overlap, and
        # a pixel of two slots holds both), they are the host form's film
        d_rad, d_w = _DeviceFloats(3 * n), _DeviceFloats(n)

        def merged():
            a.synchronize()
            rad, w = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
            np.add.at(rad, (ys, xs), d_rad.host().reshape(-1, 3))
            np.add.at(w, (ys, xs), d_w.host())
            return rad, w

        try:
            for more in (2, 0):   # spp 0: the totals again
                d_rad.poison()
                d_w.poison()
                assert a.render_continue_device(more, d_rad.p.value, d_w.p.value) == n
                rad, w = merged()
                assert np.all(d_w.host() == 5)
                assert np.array_equal(rad, out5[0]) and np.array_equal(w, out5[1])
            a.render_device(3, 5, tiles, d_rad.p.value, d_w.p.value)   # render_device starts a session too
            rad, w = a.render_continue(2, W, H)
            _check_total(a, out5, rad, w, tiles, W, H, probe=False)
            a.synchronize()
        finally:
            d_rad.free()
            d_w.free()


def test_session_rules(hip_ctx_factory):
    tiles, W, H = RAGGED, 40, 24
    with hip_ctx_factory(0) as ctx:
        cs, expect = _setup(ctx, "cornell40x24", lambda: cornell((40, 24)))
        out5 = expect(5, 5, tiles)

        def refused():
            with pytest.raises(capi.AkrError, match=NO_SESSION):
                ctx.render_continue(1, W, H)
            with pytest.raises(capi.AkrError, match=NO_SESSION):
                ctx.render_state_info()
            rad, w = ctx.render(2, 5, tiles, W, H)   # the context is still usable
            return rad, w

        refused()                                   # a new context
        cam = cs.camera
        ctx.set_camera(cam.position, cam.rotation, cam.fov, cam.resolution)
        refused()                                   # after set_camera
        ctx.render_ao(1, tiles, W, H)
        refused()                                   # after render_ao
        ctx.upload_materials(cs.materials)
        refused()                                   # after an upload
        # a trace between segments leaves the result unchanged
        rays = np.zeros(3, capi.RAY_DTYPE)
        rays["o"], rays["d"], rays["tmin"], rays["tmax"] = (0, 1, 0), (0, 0, -1), 1e-3, np.inf
        assert np.all(ctx.trace(rays)["geom_id"] == 0)
        ctx.trace(rays, any_hit=True)
        rad, w = ctx.render_continue(3, W, H)
        assert np.array_equal(rad, out5[0]) and np.array_equal(w, out5[1])
        # refused imports change nothing: the session of 5 spp stays
        sampler, film = ctx.render_state_export()
        with pytest.raises(capi.AkrError, match="tile list has"):
            ctx.render_state_import(5, 5, tiles, sampler[:-1], film[:-1])
        wrong = film.copy()
        wrong[7, 3] = 4
        with pytest.raises(capi.AkrError, match="slot 7 holds weight"):
            ctx.render_state_import(5, 5, tiles, sampler, wrong)
        assert ctx.render_state_info()["spp_done"] == 5
        rad, w = ctx.render_continue(0, W, H)
        assert np.array_equal(rad, out5[0]) and np.array_equal(w, out5[1])
        with pytest.raises(capi.AkrError, match="spp must be >= 0"):
            ctx.render_continue(-1, W, H)
        # the weight is an f32 count: a total above 2^24 is refused, the session stays
        one = [(4, 4, 5, 5)]
        ctx.render_state_import(1 << 24, 5, one, np.array([4 + 4 * W], np.uint32),
                                np.array([[1.0, 2.0, 3.0, float(1 << 24)]], np.float32))
        with pytest.raises(capi.AkrError, match="exceed 2\\^24"):
            ctx.render_continue(1, W, H)
        info = ctx.render_state_info()
        assert info["spp_done"] == 1 << 24 and info["n_pixels"] == 1
        rad, w = ctx.render_continue(0, W, H)
        assert w[4, 4] == float(1 << 24) and np.array_equal(rad[4, 4], [1, 2, 3]) and np.count_nonzero(w) == 1


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 6, max_depth: 4, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def _pfm(path):
    raw = path.read_bytes()
    return np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32)


def test_cli_checkpoint_and_resume(tmp_path):
    """render.py to 4 spp in passes of 2 with a checkpoint, then a second process resumes it to 6 spp:
    the PFM of a one-shot 6-spp run of the same scene file."""
    path = tmp_path / "box.akari"
    path.write_text(SDL.format(out=tmp_path / "default.pfm", mesh=CORNELL_MESH))
    ck = tmp_path / "box.ckpt.npz"

    def cli(*args):
        code = ("import sys; sys.path[:0] = [%r]; from akari_amd import render; sys.exit(render.main(sys.argv[1:]))"
                % str(ROOT / "akarirender-1_amd"))
        r = subprocess.run([sys.executable, "-c", code, str(path), *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    cli("--spp", "4", "--pass-spp", "2", "--checkpoint", str(ck), "--preview", "--out", str(tmp_path / "four.pfm"))
    saved = progressive.Checkpoint.load(ck)
    assert saved.spp_done == 4 and (saved.width, saved.height) == (40, 24) and np.all(saved.film[:, 3] == 4)
    assert not list(tmp_path.glob("*.tmp*")), "the checkpoint's temporary file was left behind"
    out = cli("--resume", str(ck), "--out", str(tmp_path / "resumed.pfm"))
    assert "spp 6" in out
    cli("--out", str(tmp_path / "oneshot.pfm"))
    assert np.array_equal(_pfm(tmp_path / "resumed.pfm"), _pfm(tmp_path / "oneshot.pfm"))
    assert not np.array_equal(_pfm(tmp_path / "four.pfm"), _pfm(tmp_path / "oneshot.pfm"))


def test_cpp_adapter_continue(tmp_path):
    """The C++ adapter: render 2, continue 3 equals a 5-spp render; so does 2 exported, imported into a
    second accelerator and continued by 3; a continue without a session throws the documented message."""
    exe = tmp_path / "progressive_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "progressive_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    names = [tmp_path / f"{k}.pfm" for k in ("split", "whole", "moved")]
    r = subprocess.run([str(exe), str(CORNELL_MESH), "32", "32", "2", "3", *map(str, names)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "refused=1 spp_done=5 n_pixels=1024 width=32 height=32 max_depth=5" in r.stdout
    split, whole, moved = (_pfm(p) for p in names)
    assert np.array_equal(split, whole) and np.array_equal(moved, whole)
    cs = scene.compile_scene(scene.cornell_scene(CORNELL_MESH, resolution=(32, 32)))
    with capi.HipContext(0) as ctx:
        scene.upload_scene(ctx, cs)
        rad, w = ctx.render(5, 5, [(0, 0, 32, 32)], 32, 32)
    assert np.array_equal(whole.reshape(32, 32, 3)[::-1], rad / w[..., None])
