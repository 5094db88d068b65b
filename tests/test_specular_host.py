"""Host side of the Mirror and Glass materials: the restatement against its goldens and
function vectors, the Fresnel term and Snell's law, what a mirror and a slab of glass must show, restated on the
CPU, and the parser, scene compiler, command line and adapter.  No GPU needed."""
import json
import multiprocessing as mp
import subprocess
import sys

import numpy as np
import pytest

from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from test_shade_simple_host import ask

sys.path.insert(0, str(GOLDEN))
import make_specular_golden as MS  # noqa: E402
import ref_restate as R  # noqa: E402
import specular_restate as S  # noqa: E402
import specular_scenes  # noqa: E402

F = np.float32
BLOCK = (10, 10, 14, 14)   # the block the restatement is run on again, as make_path_golden's
KAT = json.loads((GOLDEN / "specular_kat.json").read_text())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def b32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def f32(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def ulps(a, b):
    """Distance in f32 steps between two finite values of one sign."""
    return abs(int(b32(F(a))) - int(b32(F(b))))


# ----------------------------------------------------------------------------- goldens, function vectors
@pytest.mark.parametrize("name", list(MS.CONFIGS))
def test_restatement_reproduces_committed_goldens(name):
    """The goldens cannot drift from the restatement: a 4 x 4 block of every configuration, run again."""
    g = np.load(GOLDEN / f"specular_golden_{name}.npz")
    assert json.loads(str(g["configs"])) == json.loads(json.dumps(MS.CONFIGS[name]))
    x0, y0, x1, y1 = BLOCK
    px = [(x, y) for y in range(y0, y1) for x in range(x0, x1)]
    sel = (slice(y0, y1), slice(x0, x1))
    for key, _, _, env_on, depth, clamp in MS.CONFIGS[name]:
        sc = S.SpecScene(MS.build_scene(name, key))
        env = MS.restated_env() if env_on else None
        for mis in (False, True):
            k = key + ("_mis" if mis else "")
            out, _ = MS.render_pixels(sc, env, px, MS.SPP, depth, clamp, mis, parallel=False)
            assert np.array_equal(bits(out["radiance"]).reshape(4, 4, 3), bits(g[k + "_radiance"][sel])), (name, k)
            assert np.array_equal(out["seed"].reshape(4, 4), g[k + "_seed"][sel]), (name, k)
            assert np.array_equal(out["closest"].reshape(4, 4), g[k + "_closest"][sel]), (name, k)
            assert np.array_equal(out["shadow"].reshape(4, 4), g[k + "_shadow"][sel]), (name, k)
            assert np.all(g[k + "_weight"] == MS.SPP)


def test_golden_set_takes_every_new_branch_masks_nothing_and_mis_moves_no_draw():
    total = {}
    for name in MS.CONFIGS:
        g = np.load(GOLDEN / f"specular_golden_{name}.npz")
        for k, v in json.loads(str(g["counts"])).items():
            total[k] = total.get(k, 0) + v
        for key, *_ in MS.CONFIGS[name]:
            for q in ("seed", "closest", "shadow"):   # the switch adds no draw and no ray
                assert np.array_equal(g[f"{key}_{q}"], g[f"{key}_mis_{q}"]), (name, key, q)
            assert not g[key + "_mask"].any() and not g[key + "_mis_mask"].any(), (name, key)
    assert all(total.get(b, 0) >= 1 for b in MS.REQUIRED_BRANCHES), total


def test_plain_scene_restates_as_before():
    """On a scene without either material the new path loop is mis_restate's and ref_restate's."""
    g = np.load(GOLDEN / "path_golden_cornell.npz")
    sc = S.SpecScene(specular_scenes.helpers.cornell((24, 24)))
    for x, y in ((11, 12), (3, 20)):
        r = S.render_pixel(sc, None, x, y, 4, 5)
        assert np.array_equal(bits(r["radiance"]), bits(g["d5_radiance"][y, x]))
        assert (r["seed"], r["closest"], r["shadow"]) == (g["d5_seed"][y, x], g["d5_closest"][y, x], g["d5_shadow"][y, x])


def test_fresnel_vectors():
    assert len(KAT["fresnel"]) >= 18
    assert {f32(v["c"]) for v in KAT["fresnel"]} >= {F(1.0), F(0.5), F(1e-3), F(0.0)}
    assert all(f32(v["F"]) == 1 for v in KAT["fresnel"] if f32(v["c"]) == 0)    # grazing: everything reflects
    for v in KAT["fresnel"]:
        Fr, ct, r = S.fresnel(f32(v["c"]), f32(v["ior"]), bool(v["entering"]))
        assert b32(Fr) == v["F"] and b32(r) == v["r"], v
        assert (ct is None) == bool(v["tir"]) and (ct is None or b32(ct) == v["ct"]), v
    # the critical angle from inside, one float to either side
    lo, hi = (f32(b) for b in KAT["critical_cosines"])
    assert hi == np.nextafter(lo, F(1.0), dtype=np.float32)
    assert S.fresnel(lo, F(1.5), False)[:2] == (F(1.0), None)
    Fr, ct, _ = S.fresnel(hi, F(1.5), False)
    assert ct is not None and 0 < Fr <= 1
    assert abs(float(lo) - np.sqrt(1.0 - 1.0 / 2.25)) < 1e-6
    # ior 1: the pane vanishes where the operations are exact
    for c in (F(1.0), F(0.5)):
        for entering in (True, False):
            assert S.fresnel(c, F(1.0), entering)[0] == 0


def test_glass_sample_vectors():
    assert len(KAT["glass_sample"]) >= 17
    for v in KAT["glass_sample"]:
        f, wi, pdf = S.glass_sample(tuple(f32(x) for x in v["color"]), f32(v["ior"]), tuple(f32(x) for x in v["u"]),
                                    tuple(f32(x) for x in v["wo"]))
        assert [b32(x) for x in f] == v["f"] and [b32(x) for x in wi] == v["wi"] and b32(pdf) == v["pdf"], v
    # u.y exactly F refracts (the test is u.y < F), one float below reflects
    wo = (F(0.36), F(0.8), F(0.48))
    Fr = S.fresnel(F(0.8), F(1.5), True)[0]
    white = (F(1.0),) * 3
    _, wi, pdf = S.glass_sample(white, F(1.5), (F(0.9), Fr), wo)
    assert wi[1] < 0 and pdf == F(F(1.0) - Fr)
    _, wi, pdf = S.glass_sample(white, F(1.5), (F(0.9), np.nextafter(Fr, F(0.0), dtype=np.float32)), wo)
    assert wi[1] > 0 and pdf == Fr
    # the choice reads u.y, never u.x
    a = S.glass_sample(white, F(1.5), (F(0.0), F(0.5)), wo)
    b = S.glass_sample(white, F(1.5), (F(1.0), F(0.5)), wo)
    assert a == b
    # grazing: pdf 0 ends the path
    assert S.glass_sample(white, F(1.5), (F(0.5), F(0.5)), (F(0.6), F(0.0), F(0.8)))[2] == 0
    assert S.mirror_sample(white, (F(0.6), F(0.0), F(0.8)))[2] == 0


@pytest.mark.parametrize("ior", [1.0, 1.2, 1.33, 1.5, 2.4, 8.0])
def test_fresnel_at_normal_incidence(ior):
    want = ((ior - 1.0) / (ior + 1.0)) ** 2
    for entering in (True, False):
        got = S.fresnel(F(1.0), F(ior), entering)[0]
        if want == 0:
            assert got == 0
        else:
            assert ulps(got, F(((float(F(ior)) - 1.0) / (float(F(ior)) + 1.0)) ** 2)) <= 2, (ior, entering, got, want)


def test_snell_and_unit_length():
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(400):
        ior = F(rng.uniform(1.0, 3.0))
        cy = F(rng.uniform(0.05, 1.0)) * F(rng.choice([-1.0, 1.0]))
        phi = rng.uniform(0, 2 * np.pi)
        st = np.sqrt(max(0.0, 1.0 - float(cy) ** 2))
        wo = (F(st * np.cos(phi)), cy, F(st * np.sin(phi)))
        entering = bool(cy > 0)
        Fr, ct, r = S.fresnel(abs(cy), ior, entering)
        if ct is None:
            continue
        _, wi, pdf = S.glass_sample((F(1.0),) * 3, ior, (F(0.5), F(1.0)), wo)   # u.y = 1: always refracts
        assert pdf == F(F(1.0) - Fr)
        assert (wi[1] < 0) == entering
        ei, et = (1.0, float(ior)) if entering else (float(ior), 1.0)
        wo_t = np.hypot(float(wo[0]), float(wo[2]))
        wi_t = np.hypot(float(wi[0]), float(wi[2]))
        assert ulps(F(wi_t * et), F(wo_t * ei)) <= 4, (ior, wo, wi)
        assert abs(np.sqrt(sum(float(x) ** 2 for x in wi)) - 1.0) <= 1e-6, (ior, wo, wi)
        checked += 1
    assert checked > 200


def test_closures_evaluate_to_zero():
    wo, wi = (F(0.36), F(0.8), F(0.48)), (F(-0.36), F(0.8), F(-0.48))
    for closure in (("mirror", (F(1.0),) * 3), ("glass", (F(1.0),) * 3, F(1.5))):
        bsdf = R.BSDF((F(0.0), F(1.0), F(0.0)), (F(0.0), F(1.0), F(0.0)), closure)
        assert S.bsdf_evaluate(bsdf, wo, wi) == (F(0.0),) * 3
        assert S.closure_pdf(closure, wo, wi) == 0


# ----------------------------------------------------------------------------- what the estimator must show
def test_mirror_shows_the_lamp_at_full_weight():
    """A mirror facing a lamp: every pixel's reflection meets the lamp, so every sample is R * Le, at max_depth 1
    already (the ray at depth == max_depth is traced via a delta lobe).  The lamp is also the scene's only light
    and next-event estimation finds the mirror black, so all of it arrives through via_delta."""
    desc = specular_scenes.facing_mirror((8, 8))
    sc = S.SpecScene(desc)
    want = np.array([0.8 * 3.0, 0.6 * 2.0, 0.4 * 1.0])
    for depth in (1, 3):
        for mis in (False, True):
            for y in range(8):
                for x in range(8):
                    r = S.render_pixel(sc, None, x, y, 2, depth, mis=mis)
                    got = np.array(r["radiance"], np.float64) / 2
                    assert np.all(np.abs(got - want) <= 1e-5 * want), (depth, mis, x, y, got)
                    assert r["closest"] == 4 and r["shadow"] == 0
    # at max_depth 0 the mirror scatters nothing
    assert S.render_pixel(sc, None, 4, 4, 2, 0)["radiance"] == (F(0.0),) * 3


_G = {}


def _slab_samples(args):
    x, y = args
    out = []
    S.render_pixel(_G["sc"], None, x, y, _G["spp"], _G["depth"], 0.0, None, samples=out)
    return np.array(out, np.float64)


def test_glass_slab_transmits_one_minus_f_over_one_plus_f():
    """A slab between camera and lamp, 1 degree of view, 4 x 4 pixels, 4,096 spp, max_depth 16: the frame mean is
    Le (1 - F) / (1 + F), the sum over every number of internal reflections, at normal incidence, within 5
    standard errors of the mean taken from the samples' own variance (test_mis_host.py's bound)."""
    ior, Le, spp = 1.5, 2.0, 4096
    sc = S.SpecScene(specular_scenes.glass_slab(ior, (4, 4)))
    sc._mis_tri_sel = {}
    _G.update(sc=sc, spp=spp, depth=16)
    with mp.get_context("fork").Pool(min(16, mp.cpu_count())) as pool:
        s = np.array(pool.map(_slab_samples, [(x, y) for y in range(4) for x in range(4)], chunksize=1))
    assert s.shape == (16, spp, 3)
    frame = s.mean(axis=(0, 2))                      # the frame mean of each sample index
    Fn = ((ior - 1.0) / (ior + 1.0)) ** 2
    want = Le * (1.0 - Fn) / (1.0 + Fn)
    se = np.sqrt(frame.var(ddof=1) / spp)
    z = (frame.mean() - want) / se
    print(f"glass slab: frame mean {frame.mean():.5f}, expected {want:.5f}, {z:+.2f} standard errors (se {se:.5f})")
    assert se > 0 and abs(z) <= 5, (frame.mean(), want, se)


# ----------------------------------------------------------------------------- shading build, parser, compiler
def test_tables_with_a_specular_material_are_not_simple(tmp_path):
    exe = tmp_path / "shade_simple_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'akarirender-1_amd' / 'csrc'}",
                    str(ROOT / "tests" / "cpp" / "shade_simple_check.cpp"), "-o", str(exe)], check=True)
    ok = "M:0:-1:-1:-1 M:2:-1:-1:-1 L:-1"
    got = ask(exe, [ok, f"{ok} M:{capi.MAT_MIRROR}:-1:-1:-1", f"{ok} M:{capi.MAT_GLASS}:-1:-1:-1"])
    assert [g[0] for g in got] == [1, 0, 0]


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
let lamp = EmissiveMaterial {{ color: [17, 12, 4] }}
let mirror = MirrorMaterial {{ color: [0.9, 0.8, 0.7] }}
let glass = GlassMaterial {{ {glass} }}
let both = MixMaterial {{ fraction: 0.25, first: $mirror, second: $glass }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [16, 8] }},
    integrator: Path {{ spp: 2, max_depth: 3, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $both, $glass, $mirror, $lamp] }} ]
}}
"""


def _load(tmp_path, glass):
    p = tmp_path / "s.akari"
    p.write_text(SDL.format(glass=glass, out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    return scene.load_scene_file(p)


def test_parser_and_compiler(tmp_path):
    sc = _load(tmp_path, "color: [1, 1, 1], ior: 1.33")
    mats = sc.shapes[0].materials
    assert isinstance(mats[6], scene.MirrorMaterial) and mats[6].color.value == [float(F(x)) for x in (0.9, 0.8, 0.7)]
    assert isinstance(mats[5], scene.GlassMaterial) and mats[5].ior == float(F(1.33))
    assert isinstance(mats[4], scene.MixMaterial) and mats[4].first is mats[6] and mats[4].second is mats[5]
    assert _load(tmp_path, "color: [1, 1, 1]").shapes[0].materials[5].ior == 1.5      # the default
    cs = scene.compile_scene(sc)
    by_type = {m.type: m for m in cs.materials}
    assert {capi.MAT_MIRROR, capi.MAT_GLASS, capi.MAT_MIX} <= set(by_type)
    glass = by_type[capi.MAT_GLASS]
    ior_tex = cs.textures[glass.roughness]
    assert ior_tex.type == capi.TEX_CONSTANT and F(ior_tex.value[0]) == F(1.33)
    assert cs.textures[glass.color].value[0] == 1.0
    mix = by_type[capi.MAT_MIX]
    assert cs.materials[mix.first].type == capi.MAT_MIRROR and cs.materials[mix.second].type == capi.MAT_GLASS
    # the lights are still the Emissive triangles alone
    assert len(cs.lights) == 2
    # the two types and the ior are part of the scene's fingerprint
    other = scene.compile_scene(_load(tmp_path, "color: [1, 1, 1], ior: 1.34"))
    assert progressive.scene_fingerprint(cs) != progressive.scene_fingerprint(other)
    plain = specular_scenes.helpers.cornell((16, 8))
    swapped = specular_scenes.mirror_box((16, 8))
    assert progressive.scene_fingerprint(scene.compile_scene(plain)) != progressive.scene_fingerprint(scene.compile_scene(swapped))


def test_refusals(tmp_path):
    with pytest.raises(scene.SdlError, match="image-textured ior is not supported"):
        _load(tmp_path, 'color: [1, 1, 1], ior: "ior.npy"')
    for bad in ("0.5", "9", "-1.5"):
        with pytest.raises(scene.SdlError, match=r"not a finite number in \[1, 8\]"):
            _load(tmp_path, f"color: [1, 1, 1], ior: {bad}")
    with pytest.raises(scene.SdlError, match="ior is a number"):
        _load(tmp_path, "color: [1, 1, 1], ior: [1.5, 1.5, 1.5]")
    # the same through the scene compiler, for scenes built in Python
    ct = scene.ConstantTexture
    for ior, err in ((0.99, ValueError), (float("nan"), ValueError), (float("inf"), ValueError), (8.5, ValueError),
                     (ct([1.5] * 3), TypeError), (scene.ImageTexture(np.ones((2, 2, 4), np.float32)), TypeError)):
        sc = specular_scenes.helpers.cornell((8, 8))
        sc.shapes[0].materials[5] = scene.GlassMaterial(ct([1.0, 1.0, 1.0]), ior)
        with pytest.raises(err, match="GlassMaterial"):
            scene.compile_scene(sc)
    # and on the command line, before any device is touched
    p = tmp_path / "bad.akari"
    p.write_text(SDL.format(glass="color: [1, 1, 1], ior: 0.5", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    with pytest.raises(scene.SdlError, match="GlassMaterial"):
        render.main([str(p)])
    assert not (tmp_path / "o.pfm").exists()


def test_adapter_specular_demo_compiles_and_links(tmp_path):
    exe, lib = tmp_path / "specular_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "specular_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # without "run" it touches no device
