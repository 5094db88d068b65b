"""The oracle against an independent restatement of the reference's shading and path loop.

tests/golden/ref_restate.py is a second reading of the reference source in numpy f32, written
without the oracle or the device code; tests/golden/make_path_golden.py ran it into
path_kat.json (function-level vectors) and path_golden_<scene>.npz (per-pixel results).  The
oracle has to equal both bit for bit: a misreading shared by the oracle and the device code, which
the device-against-oracle tests cannot see, shows up here.  NaNs compare equal to NaNs (IEEE leaves
their sign and payload open); everything else is compared as u32 bit patterns.
"""
import json
import sys

import numpy as np
import pytest

import py_oracle as O
from akari_amd import capi, scene
from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import make_path_golden as M  # noqa: E402

KAT = json.loads((GOLDEN / "path_kat.json").read_text())


def f32(bits, k=None):
    a = np.array(bits, np.uint32).view(np.float32)
    return a if k is None else a.reshape(-1, k)


def same_bits(got, want):
    """Bit-equal, NaN matching NaN.  -> number of differing elements."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32).reshape(np.shape(got))
    nan = np.isnan(got) & np.isnan(want)
    return int(np.count_nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan))


def check(got, want, what):
    bad = same_bits(got, want)
    assert bad == 0, f"{what}: {bad} of {np.size(got)} values differ from the independent restatement"


_SCENES = {}


def oracle_scene(name):
    """(description, compiled scene, oracle scene over a host-built BVH), built once per name."""
    if name not in _SCENES:
        sc = M.build_scene(name)
        cs = scene.compile_scene(sc)
        nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
        _SCENES[name] = (sc, cs, O.OracleScene(cs, nodes, tris, capi))
    return _SCENES[name]


def golden(name):
    return np.load(GOLDEN / f"path_golden_{name}.npz")


# ----------------------------------------------------------------------------- function level
def test_disk_and_cosine_warps():
    check(O.unit_disk(f32(KAT["disk"]["u"], 2)), f32(KAT["disk"]["out"], 2), "concentric disk")
    check(O.cosine_hemisphere(f32(KAT["cosine"]["u"], 2)), f32(KAT["cosine"]["out"], 3), "cosine hemisphere")


def test_frame():
    k = KAT["frame"]
    check(O.unit_frame(f32(k["n"], 3), f32(k["w"], 3)), f32(k["out"], 12), "Frame T, B, to_local, to_world")


def test_ggx_d_g1_and_sample_wh():
    k = KAT["ggx"]
    check(O.unit_ggx(f32(k["alpha"]), f32(k["v"], 3), f32(k["m"], 3)), f32(k["out"], 2), "GGX D, G1")
    k = KAT["sample_wh"]
    check(O.unit_sample_wh(f32(k["alpha"]), f32(k["wo"], 3), f32(k["u"], 2)), f32(k["out"], 3), "GGX sample_wh")


@pytest.mark.parametrize("name", ["diffuse", "glossy"])
def test_closures(name):
    k = KAT[name + "_eval"]
    n = len(k["alpha"])
    R = np.tile(f32(k["R"]), (n, 1))
    check(O.unit_closure_eval(k["kind"], R, f32(k["alpha"]), f32(k["wo"], 3), f32(k["wi"], 3)), f32(k["out"], 3),
          name + " evaluate")
    k = KAT[name + "_sample"]
    n = len(k["alpha"])
    R = np.tile(f32(k["R"]), (n, 1))
    check(O.unit_closure_sample(k["kind"], R, f32(k["alpha"]), f32(k["u"], 2), f32(k["wo"], 3)), f32(k["out"], 7),
          name + " sample (f, wi, pdf)")


def test_texture_lookup():
    sc, cs, orc = oracle_scene("kat")
    for k in KAT["texture"]:
        tex = cs.materials[cs.mesh_slots[0][k["slot"]]].color
        check(orc.unit_texture(tex, f32(k["tc"], 2)), f32(k["out"], 3), f"texture of material slot {k['slot']}")


def test_select_material():
    sc, cs, orc = oracle_scene("kat")
    names = {capi.MAT_DIFFUSE: "diffuse", capi.MAT_GLOSSY: "glossy", capi.MAT_EMISSIVE: "emissive", capi.MAT_MIX: "mix"}
    for k in KAT["select_material"]:
        leaf, out = orc.unit_select_material(cs.mesh_slots[0][k["slot"]], f32(k["u"]), f32(k["tc"], 2))
        check(out, f32(k["out"], 2), f"select_material slot {k['slot']} (choice pdf, rescaled u)")
        for i, (kind, colour) in enumerate(k["leaf"]):
            m = cs.materials[leaf[i]]
            got = np.array(list(cs.textures[m.color].value), np.float32)
            assert names[m.type] == kind and same_bits(got, f32(colour)) == 0, \
                f"slot {k['slot']} draw {i}: resolved to {names[m.type]} {got}, restatement says {kind} {f32(colour)}"


def test_triangle_and_light_sample():
    sc, cs, orc = oracle_scene("kat")
    for k in KAT["triangle"]:
        check(orc.unit_triangle(k["gid"], f32(k["uv"], 2)), f32(k["out"], 12), f"triangle {k['gid']} p, ng, ns, tc, area")
    for k in KAT["light_sample"]:
        check(orc.unit_light_sample(k["gid"], f32(k["u"], 2), f32(k["p"], 3)), f32(k["out"], 15),
              f"light sample on triangle {k['gid']}")


def test_camera():
    for k in KAT["camera"]:
        cam = scene.PerspectiveCamera(tuple(k["position"]), tuple(k["rotation"]), k["fov"], tuple(k["resolution"]))
        r2c, c2w = O.camera_matrices(cam, capi)
        check(r2c, f32(k["r2c"]), "camera r2c")
        check(c2w, f32(k["c2w"]), "camera c2w")
        for r in k["rays"]:
            ray, final = O.camera_ray(cam, capi, r["x"], r["y"], r["seed"])
            check(ray["o"], f32(r["o"]), "camera ray origin")
            check(ray["d"], f32(r["d"]), "camera ray direction")
            assert final == r["final_seed"]


def test_distribution_and_light_list():
    for k in KAT["dist"]:
        idx, pdf = O.distribution_sample(f32(k["func"]), f32(k["u"]))
        assert idx.tolist() == k["idx"]
        check(pdf, f32(k["pdf"]), "Distribution1D pdf")
    sc, cs, orc = oracle_scene("kat")
    assert cs.light_gid.tolist() == KAT["kat_scene_lights"]["gid"]
    check(cs.power, f32(KAT["kat_scene_lights"]["power"]), "light power")


# ----------------------------------------------------------------------------- path level
CASES = [(name, depth, clamp) for name, cfgs in M.CONFIGS.items() for depth, clamp in cfgs]


def compare_with_golden(g, key, mask, rad, w, probe, what):
    """Radiance, weights, final sampler states and ray counts outside the ambiguity mask."""
    keep = ~mask
    check(rad[keep], g[key + "_radiance"][keep], what + " radiance")
    check(w[keep], g[key + "_weight"][keep], what + " weight")
    bad = np.count_nonzero(probe["seed"][keep] != g[key + "_seed"][keep])
    assert bad == 0, f"{what}: {bad} final sampler states differ"
    if np.all(probe["flags"] & capi.PROBE_RAYS):
        for k in ("closest", "shadow"):
            bad = np.count_nonzero(probe[k + "_rays"][keep] != g[f"{key}_{k}"][keep])
            assert bad == 0, f"{what}: {bad} per-pixel {k} ray counts differ"
        return True
    return False


@pytest.mark.parametrize("name,depth,clamp", CASES)
def test_oracle_render_equals_golden(name, depth, clamp):
    sc, cs, orc = oracle_scene(name)
    g = golden(name)
    rad, w, _, probe = orc.render(M.SPP, depth, ray_clamp=clamp, probe=True, n_threads=4)
    assert compare_with_golden(g, M.cfg_key(depth, clamp), g["mask"], rad, w, probe, f"{name} depth {depth}")


@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_light_list_camera_rays_and_hits(name):
    sc, cs, orc = oracle_scene(name)
    g = golden(name)
    assert cs.light_gid.tolist() == g["light_gid"].tolist()
    check(cs.power, g["light_power"], "light power")
    H, W = g["mask"].shape
    rays = np.zeros(H * W, capi.RAY_DTYPE)
    rays["o"], rays["d"] = g["ray_o"].reshape(-1, 3), g["ray_d"].reshape(-1, 3)
    rays["tmin"], rays["tmax"] = np.float32(0.001), np.inf
    for y in (0, H // 2, H - 1):            # the stored rays are the camera's
        for x in (0, W // 3, W - 1):
            ray, _ = O.camera_ray(sc.camera, capi, x, y, x + y * W)
            check(ray["o"], g["ray_o"][y, x], "camera ray origin")
            check(ray["d"], g["ray_d"][y, x], "camera ray direction")
    keep = ~g["mask"].reshape(-1)
    for hits in (orc.trace(rays, n_threads=2)[0], orc.trace_brute(rays, n_threads=2)):
        check_hits(hits["gid"], hits["t"], hits["u"], hits["v"], g, keep)


def check_hits(gid, t, u, v, g, keep):
    """Hits of the stored camera rays: ids equal up to exact duplicate triangles, t, u, v bits."""
    want = g["hit_gid"].reshape(-1)
    canon = np.append(g["canon"], 0xFFFFFFFF).astype(np.uint32)
    look = lambda a: canon[np.where(a == 0xFFFFFFFF, len(canon) - 1, a)]
    assert np.array_equal(look(np.asarray(gid, np.uint32))[keep], look(want)[keep])
    hit = keep & (want != 0xFFFFFFFF)
    tuv = g["hit_tuv"].reshape(-1, 3)
    check(np.stack([t, u, v], axis=1)[hit], tuv[hit], "t, u, v of the camera hits")


@pytest.mark.parametrize("name", ["mixed", "branches"])
def test_generator_reproduces_committed_block(name):
    """The golden cannot drift from its generator: a 4x4 block at 2 spp, run again."""
    g = golden(name)
    for k, v in M.regen_block(name).items():
        assert np.array_equal(np.asarray(v).view(np.uint32), g["block_" + k].view(np.uint32)), f"{name} block {k}"


def test_ambiguity_masks_small():
    for name in M.CONFIGS:
        share = golden(name)["mask"].mean()
        assert share <= 0.01, f"{name}: {share:.2%} of the pixels are masked"


def test_every_branch_taken():
    total = {}
    for name in M.CONFIGS:
        for k, v in json.loads(str(golden(name)["counts"])).items():
            total[k] = total.get(k, 0) + v
    lack = [b for b in M.REQUIRED_BRANCHES if total.get(b, 0) < 1]
    assert not lack, f"branches never taken over all goldens: {lack}"


def test_sampler_extreme_pixels():
    """Pixels of a 65535 x 65535 camera whose seed x + y * W makes one draw exactly 0.0 or 1.0 as the
    light-selection draw, a light-sample coordinate or the GGX u.x, or lands a Mix draw exactly on
    its fraction (the u < frac boundary): the oracle's packed per-pixel render against the golden."""
    e = np.load(GOLDEN / "path_golden_edges.npz")
    got = set(zip(e["role"].tolist(), e["value"].tolist()))
    assert {("light_select", 0.0), ("light_select", 1.0), ("light_ux", 0.0), ("light_ux", 1.0)} <= got
    W, spp, depth = (int(v) for v in e["params"])
    for name in sorted(set(e["scene"].tolist())):
        idx = np.nonzero(e["scene"] == name)[0]
        sc = M.build_scene(name, (W, W))
        cs = scene.compile_scene(sc)
        nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
        rad, w, pr = O.OracleScene(cs, nodes, tris, capi).render_pixels(e["xy"][idx], spp, depth)
        what = f"{name} pixels {e['role'][idx].tolist()}"
        check(rad, e["radiance"][idx], what + " radiance")
        check(w, e["weight"][idx], what + " weight")
        assert np.array_equal(pr["seed"], e["seed"][idx]), what + " final sampler state"
        assert np.array_equal(pr["closest_rays"], e["closest"][idx]), what + " closest rays"
        assert np.array_equal(pr["shadow_rays"], e["shadow"][idx]), what + " shadow rays"
