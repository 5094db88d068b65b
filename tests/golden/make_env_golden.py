"""Generate the environment light's known answers from the restatement env_restate.py:

  env_kat.json               function-level vectors, every float as its u32 bit pattern
  env_golden_<scene>.npz     per-pixel radiance, weight, final sampler state, closest / shadow ray
                             counts and the (empty) ambiguity mask, 24 x 24 at 4 spp like the path goldens
  env_golden_edges.npz       pixels of a 65535 x 65535 camera whose seed makes su.x exactly select_prob,
                             or the environment's lu.x or lu.y exactly 0 (found by inverting the LCG)

Maps come from an integer hash, so nothing large is stored.  Neither oracle/ nor the HIP library
computes anything here.  Run (about a minute on 16 cores):
    python tests/golden/make_env_golden.py [kat] [edges] [<scene> ...]
"""
import json
import sys
from collections import Counter
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
for p in (HERE, HERE.parent, ROOT / "akarirender-1_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import env_restate as E  # noqa: E402
import make_path_golden as M  # noqa: E402
import ref_restate as R  # noqa: E402

F = np.float32
RES = (24, 24)
SPP = 4
# scene -> configurations (key, select_prob, depth, ray_clamp)
CONFIGS = {
    "sky": [("d0", 0.5, 0, 0.0), ("d3", 0.5, 3, 0.0)],
    "cornell": [("p50d0", 0.5, 0, 0.0), ("p50d1", 0.5, 1, 0.0), ("p50d5", 0.5, 5, 0.0), ("p25d5c10", 0.25, 5, 10.0)],
    "mixed": [("d5", 0.5, 5, 0.0)],
}
REQUIRED_BRANCHES = ["miss.sky", "miss", "env.lit", "env.occluded", "env.black", "direct.lit", "direct.occluded"]


def hash_map(n, seed):
    """n x n x 3 texels in [0.25, 1.25) in steps of 1 / 256 from an integer hash (exact in f32)."""
    k = np.arange(n * n * 3, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B1)
    k = (k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    k ^= k >> np.uint64(15)
    k = (k * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    k ^= k >> np.uint64(13)
    return ((((k >> np.uint64(8)) & np.uint64(0xFF)).astype(np.float32) + F(64)) / F(256)).reshape(n, n, 3)


def rotation(axis, degrees):
    """Rodrigues in double -> the 3x3 M of d_world = M d_env."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def env_spec(name):
    """-> dict(map [N, N, 3] f32, scale, M (d_world = M d_env, f64 3x3)): the scene's environment."""
    if name == "sky":          # N = 8, one texel 1000 x the rest, above the ground (x, y > 0, z > 0)
        m = hash_map(8, 1)
        m[5, 5] *= F(1000.0)
        return dict(map=m, scale=(1.0, 1.0, 1.0), M=np.eye(3))
    if name == "cornell":      # N = 5 (odd: texel centres on the axes), turned, scaled per channel
        return dict(map=hash_map(5, 2), scale=(2.0, 1.5, 0.75), M=rotation((1.0, 2.0, 3.0), 40.0))
    if name == "skyturned":    # the edge pixels' scene: the sky scene's geometry under the turned N = 5 map
        return env_spec("cornell")
    if name == "mixed":        # N = 1: a constant sky, every direction the one texel
        return dict(map=hash_map(1, 3), scale=(1.0, 1.0, 1.0), M=np.eye(3))
    raise KeyError(name)


def sky_scene(resolution=RES):
    """A ground quad and a box under the open sky, no area light; the camera looks along +x from
    above the ground, so the frame holds sky on both sides of the map's fold (z = 0)."""
    from akari_amd import scene
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.55, 0.5])), scene.DiffuseMaterial(ct([0.3, 0.5, 0.7])),
            scene.GlossyMaterial(ct([0.9, 0.9, 0.9]), ct([0.3, 0.3, 0.3]))]
    tris = []

    def quad(a, b, c, d, n, mat):
        tris.append(([a, b, c], n, [0, 0, 1, 0, 1, 1], mat))
        tris.append(([a, c, d], n, [0, 0, 1, 1, 0, 1], mat))

    g = 4.03
    quad((-g, 0, -g), (-g, 0, g), (g, 0, g), (g, 0, -g), (0, 1, 0), 0)
    x0, x1, y0, y1, z0, z1 = 0.81, 1.93, 0.0, 1.17, -0.97, 0.43
    quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (-1, 0, 0), 1)
    quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), (1, 0, 0), 1)
    quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (0, 1, 0), 2)
    quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), (0, 0, -1), 1)
    quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (0, 0, 1), 2)
    verts = np.array([p for t in tris for p in t[0]], np.float32)
    mesh = scene.Mesh(verts, np.arange(len(verts), dtype=np.int32).reshape(-1, 3),
                      np.array([list(t[1]) * 3 for t in tris], np.float32), np.array([t[2] for t in tris], np.float32),
                      np.array([t[3] for t in tris], np.int32), mats)
    cam = scene.PerspectiveCamera(position=(-3.1, 1.3, 0.07), rotation=SKY_CAMERA_ROTATION, fov=80.0,
                                  resolution=tuple(resolution))
    return scene.Scene(camera=cam, shapes=[mesh])


SKY_CAMERA_ROTATION = (-90.0, 4.0, 0.0)


def build_scene(name, resolution=RES, select_prob=0.5):
    """The scene description with its EnvironmentLight (what the device tests upload)."""
    from akari_amd import scene
    sc = sky_scene(resolution) if name in ("sky", "skyturned") else M.build_scene(name, resolution)
    spec = env_spec(name)
    sc.environment = scene.EnvironmentLight(spec["map"], layout="octahedral", scale=spec["scale"], rotation=spec["M"],
                                            select_prob=select_prob)
    return sc


def restated_env(name, select_prob=0.5):
    spec = env_spec(name)
    return E.Environment(spec["map"], spec["scale"], select_prob, np.ascontiguousarray(spec["M"].T).astype(np.float32))


_G = {}


def _pixel(args):
    x, y, spp, depth, clamp = args
    cnt = Counter()
    return E.render_pixel(_G["sc"], _G["env"], x, y, spp, depth, clamp, cnt), cnt


def render_pixels(sc, env, pixels, spp, depth, clamp, parallel=True):
    _G["sc"], _G["env"] = sc, env
    jobs = [(x, y, spp, depth, clamp) for x, y in pixels]
    if parallel:
        with M._pool() as pool:
            res = pool.map(_pixel, jobs, chunksize=8)
    else:
        res = [_pixel(j) for j in jobs]
    n = len(pixels)
    out = dict(radiance=np.zeros((n, 3), np.float32), weight=np.zeros(n, np.float32), seed=np.zeros(n, np.uint32),
               closest=np.zeros(n, np.uint32), shadow=np.zeros(n, np.uint32), ambiguous=np.zeros(n, bool))
    total = Counter()
    for i, (r, cnt) in enumerate(res):
        total += cnt
        for k in out:
            out[k][i] = r[k]
    return out, total


def make_scene_golden(name):
    sc = R.RefScene(build_scene(name))
    W, H = sc.camera.res
    px = [(x, y) for y in range(H) for x in range(W)]
    data, counts = {}, Counter()
    mask = np.zeros(W * H, bool)
    for key, sp, depth, clamp in CONFIGS[name]:
        out, cnt = render_pixels(sc, restated_env(name, sp), px, SPP, depth, clamp)
        counts += cnt
        data[key + "_radiance"] = out["radiance"].reshape(H, W, 3)
        data[key + "_weight"] = out["weight"].reshape(H, W)
        data[key + "_seed"] = out["seed"].reshape(H, W)
        data[key + "_closest"] = out["closest"].reshape(H, W).astype(np.uint16)
        data[key + "_shadow"] = out["shadow"].reshape(H, W).astype(np.uint16)
        mask |= out["ambiguous"]
        print(f"{name} {key}: mean {out['radiance'].mean() / SPP:.4f} ambiguous {int(out['ambiguous'].sum())}", flush=True)
    assert not mask.any(), f"{name}: {int(mask.sum())} pixels have an ambiguous hit: move the geometry"
    if name == "sky":   # sky in part of the frame, on both sides of the fold
        env = restated_env(name)
        cam = sc.camera
        z = []
        for x, y in px:
            s = R.LCG(x + y * W)
            o, d = cam.generate_ray(s.next2d(), s.next2d(), (x, y))
            if R.Tracer(sc).intersect(o, d, R.EPS, R.INF) is None:
                z.append(float(env.to_map(d)[2]))
        assert 0 < len(z) < W * H and min(z) < 0 < max(z), (len(z), min(z, default=0), max(z, default=0))
        print(f"sky: {len(z)} of {W * H} first camera rays see the map, z from {min(z):.3f} to {max(z):.3f}")
    data["mask"] = mask.reshape(H, W)
    data["counts"] = np.array(json.dumps(dict(sorted(counts.items()))))
    data["configs"] = np.array(json.dumps(CONFIGS[name]))
    np.savez_compressed(HERE / f"env_golden_{name}.npz", **data)
    print(f"wrote env_golden_{name}.npz counts {dict(sorted(counts.items()))}", flush=True)
    return counts


# ----------------------------------------------------------------------------- edge pixels
EDGE_W, EDGE_SPP, EDGE_DEPTH = 65535, 2, 5
# role -> (scene, value its draw must show, sampler states whose draw is that value): su.x exactly
# select_prob beside area lights (the environment is NOT taken: su.x < select_prob fails, and the area
# lights' remapped draw is 0), and the environment's lu.x and lu.y exactly 0 (the first texel's edge,
# in-texel offset 0) where the environment is the only light.  Both maps are turned, so that no sampled
# direction has a zero component (which the brute-force tracer would flag as builder dependent).
EDGE_ROLES = {"light_select": ("cornell", 0.5, M._AT(0.5)), "env_ux": ("skyturned", 0.0, [0]),
              "env_uy": ("skyturned", 0.0, [0])}


def _edge_try(args):
    name, seed0, role, want = args
    x, y = seed0 % EDGE_W, seed0 // EDGE_W
    if y >= EDGE_W:
        return None
    roles = []
    r = E.render_pixel(_G["edge_sc_" + name], _G["edge_env_" + name], x, y, EDGE_SPP, EDGE_DEPTH, 0.0, None, EDGE_W, roles)
    if r["ambiguous"] or not any(k == role and v == F(want) for k, v in roles):
        return None
    return dict(scene=name, role=role, value=want, x=x, y=y, **{k: r[k] for k in ("radiance", "weight", "seed", "closest", "shadow")})


def make_edges():
    """As make_path_golden.make_edges: walk the LCG backwards from a state whose draw is the wanted value
    to candidate pixel seeds x + y * 65535, and keep the first pixel in which the draw lands on the role."""
    for name in sorted({v[0] for v in EDGE_ROLES.values()}):
        _G["edge_sc_" + name] = R.RefScene(build_scene(name, (EDGE_W, EDGE_W)))
        _G["edge_env_" + name] = restated_env(name)
    found = []
    pool = M._pool()
    for role, (name, want, states) in EDGE_ROLES.items():
        jobs = []
        for st in states:
            s = st
            for back in range(1, 41):
                s = R.lcg_prev(s)
                if back >= 5:                    # the first four draws are the camera's
                    jobs.append((name, s, role, want))
        hit = next((r for r in pool.imap(_edge_try, jobs, chunksize=4) if r is not None), None)
        assert hit is not None, f"no pixel reaches {role} = {want}"
        found.append(hit)
        print("edge", role, want, "->", (hit["x"], hit["y"]), flush=True)
    pool.terminate()
    np.savez_compressed(HERE / "env_golden_edges.npz", scene=np.array([f["scene"] for f in found]),
                        role=np.array([f["role"] for f in found]),
                        value=np.array([f["value"] for f in found], np.float32),
                        xy=np.array([[f["x"], f["y"]] for f in found], np.int32),
                        radiance=np.array([f["radiance"] for f in found], np.float32),
                        weight=np.array([f["weight"] for f in found], np.float32),
                        seed=np.array([f["seed"] for f in found], np.uint32),
                        closest=np.array([f["closest"] for f in found], np.uint32),
                        shadow=np.array([f["shadow"] for f in found], np.uint32),
                        params=np.array([EDGE_W, EDGE_SPP, EDGE_DEPTH], np.int32))
    print("wrote env_golden_edges.npz", flush=True)


# ----------------------------------------------------------------------------- function vectors
b32 = M.b32
KAT_MAPS = {"n1": (1, 11), "n2": (2, 12), "n5": (5, 13), "n8": (8, 14)}


def kat_env(tag):
    """The maps of the function vectors: n5 is turned and scaled, n8 has the sky scene's bright texel
    and a black row (a conditional with integral 0) and a black last column."""
    n, seed = KAT_MAPS[tag]
    m = hash_map(n, seed)
    scale, Mx = (1.0, 1.0, 1.0), np.eye(3)
    if tag == "n5":
        scale, Mx = (2.0, 1.5, 0.75), rotation((1.0, 2.0, 3.0), 40.0)
    if tag == "n8":
        m[5, 5] *= F(1000.0)
        m[2, :, :] = 0
        m[:, 7, :] = 0
    return dict(map=m, scale=scale, M=Mx)


def kat_environment(tag):
    s = kat_env(tag)
    return E.Environment(s["map"], s["scale"], 0.5, np.ascontiguousarray(s["M"].T).astype(np.float32))


def make_kat():
    kat = {}
    below, above = M.below, M.above
    # decode / encode: the six axes, the fold line |x| + |y| = 1, the four corners, the centre
    pts = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (0.5, 0.5), (-0.5, 0.5),
           (0.25, -0.75), (-0.75, -0.25), (below(0.5), 0.5), (above(0.5), 0.5), (-0.0, 0.3), (0.3, -0.0), (0.9, 0.9),
           (-0.0, -0.0)]
    r = M.lcg_floats(51, 40)
    pts = [R.vec(p) for p in pts] + [(F(F(2) * r[2 * i] - F(1)), F(F(2) * r[2 * i + 1] - F(1))) for i in range(20)]
    kat["decode"] = {"xy": b32(pts), "out": b32([E.decode(x, y)[0] + (E.decode(x, y)[1],) for x, y in pts])}
    dirs = [R.vec(d) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, 0.0, -1.0))]
    dirs += [E.decode(x, y)[0] for x, y in pts] + M.unit_vecs(53, 24)
    for tag in KAT_MAPS:
        env = kat_environment(tag)
        n = env.n
        ev = [env.eval(d) for d in dirs]
        us = [R.vec(u) for u in ((0, 0), (1, 1), (0.5, 0.5), (0, 1), (1, 0), (below(1.0), below(1.0)), (0.25, 0.75))]
        rr = M.lcg_floats(57 + n, 80)
        us += [(rr[2 * i], rr[2 * i + 1]) for i in range(40)]
        # every CDF knot of the marginal and of one row, the draws just below and above it
        for c in env.marginal.cdf[1:-1][:4]:
            us += [(F(0.3), below(c)), (F(0.3), c), (F(0.3), above(c))]
        for c in env.rows[n // 2].cdf[1:-1][:4]:
            us += [(below(c), F(0.6)), (c, F(0.6)), (above(c), F(0.6))]
        sm = [env.sample(u) for u in us]
        kat[tag] = {"n": n, "dirs": b32(dirs), "eval_rgb": b32([e[0] for e in ev]), "eval_pdf": b32([e[1] for e in ev]),
                    "eval_ij": [list(e[2]) for e in ev],
                    "u": b32(us), "sample_dir": b32([s[0] for s in sm]), "sample_rgb": b32([s[1] for s in sm]),
                    "sample_pdf": b32([s[2] for s in sm]), "sample_ij": [list(s[3]) for s in sm],
                    "marginal_cdf": b32(env.marginal.cdf), "row_cdf": b32(env.rows[n // 2].cdf)}
        # encode(decode(centre of every texel)) is that texel
        for j in range(n):
            for i in range(n):
                d, _ = E.decode(E.texel_point(i, 0.5, n), E.texel_point(j, 0.5, n))
                assert E.encode(d, n)[:2] == (i, j), (tag, i, j)
    (HERE / "env_kat.json").write_text(json.dumps(kat, separators=(",", ":")))
    print("wrote env_kat.json", {k: len(v.get("u", v.get("xy"))) // 2 for k, v in kat.items()})


def main(argv):
    what = argv or ["kat", *CONFIGS, "edges"]
    if "kat" in what:
        make_kat()
    total = Counter()
    for name in CONFIGS:
        if name in what:
            total += make_scene_golden(name)
    if set(CONFIGS) <= set(what):
        lack = [b for b in REQUIRED_BRANCHES if total[b] < 1]
        assert not lack, f"branches never taken over all goldens: {lack}"
    if "edges" in what:
        make_edges()


if __name__ == "__main__":
    main(sys.argv[1:])
