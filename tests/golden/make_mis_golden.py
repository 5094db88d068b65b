"""Generate the known answers of multiple importance sampling from the restatement
mis_restate.py:

  mis_golden_<scene>.npz     per-pixel radiance, weight, final sampler state and closest / shadow ray counts,
                             24 x 24 at 4 spp like the path and environment goldens, the switch on

The scenes are make_env_golden's (with their maps) and make_path_golden's (keys starting `noenv_`, no
environment).  Every new branch of the restatement has to be taken at least once over the set, and the
sampler states and ray counts have to equal the existing goldens' wherever those hold the same configuration:
the switch adds no draw and no ray.  Neither oracle/ nor the HIP library computes anything here.  Run (about
ten seconds on 16 cores):
    python tests/golden/make_mis_golden.py [<scene> ...]
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

import make_env_golden as G  # noqa: E402
import make_path_golden as M  # noqa: E402
import mis_restate as S  # noqa: E402
import ref_restate as R  # noqa: E402

F = np.float32
RES = (24, 24)
SPP = 4
# scene -> configurations (key, environment?, select_prob, depth, ray_clamp).  `noenv_black_d5` is `branches`
# with its ceiling light's colour set to 0: a listed triangle of power 0, so of selection pdf 0, which BSDF
# samples still hit from the front (the one terminal branch the unchanged scenes do not reach)
CONFIGS = {
    "sky": [("d3", True, 0.5, 3, 0.0)],
    "cornell": [("p50d1", True, 0.5, 1, 0.0), ("p50d2", True, 0.5, 2, 0.0), ("p50d5", True, 0.5, 5, 0.0),
                ("p25d5c10", True, 0.25, 5, 10.0), ("noenv_d2", False, 0.0, 2, 0.0), ("noenv_d5", False, 0.0, 5, 0.0)],
    "mixed": [("d5", True, 0.5, 5, 0.0)],
    "branches": [("noenv_d5", False, 0.0, 5, 0.0), ("noenv_black_d5", False, 0.0, 5, 0.0)],
}
# mis.pb_nonpositive: the pairable vertex whose sample carries nothing.  closure_sample's pdf is an absolute
# value times a quotient of squares, so "not positive" is 0 (a NaN would need cos^2 of the half vector to
# underflow), and a pdf of 0 also ends the path before direct lighting: the tick sits on that exit.
REQUIRED_BRANCHES = ["mis.term_env", "mis.term_area", "mis.term_area_back", "mis.term_area_pdf_nonpositive",
                     "mis.unpaired_last", "mis.unpaired_mix", "mis.pb_nonpositive"]


def build_scene(name, key, select_prob=0.5, resolution=RES):
    """The scene description of configuration `key` (what the device tests upload)."""
    if not key.startswith("noenv_"):
        return G.build_scene(name, resolution, select_prob)
    sc = M.build_scene(name, resolution)
    if key.startswith("noenv_black_"):
        from akari_amd import scene
        assert name == "branches"
        sc.shapes[0].materials[3] = scene.EmissiveMaterial(scene.ConstantTexture([0.0, 0.0, 0.0]))
    return sc


_G = {}


def _pixel(args):
    x, y, spp, depth, clamp, mis = args
    cnt = Counter()
    return S.render_pixel(_G["sc"], _G["env"], x, y, spp, depth, clamp, cnt, mis=mis), cnt


def render_pixels(sc, env, pixels, spp, depth, clamp, mis=True, parallel=True):
    _G["sc"], _G["env"] = sc, env
    if not hasattr(sc, "_mis_tri_sel"):   # built once, before the workers fork
        sc._mis_tri_sel = S.tri_select_pdf(sc)
    jobs = [(x, y, spp, depth, clamp, mis) for x, y in pixels]
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


def existing(name, key, env):
    """(seed, closest, shadow) of the existing golden with this configuration, or None."""
    if env:
        z = np.load(HERE / f"env_golden_{name}.npz")
        k = key
    else:
        z = np.load(HERE / f"path_golden_{name}.npz")
        k = key[len("noenv_"):]
        if k.startswith("black_"):
            return None
    if k + "_seed" not in z.files:
        return None
    return z[k + "_seed"], z[k + "_closest"], z[k + "_shadow"]


def make_scene_golden(name):
    data, counts = {}, Counter()
    for key, env_on, sp, depth, clamp in CONFIGS[name]:
        sc = R.RefScene(build_scene(name, key, sp))
        W, H = sc.camera.res
        px = [(x, y) for y in range(H) for x in range(W)]
        env = G.restated_env(name, sp) if env_on else None
        out, cnt = render_pixels(sc, env, px, SPP, depth, clamp)
        counts += cnt
        data[key + "_radiance"] = out["radiance"].reshape(H, W, 3)
        data[key + "_weight"] = out["weight"].reshape(H, W)
        data[key + "_seed"] = out["seed"].reshape(H, W)
        data[key + "_closest"] = out["closest"].reshape(H, W).astype(np.uint16)
        data[key + "_shadow"] = out["shadow"].reshape(H, W).astype(np.uint16)
        data[key + "_mask"] = out["ambiguous"].reshape(H, W)
        old = existing(name, key, env_on)
        if old is not None:   # the switch adds no draw and no ray
            assert np.array_equal(old[0], data[key + "_seed"]), (name, key, "sampler states differ from the existing golden")
            assert np.array_equal(old[1], data[key + "_closest"]), (name, key, "closest-hit counts differ")
            assert np.array_equal(old[2], data[key + "_shadow"]), (name, key, "shadow counts differ")
        print(f"{name} {key}: mean {out['radiance'].mean() / SPP:.4f} ambiguous {int(out['ambiguous'].sum())} "
              f"{'= existing seeds and counts' if old is not None else '(no existing golden)'}", flush=True)
        if env_on:
            assert not out["ambiguous"].any(), f"{name} {key}: ambiguous hits"
        else:
            assert out["ambiguous"].mean() <= 0.01, f"{name} {key}: more than 1 % of the pixels are ambiguous"
    data["counts"] = np.array(json.dumps(dict(sorted(counts.items()))))
    data["configs"] = np.array(json.dumps(CONFIGS[name]))
    np.savez_compressed(HERE / f"mis_golden_{name}.npz", **data)
    print(f"wrote mis_golden_{name}.npz counts { {k: v for k, v in sorted(counts.items()) if k.startswith('mis.')} }", flush=True)
    return counts


def main(argv):
    what = argv or list(CONFIGS)
    total = Counter()
    for name in CONFIGS:
        if name in what:
            total += make_scene_golden(name)
    if set(CONFIGS) <= set(what):
        lack = [b for b in REQUIRED_BRANCHES if total[b] < 1]
        assert not lack, f"branches never taken over all goldens: {lack}"
        print("every new branch taken:", {b: total[b] for b in REQUIRED_BRANCHES})


if __name__ == "__main__":
    main(sys.argv[1:])
