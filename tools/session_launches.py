"""Launch counts of one small session script under option stats, build by build: what a host-side change of
the session calls must leave as it was.  Each library runs in its own process (AKR_HIP_LIB; an experiment
library lives in tools/experiments/lib/): a 40x24 Cornell box with ragged tiles, render 3 spp, continue 2,
masked continue 5, adaptive render to 8, variance export, features 2 spp, both denoisers.  Prints every
build's {kernel name: launches} and whether they are the same; exits 1 when they differ.

Usage (GPU box): python tools/session_launches.py akarirender-1_amd/libakr_hip.so tools/experiments/lib/libakr_hip_x.so"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "akarirender-1_amd"))
W, H, DEPTH = 40, 24, 5
TILES = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 40, 24)]


def worker():
    import numpy as np
    from akari_amd import capi, dist, scene
    mesh = ROOT / "tests" / "golden" / "CornellBox-Original.obj.mesh"
    cs = scene.compile_scene(scene.cornell_scene(mesh, resolution=(W, H)))
    with capi.HipContext(0) as ctx:
        scene.upload_scene(ctx, cs)
        ctx.set_option("stats", 1)
        ctx.set_option("film_variance", 1)
        mask = (np.arange(dist.n_pixels(TILES)) % 2).astype(np.uint8)
        ctx.render(3, DEPTH, TILES, W, H)
        ctx.render_continue(2, W, H)
        ctx.render_continue_masked(5, mask, W, H)
        rad, w, info = ctx.render_adaptive(8, DEPTH, TILES, W, H, 0.05, min_spp=4)
        var = ctx.render_variance(W, H)
        feat = ctx.render_features(2, TILES, W, H)
        ctx.denoise(rad, w, feat)
        ctx.denoise_guided(rad, w, feat, var)
        stats = {k: int(v["launches"]) for k, v in ctx.kernel_stats().items()}
    print("RESULT " + json.dumps({"launches": stats, "adaptive": info, "film_sum": float(rad.sum())}, sort_keys=True), flush=True)


def main():
    if sys.argv[1:] == ["--worker"]:
        return worker()
    seen = []
    for lib in sys.argv[1:]:
        p = subprocess.run([sys.executable, __file__, "--worker"], env=dict(os.environ, AKR_HIP_LIB=str(Path(lib).resolve())),
                           capture_output=True, text=True, timeout=300)
        line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(p.stdout[-2000:], p.stderr[-3000:], flush=True)
            raise SystemExit(f"{lib}: worker failed with {p.returncode}")
        seen.append(json.loads(line[7:]))
        print(f"{lib}\n  {json.dumps(seen[-1], sort_keys=True)}", flush=True)
    same = all(s == seen[0] for s in seen)
    print("launch counts, adaptive info and film sum: " + ("the same in every build" if same else "DIFFERENT"), flush=True)
    raise SystemExit(0 if same else 1)


if __name__ == "__main__":
    main()
