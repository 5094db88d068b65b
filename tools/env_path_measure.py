"""What option env_path buys: a scene under envmap.procedural_sky(1024) rendered by the parent
commit's library, where an environment forces the wavefront form, against this tree's library with env_path 1
and path 1, where k_path's environment build runs.  1920 x 1080, max_depth 5, verify on; the Cornell box at
256 spp and the C3 soup view at 64 spp.  Each configuration runs in a process of its own with one context
(AKR_HIP_LIB; several contexts in a process share its hardware queues and serialise the wavefront's streams),
parent and tree alternating for --repeat rounds.  A process renders the shape once to warm up, then the timed
render (wall ms per spp), then a render of its own with option stats (per-kernel ms per spp), and prints a
hash of the timed render's film.

Usage (GPU box): python tools/env_path_measure.py --parent tools/experiments/lib/libakr_hip_parent.so
                 [--tree akarirender-1_amd/libakr_hip.so] [--repeat 3] [--scenes cornell,soup]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "akarirender-1_amd"))
W, H, DEPTH = 1920, 1080, 5
SPP = {"cornell": 256, "soup": 64}
MESH = ROOT / "tests" / "golden" / "CornellBox-Original.obj.mesh"


def build_scene(name, tris):
    from akari_amd import envmap, scene
    sc = scene.cornell_scene(MESH, resolution=(W, H)) if name == "cornell" else scene.soup_scene(n_tris=tris, resolution=(W, H))
    sc.environment = scene.EnvironmentLight(envmap.procedural_sky(1024), layout="octahedral")
    return scene.compile_scene(sc)


def worker(args):
    import numpy as np
    import torch
    from akari_amd import capi, dist, scene
    cs = build_scene(args.scene, args.tris)
    ctx = capi.HipContext(0)
    for kv in (x for x in args.opts.split(",") if x):
        k, _, v = kv.partition("=")
        ctx.set_option(k, int(v))
    if args.scene == "soup":
        nodes, tris = np.load(args.bvh + "_nodes.npy", mmap_mode="r"), np.load(args.bvh + "_tris.npy", mmap_mode="r")
        scene.upload_scene(ctx, cs, bvh=(nodes, tris), n_threads=16)
    else:
        scene.upload_scene(ctx, cs, n_threads=16)
    dev = torch.device("cuda", 0)
    tiles = dist.tile_grid(W, H, 64)
    n = dist.n_pixels(tiles)
    buf = torch.zeros(4 * n, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    spp = SPP[args.scene]

    def render():
        ctx.render_device(spp, DEPTH, tiles, buf[:3 * n].data_ptr(), buf[3 * n:].data_ptr(), stream)
        torch.cuda.synchronize(dev)

    render()                      # warm-up: the same shape
    t = time.perf_counter()
    render()
    wall = (time.perf_counter() - t) / spp * 1e3
    out = {"wall_ms_per_spp": round(wall, 4), "form": ctx.render_form()["form"], "shading": ctx.render_info()["shading"],
           "film_sha256": hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest(),
           "mean": round(float(buf[:3 * n].mean().item()) / spp, 5)}
    ctx.reset_stats()             # a render of its own with HIP events on every launch
    ctx.set_option("stats", 1)
    render()
    ctx.set_option("stats", 0)
    ks = ctx.kernel_stats()
    out["kernel_ms_per_spp"] = {k: round(v["total_ms"] / spp, 4) for k, v in ks.items() if v["launches"]}
    out["kernels_sum_ms_per_spp"] = round(sum(v["total_ms"] for v in ks.values()) / spp, 4)
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="tools/experiments/lib/libakr_hip_parent.so")
    ap.add_argument("--tree", default="akarirender-1_amd/libakr_hip.so")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--scenes", default="cornell,soup")
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--opts", default="")
    ap.add_argument("--bvh", default="/tmp/akr_env_path_bvh")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    scenes = [s for s in args.scenes.split(",") if s]
    sides = {"parent": (args.parent, ""), "tree": (args.tree, "env_path=1,path=1")}
    print(f"# {W}x{H}, max_depth {DEPTH}, procedural_sky(1024), verify on; spp {SPP}; parent: default options (an "
          f"environment forces the wavefront), tree: env_path 1, path 1; one process and one context per line", flush=True)
    if "soup" in scenes:
        import numpy as np
        from akari_amd import capi, scene
        t0 = time.time()
        cs = scene.compile_scene(scene.soup_scene(n_tris=args.tris, resolution=(W, H)))
        nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices, builder=capi.BUILDER_SBVH, n_threads=16)
        np.save(args.bvh + "_nodes.npy", nodes)
        np.save(args.bvh + "_tris.npy", tris)
        del nodes, tris, cs
        print(f"# soup SBVH built once and saved in {time.time() - t0:.1f} s", flush=True)
    res = {(s, side): [] for s in scenes for side in sides}
    try:
        for rep in range(args.repeat):
            for s in scenes:
                for side, (lib, opts) in sides.items():
                    env = dict(os.environ, AKR_HIP_LIB=str(Path(lib).resolve()))
                    cmd = [sys.executable, __file__, "--worker", "--scene", s, "--opts", opts, "--tris", str(args.tris),
                           "--bvh", args.bvh]
                    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
                    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
                    if p.returncode != 0 or line is None:   # a failed process ends the measurement: nothing more is started
                        print(p.stdout[-2000:], p.stderr[-3000:], flush=True)
                        raise SystemExit(f"{s} {side}: worker ended with {p.returncode}")
                    r = json.loads(line[7:])
                    res[(s, side)].append(r)
                    print(json.dumps({"scene": s, "side": side, "round": rep + 1, **r}), flush=True)
    finally:
        for suf in ("_nodes.npy", "_tris.npy"):
            Path(args.bvh + suf).unlink(missing_ok=True)
    print("# summary: wall ms per spp (median of the rounds; spread = max - min), the films, and the kernels' time", flush=True)
    for s in scenes:
        pw = [r["wall_ms_per_spp"] for r in res[(s, "parent")]]
        tw = [r["wall_ms_per_spp"] for r in res[(s, "tree")]]
        pm, tm, spread = statistics.median(pw), statistics.median(tw), max(pw) - min(pw)
        hashes = {r["film_sha256"] for side in sides for r in res[(s, side)]}
        tk = statistics.median(r["kernel_ms_per_spp"].get("path", 0.0) for r in res[(s, "tree")])
        pk = statistics.median(r["kernels_sum_ms_per_spp"] for r in res[(s, "parent")])
        counts = (tm - pm) if abs(tm - pm) > 2 * spread else None
        print(json.dumps({"scene": s, "spp": SPP[s], "parent_wall": pw, "tree_wall": tw, "parent_median": round(pm, 4),
                          "tree_median": round(tm, 4), "parent_spread": round(spread, 4),
                          "tree_minus_parent": round(tm - pm, 4), "ratio": round(tm / pm, 4),
                          "exceeds_twice_parent_spread": counts is not None,
                          "films_byte_equal": len(hashes) == 1,
                          "parent_forms": sorted({r["form"] for r in res[(s, "parent")]}),
                          "tree_forms": sorted({r["form"] + "/" + r["shading"] for r in res[(s, "tree")]}),
                          "tree_path_launch_ms_per_spp": tk, "parent_kernels_sum_ms_per_spp": pk}), flush=True)


if __name__ == "__main__":
    main()
