"""Where option env_forms pays: renders under envmap.procedural_sky(1024) by the parent commit's
library with env_path 1, where k_path's environment build runs whatever the form rule would choose (the
yardstick), and with env_path 0 (the wavefront, shown beside it), against this tree's library with env_path 1
and env_forms 1, where the rule chooses among k_path, k_path_defer and k_path_spec and their environment builds
run.  1920 x 1080, max_depth 5, verify on, `path` 2 everywhere.  Workloads:
  share    the 8-way share of the C3 soup view (tiles k mod 8 == 0) at 64 spp: the rule takes k_path_spec
  cornell  the whole Cornell frame at 256 spp: a cache-resident tree, whose tail form is k_path_defer; which form
           the rule picks there (the pilot's mean steps decide)
  soup     the whole soup frame at 64 spp: which form the rule picks there
Each configuration runs in a process of its own with one context (AKR_HIP_LIB), parent and tree alternating for
--repeat rounds.  A process renders the shape once to warm up, then the timed render (wall ms per spp), and
prints the form that ran and a hash of the timed render's film; the tree's `share` process then renders once
more with the counting build and prints akr_hip_path_profile's speculative samples started and dropped.

Usage (GPU box): python tools/env_forms_measure.py --parent tools/experiments/lib/libakr_hip_parent.so
                 [--tree akarirender-1_amd/libakr_hip.so] [--repeat 3] [--workloads share,cornell,soup]"""
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
SPP = {"share": 64, "cornell": 256, "soup": 64}
MESH = ROOT / "tests" / "golden" / "CornellBox-Original.obj.mesh"
SIDES = {"parent_env_path": ("parent", "env_path=1,path=2"), "parent_wavefront": ("parent", "env_path=0,path=2"),
         "tree_env_forms": ("tree", "env_path=1,env_forms=1,path=2")}
YARDSTICK = "parent_env_path"


def build_scene(workload, tris):
    from akari_amd import envmap, scene
    sc = (scene.cornell_scene(MESH, resolution=(W, H)) if workload == "cornell"
          else scene.soup_scene(n_tris=tris, resolution=(W, H)))
    sc.environment = scene.EnvironmentLight(envmap.procedural_sky(1024), layout="octahedral")
    return scene.compile_scene(sc)


def worker(args):
    import numpy as np
    import torch
    from akari_amd import capi, dist, scene
    cs = build_scene(args.workload, args.tris)
    ctx = capi.HipContext(0)
    for kv in (x for x in args.opts.split(",") if x):
        k, _, v = kv.partition("=")
        ctx.set_option(k, int(v))
    if args.workload == "cornell":
        scene.upload_scene(ctx, cs, n_threads=16)
    else:
        nodes, tris = np.load(args.bvh + "_nodes.npy", mmap_mode="r"), np.load(args.bvh + "_tris.npy", mmap_mode="r")
        scene.upload_scene(ctx, cs, bvh=(nodes, tris), n_threads=16)
    dev = torch.device("cuda", 0)
    tiles = dist.tile_grid(W, H, 64)
    if args.workload == "share":
        tiles = tiles[::8]   # rank 0 of an 8-way tile split
    n = dist.n_pixels(tiles)
    buf = torch.zeros(4 * n, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    spp = SPP[args.workload]

    def render():
        ctx.render_device(spp, DEPTH, tiles, buf[:3 * n].data_ptr(), buf[3 * n:].data_ptr(), stream)
        torch.cuda.synchronize(dev)

    render()                      # warm-up: the same shape
    t = time.perf_counter()
    render()
    wall = (time.perf_counter() - t) / spp * 1e3
    inp = ctx.render_form_inputs()
    out = {"wall_ms_per_spp": round(wall, 4), "form": ctx.render_form()["form"], "shading": ctx.render_info()["shading"],
           "pixels": n, "pixels_per_lane": inp["pixels_per_lane"], "pilot_mean_steps": inp["pilot_mean_steps"],
           "film_sha256": hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest(),
           "mean": round(float(buf[:3 * n].mean().item()) / spp, 5)}
    if args.count:                # a counting render of its own: what the camera-miss length costs the guesses
        ctx.set_option("count_tests", 1)
        ctx.reset_stats()
        render()
        prof = ctx.path_profile()
        out["counting_form"] = ctx.render_form()["form"]
        out["spec_started"], out["spec_dropped"] = prof["spec_started"], prof["spec_aborted"]
        out["counting_film_equal"] = hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest() == out["film_sha256"]
        ctx.set_option("count_tests", 0)
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="tools/experiments/lib/libakr_hip_parent.so")
    ap.add_argument("--tree", default="akarirender-1_amd/libakr_hip.so")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workloads", default="share,cornell,soup")
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--workload", default="cornell")
    ap.add_argument("--opts", default="")
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--bvh", default="/tmp/akr_env_forms_bvh")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    workloads = [s for s in args.workloads.split(",") if s]
    libs = {"parent": args.parent, "tree": args.tree}
    print(f"# {W}x{H}, max_depth {DEPTH}, procedural_sky(1024), verify on; spp {SPP}; sides {SIDES}; share = tiles k mod 8 == 0 "
          f"of the soup view; one process and one context per line", flush=True)
    if set(workloads) & {"share", "soup"}:
        import numpy as np
        from akari_amd import capi, scene
        t0 = time.time()
        cs = scene.compile_scene(scene.soup_scene(n_tris=args.tris, resolution=(W, H)))
        nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices, builder=capi.BUILDER_SBVH, n_threads=16)
        np.save(args.bvh + "_nodes.npy", nodes)
        np.save(args.bvh + "_tris.npy", tris)
        del nodes, tris, cs
        print(f"# soup SBVH built once and saved in {time.time() - t0:.1f} s", flush=True)
    res = {(s, side): [] for s in workloads for side in SIDES}
    try:
        for rep in range(args.repeat):
            for s in workloads:
                for side, (lib, opts) in SIDES.items():
                    env = dict(os.environ, AKR_HIP_LIB=str(Path(libs[lib]).resolve()))
                    cmd = [sys.executable, __file__, "--worker", "--workload", s, "--opts", opts, "--tris", str(args.tris),
                           "--bvh", args.bvh]
                    if s == "share" and side == "tree_env_forms":
                        cmd.append("--count")
                    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
                    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
                    if p.returncode != 0 or line is None:   # a failed process ends the measurement: nothing more is started
                        print(p.stdout[-2000:], p.stderr[-3000:], flush=True)
                        raise SystemExit(f"{s} {side}: worker ended with {p.returncode}")
                    r = json.loads(line[7:])
                    res[(s, side)].append(r)
                    print(json.dumps({"workload": s, "side": side, "round": rep + 1, **r}), flush=True)
    finally:
        for suf in ("_nodes.npy", "_tris.npy"):
            Path(args.bvh + suf).unlink(missing_ok=True)
    print("# summary: wall ms per spp (median of the rounds; spread = max - min of the yardstick), the forms and the films", flush=True)
    for s in workloads:
        walls = {side: [r["wall_ms_per_spp"] for r in res[(s, side)]] for side in SIDES}
        med = {side: statistics.median(w) for side, w in walls.items()}
        yw = walls[YARDSTICK]
        spread = max(yw) - min(yw)
        diff = med["tree_env_forms"] - med[YARDSTICK]
        hashes = {r["film_sha256"] for side in SIDES for r in res[(s, side)]}
        row = {"workload": s, "spp": SPP[s], "pixels": res[(s, YARDSTICK)][0]["pixels"], "walls": walls,
               "medians": {k: round(v, 4) for k, v in med.items()}, "yardstick_spread": round(spread, 4),
               "tree_minus_yardstick": round(diff, 4), "ratio": round(med["tree_env_forms"] / med[YARDSTICK], 4),
               "exceeds_twice_yardstick_spread": abs(diff) > 2 * spread, "films_byte_equal": len(hashes) == 1,
               "film_sha256": sorted(hashes),
               "forms": {side: sorted({r["form"] + "/" + r["shading"] for r in res[(s, side)]}) for side in SIDES},
               "pixels_per_lane": res[(s, "tree_env_forms")][0]["pixels_per_lane"],
               "pilot_mean_steps": res[(s, "tree_env_forms")][0]["pilot_mean_steps"]}
        spec = [r for r in res[(s, "tree_env_forms")] if "spec_started" in r]
        if spec:
            row["speculation"] = [{"form": r["counting_form"], "started": r["spec_started"], "dropped": r["spec_dropped"],
                                   "film_equal": r["counting_film_equal"]} for r in spec]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
