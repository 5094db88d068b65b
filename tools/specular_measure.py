"""What the Mirror and Glass materials cost: the 1080p Cornell box with the tall block a Mirror
and the short block a Glass (k_shade_spec, one more bounce for the rays that leave a delta lobe at the last
vertex) against this tree's own render of the unmodified box in the wavefront form (option path 0, k_shade).
1920 x 1080, max_depth 5, 64 spp, verify on.  Each configuration runs in a process of its own with one context,
the two alternating for --repeat rounds.  A process renders the shape once to warm up, then the timed render
(wall ms per spp), then a render of its own with option stats (per-kernel ms per spp and ms per shade launch).

Usage (GPU box): python tools/specular_measure.py [--repeat 3] [--spp 64]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "akarirender-1_amd"))
W, H, DEPTH = 1920, 1080, 5
MESH = ROOT / "tests" / "golden" / "CornellBox-Original.obj.mesh"


def build_scene(name):
    from akari_amd import scene
    sc = scene.cornell_scene(MESH, resolution=(W, H))
    if name == "specular":
        ct = scene.ConstantTexture
        sc.shapes[0].materials[6] = scene.MirrorMaterial(ct([0.9, 0.85, 0.8]))           # tall block
        sc.shapes[0].materials[5] = scene.GlassMaterial(ct([0.95, 0.97, 1.0]), 1.5)      # short block
    return scene.compile_scene(sc)


def worker(args):
    import torch
    from akari_amd import capi, dist, scene
    ctx = capi.HipContext(0)
    ctx.set_option("path", 0)     # the plain box in the wavefront form too; the specular box takes it anyway
    scene.upload_scene(ctx, build_scene(args.scene), n_threads=16)
    dev = torch.device("cuda", 0)
    tiles = dist.tile_grid(W, H, 64)
    n = dist.n_pixels(tiles)
    buf = torch.zeros(4 * n, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def render():
        ctx.render_device(args.spp, DEPTH, tiles, buf[:3 * n].data_ptr(), buf[3 * n:].data_ptr(), stream)
        torch.cuda.synchronize(dev)

    render()                      # warm-up: the same shape
    t = time.perf_counter()
    render()
    wall = (time.perf_counter() - t) / args.spp * 1e3
    out = {"wall_ms_per_spp": round(wall, 4), "form": ctx.render_form()["form"],
           "mean": round(float(buf[:3 * n].mean().item()) / args.spp, 5)}
    ctx.reset_stats()             # a render of its own with HIP events on every launch
    ctx.set_option("stats", 1)
    render()
    ctx.set_option("stats", 0)
    ks = ctx.kernel_stats()
    out["kernel_ms_per_spp"] = {k: round(v["total_ms"] / args.spp, 4) for k, v in ks.items() if v["launches"]}
    out["shade_launches_per_spp"] = ks["shade"]["launches"] / args.spp
    out["ms_per_shade_launch"] = round(ks["shade"]["total_ms"] / ks["shade"]["launches"], 4)
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--scene", default="plain")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    print(f"# Cornell box {W}x{H}, max_depth {DEPTH}, {args.spp} spp, option path 0 (wavefront), verify on; plain: the "
          f"unmodified box (k_shade), specular: tall block Mirror, short block Glass ior 1.5 (k_shade_spec); one "
          f"process and one context per line", flush=True)
    res = {"plain": [], "specular": []}
    for rep in range(args.repeat):
        for name in res:
            cmd = [sys.executable, __file__, "--worker", "--scene", name, "--spp", str(args.spp)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:   # a failed process ends the measurement: nothing more is started
                print(p.stdout[-2000:], p.stderr[-3000:], flush=True)
                raise SystemExit(f"{name}: worker ended with {p.returncode}")
            r = json.loads(line[7:])
            res[name].append(r)
            print(f"{name} round {rep + 1}: {json.dumps(r)}", flush=True)
    for key in ("wall_ms_per_spp", "ms_per_shade_launch"):
        a = statistics.median(r[key] for r in res["plain"])
        b = statistics.median(r[key] for r in res["specular"])
        print(f"median {key}: plain {a:.4f}, specular {b:.4f} ({(b / a - 1) * 100:+.1f} %)", flush=True)
    print(f"shade launches per spp: plain {res['plain'][0]['shade_launches_per_spp']:g}, "
          f"specular {res['specular'][0]['shade_launches_per_spp']:g}", flush=True)


if __name__ == "__main__":
    main()
