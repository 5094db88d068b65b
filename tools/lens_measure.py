"""What a thin lens costs: the 1080p Cornell box at 64 spp, max_depth 5, verify on, rendered
  pinhole_k_path    without a lens in its usual form (`path` 2: k_path), the product's default,
  pinhole_wavefront without a lens in the wavefront form (`path` 0), the form an active lens forces,
  lens_wavefront    with tests/lens_scenes.py's lens_box camera and lens (radius 0.3, focal distance 8),
                    which runs the wavefront form whatever `path` says.
pinhole_wavefront against lens_wavefront is the price of the lens itself: k_raygen_lens for k_raygen, and
camera rays that leave a disk instead of a point and so are less coherent in the closest-hit trace;
pinhole_k_path against pinhole_wavefront is the price of the forced form.  Both pinhole sides use lens_box's
camera with the lens switched off, so all three see the same view.

Each configuration runs in a process of its own with one context, the three alternating for --repeat rounds.  A
process renders once to warm up, then the timed render (wall ms per spp), then once more with option "stats" 1
for the time of every kernel (events around every launch: those times are not the timed render's), and prints
the form that ran and a hash of the timed render's film.

Usage (GPU box): python tools/lens_measure.py [--repeat 3] [--spp 64]"""
import argparse
import hashlib
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
# side -> (lens on, options)
SIDES = {"pinhole_k_path": (False, "path=2"), "pinhole_wavefront": (False, "path=0"), "lens_wavefront": (True, "path=2")}
LENS = dict(position=(0.3, 1.2, 9.0), rotation=(3.0, -2.0, 5.0), fov=15.0, lens_radius=0.3, focal_distance=8.0)


def worker(args):
    import torch
    from akari_amd import capi, dist, scene
    lens_on, opts = SIDES[args.side]
    sc = scene.cornell_scene(MESH, resolution=(W, H))
    sc.camera = scene.PerspectiveCamera(resolution=(W, H), **LENS)
    if not lens_on:
        sc.camera.lens_radius = sc.camera.focal_distance = 0.0
    ctx = capi.HipContext(0)
    for kv in (x for x in opts.split(",") if x):
        k, _, v = kv.partition("=")
        ctx.set_option(k, int(v))
    scene.upload_scene(ctx, scene.compile_scene(sc), n_threads=16)
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
    out = {"wall_ms_per_spp": round(wall, 4), "form": ctx.render_form()["form"], "ordered": ctx.render_form()["ordered"],
           "lens": list(ctx.lens()), "film_sha256": hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest(),
           "mean": round(float(buf[:3 * n].mean().item()) / args.spp, 5)}
    ctx.set_option("stats", 1)    # a render of its own: events around every launch
    ctx.reset_stats()
    render()
    ks = ctx.kernel_stats()
    out["kernel_ms_per_spp"] = {k: round(v["total_ms"] / args.spp, 4) for k, v in sorted(ks.items())
                                if k in ("raygen", "trace_closest", "trace_shadow", "shade", "splat", "path", "pilot")}
    out["stats_film_equal"] = hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest() == out["film_sha256"]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--side", default="lens_wavefront", choices=list(SIDES))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    print(f"# Cornell box {W}x{H}, {args.spp} spp, max_depth {DEPTH}, verify on; camera and lens {LENS}; sides {SIDES}; "
          f"one process and one context per line", flush=True)
    res = {side: [] for side in SIDES}
    for rep in range(args.repeat):
        for side in SIDES:
            cmd = [sys.executable, __file__, "--worker", "--side", side, "--spp", str(args.spp)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:   # a failed process ends the measurement: nothing more is started
                print(p.stdout[-2000:], p.stderr[-3000:], flush=True)
                raise SystemExit(f"{side}: worker ended with {p.returncode}")
            r = json.loads(line[7:])
            res[side].append(r)
            print(json.dumps({"side": side, "round": rep + 1, **r}), flush=True)
    print("# summary: medians over the rounds, ms per spp; spread = max - min of a side's wall times", flush=True)
    med = {}
    for side, rs in res.items():
        walls = [r["wall_ms_per_spp"] for r in rs]
        kernels = {k: round(statistics.median(r["kernel_ms_per_spp"].get(k, 0.0) for r in rs), 4)
                   for k in sorted({k for r in rs for k in r["kernel_ms_per_spp"]})}
        med[side] = statistics.median(walls)
        print(json.dumps({"side": side, "forms": sorted({r["form"] for r in rs}), "wall_ms_per_spp": walls,
                          "median": round(med[side], 4), "spread": round(max(walls) - min(walls), 4),
                          "kernel_ms_per_spp": kernels, "films": sorted({r["film_sha256"] for r in rs}),
                          "stats_film_equal": all(r["stats_film_equal"] for r in rs)}), flush=True)
    print(json.dumps({"lens_over_pinhole_wavefront": round(med["lens_wavefront"] / med["pinhole_wavefront"], 4),
                      "wavefront_over_k_path_pinhole": round(med["pinhole_wavefront"] / med["pinhole_k_path"], 4),
                      "lens_over_k_path_pinhole": round(med["lens_wavefront"] / med["pinhole_k_path"], 4)}), flush=True)


if __name__ == "__main__":
    main()
