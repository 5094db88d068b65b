"""What adaptive sampling costs and buys: on the Cornell box at 1080p and on the
C3 view (10M-triangle soup, 1920x1080), an adaptive render at a threshold chosen so that roughly half
the samples of the cap are drawn, against the uniform render of the cap on the same context.

Per scene it prints one JSON line: the samples drawn as a share of the uniform cap, the wall time of the
adaptive render (device form) against the uniform render's, the convergence test's and the compaction's
own time per pass (option "stats"), and the per-sample time of every subset pass (the stepwise form,
timed on the host) against the uniform per-sample time.

Usage (GPU box): python tools/adaptive_cost.py [--cap 256] [--min-spp 16] [--scenes cornell,soup10m]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "akarirender-1_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--scenes", default="cornell,soup10m")
    ap.add_argument("--share", type=float, default=0.5, help="the share of the cap's samples to aim for")
    args = ap.parse_args()
    import numpy as np
    import torch
    from akari_amd import capi, dist, scene
    W, H, depth = 1920, 1080, 5
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    film = torch.zeros(4 * W * H, device=dev)
    tiles = dist.tiles_for_rank(W, H, 64, 0, 1)
    npx = dist.n_pixels(tiles)
    d_rad, d_w = film[:3 * npx].data_ptr(), film[3 * npx:4 * npx].data_ptr()
    for name in args.scenes.split(","):
        if name == "cornell":
            sc = scene.cornell_scene(ROOT / "tests" / "golden" / "CornellBox-Original.obj.mesh", resolution=(W, H))
        else:
            n = {"soup100k": 100_000, "soup1m": 1_000_000, "soup10m": 10_000_000}[name]
            sc = scene.soup_scene(n_tris=n, resolution=(W, H))
        cs = scene.compile_scene(sc)
        with capi.HipContext(0) as ctx:
            t0 = time.time()
            scene.upload_scene(ctx, cs, builder=capi.BUILDER_SBVH, n_threads=16)
            print(f"{name}: {cs.n_tris} tris, built in {time.time() - t0:.1f} s", flush=True)

            def timed(fn):
                torch.cuda.synchronize(dev)
                t = time.perf_counter()
                out = fn()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t) * 1e3, out

            ctx.render_device(args.min_spp, depth, tiles, d_rad, d_w, stream)   # warm: kernels loaded, buffers sized
            uniform_ms = min(timed(lambda: ctx.render_device(args.cap, depth, tiles, d_rad, d_w, stream))[0]
                             for _ in range(2))
            uniform_form = ctx.render_form()

            def adaptive(threshold):
                return ctx.render_adaptive_device(args.cap, depth, tiles, d_rad, d_w, threshold, min_spp=args.min_spp,
                                                  stream=stream)[1]

            # the threshold: bisection (in log space) between the smallest positive and the largest strip
            # error of the first test, on the share of the cap's samples drawn
            adaptive(float("inf"))
            err = ctx.adaptive_error()[0]
            lo, hi = float(err[err > 0].min()) / 64, float(err.max())
            first_test = dict(zero=int((err == 0).sum()), smallest_positive=float(err[err > 0].min()),
                              median=float(np.median(err)), largest=float(err.max()))
            full = npx * args.cap
            threshold = share = None
            trace = []
            for _ in range(10):
                mid = float(np.sqrt(lo * hi))
                s = adaptive(mid)["samples"] / full
                trace.append((mid, round(s, 4)))
                if threshold is None or abs(s - args.share) < abs(share - args.share):
                    threshold, share = mid, s
                if s > args.share:
                    lo = mid   # too many samples: stop more strips
                else:
                    hi = mid
            runs = [timed(lambda: adaptive(threshold)) for _ in range(2)]
            adaptive_ms, info = min(runs, key=lambda r: r[0])
            # the test's and the compaction's own time: HIP events around their launches
            ctx.set_option("stats", 1)
            ctx.reset_stats()
            adaptive(threshold)
            stats = ctx.kernel_stats()
            ctx.set_option("stats", 0)
            per_pass = {k: round(stats[k]["total_ms"] / stats[k]["launches"], 4) for k in ("adaptive_test", "compact")
                        if k in stats}
            # every pass on its own: the stepwise form, each step timed on the host (it includes the test,
            # the compaction and the in-band film check)
            t = time.perf_counter()
            step_info, more = ctx.adaptive_begin(args.cap, depth, tiles, threshold, min_spp=args.min_spp)
            passes = [dict(to_spp=step_info["spp_max"], samples=step_info["samples"],
                           ms=round((time.perf_counter() - t) * 1e3, 3))]
            while more:
                before = step_info["samples"]
                t = time.perf_counter()
                step_info, more = ctx.adaptive_step()
                passes.append(dict(to_spp=step_info["spp_max"], samples=step_info["samples"] - before,
                                   ms=round((time.perf_counter() - t) * 1e3, 3), form=ctx.render_form()["form"]))
            for p in passes:
                p["ns_per_sample"] = round(p["ms"] * 1e6 / max(1, p["samples"]), 4)
            print(json.dumps(dict(
                scene=name, pixels=npx, cap=args.cap, min_spp=args.min_spp, threshold=threshold,
                samples=info["samples"], share_of_cap=round(info["samples"] / full, 4), passes=info["passes"],
                spp_min=info["spp_min"], spp_max=info["spp_max"], strips=info["strips"],
                strips_at_cap=info["strips_at_cap"], uniform_ms=round(uniform_ms, 3), uniform_form=uniform_form,
                uniform_ns_per_sample=round(uniform_ms * 1e6 / full, 4), adaptive_ms=round(adaptive_ms, 3),
                adaptive_over_uniform=round(adaptive_ms / uniform_ms, 4),
                adaptive_ns_per_sample=round(adaptive_ms * 1e6 / info["samples"], 4), ms_per_launch=per_pass,
                first_test_strip_errors=first_test, threshold_search=trace,
                stepwise_passes=passes)), flush=True)


if __name__ == "__main__":
    main()
