"""What k_path's pop site and push pay per traversal iteration ("bounded pop"): a 1-spp
counting pass of the C3 frame (or of rank 0's share of an N-way split), forced to k_path, with the pop
site waiting for its slowest lane (path_pop_rounds 255, path_pop_keep 1: stack_pop's behaviour) unless
--pop-rounds / --pop-keep say otherwise.

  rounds_per_pop_iter   pop rounds a wave runs in an iteration in which some lane pops
  rounds_per_pop_lane   rounds a popping lane needs itself
  pop_iter_share        iterations with a pop, of all traversal iterations
  push_slow_share       push iterations in which some lane has fewer than four free LDS rows (the
                        general push before the fit test), of the iterations with a push
  push_would_fit_share  of the iterations with a push: those slow ones whose entries all fit in LDS

Usage (GPU box): python tools/pop_push_counts.py [--tris 10000000] [--split 8] [--pop-rounds R --pop-keep K]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "akarirender-1_amd"))
W, H = 1920, 1080


def ratios(pp, counts):
    cl, sh = (counts["per_mode"][m] for m in ("closest", "shadow"))
    d = lambda a, b: round(a / max(1, b), 4)
    return {"rounds_per_pop_iter": d(pp["pop_rounds"], pp["pop_iters"]),
            "rounds_per_pop_lane": d(pp["pop_lane_rounds"], pp["pop_lanes"]),
            "popping_lanes_per_pop_iter": d(pp["pop_lanes"], pp["pop_iters"]),
            "pop_iter_share": d(pp["pop_iters"], pp["trav_iters"]),
            "push_iter_share": d(pp["push_iters"], pp["trav_iters"]),
            "push_slow_share": d(pp["push_slow"], pp["push_iters"]),
            "push_would_fit_share": d(pp["push_would_fit"], pp["push_iters"]),
            "visiting_lanes_per_iter": d(cl["visits"] + sh["visits"], pp["trav_iters"]),
            "deep_rays": cl["deep_rays"] + sh["deep_rays"], "rays": cl["rays"] + sh["rays"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--split", type=int, default=1, help="N > 1: rank 0's share of an N-way tile split")
    ap.add_argument("--pop-rounds", type=int, default=255)
    ap.add_argument("--pop-keep", type=int, default=1)
    ap.add_argument("--spp", type=int, default=1)
    args = ap.parse_args()
    import torch
    from akari_amd import capi, dist, scene
    cs = scene.compile_scene(scene.soup_scene(n_tris=args.tris, resolution=(W, H)))
    ctx = capi.HipContext(0)
    scene.upload_scene(ctx, cs, builder=capi.BUILDER_SBVH, n_threads=16)
    for k, v in (("path", 1), ("path_defer", 0), ("path_spec", 0), ("path_pop_rounds", args.pop_rounds),
                 ("path_pop_keep", args.pop_keep)):
        ctx.set_option(k, v)
    tiles = dist.tiles_for_rank(W, H, 64, 0, args.split) if args.split > 1 else dist.tile_grid(W, H, 64)
    n = dist.n_pixels(tiles)
    dev = torch.device("cuda", 0)
    film = torch.zeros(4 * n, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ctx.render_device(1, 5, tiles, film[:3 * n].data_ptr(), film[3 * n:].data_ptr(), stream)   # warm
    ctx.set_option("count_tests", 1)
    ctx.reset_stats()
    ctx.render_device(args.spp, 5, tiles, film[:3 * n].data_ptr(), film[3 * n:].data_ptr(), stream)
    torch.cuda.synchronize(dev)
    pp, counts = ctx.path_profile(), ctx.trace_counts()
    ctx.set_option("count_tests", 0)
    assert ctx.render_form()["form"] == "k_path"
    keys = ("trav_iters", "pop_iters", "pop_rounds", "pop_lane_rounds", "pop_lanes", "push_iters", "push_slow",
            "push_would_fit")
    print(json.dumps({"tris": cs.n_tris, "split": args.split, "spp": args.spp, "pop_rounds_opt": args.pop_rounds,
                      "pop_keep_opt": args.pop_keep, **{k: pp[k] for k in keys}, **ratios(pp, counts)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
