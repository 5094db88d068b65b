"""SceneNode::render (core/nodes/scene.cpp:112-160) on the HIP path: upload the scene through the
C-ABI, run the scene's integrator node on the GPU, and write the film.

The integrator node picks the C-ABI call the reference's compile_gpu would have produced
(core/nodes/integrator.cpp:26-84):
  Path -> akr_hip_render (gpu::PathTracer: spp, max_depth, tile_size, ray_clamp)
  AO   -> akr_hip_render_ao (AmbientOcclusion: spp, occlude)
The reference's GPU AO adds acc/spp once per pixel with weight 1 (gpu/cuda/integrator.cpp:83-90),
its CPU AO adds every sample with weight 1 (cpu/integrator.cpp:78); both resolve to the same
image acc/spp, and this film holds the CPU form (radiance = acc, weight = spp).

Usage: python -m akari_amd.render scene.akari [--out image.png|.pfm] [--gpus N]
       ... [--pass-spp N] [--preview] [--time-budget SECONDS] [--checkpoint FILE] [--resume FILE]
The second line renders a Path scene on one GPU in passes (akari_amd/progressive.py): the output is
rewritten after each pass, the render stops after the pass that exceeds the budget, the session is
saved after each pass, or a saved one is continued up to the scene's spp.
       ... --adaptive THRESHOLD [--min-spp N] [--pass-spp N] [--spp-map FILE.pfm] [--preview] [--time-budget S]
The third line renders a Path scene adaptively: N samples for every pixel (default
16), then passes only over the 64-pixel strips whose error is above THRESHOLD, up to the scene's spp
(the cap); --spp-map writes each pixel's sample count.  Checkpoints do not hold an adaptive film.
"""
from __future__ import annotations

import argparse
import math
import sys
import time
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, film, progressive, scene
from .dist import tile_grid


def _tiles(sc: scene.Scene, tile_size: int) -> List[Tuple[int, int, int, int]]:
    w, h = (int(v) for v in sc.camera.resolution)
    return tile_grid(w, h, max(1, int(tile_size)))


def render_scene(sc: scene.Scene, devices: Sequence[int] = (0,), **build_kw) -> Tuple[np.ndarray, np.ndarray]:
    """Render `sc` with its integrator node; returns the film (radiance [H,W,3], weight [H,W])."""
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    it = sc.integrator
    ctxs = [capi.HipContext(d) for d in devices]
    try:
        for c in ctxs:
            scene.upload_scene(c, cs, **build_kw)
        if isinstance(it, scene.AOIntegrator):
            if len(ctxs) != 1:
                raise ValueError("the AO integrator renders on one device")
            return ctxs[0].render_ao(it.spp, _tiles(sc, 16), w, h, occlude=it.occlude)
        if isinstance(it, scene.PathIntegrator):
            tiles = _tiles(sc, it.tile_size)
            if len(ctxs) == 1:
                return ctxs[0].render(it.spp, it.max_depth, tiles, w, h, ray_clamp=it.ray_clamp)
            return capi.render_node(ctxs, it.spp, it.max_depth, tiles, w, h, ray_clamp=it.ray_clamp)
        raise ValueError(f"integrator {type(it).__name__} is not supported on gpu")
    finally:
        for c in ctxs:
            c.close()


def render_scene_progressive(sc: scene.Scene, device: int = 0, pass_spp: Optional[int] = None,
                             on_pass=None, time_budget: Optional[float] = None, checkpoint=None, resume=None,
                             **build_kw) -> Tuple[np.ndarray, np.ndarray, int]:
    """Render a Path scene in passes on one device; returns (radiance, weight, spp_done).

    pass_spp: samples per pass (default: each pass doubles the samples done); on_pass(spp_done,
    radiance, weight) after each pass; checkpoint: file the session is saved to after each pass;
    resume: checkpoint file whose session is continued up to the integrator's spp."""
    it = sc.integrator
    if not isinstance(it, scene.PathIntegrator):
        raise ValueError("progressive rendering needs the Path integrator")
    ck = progressive.Checkpoint.load(resume) if resume is not None else None
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    tiles = _tiles(sc, it.tile_size)
    if ck is not None:  # checked before a device is touched
        ck.check(cs, tiles, w, h)
        if ck.max_depth != it.max_depth or ck.ray_clamp != float(np.float32(it.ray_clamp)) or ck.flags != 0:
            raise progressive.CheckpointError(
                f"checkpoint was rendered with max_depth {ck.max_depth}, ray_clamp {ck.ray_clamp}, flags {ck.flags}; "
                f"the scene asks for max_depth {it.max_depth}, ray_clamp {it.ray_clamp}")
        if ck.spp_done > it.spp:
            raise progressive.CheckpointError(f"checkpoint holds {ck.spp_done} spp, more than the {it.spp} asked for")
    with capi.HipContext(device) as ctx:
        scene.upload_scene(ctx, cs, **build_kw)
        if ck is not None:
            ck.restore(ctx, cs, tiles)

        def each_pass(done, rad, wt):
            if checkpoint is not None:
                progressive.Checkpoint.capture(ctx, cs, tiles).save(checkpoint)
            return on_pass(done, rad, wt) if on_pass is not None else None

        return progressive.render_progressive(ctx, it.spp, it.max_depth, tiles, w, h,
                                              schedule=pass_spp if pass_spp is not None else "double",
                                              on_pass=each_pass, time_budget=time_budget, ray_clamp=it.ray_clamp,
                                              resume=ck is not None)


def render_scene_adaptive(sc: scene.Scene, threshold: float, device: int = 0, min_spp: int = 16,
                          pass_spp: Optional[int] = None, on_pass=None, time_budget: Optional[float] = None,
                          **build_kw):
    """Render a Path scene adaptively on one device; returns (radiance, weight, info).  The integrator's
    spp is the cap; weight holds each pixel's sample count (progressive.render_adaptive)."""
    it = sc.integrator
    if not isinstance(it, scene.PathIntegrator):
        raise ValueError("adaptive rendering needs the Path integrator")
    progressive.check_adaptive_args(threshold, min_spp, pass_spp or 0, it.spp)
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    with capi.HipContext(device) as ctx:
        scene.upload_scene(ctx, cs, **build_kw)
        return progressive.render_adaptive(ctx, it.spp, it.max_depth, _tiles(sc, it.tile_size), w, h, threshold,
                                           min_spp=min_spp, pass_spp=pass_spp or 0, on_pass=on_pass,
                                           time_budget=time_budget, ray_clamp=it.ray_clamp)


def write_spp_map(path: str, weight: np.ndarray) -> None:
    """Each pixel's sample count as a linear float map (the count in all three channels)."""
    counts = np.repeat(np.asarray(weight, np.float32)[..., None], 3, axis=-1)
    film.write_pfm(path, counts, np.ones_like(weight, dtype=np.float32))


def write_film(path: str, radiance: np.ndarray, weight: np.ndarray) -> None:
    """Film::write_image (core/film.h:97-113): PNG is sRGB 8-bit, PFM keeps linear floats."""
    if path.lower().endswith(".pfm"):
        film.write_pfm(path, radiance, weight)
    else:
        film.write_png(path, radiance, weight)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="akari_amd.render", description=__doc__.splitlines()[0])
    ap.add_argument("scene")
    ap.add_argument("--out", default=None, help="output image (default: the scene's `output` field)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--spp", type=int, default=None, help="override the integrator's spp")
    ap.add_argument("--pass-spp", type=int, default=None, metavar="N",
                    help="render in passes of N samples (default with the options below: each pass doubles the samples)")
    ap.add_argument("--preview", action="store_true", help="rewrite the output after each pass")
    ap.add_argument("--time-budget", type=float, default=None, metavar="SECONDS",
                    help="stop after the first pass that ends past this many seconds of rendering")
    ap.add_argument("--checkpoint", default=None, metavar="FILE", help="save the render session after each pass")
    ap.add_argument("--resume", default=None, metavar="FILE", help="continue a saved session up to the scene's spp")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD",
                    help="adaptive sampling: stop sampling a 64-pixel strip once its error is at or below THRESHOLD; "
                         "the scene's spp (or --spp) is the cap")
    ap.add_argument("--min-spp", type=int, default=16, metavar="N",
                    help="with --adaptive: samples every pixel gets before the first test (default 16)")
    ap.add_argument("--spp-map", default=None, metavar="FILE.pfm",
                    help="with --adaptive: write each pixel's sample count")
    args = ap.parse_args(argv)
    if args.adaptive is not None:  # refused before the scene is read
        if args.checkpoint is not None or args.resume is not None:
            ap.error("--adaptive cannot be combined with --checkpoint or --resume: a checkpoint holds a film "
                     "with one sample count for every pixel")
        if not args.adaptive >= 0:
            ap.error("--adaptive needs a threshold >= 0")
        if args.min_spp < 1:
            ap.error("--min-spp needs at least one sample")
    elif args.spp_map is not None:
        ap.error("--spp-map needs --adaptive")
    passes = args.adaptive is not None or (args.pass_spp is not None or args.preview or args.time_budget is not None or
              args.checkpoint is not None or args.resume is not None)
    if passes:  # checked before the scene is uploaded: no device is needed to refuse these
        if args.gpus != 1:
            ap.error("--pass-spp, --preview, --time-budget, --checkpoint and --resume render on one GPU (--gpus 1)")
        if args.pass_spp is not None and args.pass_spp < 1:
            ap.error("--pass-spp needs at least one sample per pass")
        if args.time_budget is not None and not args.time_budget > 0:
            ap.error("--time-budget needs a positive number of seconds")
        if args.resume is not None and not Path(args.resume).is_file():
            ap.error(f"--resume: no checkpoint file {args.resume}")
    sc = scene.load_scene_file(args.scene)
    if args.spp is not None:
        sc.integrator.spp = args.spp
    if passes and not isinstance(sc.integrator, scene.PathIntegrator):
        ap.error(f"--pass-spp, --preview, --time-budget, --checkpoint, --resume and --adaptive need the Path integrator; "
                 f"the scene's is {type(sc.integrator).__name__}")
    out = args.out or sc.output
    t0 = time.time()
    if args.adaptive is not None:
        def show_adaptive(info, rad, wt):
            if args.preview:
                write_film(out, rad, wt)
                print(f"pass {info['passes']} to {info['spp_max']} spp, {info['samples']} samples: "
                      f"{time.time() - t0:.2f}s -> {out}", flush=True)

        try:
            per_pass = args.preview or args.time_budget is not None
            rad, wt, info = render_scene_adaptive(sc, args.adaptive, 0, min_spp=args.min_spp, pass_spp=args.pass_spp,
                                                  on_pass=show_adaptive if per_pass else None,
                                                  time_budget=args.time_budget)
        except ValueError as e:
            ap.error(str(e))
        done = f"{info['spp_min']}..{info['spp_max']} ({info['samples']} samples in {info['passes']} passes)"
        if args.spp_map is not None:
            write_spp_map(args.spp_map, wt)
    elif passes:
        def show(done, rad, wt):
            if args.preview:
                write_film(out, rad, wt)
                print(f"pass to {done} spp: {time.time() - t0:.2f}s -> {out}", flush=True)

        try:
            rad, wt, done = render_scene_progressive(sc, 0, pass_spp=args.pass_spp, on_pass=show,
                                                     time_budget=args.time_budget, checkpoint=args.checkpoint,
                                                     resume=args.resume)
        except progressive.CheckpointError as e:
            ap.error(str(e))
    else:
        rad, wt = render_scene(sc, devices=list(range(args.gpus)))
        done = sc.integrator.spp
    write_film(out, rad, wt)
    print(f"{type(sc.integrator).__name__} {sc.camera.resolution[0]}x{sc.camera.resolution[1]} "
          f"spp {done}: {time.time() - t0:.2f}s -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
