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
       ... --denoise [--denoise-iters N] [--feature-spp N] [--aov PREFIX]
With any of the lines above, --denoise writes the film filtered by the edge-avoiding a-trous filter
 as the output, previews included: the feature pass (albedo, normal, depth; N camera
samples per pixel, default 2) runs once per run, the filter once per written film.  --aov writes
PREFIX.albedo.pfm, PREFIX.normal.pfm and PREFIX.depth.pfm, with or without --denoise.
       ... --denoise --denoise-variance   with --pass-spp, --preview or --adaptive
The session tracks the variance of every pixel's mean from its passes and each film is
filtered by the variance-guided filter, whose colour stop follows how converged a pixel is.  One call is one
batch, so the render has to run in passes; --aov then also writes PREFIX.variance.pfm.
       ... --env FILE --env-path
With an environment, --env-path sets library option "env_path" on every context: the persistent path
kernel renders the scene where the render form rule takes it.  The image is the same.
       ... --env FILE --env-path --env-forms
--env-forms (with --env-path) sets library option "env_forms" on every context as well: the form rule then
chooses among k_path, k_path_defer and k_path_spec as it does without an environment, which
is what a rank's share of a --gpus N render takes.  The image is the same.
       ... --lens-radius R (--focal-distance D | --focus-at X Y)
A thin-lens camera: depth of field around the plane at distance D along the view axis, or
around what the centre of pixel (X, Y) sees.  The camera node's lens_radius and focal_distance do the same;
every line above works with it, --denoise and --gpus N included.
"""
from __future__ import annotations

import argparse
import math
import sys
import time
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi, denoise, envmap, film, lens, progressive, scene
from .dist import tile_grid


def _tiles(sc: scene.Scene, tile_size: int) -> List[Tuple[int, int, int, int]]:
    w, h = (int(v) for v in sc.camera.resolution)
    return tile_grid(w, h, max(1, int(tile_size)))


class FilmPost:
    """--denoise / --aov: the feature pass once per run on the context that holds the
    scene, and the filter of every film handed to finish().  `image` is the last filtered mean colour
    [H, W, 3] (None without --denoise), `features` the feature sums [H, W, 12]."""

    def __init__(self, do_denoise: bool, iterations: Optional[int] = None, feature_spp: Optional[int] = None,
                 per_pass: bool = False, guided: bool = False):
        self.do_denoise = bool(do_denoise)
        self.guided = bool(guided)   # --denoise-variance: the session tracks the variance, the guided filter runs
        self.params = {} if iterations is None else {"iterations": int(iterations)}
        (denoise.guided_params if self.guided else denoise.params)(**self.params)   # refused here, before a device is touched
        self.variance = None   # with `guided`: [H, W, 4] of the last film handed to finish()
        self.feature_spp = denoise.DEFAULT_FEATURE_SPP if feature_spp is None else int(feature_spp)
        if self.feature_spp < 1:
            raise ValueError("the feature pass needs at least one sample")
        self.per_pass = bool(per_pass) and self.do_denoise
        self.features = self.image = self._film = None

    def start(self, ctx: "capi.HipContext") -> None:
        """Before the first render of the run: the session's variance tracker is an option read when it starts."""
        if self.guided:
            ctx.set_option("film_variance", 1)

    def bind(self, tiles, width: int, height: int, demodulate: bool = True) -> None:
        """The run's tile list and frame; demodulate=False for films that are not albedo times lighting (AO)."""
        self.tiles, self.width, self.height = tiles, int(width), int(height)
        if not demodulate:
            self.params["demodulate"] = False

    def finish(self, ctx: "capi.HipContext", radiance, weight) -> None:
        if self._film is radiance:   # this film is done already (the last pass's preview)
            return
        if self.features is None:
            self.features = ctx.render_features(self.feature_spp, self.tiles, self.width, self.height)
        if self.guided:
            self.variance = ctx.render_variance(self.width, self.height)
        if self.do_denoise and self.guided:
            self.image = ctx.denoise_guided(radiance, weight, self.features, self.variance, **self.params)
        elif self.do_denoise:
            self.image = ctx.denoise(radiance, weight, self.features, **self.params)
        self._film = radiance

    def write_aov(self, prefix: str) -> None:
        albedo, normal, depth, _ = denoise.split_features(self.features)
        one = np.ones(depth.shape, np.float32)
        film.write_pfm(prefix + ".albedo.pfm", albedo, one)
        film.write_pfm(prefix + ".normal.pfm", normal, one)
        film.write_pfm(prefix + ".depth.pfm", np.repeat(depth[..., None], 3, axis=-1), one)
        if self.variance is not None:   # the variance of each pixel's mean colour (0 where it has fewer than two batches)
            film.write_pfm(prefix + ".variance.pfm", np.ascontiguousarray(self.variance[..., :3]), one)


def render_scene(sc: scene.Scene, devices: Sequence[int] = (0,), post: Optional[FilmPost] = None,
                 env_path: bool = False, env_forms: bool = False, **build_kw) -> Tuple[np.ndarray, np.ndarray]:
    """Render `sc` with its integrator node; returns the film (radiance [H,W,3], weight [H,W]).  With
    `post`, the features and the filter run on the first device after the film is gathered.
    env_path: option "env_path" on every context (a choice of form under an environment, same bits);
    env_forms: option "env_forms" as well (set only when asked for)."""
    cs = scene.compile_scene(sc)
    w, h = (int(v) for v in sc.camera.resolution)
    it = sc.integrator
    ctxs = [capi.HipContext(d) for d in devices]
    try:
        for c in ctxs:
            scene.upload_scene(c, cs, **build_kw)
            if getattr(it, "mis", False):   # a session switch, read when the render starts
                c.set_option("mis", 1)
            c.set_option("env_path", 1 if env_path else 0)
            if env_forms:
                c.set_option("env_forms", 1)
        if isinstance(it, scene.AOIntegrator):
            if len(ctxs) != 1:
                raise ValueError("the AO integrator renders on one device")
            tiles = _tiles(sc, 16)
            rad, wt = ctxs[0].render_ao(it.spp, tiles, w, h, occlude=it.occlude)
        elif isinstance(it, scene.PathIntegrator):
            tiles = _tiles(sc, it.tile_size)
            if len(ctxs) == 1:
                rad, wt = ctxs[0].render(it.spp, it.max_depth, tiles, w, h, ray_clamp=it.ray_clamp)
            else:
                rad, wt = capi.render_node(ctxs, it.spp, it.max_depth, tiles, w, h, ray_clamp=it.ray_clamp)
        else:
            raise ValueError(f"integrator {type(it).__name__} is not supported on gpu")
        if post is not None:
            post.bind(tiles, w, h, demodulate=isinstance(it, scene.PathIntegrator))
            post.finish(ctxs[0], rad, wt)
        return rad, wt
    finally:
        for c in ctxs:
            c.close()


def render_scene_progressive(sc: scene.Scene, device: int = 0, pass_spp: Optional[int] = None,
                             on_pass=None, time_budget: Optional[float] = None, checkpoint=None, resume=None,
                             post: Optional[FilmPost] = None, env_path: bool = False, env_forms: bool = False,
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
        ck.check(cs, tiles, w, h, it.mis)
        if ck.max_depth != it.max_depth or ck.ray_clamp != float(np.float32(it.ray_clamp)) or ck.flags != 0:
            raise progressive.CheckpointError(
                f"checkpoint was rendered with max_depth {ck.max_depth}, ray_clamp {ck.ray_clamp}, flags {ck.flags}; "
                f"the scene asks for max_depth {it.max_depth}, ray_clamp {it.ray_clamp}")
        if ck.spp_done > it.spp:
            raise progressive.CheckpointError(f"checkpoint holds {ck.spp_done} spp, more than the {it.spp} asked for")
    with capi.HipContext(device) as ctx:
        scene.upload_scene(ctx, cs, **build_kw)
        ctx.set_option("mis", 1 if it.mis else 0)   # before the restore: a session reads it when it starts
        ctx.set_option("env_path", 1 if env_path else 0)   # read at every render and continue; not in the checkpoint
        if env_forms:   # the same: a choice of form, the same bits
            ctx.set_option("env_forms", 1)
        if post is not None:
            post.start(ctx)   # before the restore: an imported film is the tracker's first batch
            post.bind(tiles, w, h)
        if ck is not None:
            ck.restore(ctx, cs, tiles, it.mis)

        def each_pass(done, rad, wt):
            if checkpoint is not None:
                progressive.Checkpoint.capture(ctx, cs, tiles, it.mis).save(checkpoint)
            if post is not None and post.per_pass:   # the feature pass and the filter keep the session
                post.finish(ctx, rad, wt)
            return on_pass(done, rad, wt) if on_pass is not None else None

        out = progressive.render_progressive(ctx, it.spp, it.max_depth, tiles, w, h,
                                             schedule=pass_spp if pass_spp is not None else "double",
                                             on_pass=each_pass, time_budget=time_budget, ray_clamp=it.ray_clamp,
                                             resume=ck is not None)
        if post is not None:
            post.finish(ctx, out[0], out[1])
        return out


def render_scene_adaptive(sc: scene.Scene, threshold: float, device: int = 0, min_spp: int = 16,
                          pass_spp: Optional[int] = None, on_pass=None, time_budget: Optional[float] = None,
                          post: Optional[FilmPost] = None, env_path: bool = False, env_forms: bool = False, **build_kw):
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
        ctx.set_option("mis", 1 if it.mis else 0)
        ctx.set_option("env_path", 1 if env_path else 0)
        if env_forms:
            ctx.set_option("env_forms", 1)
        tiles = _tiles(sc, it.tile_size)
        each = on_pass
        if post is not None:
            post.start(ctx)
            post.bind(tiles, w, h)
            if on_pass is not None and post.per_pass:
                def each(info, rad, wt):
                    post.finish(ctx, rad, wt)
                    return on_pass(info, rad, wt)
        out = progressive.render_adaptive(ctx, it.spp, it.max_depth, tiles, w, h, threshold,
                                          min_spp=min_spp, pass_spp=pass_spp or 0, on_pass=each,
                                          time_budget=time_budget, ray_clamp=it.ray_clamp)
        if post is not None:
            post.finish(ctx, out[0], out[1])
        return out


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
    ap.add_argument("--denoise", action="store_true",
                    help="write the film filtered by the edge-avoiding a-trous filter (previews included)")
    ap.add_argument("--denoise-iters", type=int, default=None, metavar="N",
                    help=f"with --denoise: filter iterations, 1..{denoise.MAX_ITERATIONS} "
                         f"(default {denoise.DEFAULTS['iterations']})")
    ap.add_argument("--feature-spp", type=int, default=None, metavar="N",
                    help=f"with --denoise or --aov: camera samples per pixel of the feature pass "
                         f"(default {denoise.DEFAULT_FEATURE_SPP})")
    ap.add_argument("--aov", default=None, metavar="PREFIX",
                    help="write PREFIX.albedo.pfm, PREFIX.normal.pfm and PREFIX.depth.pfm "
                         "(and PREFIX.variance.pfm with --denoise-variance)")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="with --denoise and one of --pass-spp, --preview, --adaptive: track each pixel's variance "
                         "from the passes and filter with the variance-guided filter")
    ap.add_argument("--env", default=None, metavar="FILE",
                    help="light the scene with this lat-long environment image (.pfm, .hdr, .npy); replaces the "
                         "scene's EnvironmentLight")
    ap.add_argument("--env-scale", type=float, default=None, metavar="S", help="multiply the environment by S")
    ap.add_argument("--env-rotate", type=float, default=None, metavar="DEGREES",
                    help="turn the environment about the vertical axis")
    ap.add_argument("--mis", action="store_true",
                    help="Path integrator: combine the light sample and the BSDF sample of direct lighting by the "
                         "power heuristic (multiple importance sampling); the scene's `mis` field does the same")
    ap.add_argument("--env-path", action="store_true",
                    help="with an environment: let the persistent path kernel render the scene where the render "
                         "form rule takes it (library option env_path); the image is the same, bit for bit")
    ap.add_argument("--env-forms", action="store_true",
                    help="with --env-path: let the render form rule choose among k_path, k_path_defer and k_path_spec "
                         "as it does without an environment (library option env_forms); the image is the same")
    ap.add_argument("--env-res", type=int, default=None, metavar="N",
                    help="resolution of the octahedral map made from a lat-long image, 1..2048")
    ap.add_argument("--lens-radius", type=float, default=None, metavar="R",
                    help="thin-lens camera: the lens radius in scene units (0: pinhole); replaces the camera's "
                         "lens_radius")
    ap.add_argument("--focal-distance", type=float, default=None, metavar="D",
                    help="thin-lens camera: the distance of the plane of focus along the view axis; replaces the "
                         "camera's focal_distance")
    ap.add_argument("--focus-at", type=int, nargs=2, default=None, metavar=("X", "Y"),
                    help="thin-lens camera: focus on what the centre of pixel (X, Y) sees")
    args = ap.parse_args(argv)
    for name, v in (("--lens-radius", args.lens_radius), ("--focal-distance", args.focal_distance)):
        if v is not None and not (math.isfinite(v) and v >= 0):  # refused before the scene is read
            ap.error(f"{name} needs a finite number >= 0")
    if args.focus_at is not None and args.focal_distance is not None:
        ap.error("--focus-at cannot be combined with --focal-distance")
    if args.env_res is not None and not 1 <= args.env_res <= 2048:  # refused before the scene is read
        ap.error("--env-res needs 1..2048")
    if args.env_scale is not None and not args.env_scale >= 0:
        ap.error("--env-scale needs a number >= 0")
    if args.env_forms and not args.env_path:
        ap.error("--env-forms needs --env-path")
    if args.denoise_iters is not None:  # refused before the scene is read
        if not args.denoise:
            ap.error("--denoise-iters needs --denoise")
        if not 1 <= args.denoise_iters <= denoise.MAX_ITERATIONS:
            ap.error(f"--denoise-iters needs 1..{denoise.MAX_ITERATIONS}")
    if args.feature_spp is not None:
        if not args.denoise and args.aov is None:
            ap.error("--feature-spp needs --denoise or --aov")
        if args.feature_spp < 1:
            ap.error("--feature-spp needs at least one sample")
    if args.aov is not None and not args.aov:
        ap.error("--aov needs a file prefix")
    if args.denoise_variance:  # refused before the scene is read
        if not args.denoise:
            ap.error("--denoise-variance needs --denoise")
        if args.pass_spp is None and not args.preview and args.adaptive is None:
            ap.error("--denoise-variance needs one of --pass-spp, --preview, --adaptive: the variance comes from the "
                     "spread of the passes, and one call is one batch")
        if args.gpus != 1:
            ap.error("--denoise-variance renders on one GPU (--gpus 1)")
    post = None
    if args.denoise or args.aov is not None:
        post = FilmPost(args.denoise, args.denoise_iters, args.feature_spp, per_pass=args.preview,
                        guided=args.denoise_variance)
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
    if args.mis:
        if not isinstance(sc.integrator, scene.PathIntegrator):
            ap.error(f"--mis needs the Path integrator; the scene's is {type(sc.integrator).__name__}")
        sc.integrator.mis = True
    if args.env is not None:
        try:
            sc.environment = scene.EnvironmentLight(envmap.read_map(args.env), layout="latlong")
        except (OSError, ValueError) as e:
            ap.error(f"--env: {e}")
    if sc.environment is None and (args.env_scale is not None or args.env_rotate is not None or args.env_res is not None):
        ap.error("--env-scale, --env-rotate and --env-res need an environment (--env, or the scene's EnvironmentLight)")
    if sc.environment is not None:
        if args.env_scale is not None:
            sc.environment.scale = (args.env_scale,) * 3
        if args.env_rotate is not None:
            sc.environment.rotation = (0.0, args.env_rotate, 0.0)
        if args.env_res is not None:
            sc.environment.resolution = args.env_res
    if passes and not isinstance(sc.integrator, scene.PathIntegrator):
        ap.error(f"--pass-spp, --preview, --time-budget, --checkpoint, --resume and --adaptive need the Path integrator; "
                 f"the scene's is {type(sc.integrator).__name__}")
    cam = sc.camera
    if args.lens_radius is not None:
        cam.lens_radius = float(np.float32(args.lens_radius))
    if args.focal_distance is not None:
        cam.focal_distance = float(np.float32(args.focal_distance))
    if args.focus_at is not None:  # a probe ray on the first device, before the render's contexts exist
        try:
            with capi.HipContext(0) as probe:
                scene.upload_scene(probe, scene.compile_scene(sc))
                cam.focal_distance = lens.autofocus(probe, cam, *args.focus_at)
        except ValueError as e:
            ap.error(str(e))
        print(f"focus at pixel ({args.focus_at[0]}, {args.focus_at[1]}): focal distance {cam.focal_distance:.9g}",
              flush=True)
    if cam.lens_radius > 0 and not cam.focal_distance > 0:
        ap.error("a lens radius > 0 needs a focal distance > 0 (--focal-distance, --focus-at or the camera's field)")
    out = args.out or sc.output
    t0 = time.time()

    def write_out(rad, wt):
        """The output image: the filtered film with --denoise, else the film."""
        if post is not None and post.image is not None:
            write_film(out, post.image, np.ones(post.image.shape[:2], np.float32))
        else:
            write_film(out, rad, wt)

    if args.adaptive is not None:
        def show_adaptive(info, rad, wt):
            if args.preview:
                write_out(rad, wt)
                print(f"pass {info['passes']} to {info['spp_max']} spp, {info['samples']} samples: "
                      f"{time.time() - t0:.2f}s -> {out}", flush=True)

        try:
            per_pass = args.preview or args.time_budget is not None
            rad, wt, info = render_scene_adaptive(sc, args.adaptive, 0, min_spp=args.min_spp, pass_spp=args.pass_spp,
                                                  on_pass=show_adaptive if per_pass else None,
                                                  time_budget=args.time_budget, post=post, env_path=args.env_path, env_forms=args.env_forms)
        except ValueError as e:
            ap.error(str(e))
        done = f"{info['spp_min']}..{info['spp_max']} ({info['samples']} samples in {info['passes']} passes)"
        if args.spp_map is not None:
            write_spp_map(args.spp_map, wt)
    elif passes:
        def show(done, rad, wt):
            if args.preview:
                write_out(rad, wt)
                print(f"pass to {done} spp: {time.time() - t0:.2f}s -> {out}", flush=True)

        try:
            rad, wt, done = render_scene_progressive(sc, 0, pass_spp=args.pass_spp, on_pass=show,
                                                     time_budget=args.time_budget, checkpoint=args.checkpoint,
                                                     resume=args.resume, post=post, env_path=args.env_path, env_forms=args.env_forms)
        except progressive.CheckpointError as e:
            ap.error(str(e))
    else:
        rad, wt = render_scene(sc, devices=list(range(args.gpus)), post=post, env_path=args.env_path, env_forms=args.env_forms)
        done = sc.integrator.spp
    write_out(rad, wt)
    if args.aov is not None:
        post.write_aov(args.aov)
    print(f"{type(sc.integrator).__name__} {sc.camera.resolution[0]}x{sc.camera.resolution[1]} "
          f"spp {done}: {time.time() - t0:.2f}s -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
