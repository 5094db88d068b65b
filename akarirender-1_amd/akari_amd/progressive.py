"""Progressive passes and checkpoints on a context's render session.

A path render can be continued: akr_hip_render_continue adds samples to every film slot from the
sampler state and film sums the last segment left, so a + b samples in two segments are the a + b
samples of one render, bit for bit.  This module builds the user-facing pieces on that: a render in
passes (preview after each pass, an optional time budget) and a checkpoint file that carries a
session to another process.
"""
from __future__ import annotations

import hashlib
import os
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, List, Optional, Union

import numpy as np

from . import capi

Schedule = Union[str, int]


def pass_chunks(total: int, schedule: Schedule = "double", done: int = 0, first: int = 1) -> List[int]:
    """Samples per pass that take a slot from `done` to `total` samples.

    schedule "double": the pass doubles the samples done (`first` samples when none are: 1, 1, 2, 4, ...),
    so every preview has twice the samples of the one before; an int N: passes of N samples.  The
    chunks sum to total - done; only the last one can be short."""
    total, done = int(total), int(done)
    if total < done:
        raise ValueError(f"{done} samples are done already, more than the {total} asked for")
    if isinstance(schedule, str):
        if schedule != "double":
            raise ValueError(f"unknown schedule {schedule!r} (\"double\" or a chunk size)")
        if first < 1:
            raise ValueError("the first pass needs at least one sample")
        fixed = 0
    else:
        fixed = int(schedule)
        if fixed < 1:
            raise ValueError("a pass needs at least one sample")
    out = []
    while done < total:
        n = min(fixed or (done if done > 0 else int(first)), total - done)
        out.append(n)
        done += n
    return out


def render_progressive(ctx: "capi.HipContext", spp: int, max_depth: int, tiles, width: int, height: int,
                       schedule: Schedule = "double", on_pass: Optional[Callable] = None,
                       time_budget: Optional[float] = None, ray_clamp: float = 0.0, exact_cull: bool = False,
                       resume: bool = False, clock: Callable[[], float] = time.monotonic):
    """Render `spp` samples per pixel of `tiles` in passes; returns (radiance, weight, spp_done).

    The first pass starts a session (HipContext.render), the others continue it; with `resume` the
    context's session (a restored Checkpoint) is continued up to a total of `spp`.  After every pass
    `on_pass(spp_done, radiance, weight)` gets the film so far (fresh full-frame buffers); a true
    return value stops the render.  `time_budget` (seconds) stops it after the first pass that ends
    past the budget, so at least one pass is rendered.  The film of k passes is the film of one render
    of their samples, bit for bit."""
    done = 0
    if resume:
        info = ctx.render_state_info()
        if (info["width"], info["height"]) != (int(width), int(height)):
            raise ValueError("the session was rendered at another resolution")
        done = info["spp_done"]
    chunks = pass_chunks(spp, schedule, done)
    t0 = clock()
    rad = wt = None
    if not chunks:  # nothing to add: the session's film as it stands (an empty film when there is none)
        if resume:
            rad, wt = ctx.render_continue(0, width, height)
        else:
            rad, wt = ctx.render(0, max_depth, tiles, width, height, ray_clamp=ray_clamp, exact_cull=exact_cull)
    for k, n in enumerate(chunks):
        if k == 0 and not resume:
            rad, wt = ctx.render(n, max_depth, tiles, width, height, ray_clamp=ray_clamp, exact_cull=exact_cull)
        else:
            rad, wt = ctx.render_continue(n, width, height)
        done += n
        if on_pass is not None and on_pass(done, rad, wt):
            break
        if time_budget is not None and clock() - t0 >= time_budget:
            break
    return rad, wt, done


def adaptive_totals(min_spp: int, pass_spp: int, cap: int) -> List[int]:
    """The sample counts a still-active slot of an adaptive render passes through:
    min_spp, then pass_spp more per pass (0: each pass doubles the count), clipped at `cap`.  A cap at
    or below min_spp is a plain render of `cap` samples: one total, no test."""
    min_spp, pass_spp, cap = int(min_spp), int(pass_spp), int(cap)
    if min_spp < 1:
        raise ValueError("min_spp must be at least 1")
    if pass_spp < 0:
        raise ValueError("pass_spp must be >= 0 (0: passes double)")
    if cap < 0:
        raise ValueError("the cap must be >= 0")
    out = [min(min_spp, cap)]
    while out[-1] < cap:
        out.append(min(cap, out[-1] + pass_spp if pass_spp > 0 else 2 * out[-1]))
    return out


def check_adaptive_args(threshold: float, min_spp: int, pass_spp: int, cap: int) -> None:
    """The argument rules of an adaptive render, checked before a device is touched."""
    t = float(threshold)
    if not t >= 0.0:  # NaN fails too
        raise ValueError("the adaptive threshold must be >= 0 and not NaN")
    adaptive_totals(min_spp, pass_spp, cap)
    if int(cap) > capi.MAX_SESSION_SPP:
        raise ValueError("the cap exceeds 2^24 samples per pixel")


def render_adaptive(ctx: "capi.HipContext", cap_spp: int, max_depth: int, tiles, width: int, height: int,
                    threshold: float, min_spp: int = 16, pass_spp: int = 0, on_pass: Optional[Callable] = None,
                    time_budget: Optional[float] = None, ray_clamp: float = 0.0, exact_cull: bool = False,
                    clock: Callable[[], float] = time.monotonic):
    """Adaptive render of `tiles`: returns (radiance, weight, info).

    Every pixel gets min_spp samples; then passes add samples to the 64-slot strips whose error is above
    `threshold` (pass_spp per pass, 0: doubling), up to cap_spp.  The weight holds each pixel's sample
    count; info has passes, spp_min, spp_max, samples, strips and strips_at_cap.  Without on_pass and
    time_budget this is one library call; with either, the render runs pass by pass: after each pass
    `on_pass(info, radiance, weight)` gets the film so far (a true return stops the render), and
    `time_budget` (seconds) stops it after the first pass that ends past the budget.  The passes done
    give the same film either way."""
    check_adaptive_args(threshold, min_spp, pass_spp, cap_spp)
    if on_pass is None and time_budget is None:
        return ctx.render_adaptive(cap_spp, max_depth, tiles, width, height, threshold, min_spp=min_spp,
                                   pass_spp=pass_spp, ray_clamp=ray_clamp, exact_cull=exact_cull)
    t0 = clock()
    info, more = ctx.adaptive_begin(cap_spp, max_depth, tiles, threshold, min_spp=min_spp, pass_spp=pass_spp,
                                    ray_clamp=ray_clamp, exact_cull=exact_cull)
    while True:
        rad, wt = ctx.render_continue(0, width, height)
        if on_pass is not None and on_pass(info, rad, wt):
            break
        if not more or (time_budget is not None and clock() - t0 >= time_budget):
            break
        info, more = ctx.adaptive_step()
    return rad, wt, info


def scene_fingerprint(cs, mis: bool = False) -> str:
    """SHA-256 over a CompiledScene's arrays and camera, and the `mis` switch when it is on: what a film's
    samples depend on."""
    h = hashlib.sha256()

    def add(tag, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        h.update(f"{tag}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())

    add("vertices", cs.vertices, np.float32)
    add("indices", cs.indices, np.int32)
    add("normals", cs.normals, np.float32)
    add("texcoords", cs.texcoords, np.float32)
    add("matid", cs.matid, np.int32)
    add("mesh_base", cs.mesh_base, np.uint32)
    for m in cs.materials:
        h.update(b"material;" + bytes(m))
    for t in cs.textures:
        h.update(b"texture;" + bytes(t))
    for k, im in enumerate(cs.images):
        add(f"image{k}", im, np.float32)
    add("lights", np.asarray(cs.lights, np.int64).reshape(-1, 2), np.int64)
    add("power", cs.power, np.float32)
    cam = cs.camera
    add("cam_position", cam.position, np.float32)
    add("cam_rotation", cam.rotation, np.float32)
    add("cam_fov", [cam.fov], np.float64)
    add("cam_resolution", cam.resolution, np.int32)
    lens = (np.float32(getattr(cam, "lens_radius", 0.0)), np.float32(getattr(cam, "focal_distance", 0.0)))
    if lens[0] > 0 and lens[1] > 0:  # an inactive lens is the pinhole: it keeps the fingerprint it always had
        add("cam_lens", lens, np.float32)
    if mis:  # a render without it keeps the fingerprint it always had
        add("mis", [1], np.int32)
    env = getattr(cs, "environment", None)
    if env is not None:  # a scene without one keeps the fingerprint it always had
        add("env_map", env.map, np.float32)
        add("env_scale", env.scale, np.float32)
        add("env_select_prob", [env.select_prob], np.float32)
        add("env_world_to_env", env.world_to_env, np.float32)
    return h.hexdigest()


class CheckpointError(ValueError):
    """A checkpoint that cannot be read, or that belongs to another scene, resolution or tile list."""


@dataclass
class Checkpoint:
    """A render session on disk: one .npz with the format version, resolution, tiles, parameters,
    samples done, the slots' sampler states and film sums, and the scene's fingerprint."""
    width: int
    height: int
    tiles: np.ndarray        # int32 [n, 4], as given to the render
    spp_done: int
    max_depth: int
    ray_clamp: float
    flags: int
    sampler: np.ndarray      # uint32 [n_pixels]
    film: np.ndarray         # float32 [n_pixels, 4]
    fingerprint: str

    FORMAT_VERSION = 1

    @classmethod
    def capture(cls, ctx: "capi.HipContext", cs, tiles, mis: bool = False) -> "Checkpoint":
        """The context's session, rendered over `tiles` of the compiled scene `cs` (`mis`: with option "mis")."""
        info = ctx.render_state_info()
        sampler, film = ctx.render_state_export()
        return cls(info["width"], info["height"], capi.rect_array(tiles), info["spp_done"], info["max_depth"],
                   float(info["ray_clamp"]), info["flags"], sampler, film, scene_fingerprint(cs, mis))

    def save(self, path) -> None:
        """Written under a temporary name and renamed: a reader never sees half a file."""
        path = Path(path)
        tmp = path.with_name(path.name + f".tmp{os.getpid()}")
        try:
            with open(tmp, "wb") as f:
                np.savez(f, version=np.int32(self.FORMAT_VERSION), resolution=np.array([self.width, self.height], np.int32),
                         tiles=capi.rect_array(self.tiles), spp_done=np.int32(self.spp_done),
                         max_depth=np.int32(self.max_depth), ray_clamp=np.float32(self.ray_clamp),
                         flags=np.int32(self.flags), sampler=np.ascontiguousarray(self.sampler, np.uint32),
                         film=np.ascontiguousarray(self.film, np.float32), fingerprint=np.array(self.fingerprint))
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        finally:
            if tmp.exists():
                tmp.unlink()

    @classmethod
    def load(cls, path) -> "Checkpoint":
        try:
            with np.load(path, allow_pickle=False) as z:
                version = int(z["version"])
                if version != cls.FORMAT_VERSION:
                    raise CheckpointError(f"{path}: checkpoint format {version}, this build reads {cls.FORMAT_VERSION}")
                w, h = (int(v) for v in z["resolution"])
                ck = cls(w, h, capi.rect_array(z["tiles"]), int(z["spp_done"]), int(z["max_depth"]),
                         float(z["ray_clamp"]), int(z["flags"]), np.ascontiguousarray(z["sampler"], np.uint32),
                         np.ascontiguousarray(z["film"], np.float32), str(z["fingerprint"]))
        except CheckpointError:
            raise
        except Exception as e:  # not an .npz, or a field is missing
            raise CheckpointError(f"{path}: not a render checkpoint ({e})") from e
        if ck.film.shape != (ck.sampler.size, 4):
            raise CheckpointError(f"{path}: {ck.sampler.size} sampler states but film of shape {ck.film.shape}")
        return ck

    def check(self, cs, tiles, width: int, height: int, mis: bool = False) -> None:
        """Raises CheckpointError unless the checkpoint was rendered from this scene, at this
        resolution, over this tile list, with this value of the `mis` switch."""
        if (self.width, self.height) != (int(width), int(height)):
            raise CheckpointError(f"checkpoint resolution {self.width}x{self.height}, scene {width}x{height}")
        if not np.array_equal(capi.rect_array(tiles), self.tiles):
            raise CheckpointError("checkpoint tile list differs from the render's")
        if scene_fingerprint(cs, mis) != self.fingerprint:
            if scene_fingerprint(cs, not mis) == self.fingerprint:
                raise CheckpointError(f"checkpoint was rendered with mis {'off' if mis else 'on'}, the render asks for "
                                      f"mis {'on' if mis else 'off'}: the two estimators do not continue one another")
            raise CheckpointError("checkpoint was rendered from another scene or camera (fingerprint differs)")

    def restore(self, ctx: "capi.HipContext", cs, tiles, mis: bool = False) -> None:
        """Establish the checkpoint's session on `ctx`, which holds the uploaded scene `cs`; option "mis" is
        set to `mis` first, since the session reads it when it starts."""
        w, h = (int(v) for v in cs.camera.resolution)
        self.check(cs, tiles, w, h, mis)
        ctx.set_option("mis", 1 if mis else 0)
        ctx.render_state_import(self.spp_done, self.max_depth, self.tiles, self.sampler, self.film,
                                ray_clamp=self.ray_clamp, exact_cull=bool(self.flags & capi.PT_EXACT_CULL))
