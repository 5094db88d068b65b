"""Thin-lens helpers of the command line: the pinhole ray through a pixel's centre and the
autofocus arithmetic of `--focus-at X Y`.

The lens itself is the library's (akr_hip_set_lens); nothing here renders.  The ray is the camera's of
kernel/camera.h:45-86 at u2 = (0.5, 0.5) in numpy f32; it aims a probe, so it need not match the device's
rounding bit for bit.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

F32 = np.float32
EPS = F32(0.001)   # Ray3f's tmin (common/math.h:41)


def _rot(axis: int, deg: float) -> np.ndarray:
    t = float(F32(F32(deg) * F32(math.pi) / F32(180.0)))
    s, c = F32(math.sin(t)), F32(math.cos(t))
    m = np.eye(4, dtype=F32)
    if axis == 0:      # rotate_x (math.h:274-279)
        m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    elif axis == 1:    # rotate_y (math.h:281-286)
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    else:              # rotate_z (math.h:288-293)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def camera_matrices(cam) -> Tuple[np.ndarray, np.ndarray]:
    """(r2c, c2w) of a PerspectiveCamera (core/nodes/camera.cpp:32-47, kernel/camera.h:45-59)."""
    tr = np.eye(4, dtype=F32)
    tr[:3, 3] = np.asarray(cam.position, F32)
    c2w = (tr @ (_rot(1, cam.rotation[0]) @ (_rot(0, cam.rotation[1]) @ _rot(2, cam.rotation[2])))).astype(F32)
    rx, ry = (int(v) for v in cam.resolution)
    s = F32(math.atan(float(F32(float(cam.fov) * float(F32(math.pi)) / 180.0)) / 2.0))
    sx, sy = (s, F32(s * F32(ry) / F32(rx))) if rx > ry else (F32(s * F32(rx) / F32(ry)), s)
    # scale(1 / res) -> scale(2) -> translate(-1) -> scale(1, -1) -> scale(sx, sy)
    r2c = np.eye(4, dtype=F32)
    r2c[0, 0], r2c[0, 3] = F32(sx * F32(2.0) / F32(rx)), F32(-sx)
    r2c[1, 1], r2c[1, 3] = F32(-sy * F32(2.0) / F32(ry)), F32(sy)
    return r2c, c2w


def pinhole_ray(cam, x: int, y: int):
    """The pinhole ray through the centre of pixel (x, y) -> (origin, world direction, camera-space direction)."""
    r2c, c2w = camera_matrices(cam)
    p = r2c @ np.array([F32(x) + F32(0.5), F32(y) + F32(0.5), 0, 1], F32)
    d_cam = np.array([p[0], p[1], F32(-1.0)], F32)
    d_cam = (d_cam / F32(np.sqrt(F32(d_cam @ d_cam)))).astype(F32)
    return c2w[:3, 3].copy(), (c2w[:3, :3] @ d_cam).astype(F32), d_cam


def focal_distance_from_hit(t, d_cam) -> float:
    """The focal distance that puts the hit at distance `t` along the unit camera-space direction `d_cam` on
    the plane of focus: t * |d_cam.z| in f32 (the inverse of camera.h:76's ft = focal_distance / |d.z|)."""
    t = F32(t)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"autofocus: the hit distance {t} is not a finite number > 0")
    return float(F32(t * F32(abs(F32(d_cam[2])))))


def autofocus(ctx, cam, x: int, y: int) -> float:
    """Trace the pinhole ray through pixel (x, y) with akr_hip_trace on a context that holds the scene and
    return the focal distance of what it hits; a miss is a ValueError that names the pixel."""
    from . import capi
    w, h = (int(v) for v in cam.resolution)
    if not (0 <= x < w and 0 <= y < h):
        raise ValueError(f"--focus-at: pixel ({x}, {y}) is outside the {w} x {h} frame")
    o, d, d_cam = pinhole_ray(cam, x, y)
    rays = np.zeros(1, capi.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmin"], rays["tmax"] = o, d, EPS, np.inf
    hit = ctx.trace(rays)[0]
    if int(hit["prim_id"]) < 0 or not np.isfinite(hit["t"]):
        raise ValueError(f"--focus-at: the ray through pixel ({x}, {y}) hits nothing")
    return focal_distance_from_hit(hit["t"], d_cam)
