"""Parameters of the edge-avoiding a-trous filter of the film and views of its feature buffers
(include/akr_hip.h).  Everything here runs on the host and is checked before a
device is touched; the filter itself is HipContext.denoise / denoise_device (csrc/denoise.hip).
"""
from __future__ import annotations

import math

import numpy as np

from . import capi

# The library's defaults: the values the filter's definition was tried with, on the oracle's Cornell
# box 128x128 (4-spp film, 2 feature samples; filtered relMSE 0.28 of the raw film's)
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_depth=0.02, sigma_albedo=0.3, sigma_color=0.5,
                demodulate=True)
# The variance-guided filter takes the same parameters and sigma_variance: the sweep over
# 1 / 2 / 4 / 8 on the same set-up gave relMSE 0.00741 / 0.00462 / 0.00483 / 0.00695 at 4 spp,
# 0.00253 / 0.00205 / 0.00280 / 0.00444 at 16 and 0.00085 / 0.00084 / 0.00130 / 0.00240 at 64
DEFAULT_SIGMA_VARIANCE = 2.0
VARIANCE_FLOATS = 4   # (vr, vg, vb, K) per pixel, as akr_hip_render_variance returns it
MAX_ITERATIONS = 8
MAX_SQUARINGS = 8
DEFAULT_FEATURE_SPP = 2


def check(iterations, normal_squarings, sigma_depth, sigma_albedo, sigma_color) -> None:
    """The parameter rules of akr_hip_denoise; raises ValueError."""
    for name, v, hi in (("iterations", iterations, MAX_ITERATIONS), ("normal_squarings", normal_squarings, MAX_SQUARINGS)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"denoise: {name} must be an integer")
    if not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"denoise: iterations must be in 1..{MAX_ITERATIONS}")
    if not 0 <= int(normal_squarings) <= MAX_SQUARINGS:
        raise ValueError(f"denoise: normal_squarings must be in 0..{MAX_SQUARINGS}")
    for name, v in (("sigma_depth", sigma_depth), ("sigma_albedo", sigma_albedo)):
        if not (float(v) > 0.0 and math.isfinite(float(v))):   # NaN fails too
            raise ValueError(f"denoise: {name} must be > 0 and finite")
    if math.isnan(float(sigma_color)):
        raise ValueError("denoise: sigma_color must not be NaN (<= 0 disables the colour stop)")


def params(**kw) -> "capi.DenoiseParams":
    """akr_denoise_params from keyword arguments over DEFAULTS (demodulate=False: AO films)."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"denoise: unknown parameter(s) {sorted(unknown)}")
    p = dict(DEFAULTS, **kw)
    check(p["iterations"], p["normal_squarings"], p["sigma_depth"], p["sigma_albedo"], p["sigma_color"])
    return capi.DenoiseParams(int(p["iterations"]), int(p["normal_squarings"]), float(p["sigma_depth"]),
                              float(p["sigma_albedo"]), float(p["sigma_color"]),
                              0 if p["demodulate"] else capi.DENOISE_NO_DEMODULATE)


def guided_params(**kw) -> "capi.DenoiseGuidedParams":
    """akr_denoise_guided_params: the keywords of params() and sigma_variance (> 0 and finite)."""
    kw = dict(kw)
    sv = kw.pop("sigma_variance", DEFAULT_SIGMA_VARIANCE)
    base = params(**kw)
    if isinstance(sv, bool) or not (float(sv) > 0.0 and math.isfinite(float(sv))):   # NaN fails too
        raise ValueError("denoise: sigma_variance must be > 0 and finite")
    return capi.DenoiseGuidedParams(base, float(sv))


def check_variance_shape(weight, variance) -> None:
    want = weight.shape + (VARIANCE_FLOATS,)
    if variance.shape != want:
        raise ValueError(f"denoise: variance has shape {variance.shape}, the weight asks for {want}")


def check_shapes(radiance, weight, features) -> None:
    if weight.ndim != 2 or weight.size == 0:
        raise ValueError("denoise: weight must be a non-empty [H, W] array")
    h, w = weight.shape
    if radiance.shape != (h, w, 3):
        raise ValueError(f"denoise: radiance has shape {radiance.shape}, the weight asks for {(h, w, 3)}")
    if features.shape != (h, w, capi.FEATURE_FLOATS):
        raise ValueError(f"denoise: features have shape {features.shape}, the weight asks for {(h, w, capi.FEATURE_FLOATS)}")


def split_features(features):
    """The feature sums [H, W, 12] as images: (albedo [H, W, 3], normal [H, W, 3], depth [H, W],
    coverage [H, W]).  Albedo, normal and depth are means over the samples that hit (0 where none
    did); the normal is not renormalised; coverage is the hit count."""
    f = np.asarray(features, np.float32)
    if f.ndim != 3 or f.shape[2] != capi.FEATURE_FLOATS:
        raise ValueError(f"features must be [H, W, {capi.FEATURE_FLOATS}], got {f.shape}")
    hits = f[..., 3]
    d = np.where(hits > 0, hits, np.float32(1))[..., None]
    some = (hits > 0)[..., None]
    albedo = np.where(some, f[..., 0:3] / d, np.float32(0)).astype(np.float32)
    normal = np.where(some, f[..., 4:7] / d, np.float32(0)).astype(np.float32)
    depth = np.where(some[..., 0], f[..., 7] / d[..., 0], np.float32(0)).astype(np.float32)
    return albedo, normal, depth, hits.copy()
