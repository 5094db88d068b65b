"""Environment maps for scene.EnvironmentLight: readers (.pfm, Radiance .hdr, .npy), the lat-long to
octahedral resampling, and a closed-form sky for tests and measurements without files.

The octahedral layout is DESIGN.md section 3.17's: texel (i, j) of an N x N map covers
x in [-1 + 2i/N, -1 + 2(i+1)/N] of the square [-1, 1]^2 (y likewise with the row j), z = 1 - |x| - |y|,
the lower hemisphere folded into the corners.  +y is up in a lat-long image (row 0 is the zenith) and
its column 0 looks along -z, turning towards +x.  Host side, numpy f64: the device reads only the result.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np


class EnvMapError(ValueError):
    pass


# ----------------------------------------------------------------------------- readers
def read_pfm(path) -> np.ndarray:
    """Portable float map, colour (PF) or grey (Pf), either byte order -> float32 [h, w, 3], top row first."""
    raw = Path(path).read_bytes()
    m = re.match(rb"(P[Ff])\s+(\d+)\s+(\d+)\s+([-+0-9.eE]+)[^\n]*\n", raw)
    if not m:
        raise EnvMapError(f"{path}: not a PFM file")
    ch = 3 if m.group(1) == b"PF" else 1
    w, h = int(m.group(2)), int(m.group(3))
    order = "<" if float(m.group(4)) < 0 else ">"
    body = raw[m.end():]
    if len(body) < 4 * w * h * ch:
        raise EnvMapError(f"{path}: {len(body)} bytes of pixels, {4 * w * h * ch} expected")
    a = np.frombuffer(body[:4 * w * h * ch], order + "f4").reshape(h, w, ch)[::-1].astype(np.float32)
    return np.ascontiguousarray(np.repeat(a, 3, axis=2) if ch == 1 else a)


def _rgbe_to_float(px: np.ndarray) -> np.ndarray:
    """[..., 4] uint8 RGBE -> float32 rgb: mantissa * 2^(e - 136), 0 where e == 0."""
    e = px[..., 3].astype(np.int32)
    f = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return (px[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)


def decode_hdr(raw: bytes, name="hdr") -> np.ndarray:
    """Radiance RGBE picture (-Y h +X w; flat or new-style run-length rows) -> float32 [h, w, 3]."""
    if not raw.startswith(b"#?"):
        raise EnvMapError(f"{name}: not a Radiance file")
    end = raw.find(b"\n\n")
    if end < 0:
        raise EnvMapError(f"{name}: no end of header")
    header = raw[:end]
    if b"FORMAT=" in header and b"32-bit_rle_rgbe" not in header:
        raise EnvMapError(f"{name}: only 32-bit_rle_rgbe pictures are read")
    nl = raw.find(b"\n", end + 2)
    m = re.match(rb"-Y\s+(\d+)\s+\+X\s+(\d+)\s*$", raw[end + 2:nl])
    if not m:
        raise EnvMapError(f"{name}: only the -Y h +X w orientation is read")
    h, w = int(m.group(1)), int(m.group(2))
    data = np.frombuffer(raw, np.uint8, offset=nl + 1)
    out = np.zeros((h, w, 4), np.uint8)
    pos = 0
    for y in range(h):
        rle = (8 <= w < 32768 and pos + 4 <= data.size and data[pos] == 2 and data[pos + 1] == 2 and
               (int(data[pos + 2]) << 8 | int(data[pos + 3])) == w)
        if not rle:      # flat: w RGBE pixels (old-style runs are not produced by any current writer)
            if pos + 4 * w > data.size:
                raise EnvMapError(f"{name}: row {y} is cut short")
            out[y] = data[pos:pos + 4 * w].reshape(w, 4)
            pos += 4 * w
            continue
        pos += 4
        for c in range(4):   # each channel of the row on its own: runs (count > 128) and literals
            x = 0
            while x < w:
                if pos >= data.size:
                    raise EnvMapError(f"{name}: row {y} is cut short")
                n = int(data[pos])
                pos += 1
                if n > 128:
                    n -= 128
                    if n == 0 or x + n > w or pos >= data.size:
                        raise EnvMapError(f"{name}: bad run in row {y}")
                    out[y, x:x + n, c] = data[pos]
                    pos += 1
                else:
                    if n == 0 or x + n > w or pos + n > data.size:
                        raise EnvMapError(f"{name}: bad literal in row {y}")
                    out[y, x:x + n, c] = data[pos:pos + n]
                    pos += n
                x += n
    return _rgbe_to_float(out)


def read_hdr(path) -> np.ndarray:
    return decode_hdr(Path(path).read_bytes(), str(path))


def read_map(path) -> np.ndarray:
    """An environment image by its suffix -> float32 [h, w, 3]."""
    path = Path(path)
    suffix = path.suffix.lower()
    if suffix == ".pfm":
        a = read_pfm(path)
    elif suffix == ".hdr":
        a = read_hdr(path)
    elif suffix == ".npy":
        a = np.asarray(np.load(path), np.float32)
        if a.ndim == 2:
            a = np.repeat(a[..., None], 3, axis=2)
        if a.ndim != 3 or a.shape[2] not in (3, 4):
            raise EnvMapError(f"{path}: an image is [h, w], [h, w, 3] or [h, w, 4], not {a.shape}")
        a = a[..., :3]
    else:
        raise EnvMapError(f"{path}: unsupported environment image format {path.suffix} (.pfm, .hdr, .npy)")
    return np.ascontiguousarray(a, np.float32)


# ----------------------------------------------------------------------------- layouts
def octahedral_directions(n: int, sub: int = 1, j0: int = 0, j1: int = None) -> np.ndarray:
    """Unit directions (f64) of the sub x sub sample points of every texel of rows [j0, j1) ->
    [j1 - j0, n, sub, sub, 3] (row j first)."""
    j1 = n if j1 is None else j1
    t = (np.arange(n * sub) + 0.5) / (n * sub) * 2.0 - 1.0
    x, y = np.meshgrid(t, t[j0 * sub:j1 * sub])   # y varies with the row
    z = 1.0 - np.abs(x) - np.abs(y)
    sx, sy = np.where(x < 0, -1.0, 1.0), np.where(y < 0, -1.0, 1.0)
    fx, fy = np.where(z < 0, (1.0 - np.abs(y)) * sx, x), np.where(z < 0, (1.0 - np.abs(x)) * sy, y)
    q = np.stack([fx, fy, z], axis=-1)
    d = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return d.reshape(j1 - j0, sub, n, sub, 3).transpose(0, 2, 1, 3, 4)


def latlong_lookup(img: np.ndarray, d: np.ndarray) -> np.ndarray:
    """Nearest texel of a lat-long image for unit directions d [..., 3]."""
    h, w = img.shape[:2]
    theta = np.arccos(np.clip(d[..., 1], -1.0, 1.0))            # 0 at +y
    phi = np.arctan2(d[..., 0], -d[..., 2])                     # 0 along -z, towards +x
    r = np.clip((theta / np.pi * h).astype(np.int64), 0, h - 1)
    c = np.clip(((phi / (2 * np.pi)) % 1.0 * w).astype(np.int64), 0, w - 1)
    return img[r, c]


def latlong_to_octahedral(img, n: int, supersample: int = 4) -> np.ndarray:
    """Resample a lat-long image [h, w, 3] into an n x n octahedral map.  Each texel is the solid-angle
    weighted mean of supersample^2 points spread over its area, so a small sun is not missed."""
    img = np.asarray(img, np.float32)
    if img.ndim != 3 or img.shape[2] < 3 or n < 1 or supersample < 1:
        raise EnvMapError("latlong_to_octahedral: an image [h, w, 3], n >= 1 and supersample >= 1 are needed")
    s = int(supersample)
    src = img[..., :3].astype(np.float64)
    t = (np.arange(n * s) + 0.5) / (n * s) * 2.0 - 1.0
    out = np.zeros((n, n, 3), np.float32)
    rows = max(1, (1 << 20) // (n * s * s))              # about a million points at a time
    for j0 in range(0, n, rows):
        j1 = min(n, j0 + rows)
        x, y = np.meshgrid(t, t[j0 * s:j1 * s])
        d = octahedral_directions(n, s, j0, j1)
        # d omega = dx dy / |q|^3 and |q|_2 is the same on both sides of the fold's mirror
        z = 1.0 - np.abs(x) - np.abs(y)
        fx, fy = np.where(z < 0, 1.0 - np.abs(y), np.abs(x)), np.where(z < 0, 1.0 - np.abs(x), np.abs(y))
        wgt = (fx * fx + fy * fy + z * z) ** -1.5
        wgt = wgt.reshape(j1 - j0, s, n, s).transpose(0, 2, 1, 3)[..., None]
        val = latlong_lookup(src, d)
        out[j0:j1] = (val * wgt).sum(axis=(2, 3)) / wgt.sum(axis=(2, 3))
    return out


def procedural_sky(n: int, sun_dir=(0.3, 0.8, 0.5), sun_radiance=400.0, sun_angle_deg=3.0,
                   zenith=(0.25, 0.45, 1.0), horizon=(0.9, 0.9, 0.95), ground=(0.12, 0.11, 0.1),
                   supersample: int = 4) -> np.ndarray:
    """A closed-form sky as an n x n octahedral map (+y up): a zenith-to-horizon gradient, a dim ground
    below, and a sun disc of `sun_angle_deg` radius; texels are means over at least supersample^2 points,
    and over as many as it takes for the points to be closer together than the sun is wide."""
    sub = max(int(supersample), int(np.ceil(5.0 / (n * np.radians(sun_angle_deg)))))
    s = np.asarray(sun_dir, np.float64)
    s = s / np.linalg.norm(s)
    out = np.zeros((n, n, 3), np.float32)
    rows = max(1, (1 << 20) // (n * sub * sub))          # about a million points at a time
    for j0 in range(0, n, rows):
        d = octahedral_directions(n, sub, j0, min(n, j0 + rows))
        up = d[..., 1]
        k = np.clip(up, 0.0, 1.0)[..., None] ** 0.5
        sky = np.asarray(horizon, np.float64) * (1.0 - k) + np.asarray(zenith, np.float64) * k
        col = np.where(up[..., None] >= 0, sky, np.asarray(ground, np.float64))
        col = col + np.where((d @ s)[..., None] >= np.cos(np.radians(sun_angle_deg)), float(sun_radiance), 0.0)
        out[j0:j0 + rows] = col.mean(axis=(2, 3))
    return out


def rotation_matrix(rotation) -> np.ndarray:
    """world_to_env R (f64 3x3) of an EnvironmentLight's `rotation`: a 3x3 matrix M with d_world = M d_env,
    or Euler angles in degrees (x, y, z) applied in that order, M = Rz Ry Rx.  R = M^T."""
    r = np.asarray(rotation, np.float64)
    if r.shape == (3, 3):
        m = r
    elif r.shape == (3,):
        ax, ay, az = np.radians(r)
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        m = rz @ ry @ rx
    else:
        raise EnvMapError("rotation: three Euler angles in degrees or a 3x3 matrix")
    return np.ascontiguousarray(m.T)
