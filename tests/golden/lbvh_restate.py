"""The GPU LBVH builder (csrc/lbvh.hip) restated in numpy, from the header comment of lbvh.hip and
Karras 2012 ("Maximizing parallelism in the construction of BVHs, octrees, and k-d trees").

The builder's output is a function of the mesh alone: a stable sort of (Morton code, triangle)
pairs, internal node i of Karras' numbering in record i + 1, leaves in sorted order, boxes that are
minima and maxima of vertex coordinates.  This file states that function without the kernels' means:

  codes    bit by bit (no magic-mask spread)
  tree     top-down over ranges of the augmented keys (code << 32 | sorted index), the split found by
           bisection for the first key that has the range's highest differing bit set; Karras' node
           numbering follows from "a node's index is an end of its range": the left child of a split
           after position g is internal node g, the right one internal node g + 1
  boxes    each child box is the minimum / maximum over the child's range of leaf boxes, taken on
           order-preserving integer keys (so -0.0 < +0.0, as the device's min / max instructions
           order them); nothing is handed up from the leaves

All float arithmetic is f32 and unfused.  It shares no code with the library and imports none of it.
NaN and infinite coordinates are outside its domain.
"""
from bisect import bisect_left

import numpy as np

F = np.float32
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
CELLS = 2097151          # 2^21 - 1: the largest cell index of an axis
MAX_DEPTH = 64           # AKR_BVH_MAX_DEPTH: the deepest tree build_lbvh_gpu accepts

# include/akr_bvh_format.h akr_bvh_node / akr_bvh_tri (tests assert these equal capi's dtypes)
NODE_DTYPE = np.dtype([("bxy0", np.float32, 4), ("bxy1", np.float32, 4), ("bz", np.float32, 4),
                       ("child", np.uint32, 2), ("axis", np.uint32), ("_pad", np.uint32)])
TRI_DTYPE = np.dtype([("v0", np.float32, 3), ("gid", np.uint32), ("e1", np.float32, 3), ("_p0", np.uint32),
                      ("e2", np.float32, 3), ("_p1", np.uint32)])


def okey(x):
    """f32 -> int32 in the floats' total order (-0.0 below +0.0).  Its own inverse on the bits."""
    b = np.ascontiguousarray(x, np.float32).view(np.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def okey_inv(k):
    k = np.ascontiguousarray(k, np.int32)
    return (k ^ ((k >> 31) & 0x7FFFFFFF)).view(np.float32)


def tri_boxes(vertices, indices):
    """(lo, hi) [n, 3] f32: per-triangle minima and maxima, signed zeros ordered."""
    k = okey(np.asarray(vertices, np.float32)[np.asarray(indices)])          # [n, 3 corners, 3 axes]
    return okey_inv(k.min(axis=1)), okey_inv(k.max(axis=1))


def centres(vertices, indices):
    """Box centres 0.5 * mn + 0.5 * mx in f32 (two products, one sum: unfused)."""
    lo, hi = tri_boxes(vertices, indices)
    return (F(0.5) * lo + F(0.5) * hi).astype(np.float32)


def cells_f32(c):
    """21-bit cell of every centre on every axis, as the builder quantises: scene bounds over the
    centres, t = (c - lo) / ext (0 where ext is not positive) clamped to [0, 1], trunc(t * 2097151f)."""
    c = np.asarray(c, np.float32)
    lo, hi = okey_inv(okey(c).min(axis=0)), okey_inv(okey(c).max(axis=0))
    ext = (hi - lo).astype(np.float32)
    safe = np.where(ext > 0, ext, F(1.0)).astype(np.float32)
    t = np.where(ext > 0, ((c - lo).astype(np.float32) / safe).astype(np.float32), F(0.0)).astype(np.float32)
    t = np.minimum(np.maximum(t, F(0.0)), F(1.0))
    return (t * F(CELLS)).astype(np.float32).astype(np.uint64)


def interleave(cells):
    """63-bit Morton code: bit k of x, y, z at code bits 3k + 2, 3k + 1, 3k (x's MSB is bit 62)."""
    cells = np.asarray(cells, np.uint64)
    code = np.zeros(cells.shape[0], np.uint64)
    for k in range(21):
        for axis in range(3):
            code |= ((cells[:, axis] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + 2 - axis)
    return code


def code_axis(bit):
    """The axis whose cell bit sits at Morton bit `bit`."""
    return 2 - bit % 3


def morton(vertices, indices):
    """(codes uint64 [n], cells uint64 [n, 3], centres f32 [n, 3]) in triangle order."""
    c = centres(vertices, indices)
    q = cells_f32(c)
    return interleave(q), q, c


def code_cells_f64(vertices, indices):
    """The builder's own f32 centres, and their cells quantised in float64: bounds, t = (c - lo) / ext
    and floor(t * 2097151) without f32 rounding.  The high-precision reference of the quantisation."""
    c = centres(vertices, indices).astype(np.float64)
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = hi - lo
    t = np.where(ext > 0, (c - lo) / np.where(ext > 0, ext, 1.0), 0.0)
    cells = np.floor(np.clip(t, 0.0, 1.0) * float(CELLS)).astype(np.int64)
    return c, cells


def split_ranges(codes_sorted):
    """Karras' tree over sorted codes.  Returns (left, right, axis, first, last) per internal node
    (n - 1 of them): children as ints (>= 0 an internal node, < 0 the leaf ~child), the axis of the
    split bit, and the node's range of sorted positions."""
    n = len(codes_sorted)
    aug = [(int(c) << 32) | i for i, c in enumerate(codes_sorted)]     # equal codes: separated by position
    left, right = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    axis = np.zeros(n - 1, np.uint32)
    first, last = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    todo = [(0, 0, n - 1)] if n > 1 else []
    while todo:
        node, a, b = todo.pop()
        bit = (aug[a] ^ aug[b]).bit_length() - 1           # the highest bit in which the range's ends differ
        bound = (aug[b] >> bit) << bit                     # the smallest key with the ends' prefix and that bit set
        g = bisect_left(aug, bound, a, b + 1) - 1          # the last position whose key has it clear
        first[node], last[node] = a, b
        # the bit is a code bit (position >= 32 of the key) unless the whole range has one code
        axis[node] = code_axis(bit - 32) if bit >= 32 else 0
        for side, (ca, cb, idx) in ((left, (a, g, g)), (right, (g + 1, b, g + 1))):
            if ca == cb:
                side[node] = ~ca
            else:
                side[node] = idx
                todo.append((idx, ca, cb))
    return left, right, axis, first, last


def _range_reduce(keys, a, b, ufunc):
    """ufunc-reduce keys[a[i] : b[i] + 1] along axis 0 for every i (a <= b)."""
    padded = np.concatenate([keys, keys[-1:]])             # b + 1 may be len(keys)
    at = np.stack([np.asarray(a), np.asarray(b) + 1], axis=1).reshape(-1)
    return ufunc.reduceat(padded, at, axis=0)[0::2]


def restate(vertices, indices):
    """(nodes, tris) of build_lbvh_gpu for this mesh, n >= 1 triangles."""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    indices = np.ascontiguousarray(indices, np.int64).reshape(-1, 3)
    n = indices.shape[0]
    assert n >= 1
    codes, _, _ = morton(vertices, indices)
    order = np.argsort(codes, kind="stable")
    v = vertices[indices[order]]
    tris = np.zeros(n, TRI_DTYPE)
    tris["v0"] = v[:, 0]
    tris["e1"] = (v[:, 1] - v[:, 0]).astype(np.float32)
    tris["e2"] = (v[:, 2] - v[:, 0]).astype(np.float32)
    tris["gid"] = order
    lo, hi = tri_boxes(vertices, indices[order])
    klo, khi = okey(lo), okey(hi)

    nodes = np.zeros(n, NODE_DTYPE)                        # the virtual root and n - 1 internal nodes

    def put(rec, side, blo, bhi):
        xy = "bxy0" if side == 0 else "bxy1"
        nodes[xy][rec, 0], nodes[xy][rec, 1] = blo[..., 0], bhi[..., 0]
        nodes[xy][rec, 2], nodes[xy][rec, 3] = blo[..., 1], bhi[..., 1]
        nodes["bz"][rec, 2 * side], nodes["bz"][rec, 2 * side + 1] = blo[..., 2], bhi[..., 2]

    inf = np.full(3, np.inf, np.float32)
    put(0, 0, okey_inv(klo.min(axis=0)), okey_inv(khi.max(axis=0)))
    put(0, 1, inf, -inf)
    nodes["child"][0] = (LEAF if n == 1 else 1, EMPTY)     # one triangle: the leaf itself (first 0, count 1)
    if n == 1:
        return nodes, tris
    left, right, axis, first, last = split_ranges(codes[order])
    rec = np.arange(1, n)
    ref = lambda c: np.where(c < 0, LEAF | (~c << 3), c + 1).astype(np.uint32)
    nodes["child"][rec, 0], nodes["child"][rec, 1] = ref(left), ref(right)
    nodes["axis"][rec] = axis
    mid = np.where(left < 0, ~left, left)                  # the last position of the left child's range
    put(rec, 0, okey_inv(_range_reduce(klo, first, mid, np.minimum)), okey_inv(_range_reduce(khi, first, mid, np.maximum)))
    put(rec, 1, okey_inv(_range_reduce(klo, mid + 1, last, np.minimum)), okey_inv(_range_reduce(khi, mid + 1, last, np.maximum)))
    return nodes, tris


def depth(nodes):
    """Levels below the virtual root, leaves counted (the real root is level 1): build_lbvh_gpu's max_depth."""
    best, todo = 0, [(int(nodes["child"][0][0]), 1)]
    while todo:
        r, d = todo.pop()
        if r == EMPTY:
            continue
        best = max(best, d)
        if not r & LEAF:
            todo += [(int(nodes["child"][r][0]), d + 1), (int(nodes["child"][r][1]), d + 1)]
    return best


def first_difference(got, want):
    """None when the two record arrays are equal byte for byte, else (record, field, got, want) of
    the first record that differs (fields compared as bit patterns, so -0.0 != +0.0 and NaN == NaN)."""
    if got.shape != want.shape:
        return ("shape", None, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return None
    w = got.dtype.itemsize // 4
    diff = np.nonzero((got.view(np.uint32).reshape(-1, w) != want.view(np.uint32).reshape(-1, w)).any(axis=1))[0]
    i = int(diff[0])
    for name in got.dtype.names:
        if got[name][i].tobytes() != want[name][i].tobytes():
            return (i, name, got[name][i].tolist(), want[name][i].tolist())
    raise AssertionError("records differ outside their fields")
