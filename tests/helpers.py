"""Shared test inputs: seeded ray batches and small scenes."""
import numpy as np

from akari_amd import capi, scene


def random_rays(n, seed, lo, hi, tmin=1e-3, tmax=np.inf):
    """Origins uniform in the box [lo, hi]^3, directions uniform on the sphere (normalised in f32)."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, capi.RAY_DTYPE)
    r["o"] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    r["d"] = d
    r["tmin"] = np.float32(tmin)
    r["tmax"] = np.float32(tmax)
    return r


def edge_rays(center=(0.0, 0.0, 0.0)):
    """Axis-aligned directions (zero components -> inf/NaN slabs), degenerate intervals, +-0."""
    c = np.asarray(center, np.float32)
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, -1, 0.0),
            (0.5, 0.5, 0.0), (0, 0.5, -0.5), (1e-30, 1, 0)]
    rays = []
    for d in dirs:
        d = np.asarray(d, np.float32)
        d = d / np.float32(np.sqrt(np.float32(np.dot(d, d))))
        for tmin, tmax in ((1e-3, np.inf), (0.0, np.inf), (1e-3, 1e-3), (5.0, 1.0), (1e-3, 0.5)):
            r = np.zeros(1, capi.RAY_DTYPE)
            r["o"], r["d"], r["tmin"], r["tmax"] = c, d, tmin, tmax
            rays.append(r)
    return np.concatenate(rays)


def cornell(resolution=(64, 64)):
    from conftest import CORNELL_MESH
    return scene.cornell_scene(CORNELL_MESH, resolution=resolution)


def small_soup(n_tris=20000, resolution=(96, 54), seed=42, r=0.01):
    return scene.soup_scene(n_tris=n_tris, resolution=resolution, seed=seed, r=r)


def scaled_soup(k, resolution=(24, 24)):
    """The 20,000-triangle soup of large triangles (r = 0.2) with every vertex multiplied by 2^k:
    an exact scaling, so the tree and every hit are the k = 0 scene's, scaled."""
    sc = small_soup(20_000, resolution, r=0.2)
    m = sc.shapes[0]
    m.vertices = (np.asarray(m.vertices, np.float32) * np.float32(2.0 ** k)).astype(np.float32)
    return sc


def scaled_rays(rays, k):
    """A batch for scaled_soup(k): origins and tmin times 2^k (exact), directions untouched."""
    r = rays.copy()
    r["o"] = (r["o"] * np.float32(2.0 ** k)).astype(np.float32)
    r["tmin"] = (r["tmin"] * np.float32(2.0 ** k)).astype(np.float32)
    return r


def far_origin_rays(k, log2_dist, n=1 << 12, seed=3):
    """Rays aimed at points of scaled_soup(k) (the origins of random_rays(n, seed, -1, 1), scaled)
    from the distance 2^log2_dist along their own directions, tmin 0."""
    r = random_rays(n, seed, -1.0, 1.0, tmin=0.0)
    target = r["o"].astype(np.float64) * 2.0 ** k
    r["o"] = (target - r["d"].astype(np.float64) * 2.0 ** log2_dist).astype(np.float32)
    return r


def near_axis_rays(e, n=1 << 12, seed=5):
    """random_rays(n, seed, -1.2, 1.2) with one direction component per ray, cycling through the
    axes, overwritten by +-2^e (the sign alternates every three rays)."""
    r = random_rays(n, seed, -1.2, 1.2)
    i = np.arange(n)
    d = r["d"].copy()
    d[i, i % 3] = np.where((i // 3) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(2.0 ** e)
    r["d"] = d
    return r


LEAN_REFUSALS = ("tmin", "zero_d", "far_o", "steep", "tmax")


def refuse_lean(rays, which, reason):
    """The rays `which` (a boolean mask) changed so that the lean traversal must refuse them
    (kernels.hip lean_ok), for one of its reasons: a negative tmin, a zero direction component, an
    origin component above 2^60, a 1 / d above 2^64, tmax = -inf."""
    r = rays.copy()
    idx = np.flatnonzero(which)
    if reason == "tmin":
        r["tmin"][idx] = np.float32(-1e-3)
    elif reason == "zero_d":
        d = r["d"].copy()
        d[idx, idx % 3] = np.where(idx % 2 == 0, 0.0, -0.0).astype(np.float32)
        r["d"] = d
    elif reason == "far_o":    # aimed at its old origin from 2^61 away
        r["o"][idx] = (r["o"][idx].astype(np.float64) - r["d"][idx].astype(np.float64) * 2.0 ** 61).astype(np.float32)
        r["tmin"][idx] = np.float32(0.0)
    elif reason == "steep":
        d = r["d"].copy()
        d[idx, idx % 3] = np.float32(2.0 ** -65)
        r["d"] = d
    elif reason == "tmax":
        r["tmax"][idx] = np.float32(-np.inf)
    else:
        raise ValueError(reason)
    return r


def refusal_mask(n, pattern):
    """Which rays of a batch of n the mixed-wave tests refuse: one lane of each wave of 64, every
    other lane, all lanes but one, or the second half of each wave."""
    lane = np.arange(n) % 64
    return {"1in64": lane == 37, "alternate": lane % 2 == 1, "63in64": lane != 37, "half": lane >= 32}[pattern]


def lean_expected(rays, gate=True):
    """kernels.hip lean_ok restated on a host batch: which rays the tight wide kernel takes through
    the lean loop (`gate`: the wide view passed the 2^40 test and option lean is on)."""
    f = np.float32
    o, d = rays["o"], rays["d"]
    with np.errstate(divide="ignore", over="ignore"):
        invd = (f(1.0) / d).astype(f)
    ok = np.isfinite(o).all(1) & np.isfinite(invd).all(1) & (invd != 0).all(1)
    ok &= ~np.isnan(rays["tmin"]) & ~np.isnan(rays["tmax"])
    ok &= (rays["tmin"] >= 0) & (rays["tmax"] > -np.inf)
    ok &= (np.abs(o).max(1) <= f(2.0 ** 60)) & (np.abs(invd).max(1) <= f(2.0 ** 64))
    return ok & bool(gate)


RAY_STEPS_EXACT = 0xFFFFFFFF    # option ray_steps: the ray went through the exact BVH2 walk


def interval_variants(rays, t_hit):
    """{name: batch}: `rays` (all of which hit at t_hit in the oracle's closest-hit trace) with the
    interval's ends put on the hit, one float to either side of it, and at the zeros and the smallest
    subnormal and normal numbers."""
    f = np.float32
    t = np.asarray(t_hit, f)
    out = {}
    for name, v in (("tmax=t", t), ("tmax=t+", np.nextafter(t, f(np.inf))), ("tmax=t-", np.nextafter(t, f(-np.inf))),
                    ("tmax=+0", f(0.0)), ("tmax=-0", f(-0.0)), ("tmax=2^-149", f(2.0 ** -149)), ("tmax=2^-126", f(2.0 ** -126))):
        r = rays.copy()
        r["tmax"] = v
        out[name] = r
    for name, v in (("tmin=t", t), ("tmin=t+", np.nextafter(t, f(np.inf))), ("tmin=t-", np.nextafter(t, f(-np.inf))),
                    ("tmin=-0", f(-0.0))):
        r = rays.copy()
        r["tmin"] = v
        out[name] = r
    return out


def nonfinite_rays(center=(0.0, 0.0, 0.0)):
    """A small batch outside every arithmetic assumption: an infinite or NaN origin component, a NaN
    tmax, a NaN tmin, an all-zero direction, a NaN and an infinite direction component, tmax -inf,
    tmin +inf (rays 0..11, none of which can hit); rays 12..15 are ordinary."""
    base = random_rays(16, 41, -0.5, 0.5)
    base["o"] += np.asarray(center, np.float32)
    o, d = base["o"].copy(), base["d"].copy()
    o[0, 0], o[1, 1], o[2, 2] = np.inf, -np.inf, np.nan
    base["tmax"][3] = np.nan
    base["tmin"][4] = np.nan
    d[5] = 0.0
    d[6] = (0.0, -0.0, 0.0)
    d[7, 0] = np.nan
    d[8, 1] = np.inf
    o[9], d[9] = np.inf, 0.0
    base["tmax"][10] = -np.inf
    base["tmin"][11] = np.inf
    base["o"], base["d"] = o, d
    return base


FAR_CAMERA_SCALE = 30
FAR_CAMERA_LOG2_Z = 61


def far_camera_soup(resolution=(24, 24)):
    """scaled_soup(30) seen from (0, 0, 2^61) through a field of view that just frames it: every
    camera ray starts beyond the lean traversal's 2^60 origin bound, every bounce and shadow ray
    inside it."""
    sc = scaled_soup(FAR_CAMERA_SCALE, resolution)
    fov = np.degrees(2.0 * np.arctan(1.6 * 2.0 ** FAR_CAMERA_SCALE / 2.0 ** FAR_CAMERA_LOG2_Z))
    sc.camera = scene.PerspectiveCamera(position=(0.0, 0.0, 2.0 ** FAR_CAMERA_LOG2_Z), rotation=(0.0, 0.0, 0.0),
                                        fov=float(fov), resolution=tuple(resolution))
    return sc


def tri_scene(tris, mats, mat_ids, cam):
    """One mesh of unshared-vertex triangles [n, 3, 3] with their geometric normals (up where a
    triangle has no area)."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = len(tris)
    t64 = tris.astype(np.float64)
    nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(length > 1e-20, nrm / np.maximum(length, 1e-20), np.array([0.0, 1.0, 0.0]))
    mesh = scene.Mesh(tris.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3),
                      np.repeat(nrm.astype(np.float32), 3, axis=0).reshape(n, 9),
                      np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1)), np.asarray(mat_ids, np.int32), mats)
    return scene.Scene(camera=cam, shapes=[mesh])


def _grey_and_light():
    ct = scene.ConstantTexture
    return [scene.DiffuseMaterial(ct([0.6, 0.55, 0.5])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]), double_sided=True)]


_CAM = dict(position=(0.0, 0.0, 4.0), rotation=(0.0, 0.0, 0.0), fov=40.0, resolution=(24, 24))


def soup_total(total, resolution=(24, 24), seed=42):
    """The seeded soup with `total` triangles in all, its two-triangle light quad included; below
    three triangles, the first `total` of the one-triangle soup and its quad."""
    sc = small_soup(max(total - 2, 1), resolution, seed)
    if total < 3:
        m = sc.shapes[0]
        m.vertices, m.indices = m.vertices[:3 * total], m.indices[:total]
        m.normals, m.texcoords, m.material_indices = m.normals[:total], m.texcoords[:total], m.material_indices[:total]
    assert sc.shapes[0].n_tris == total
    return sc


def shifted_soup(total=1000, offset=(-1000.0, 2000.0, 0.5)):
    """The `total`-triangle soup moved far from the origin: negative and large coordinates, centres
    whose low bits are lost, a scene bound that cancels in c - lo."""
    sc = soup_total(total)
    m = sc.shapes[0]
    m.vertices = (np.asarray(m.vertices, np.float32) + np.asarray(offset, np.float32)).astype(np.float32)
    return sc


def duplicates_soup():
    """The 500-triangle soup (and its quad) with triangles 100..199 made copies of triangle 0."""
    sc = small_soup(500)
    m = sc.shapes[0]
    m.vertices[3 * 100:3 * 200] = np.tile(m.vertices[0:3], (100, 1))
    return sc


def sheet_scene(quads=16):
    """quads x quads squares, two triangles each, in the plane z = 0: no extent along z."""
    tris = []
    for y in range(quads):
        for x in range(quads):
            a, b, c, d = (x, y, 0.0), (x + 1, y, 0.0), (x + 1, y + 1, 0.0), (x, y + 1, 0.0)
            tris += [[a, b, c], [a, c, d]]
    return tri_scene(np.array(tris, np.float32) / np.float32(quads), _grey_and_light(), [0] * len(tris),
                     scene.PerspectiveCamera(**_CAM))


def identical_scene(n=300):
    """n copies of one triangle: one Morton code, a tree built from sorted positions alone."""
    tri = [(0.25, -0.5, 0.125), (1.0, 0.75, -0.25), (-0.5, 0.5, 0.5)]
    return tri_scene(np.array([tri] * n, np.float32), _grey_and_light(), [0] * n, scene.PerspectiveCamera(**_CAM))


def signed_zero_pair():
    """Two triangles in planes x = -0.0 and x = +0.0 (every x coordinate carries its triangle's sign
    of zero, so the centres' x are -0.0 and +0.0) whose centres differ along y."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    tris = np.array([[(pz, 2.0, 0.0), (pz, 3.0, 0.0), (pz, 2.0, 1.0)],
                     [(nz, 0.0, 0.0), (nz, 1.0, 0.0), (nz, 0.0, 1.0)]], np.float32)
    assert np.signbit(tris[1, :, 0]).all() and not np.signbit(tris[0, :, 0]).any()
    return tri_scene(tris, _grey_and_light(), [0, 0], scene.PerspectiveCamera(**_CAM))


CHAIN_CELLS = 2097151   # 2^21 - 1, the builder's largest cell index


def chain_cells(n_tris=65):
    """The cells [n, 3] the chain scene's triangles are meant to fall in."""
    cells = np.zeros((n_tris, 3), np.int64)
    for j in range(63):
        cells[j, j % 3] = 1 << (20 - j // 3)
    cells[64] = CHAIN_CELLS
    return cells


def _chain_geometry(n_tris):
    """(centres, half-extents) of the chain scene's triangles in world units."""
    cells = chain_cells(65).astype(np.float64)
    centre = np.where((cells > 0) & (cells < CHAIN_CELLS), cells + 0.5, cells)
    half = np.maximum(0.25, cells.max(axis=1) / 4.0)
    half[64] = 2.0 ** 19
    if n_tris == 66:
        centre, half = np.concatenate([centre, centre[63:64]]), np.concatenate([half, half[63:64]])
    return centre * CHAIN_UNIT, half * CHAIN_UNIT


CHAIN_UNIT = 2.0 ** -20    # world units per cell: a power of two, so every quotient (c - lo) / ext is the cells' own
_CHAIN_CORNERS = np.array([(-1, -1, -1), (1, 1, -1), (-1, 1, 1)], np.float64)      # spans [-h, h] on every axis


def chain_scene(n_tris=65, resolution=(24, 24)):
    """The deepest tree the LBVH builder accepts.  In units of one cell (2^-20 world units, the scene
    spanning [0, 2) like the other test scenes): triangle j < 63 has its box centre at
    2^(20 - j // 3) + 0.5 on axis j % 3 and at 0 on the other two, so its Morton code is the single bit
    62 - j; triangle 63 is centred at the origin (code 0) and triangle 64, the light, at 2097151 on every
    axis (all 63 bits), which makes the scene bounds of the centres [0, 2097151]^3.  Sorted, the codes are
    0, 2^0, ..., 2^62, 2^63 - 1: below the root every split peels one triangle off the top of what is
    left, a chain.  With 65 triangles the tree has 64 levels (leaves counted); with 66, a copy of
    triangle 63 appended, the bottom leaf becomes a node: 65 levels.  Every triangle's half-extent is a
    power of two that keeps centre - h and centre + h exact in f32, so 0.5 * mn + 0.5 * mx is the centre
    exactly; the triangles grow with their distance from the origin so that the camera sees some."""
    assert n_tris in (65, 66)
    centre, half = _chain_geometry(n_tris)
    tris = centre[:, None, :] + half[:, None, None] * _CHAIN_CORNERS[None]
    assert np.array_equal(tris.astype(np.float32).astype(np.float64), tris)   # every coordinate exact in f32
    tris[64] = tris[64][[0, 2, 1]]             # the light's front (its next-event sampling is one-sided) towards the chain
    mat_ids = [0] * n_tris
    mat_ids[64] = 1
    cam = scene.PerspectiveCamera(position=(0.0, 0.0, 4.0), rotation=(0.0, 0.0, 0.0), fov=60.0,
                                  resolution=tuple(resolution))
    return tri_scene(tris, _grey_and_light(), mat_ids, cam)


def chain_rays(seed=3):
    """Rays for the chain scene: along its diagonal in both directions (through the origin triangle
    and the far one, inside every box of the chain), jittered copies of them, and rays aimed at the
    centroid of every triangle from points around the scene."""
    rng = np.random.default_rng(seed)
    centre, half = _chain_geometry(65)
    centroid = centre + half[:, None] * _CHAIN_CORNERS.mean(axis=0)
    diag = np.ones(3) / np.sqrt(3.0)
    o = [-0.1 * np.ones(3), 3.0 * np.ones(3)] + [-0.1 * np.ones(3) + 1e-6 * rng.normal(size=3) for _ in range(64)]
    d = [diag, -diag] + [diag + 1e-6 * rng.normal(size=3) for _ in range(64)]
    for t, h in zip(centroid, half):
        for _ in range(16):
            p = rng.uniform(-1.0, 3.0, 3)
            o.append(p)
            d.append(t + rng.normal(size=3) * 0.05 * h - p)
    d = np.array(d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros(len(o), capi.RAY_DTYPE)
    r["o"], r["d"] = np.array(o, np.float32), d.astype(np.float32)
    r["tmin"], r["tmax"] = np.float32(1e-3), np.float32(np.inf)
    return r


def chain_axis_rays():
    """Three rays from beside the chain scene's origin, each a hair off one axis (every 1 / d finite, so
    they stay in the wide traversal) with tmin 0: inside the origin triangle's box and, along their axis,
    through the box of each of its 21 triangles."""
    r = np.zeros(3, capi.RAY_DTYPE)
    for a in range(3):
        d = np.full(3, 2.0 ** -30)
        d[a] = 1.0
        r["d"][a] = (d / np.linalg.norm(d)).astype(np.float32)
    r["o"] = np.array([2.0 ** -23, 2.0 ** -24, 2.0 ** -25], np.float32)   # every half-extent is at least 2^-22
    r["tmin"], r["tmax"] = np.float32(0.0), np.float32(np.inf)
    return r


# The inputs on which the LBVH builder's tree is pinned (test_lbvh_host.py, test_gpu_lbvh.py), the
# smallest that reach each mechanism; triangle counts include the soups' light quad
LBVH_INPUTS = {
    **{f"soup{n}": (lambda n=n: soup_total(n)) for n in (1, 2, 3, 255, 256, 257, 20000)},   # 256: the kernels' block
    "cornell": lambda: cornell((24, 24)),          # several meshes: gid is a global id
    "sheet": sheet_scene,                          # ext == 0 on z: the quantiser's other branch
    "identical": identical_scene,                  # one code: index splits, axis 0 throughout
    "duplicates": duplicates_soup,                 # a run of equal codes inside distinct ones
    "shifted": shifted_soup,                       # negative, large, cancelling coordinates
    "signed_zeros": signed_zero_pair,              # bounds -0.0 and +0.0 on one axis
    "chain65": lambda: chain_scene(65),            # depth 64, the deepest accepted
}


def subtree_leaves(nodes):
    """For a BVH2 export of one-triangle leaves: (internal records, parents first; sets) where
    sets[r] = [leaf positions below child 0 of record r, those below child 1], gathered by brute
    force over the child links."""
    sets = {}
    order, todo = [], [int(nodes["child"][0][0])]
    while todo:
        r = todo.pop()
        if r & 0x80000000:
            continue
        order.append(r)
        todo += [int(nodes["child"][r][0]), int(nodes["child"][r][1])]
    leaf = lambda ref: np.array([(ref & 0x7FFFFFFF) >> 3], np.int64)
    for r in reversed(order):                      # children before parents
        kids = [int(nodes["child"][r][k]) for k in (0, 1)]
        sets[r] = [leaf(c) if c & 0x80000000 else np.concatenate(sets[c]) for c in kids]
    return order, sets


def check_split_planes(nodes, tris, cells):
    """The split planes of a Morton-code BVH2 export against cells [n_tris, 3] quantised in high
    precision (lbvh_restate.code_cells_f64), which may differ from the builder's f32 cells by one.
    Along its `axis` a node's leaves fill part of an aligned block of 2^(k+1) cells, the left subtree
    in its lower half and the right subtree in its upper half; the plane between the halves is at cell
    P = (hi >> k) << k, k the highest bit in which the block's lowest and highest occupied cells lo, hi
    differ.  The high-precision lo and hi are each within one cell of the builder's, so the builder's
    plane is among the at most nine planes of (lo + {-1, 0, 1}, hi + {-1, 0, 1}); against one of them
    every left centre must lie below the plane plus one cell (cell <= P) and every right centre above
    it minus one cell (cell >= P - 1).  Returns the records of the nodes for which none does."""
    order, sets = subtree_leaves(nodes)
    gid = tris["gid"].astype(np.int64)
    cells = np.asarray(cells, np.int64)
    bad = []
    for r in order:
        a = int(nodes["axis"][r])
        if a > 2:
            bad.append(r)
            continue
        left, right = cells[gid[sets[r][0]], a], cells[gid[sets[r][1]], a]
        lmax, rmin = int(left.max()), int(right.min())
        lo, hi = min(int(left.min()), rmin), max(lmax, int(right.max()))
        ok = False
        for l in (lo - 1, lo, lo + 1):
            for h in (hi - 1, hi, hi + 1):
                if 0 <= l < h <= CHAIN_CELLS:
                    k = (l ^ h).bit_length() - 1
                    p = (h >> k) << k
                    ok = ok or (lmax <= p and rmin >= p - 1)
        if not ok:
            bad.append(r)
    return bad


def check_sbvh(cs, nodes, tris, max_leaf, budget=0.5, samples=6):
    """Invariants of an SBVH export (references may be clipped and duplicated): every triangle in
    at least one leaf and at most budget * n extra records, records equal to the mesh, child boxes
    inside their parents, and every triangle covered by the union of its leaf boxes (a barycentric
    grid of points, in f64, each inside at least one of the triangle's leaf boxes)."""
    n = cs.n_tris
    g = tris["gid"].astype(np.int64)
    assert set(g.tolist()) == set(range(n)) and len(g) <= n + int(budget * n) + 1
    v = cs.vertices[cs.indices]
    assert np.array_equal(tris["v0"], v[g, 0])
    assert np.array_equal(tris["e1"], (v[g, 1] - v[g, 0]).astype(np.float32))
    assert np.array_equal(tris["e2"], (v[g, 2] - v[g, 0]).astype(np.float32))
    leaf_lo = np.zeros((len(g), 3), np.float64)
    leaf_hi = np.zeros((len(g), 3), np.float64)
    root_lo = np.array([nodes[0]["bxy0"][0], nodes[0]["bxy0"][2], nodes[0]["bz"][0]], np.float32)
    root_hi = np.array([nodes[0]["bxy0"][1], nodes[0]["bxy0"][3], nodes[0]["bz"][1]], np.float32)
    stack = [(int(nodes[0]["child"][0]), root_lo, root_hi, root_lo, root_hi, 1)]
    while stack:
        ref, lo, hi, plo, phi, depth = stack.pop()
        assert depth <= 64 and np.all(lo >= plo) and np.all(hi <= phi)
        if ref & 0x80000000:
            first, cnt = (ref & 0x7FFFFFFF) >> 3, (ref & 7) + 1
            assert cnt <= max_leaf
            leaf_lo[first:first + cnt] = lo
            leaf_hi[first:first + cnt] = hi
        else:
            nd = nodes[ref]
            for k, (bxy, bz) in enumerate(((nd["bxy0"], nd["bz"][:2]), (nd["bxy1"], nd["bz"][2:]))):
                clo = np.array([bxy[0], bxy[2], bz[0]], np.float32)
                chi = np.array([bxy[1], bxy[3], bz[1]], np.float32)
                stack.append((int(nd["child"][k]), clo, chi, lo, hi, depth + 1))
    vd = v.astype(np.float64)
    bary = [(a / samples, b / samples) for a in range(samples + 1) for b in range(samples + 1 - a)]
    order = np.argsort(g, kind="stable")
    starts = np.searchsorted(g[order], np.arange(n + 1))
    for tri in range(n):
        idx = order[starts[tri]:starts[tri + 1]]
        lo, hi = leaf_lo[idx], leaf_hi[idx]
        for a, b in bary:
            p = (1 - a - b) * vd[tri, 0] + a * vd[tri, 1] + b * vd[tri, 2]
            eps = 1e-12 * (1.0 + np.abs(p))   # f64 rounding of the combination, far below an f32 ulp
            assert np.any(np.all((p >= lo - eps) & (p <= hi + eps), axis=1)), f"triangle {tri} point {a, b} not covered"
    return len(g) - n


def mixed_scene(resolution=(48, 48)):
    """Cornell geometry with Glossy / Mix materials and a two-sided emitter (BSDF coverage)."""
    sc = cornell(resolution)
    m = sc.shapes[0]
    ct = scene.ConstantTexture
    glossy = scene.GlossyMaterial(ct([0.9, 0.8, 0.7]), ct([0.4, 0.4, 0.4]))
    mix = scene.MixMaterial(ct([0.3, 0.3, 0.3]), scene.DiffuseMaterial(ct([0.2, 0.7, 0.2])), glossy)
    m.materials[5] = glossy       # short box
    m.materials[6] = mix          # tall box
    m.materials[7] = scene.EmissiveMaterial(ct([17.0, 12.0, 4.0]), double_sided=True)
    return sc


def textured_scene(resolution=(48, 48)):
    """Cornell geometry with image textures on diffuse, glossy roughness, mix fraction and emitter
    colour (a15); texcoords stretched to [-1, 2] so the fmod wrap and the clamp are exercised."""
    sc = mixed_scene(resolution)
    m = sc.shapes[0]
    rng = np.random.default_rng(11)
    img = lambda h, w: scene.ImageTexture(rng.random((h, w, 4), dtype=np.float32))
    m.texcoords = (np.asarray(m.texcoords, np.float32) * np.float32(3.0) - np.float32(1.0)).astype(np.float32)
    ct = scene.ConstantTexture
    m.materials[0] = scene.DiffuseMaterial(img(23, 37))                       # floor
    m.materials[2] = scene.GlossyMaterial(img(5, 7), img(9, 4))               # back wall: roughness image
    m.materials[6] = scene.MixMaterial(img(16, 16), scene.DiffuseMaterial(img(3, 3)),
                                       scene.GlossyMaterial(ct([0.8, 0.8, 0.8]), ct([0.3, 0.3, 0.3])))
    m.materials[7] = scene.EmissiveMaterial(scene.ImageTexture(rng.random((4, 6, 4), dtype=np.float32) * 20),
                                            double_sided=False)
    return sc


def branches_scene(resolution=(24, 24)):
    """Twelve triangles that reach the path loop's rare branches (tests/golden/make_path_golden.py
    counts them): a glossy floor of roughness 0.05 seen at grazing angles, half of it with its
    shading normals turned down; a Mix(0.5, Diffuse, Emissive) back wall; a nested Mix side wall; a
    one-sided ceiling light; a triangle without a material; a one-sided emitter seen from its back;
    a double-sided emitter; and, last in the light list, a zero-area emissive triangle.  No right
    wall: rays leave the scene there."""
    ct = scene.ConstantTexture
    diffuse = scene.DiffuseMaterial(ct([0.6, 0.5, 0.4]))
    glossy = scene.GlossyMaterial(ct([0.9, 0.85, 0.8]), ct([0.05, 0.05, 0.05]))
    mats = [glossy,
            scene.MixMaterial(ct([0.5, 0.5, 0.5]), diffuse, scene.EmissiveMaterial(ct([5.0, 5.0, 5.0]))),
            scene.MixMaterial(ct([0.3, 0.3, 0.3]),
                              scene.MixMaterial(ct([0.5, 0.5, 0.5]), diffuse,
                                                scene.GlossyMaterial(ct([0.7, 0.7, 0.9]), ct([0.5, 0.5, 0.5]))),
                              scene.DiffuseMaterial(ct([0.2, 0.6, 0.3]))),
            scene.EmissiveMaterial(ct([20.0, 18.0, 15.0])),
            scene.EmissiveMaterial(ct([4.0, 1.0, 1.0])),
            scene.EmissiveMaterial(ct([1.0, 4.0, 1.0]), double_sided=True),
            scene.EmissiveMaterial(ct([3.0, 3.0, 3.0]))]
    quad_tc = [[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]]
    tri_tc = [0, 0, 1, 0, 0, 1]
    tris = [  # (three vertices, shading normal, texcoords, material slot)
        ([(-2, 0, 4), (2, 0, 4), (2, 0, -2)], (0, 1, 0), quad_tc[0], 0),            # floor
        ([(-2, 0, 4), (2, 0, -2), (-2, 0, -2)], (0, -1, 0), quad_tc[1], 0),         # floor, normals down
        ([(-2, 0, -2), (2, 0, -2), (2, 3, -2)], (0, 0, 1), quad_tc[0], 1),          # back wall
        ([(-2, 0, -2), (2, 3, -2), (-2, 3, -2)], (0, 0, 1), quad_tc[1], 1),
        ([(-2, 0, 4), (-2, 0, -2), (-2, 3, -2)], (1, 0, 0), quad_tc[0], 2),         # left wall
        ([(-2, 0, 4), (-2, 3, -2), (-2, 3, 4)], (1, 0, 0), quad_tc[1], 2),
        ([(-1, 3, -1), (1, 3, -1), (1, 3, 1)], (0, -1, 0), quad_tc[0], 3),          # ceiling light, faces down
        ([(-1, 3, -1), (1, 3, 1), (-1, 3, 1)], (0, -1, 0), quad_tc[1], 3),
        ([(0.5, 0.5, 0), (1.5, 0.5, 0), (1.0, 1.5, 0)], (0, 0, 1), tri_tc, -1),     # no material
        ([(-1.5, 0.5, 0.5), (-1.0, 1.5, 0.5), (-0.5, 0.5, 0.5)], (0, 0, -1), tri_tc, 4),   # faces away
        ([(-0.25, 1.75, -0.5), (0.25, 1.75, -0.5), (0, 2.25, -0.5)], (0, 0, 1), tri_tc, 5),  # double sided
        ([(1.0, 2.0, -1), (1.25, 2.25, -1), (1.5, 2.5, -1)], (0, 0, 1), tri_tc, 6),          # zero area
    ]
    verts = np.array([p for t in tris for p in t[0]], np.float32)
    mesh = scene.Mesh(verts, np.arange(len(verts), dtype=np.int32).reshape(-1, 3),
                      np.array([list(t[1]) * 3 for t in tris], np.float32),
                      np.array([t[2] for t in tris], np.float32),
                      np.array([t[3] for t in tris], np.int32), mats)
    cam = scene.PerspectiveCamera(position=(0.3, 0.4, 3.9), rotation=(0.0, 0.0, 0.0), fov=70.0,
                                  resolution=tuple(resolution))
    return scene.Scene(camera=cam, shapes=[mesh])


def kat_scene():
    """The inputs of the function-level vectors (tests/golden/path_kat.json): one mesh whose
    material slots hold image textures of odd sizes, Mix materials of fraction 0, 1 and 0.5, a
    nested Mix, and emissive triangles seen face-on, edge-on and with zero area.  Every leaf
    material has its own colour, which is how a vector names the material a Mix resolved to."""
    ct = scene.ConstantTexture
    rng = np.random.default_rng(5)
    img = lambda h, w: scene.ImageTexture(rng.random((h, w, 4), dtype=np.float32))
    d = lambda c: scene.DiffuseMaterial(ct([c, c, c]))
    g = lambda c: scene.GlossyMaterial(ct([c, c, c]), ct([0.3, 0.3, 0.3]))
    mats = [scene.DiffuseMaterial(img(5, 7)),                                   # 0
            scene.DiffuseMaterial(img(3, 3)),                                   # 1
            scene.DiffuseMaterial(img(1, 11)),                                  # 2
            scene.MixMaterial(ct([0.0, 0.0, 0.0]), d(0.11), g(0.12)),           # 3
            scene.MixMaterial(ct([1.0, 1.0, 1.0]), d(0.13), g(0.14)),           # 4
            scene.MixMaterial(ct([0.5, 0.5, 0.5]), d(0.15), g(0.16)),           # 5
            scene.MixMaterial(ct([0.25, 0.9, 0.9]),                             # 6: nested on both sides
                              scene.MixMaterial(ct([0.5, 0.5, 0.5]), d(0.17), g(0.18)),
                              scene.MixMaterial(img(4, 6), d(0.19), scene.EmissiveMaterial(ct([0.2, 0.2, 0.2])))),
            scene.EmissiveMaterial(img(2, 3)),                                  # 7
            scene.EmissiveMaterial(ct([3.0, 2.0, 1.0]), double_sided=True)]     # 8
    tris = [
        ([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 0),
        ([(0.3, -1.2, 2.0), (1.7, 0.4, 2.5), (-0.9, 0.8, 3.1)], [(0.1, 0.2, 0.9), (-0.3, 0.1, 0.8), (0, 0, 1)],
         [-0.5, 0.25, 1.75, 1.0, 0.5, -1.25], 1),
        ([(-1, 2, -1), (1, 2, -1), (1, 2, 1)], [(0, -1, 0)] * 3, [0, 0, 1, 0, 1, 1], 7),      # light, faces down
        ([(-1, 2, -1), (1, 2, 1), (-1, 2, 1)], [(0, -1, 0)] * 3, [0, 0, 1, 1, 0, 1], 8),
        ([(2, 0, 0), (2.5, 0.5, 0), (3, 1, 0)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 8),      # zero area
        ([(4, 0, 0), (5, 0, 0), (4, 1, 0)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 2),
        ([(4, 0, 1), (5, 0, 1), (4, 1, 1)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 3),
        ([(4, 0, 2), (5, 0, 2), (4, 1, 2)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 4),
        ([(4, 0, 3), (5, 0, 3), (4, 1, 3)], [(0, 0, 1)] * 3, [0, 0, 1, 0, 0, 1], 5),
        ([(4, 0, 4), (5, 0, 4), (4, 1, 4)], [(0, 0, 1)] * 3, [0.2, 0.1, 0.9, 0.3, 0.4, 0.8], 6),
    ]
    verts = np.array([p for t in tris for p in t[0]], np.float32)
    mesh = scene.Mesh(verts, np.arange(len(verts), dtype=np.int32).reshape(-1, 3),
                      np.array([[c for nrm in t[1] for c in nrm] for t in tris], np.float32),
                      np.array([t[2] for t in tris], np.float32),
                      np.array([t[3] for t in tris], np.int32), mats)
    cam = scene.PerspectiveCamera(position=(0.5, 0.5, 8.0), rotation=(0.0, 0.0, 0.0), fov=40.0, resolution=(16, 16))
    return scene.Scene(camera=cam, shapes=[mesh])


def dark_scene(resolution=(8, 8)):
    """The Cornell box with its light turned into a wall: no area light, so select_light's and
    compute_direct_lighting's no-light branches run."""
    sc = cornell(resolution)
    sc.shapes[0].materials[7] = scene.DiffuseMaterial(scene.ConstantTexture([0.5, 0.5, 0.5]))
    return sc


def hits_to_gid(hits, mesh_base):
    gid = np.full(hits.shape[0], 0xFFFFFFFF, np.uint32)
    ok = hits["geom_id"] >= 0
    gid[ok] = mesh_base[hits["geom_id"][ok]] + hits["prim_id"][ok].astype(np.uint32)
    return gid


def check_bvh(cs, nodes, tris, max_leaf):
    """Invariants of an exported BVH2: every triangle in exactly one leaf, leaf records equal to
    the mesh (e1, e2 as f32 subtractions), child boxes containing their subtrees, depth <= 64."""
    n = cs.n_tris
    assert sorted(tris["gid"].tolist()) == list(range(n)), "every triangle in exactly one leaf"
    v = cs.vertices[cs.indices]
    g = tris["gid"]
    assert np.array_equal(tris["v0"], v[g, 0])
    assert np.array_equal(tris["e1"], (v[g, 1] - v[g, 0]).astype(np.float32))
    assert np.array_equal(tris["e2"], (v[g, 2] - v[g, 0]).astype(np.float32))
    # walk: child boxes contain their subtree's triangles, depth bounded, leaf sizes bounded
    stack = [(int(nodes[0]["child"][0]), nodes[0]["bxy0"], nodes[0]["bz"][:2], 1)]
    seen = 0
    while stack:
        ref, bxy, bz, depth = stack.pop()
        assert depth <= 64
        lo = np.array([bxy[0], bxy[2], bz[0]], np.float32)
        hi = np.array([bxy[1], bxy[3], bz[1]], np.float32)
        if ref & 0x80000000:
            first, cnt = (ref & 0x7FFFFFFF) >> 3, (ref & 7) + 1
            assert cnt <= max_leaf
            pts = v[tris["gid"][first:first + cnt]].reshape(-1, 3)
            assert np.all(pts >= lo) and np.all(pts <= hi)
            seen += cnt
        else:
            nd = nodes[ref]
            assert nd["axis"] < 3
            stack.append((int(nd["child"][0]), nd["bxy0"], nd["bz"][:2], depth + 1))
            stack.append((int(nd["child"][1]), nd["bxy1"], nd["bz"][2:], depth + 1))
    assert seen == n


# ref.png blocks where the reference's image was made by a different estimator: the
# ceiling strip in the 1-cm gap above the one-sided light (y 1.98 vs ceiling 1.99), block row 2.
REFPNG_LIGHT_GAP = [(2, c) for c in range(11, 21)]


def refpng_ztest(rad, w, golden):
    """Per-block z statistic of the grey level (channel mean of the sRGB8 image, 16x16 blocks)
    against the reference's ref.png, z = (ours - ref) / sqrt((var_ours + var_ref) / 256), each
    variance the image's own within-block pixel variance (per-block z-test; spatial
    variation inside a block only inflates sigma).  Returns z [32, 32]."""
    from akari_amd import film
    grey = film.to_srgb8(rad, w).astype(np.float64).mean(axis=2).reshape(32, 16, 32, 16)
    mo, vo = grey.mean(axis=(1, 3)), grey.var(axis=(1, 3), ddof=1)
    mr, vr = np.asarray(golden["grey_mean"]), np.asarray(golden["grey_var"])
    return (mo - mr) / np.sqrt((vo + vr) / 256.0 + 1e-12)


def refpng_verdict(z):
    """(fraction of blocks outside the light gap with |z| <= 3, failing blocks outside the gap,
    gap blocks where ref.png is brighter by more than 3 sigma)."""
    gap = np.zeros(z.shape, bool)
    for r, c in REFPNG_LIGHT_GAP:
        gap[r, c] = True
    ok = np.abs(z) <= 3
    outside = ~gap
    fails = [(int(r), int(c), round(float(z[r, c]), 1)) for r, c in np.argwhere(outside & ~ok)]
    gap_darker = int(np.count_nonzero(gap & (z < -3)))
    return ok[outside].mean(), fails, gap_darker


def slot_pixels(tiles, width, height):
    """(ys, xs) of every film slot in packed tile order (tiles clipped to the frame, row-major
    inside a tile): the order of akr_hip_render_device's output and of akr_hip_pixel_probe."""
    ys, xs = [], []
    for x0, y0, x1, y1 in tiles:
        x0, y0, x1, y1 = max(0, x0), max(0, y0), min(width, x1), min(height, y1)
        if x1 <= x0 or y1 <= y0:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        ys.append(yy.reshape(-1))
        xs.append(xx.reshape(-1))
    if not ys:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ys), np.concatenate(xs)


def check_probe(gpu, orc_frame, tiles, width, height, what=""):
    """Compare a device pixel probe (slot order) with the oracle's frame-indexed probe: the final
    sampler state always, the ray counts when the device recorded them.  Returns whether it
    compared ray counts."""
    ys, xs = slot_pixels(tiles, width, height)
    exp = orc_frame[ys, xs]
    assert len(gpu) == len(exp)
    assert np.all(gpu["flags"] & capi.PROBE_SEED), f"{what}: seeds not recorded"
    bad = np.count_nonzero(gpu["seed"] != exp["seed"])
    assert bad == 0, f"{what}: {bad} of {len(exp)} final sampler states differ from the oracle"
    rays = bool(np.all(gpu["flags"] & capi.PROBE_RAYS))
    if rays:
        for k in ("closest_rays", "shadow_rays"):
            bad = np.count_nonzero(gpu[k] != exp[k])
            assert bad == 0, f"{what}: {bad} of {len(exp)} per-pixel {k} differ from the oracle"
    return rays
