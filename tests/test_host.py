"""CPU-only checks of the host side: C-ABI library surface, BVH builder invariants, traversal
builder-independence, scene language, soup generator (no GPU needed)."""
import ctypes as C
import re

import numpy as np
import pytest

import py_oracle as O
from akari_amd import capi, scene
from conftest import CORNELL_MESH, ROOT
from helpers import check_bvh as _check_bvh, check_sbvh, cornell, random_rays, small_soup


def test_library_exports_every_declared_symbol():
    hdr = (ROOT / "include" / "akr_hip.h").read_text()
    declared = set(re.findall(r"\b(akr_(?:hip|bvh)_\w+)\s*\(", hdr))
    assert len(declared) >= 25
    lib = C.CDLL(str(capi.LIB_PATH))
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    assert set(capi.EXPORTS) == declared, "ctypes binding out of sync with include/akr_hip.h"
    assert capi.load_library().akr_hip_api_version() == 3


def test_product_build_compiles_no_probe_or_ab_variant():
    """The product library is built from the Makefile's flags alone (no -D), and its sources hold no
    timing probe or A/B build switch: an inexact probe (not bit-exact by design) can never be
    compiled into libakr_hip.so.  Experiments live as patches under tools/experiments/ and build
    into tools/experiments/lib/, the only place capi.load_library's override accepts."""
    csrc = ROOT / "akarirender-1_amd" / "csrc"
    mk = (csrc / "Makefile").read_text()
    flags = [ln for ln in mk.splitlines() if ln.startswith(("FLAGS", "HIPCC", "\t$(HIPCC)", "\tg++"))]
    assert flags and not any(re.search(r"(^|\s)-D", ln) for ln in flags), flags
    assert "variant" not in mk
    banned = re.compile(r"AKR_PROBE_(?!SEED|RAYS)|AKR_STACK16|AKR_PK_FMA|AKR_POP2|AKR_SPEC_PRIO|AKR_NEXT_SELECT|AKR_PATH_CALL_SHADE|"
                        r"AKR_ROOT_SGPR|AKR_STREAM_DEBUG|AKR_ONE_POP")
    for f in sorted(csrc.glob("*")):
        if f.suffix in (".hip", ".h", ".cpp", ".hpp"):
            hits = [i + 1 for i, ln in enumerate(f.read_text().splitlines()) if banned.search(ln)]
            assert not hits, f"{f.name}: probe / A-B switch at lines {hits}"
    # the only preprocessor conditionals left are the header guard of device code and tuning defaults
    allowed = re.compile(r"#\s*(ifndef AKR_(TRACE_BLOCK|STACK_LDS|REFILL_MIN|REFILL_MIN_ANY|WHILE_EXIT|WHILE_EXIT_ANY|WHILE_EXIT_PATH|WHILE_EXIT_SPEC|"
                         r"WORK_SHARDS|TRACE_WAVES|PATH_WAVES|SHADE_BLOCK)\b|if defined\(__HIP_DEVICE_COMPILE__\)|"
                         r"if defined\(__HIPCC__\)|ifdef __HIPCC__)")
    for f in sorted(csrc.glob("*")):
        if f.suffix in (".hip", ".h", ".cpp", ".hpp"):
            for i, ln in enumerate(f.read_text().splitlines()):
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", ln):
                    assert allowed.match(ln.strip()), f"{f.name}:{i + 1}: {ln.strip()}"
    with pytest.raises(ImportError, match="tools/experiments"):
        import subprocess, sys
        r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'akarirender-1_amd'); "
                            "from akari_amd import capi"], cwd=ROOT, capture_output=True, text=True,
                           env={**__import__("os").environ, "AKR_HIP_LIB": "/tmp/other.so"})
        raise ImportError(r.stderr)


def test_tile_arrays_pass_without_copy():
    """render calls take the tile list as an (n, 4) int32 array from capi.rect_array without a
    copy (the bench converts once, outside its timed region), or as a list of tuples."""
    tiles = [(0, 0, 32, 32), (32, 0, 40, 17), (-5, 3, 7, 9)]
    arr = capi.rect_array(tiles)
    assert arr.dtype == np.int32 and arr.shape == (3, 4) and arr.flags.c_contiguous
    got, n = capi.HipContext._rects(arr)
    assert got is arr and n == 3
    lst, n2 = capi.HipContext._rects(tiles)
    assert n2 == 3 and [(r.x0, r.y0, r.x1, r.y1) for r in lst] == tiles
    assert capi._arr_ptr(arr).value == arr.ctypes.data
    for bad in (arr.astype(np.int64), arr[:, :3].copy(), np.asfortranarray(np.tile(arr, (1, 2))[:, ::2])):
        with pytest.raises(ValueError):
            capi.HipContext._rects(bad)


def test_create_without_device_fails_cleanly():
    if capi.device_count() > 0:
        pytest.skip("a device is visible")
    h = C.c_void_p()
    assert capi.load_library().akr_hip_create(0, C.byref(h)) != 0 and not h.value
    assert capi.load_library().akr_hip_last_error(None) == b"null context"


@pytest.mark.parametrize("leaf", [1, 4, 8])
def test_bvh_builder_invariants(leaf):
    cs = scene.compile_scene(small_soup(20_000))
    nodes, tris, info = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=leaf)
    assert info.max_leaf <= leaf and info.n_tris == cs.n_tris and info.max_depth <= 64
    _check_bvh(cs, nodes, tris, leaf)


@pytest.mark.parametrize("builder", [capi.BUILDER_SAH, capi.BUILDER_SBVH])
def test_bvh_degenerate_inputs(builder):
    # identical triangles (all centroids equal) force the median split; zero-area triangles stay in
    v = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (300, 1))
    v[-3:] = [[0.5, 0.5, 0.5]] * 3
    idx = np.arange(900, dtype=np.int32).reshape(-1, 3)
    nodes, tris, info = capi.build_bvh_host(v, idx, max_leaf_size=4, builder=builder)
    assert set(tris["gid"].tolist()) == set(range(300))
    if builder == capi.BUILDER_SAH:
        assert sorted(tris["gid"].tolist()) == list(range(300))
    assert info.max_depth <= 64
    # a single triangle, axis-aligned (flat) triangles, a point, huge coordinates
    for tri in ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 0, 0], [0, 0, 0]],
                [[-1e30, 0, 0], [1e30, 0, 0], [0, 1e30, 0]]):
        n1, t1, _ = capi.build_bvh_host(np.array(tri, np.float32), np.array([[0, 1, 2]], np.int32), builder=builder)
        assert t1["gid"].tolist() == [0]
    flat = np.random.default_rng(3).uniform(-1, 1, (3000, 3)).astype(np.float32)
    flat[:, 2] = 0.0
    nf, tf, inf_ = capi.build_bvh_host(flat, np.arange(3000, dtype=np.int32).reshape(-1, 3), builder=builder)
    assert set(tf["gid"].tolist()) == set(range(1000)) and inf_.max_depth <= 64
    n0, t0, _ = capi.build_bvh_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), builder=builder)
    assert n0.shape[0] == 1 and t0.shape[0] == 0 and n0[0]["child"][0] == 0xFFFFFFFF
    with pytest.raises(capi.AkrError):
        capi.build_bvh_host(v, np.array([[0, 1, 5000]], np.int32), builder=builder)


def _bvh2_leaf_order(nodes, signs):
    """Leaves of the BVH2 in the reference's depth-first order for a ray direction with these
    component signs (near child = left iff d[axis] > 0, bvh-accelerator.h:508-514)."""
    out, stack = [], [int(nodes[0]["child"][0])]
    while stack:
        r = stack.pop()
        if r == 0xFFFFFFFF:
            continue
        if r & 0x80000000:
            out.append(((r & 0x7FFFFFFF) >> 3, (r & 7) + 1))
            continue
        nd = nodes[r]
        c0, c1 = int(nd["child"][0]), int(nd["child"][1])
        near, far = (c0, c1) if signs[nd["axis"]] else (c1, c0)
        stack += [far, near]
    return out


def _wide_walk(wide, signs):
    """Depth-first walk of the wide view with the kernel's slot order; yields (leaf, path boxes)."""
    wn, lv, root = wide
    out = []

    def slot_boxes(nd):
        ex = [(int(nd["meta"]) >> (8 * k)) & 0xFF for k in range(3)]
        s = [np.float32(2.0 ** (e - 127)) for e in ex]
        boxes = []
        for k in range(4):
            q = [(int(nd["q"][j]) >> (8 * k)) & 0xFF for j in range(6)]
            lo = [np.float32(np.float32(q[2 * a]) * s[a] + nd["origin"][a]) for a in range(3)]
            hi = [np.float32(np.float32(q[2 * a + 1]) * s[a] + nd["origin"][a]) for a in range(3)]
            boxes.append((np.array(lo, np.float32), np.array(hi, np.float32)))
        return boxes

    def visit(ref, path):
        if ref == 0xFFFFFFFF:
            return
        if ref & 0x80000000:
            out.append((ref & 0x7FFFFFFF, path))
            return
        nd = wn[ref]
        octant = sum(1 << a for a in range(3) if signs[a])
        perm = (int(nd["order"][octant >> 2]) >> (8 * (octant & 3))) & 0xFF
        pos = [(perm >> (2 * k)) & 3 for k in range(4)]
        assert sorted(pos) == [0, 1, 2, 3]
        boxes = slot_boxes(nd)
        for k in sorted(range(4), key=lambda k: pos[k]):
            visit(int(nd["child"][k]), path + [boxes[k]])

    visit(root, [])
    return out


@pytest.mark.parametrize("collapse", [capi.COLLAPSE_SAH, capi.COLLAPSE_BALANCED])
@pytest.mark.parametrize("builder", ["sah", "sbvh"])
@pytest.mark.parametrize("leaf", [1, 4])
def test_wide_view_invariants(leaf, builder, collapse):
    """The 4-wide traversal view (both treelet choices): every leaf's exact box lies inside every
    quantized slot box on its path (the wide test can only pass more often), leaf records cover the
    triangles once, every node's order bytes are permutations, and for every direction octant the
    leaves come in the BVH2 depth-first order."""
    cs = scene.compile_scene(small_soup(5_000, r=0.01 if builder == "sah" else 0.2))
    nodes, tris, info, wide = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=leaf, wide=True,
                                                  builder=capi.BUILDER_SBVH if builder == "sbvh" else 0,
                                                  wide_collapse=collapse)
    wn, lv, root = wide
    assert sorted((int(l["first"]), int(l["count"])) for l in lv) == sorted(_bvh2_leaf_order(nodes, (1, 1, 1)))
    for octant in range(8):
        signs = tuple(bool(octant >> a & 1) for a in range(3))
        walk = _wide_walk(wide, signs)
        assert [(int(lv[i]["first"]), int(lv[i]["count"])) for i, _ in walk] == _bvh2_leaf_order(nodes, signs)
        if octant == 0:
            for i, path in walk:
                for lo, hi in path:
                    assert np.all(lo <= lv[i]["lo"]) and np.all(hi >= lv[i]["hi"])


def test_bvh_validate_accepts_built_trees_and_rejects_malformed_ones():
    """akr_bvh_validate, the check akr_hip_import_accel runs before it adopts a foreign BVH2: every
    tree the builders make passes with its depth; a reference out of range, a node reached twice
    (a cycle or a DAG), a leaf beyond the triangles, a triangle id beyond the scene, a bad split axis,
    a NaN box, a node 0 that is not the virtual root or an over-deep chain are rejected."""
    cs = scene.compile_scene(small_soup(3_000))
    for b in (capi.BUILDER_SAH, capi.BUILDER_SBVH):
        nodes, tris, info = capi.build_bvh_host(cs.vertices, cs.indices, builder=b)
        assert capi.validate_bvh(nodes, tris, cs.n_tris) == info.max_depth
    nodes, tris, info = capi.build_bvh_host(cs.vertices, cs.indices)
    internal = [i for i in range(1, len(nodes)) if not (int(nodes[i]["child"][0]) & 0x80000000)]
    k = internal[len(internal) // 2]

    def bad(mut_nodes=None, mut_tris=None, n_scene=cs.n_tris):
        n, t = nodes.copy(), tris.copy()
        if mut_nodes:
            mut_nodes(n)
        if mut_tris:
            mut_tris(t)
        with pytest.raises(capi.AkrError):
            capi.validate_bvh(n, t, n_scene)

    bad(lambda n: n[k]["child"].__setitem__(0, len(nodes) + 5))                    # out of range
    bad(lambda n: n[k]["child"].__setitem__(0, int(n[0]["child"][0])))             # back to the root: a cycle
    bad(lambda n: n[k]["child"].__setitem__(0, 0))                                  # the virtual root
    bad(lambda n: n[k]["child"].__setitem__(1, 0x80000000 | (len(tris) << 3) | 3))  # leaf beyond the triangles
    bad(mut_tris=lambda t: t["gid"].__setitem__(7, cs.n_tris))                      # triangle id beyond the scene
    bad(lambda n: n[k].__setitem__("axis", 3))
    bad(lambda n: n[k]["bz"].__setitem__(1, np.nan))
    bad(lambda n: n[0]["child"].__setitem__(1, 1))                                  # node 0 not the virtual root
    bad(n_scene=0)
    # a chain deeper than AKR_BVH_MAX_DEPTH (64): node i -> node i + 1, the other child a leaf
    deep = np.zeros(70, capi.NODE_DTYPE)
    deep["child"][:, 1] = 0x80000000
    for i in range(1, 69):
        deep[i]["child"][0] = i + 1
    deep[0]["child"] = [1, 0xFFFFFFFF]
    deep[69]["child"] = [0x80000000, 0x80000000]
    deep["axis"] = 0
    with pytest.raises(capi.AkrError):
        capi.validate_bvh(deep, tris[:1], cs.n_tris)
    empty = np.zeros(1, capi.NODE_DTYPE)
    empty[0]["child"] = [0xFFFFFFFF, 0xFFFFFFFF]
    assert capi.validate_bvh(empty, tris[:0], 0) == 0


@pytest.mark.parametrize("builder", ["sah", "sbvh"])
def test_wide_view_preorder_parallel(builder):
    """Large enough that the collapse runs subtrees on the thread pool (bvh_wide.cpp: pending
    subtrees below 4096 wide nodes become tasks): nodes must still come in depth-first preorder,
    leaves in the order that walk meets them, and two builds must agree byte for byte."""
    cs = scene.compile_scene(small_soup(60_000, r=0.01 if builder == "sah" else 0.05))
    b = capi.BUILDER_SBVH if builder == "sbvh" else capi.BUILDER_SAH
    nodes, tris, info, (wn, lv, root) = capi.build_bvh_host(cs.vertices, cs.indices, wide=True, builder=b)
    assert len(wn) > 3 * 4096
    _, _, _, (wn2, lv2, root2) = capi.build_bvh_host(cs.vertices, cs.indices, wide=True, builder=b)
    assert root == root2 == 0 and wn.tobytes() == wn2.tobytes() and lv.tobytes() == lv2.tobytes()
    # the serial build (one thread: BVH2 build and the whole collapse on the calling thread) agrees
    # byte for byte with the default thread pool
    n1, t1, _, (wn1, lv1, root1) = capi.build_bvh_host(cs.vertices, cs.indices, wide=True, builder=b, n_threads=1)
    assert n1.tobytes() == nodes.tobytes() and t1.tobytes() == tris.tobytes()
    assert root1 == 0 and wn1.tobytes() == wn.tobytes() and lv1.tobytes() == lv.tobytes()
    next_node, next_leaf = [0], [0]
    stack = [root]
    while stack:
        ref = stack.pop()
        if ref & 0x80000000:
            assert ref & 0x7FFFFFFF == next_leaf[0]
            next_leaf[0] += 1
            continue
        assert ref == next_node[0]
        next_node[0] += 1
        stack.extend(int(c) for c in reversed(wn[ref]["child"]) if int(c) != 0xFFFFFFFF)
    assert next_node[0] == len(wn) and next_leaf[0] == len(lv)
    assert sorted((int(l["first"]), int(l["count"])) for l in lv) == sorted(_bvh2_leaf_order(nodes, (1, 1, 1)))


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("mk", ["cornell", "soup", "big_soup"])
def test_sbvh_builder_invariants(mk, leaf):
    """The SBVH builder (the reference's spatial splits, bvh-accelerator.h:125-475): clipped and
    duplicated references within the budget, every triangle covered by its leaf boxes."""
    sc = {"cornell": cornell, "soup": lambda: small_soup(20_000), "big_soup": lambda: small_soup(3_000, r=0.3)}[mk]()
    cs = scene.compile_scene(sc)
    nodes, tris, info = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=leaf, builder=capi.BUILDER_SBVH)
    extra = check_sbvh(cs, nodes, tris, leaf)
    assert info.n_tris == cs.n_tris + extra
    if mk == "big_soup":   # large overlapping triangles: spatial splits must have happened
        assert extra > 0
        _, _, sah = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=leaf)
        assert info.sah_cost < sah.sah_cost
    nodes2, tris2, info2 = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=leaf,
                                               builder=capi.BUILDER_SBVH, spatial_budget=0.05)
    assert check_sbvh(cs, nodes2, tris2, leaf, budget=0.05) <= 0.05 * cs.n_tris + 1


@pytest.mark.parametrize("builder", ["sah", "sbvh"])
@pytest.mark.parametrize("mk", ["cornell", "soup", "big_soup"])
def test_oracle_bvh_matches_brute_force(mk, builder):
    sc = {"cornell": cornell, "soup": lambda: small_soup(20_000), "big_soup": lambda: small_soup(3_000, r=0.3)}[mk]()
    cs = scene.compile_scene(sc)
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices,
                                         builder=capi.BUILDER_SBVH if builder == "sbvh" else capi.BUILDER_SAH)
    orc = O.OracleScene(cs, nodes, tris, capi)
    lo, hi = (-0.9, 0.9) if mk == "cornell" else (-1.1, 1.1)
    rays = random_rays(4096, 11, lo, hi)
    if mk == "cornell":
        rays["o"][:, 1] += 1.0
    bh = orc.trace_brute(rays)
    for exact in (False, True):
        h, nbox, ntri = orc.trace(rays, exact_cull=exact)
        same = h["gid"] == bh["gid"]
        assert same.mean() >= 0.9999
        assert np.array_equal(h["t"][same], bh["t"][same])
    _, box_exact, _ = orc.trace(rays, exact_cull=True)
    _, box_tight, _ = orc.trace(rays, exact_cull=False)
    assert box_tight <= box_exact
    for any_hit in (True,):
        ha, _, _ = orc.trace(rays, any_hit=True)
        assert np.array_equal(ha["gid"] != 0xFFFFFFFF, bh["gid"] != 0xFFFFFFFF)


def test_oracle_render_tight_equals_exact_cull():
    cs = scene.compile_scene(cornell((24, 24)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = O.OracleScene(cs, nodes, tris, capi)
    a, wa, sa = orc.render(4, 5, exact_cull=False)
    b, wb, sb = orc.render(4, 5, exact_cull=True)
    assert np.array_equal(a, b) and np.array_equal(wa, wb)
    assert sa["box_tests"] < sb["box_tests"]


def test_oracle_render_tiles_accumulate_and_threads():
    cs = scene.compile_scene(cornell((20, 12)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = O.OracleScene(cs, nodes, tris, capi)
    full, wf, _ = orc.render(3, 5, n_threads=1)
    part = [(0, 0, 7, 12), (7, 0, 20, 5), (7, 5, 20, 12)]
    r, w, _ = orc.render(3, 5, tiles=part, n_threads=4)
    assert np.array_equal(full, r) and np.array_equal(wf, w)
    r2, w2, _ = orc.render(3, 5, tiles=part, radiance=r.copy(), weight=w.copy())
    assert np.array_equal(r2, 2 * full) and np.all(w2 == 6)


def _lcg_draws(start, final, limit):
    """Per pixel: LCG steps (kernel/sampler.h:54-67, s -> 1103515245 s + 12345 mod 2^32) from
    `start` to `final`, or -1 if not reached within `limit`."""
    s = start.astype(np.uint64)
    f = final.astype(np.uint64)
    out = np.full(s.shape, -1, np.int64)
    for k in range(limit + 1):
        out[(out < 0) & (s == f)] = k
        s = (s * 1103515245 + 12345) & 0xFFFFFFFF
    return out


@pytest.mark.parametrize("depth", [0, 1, 5])
def test_oracle_pixel_probe_properties(depth):
    """The oracle's per-pixel fingerprint (orc_render_probe, the checker of the GPU pixel probe):
    the final sampler state lies 4 + 6k (+2 per zero-pdf BSDF sample) draws per sample after the
    pixel's seed x + y W (pathtracer.h:61-131), closest-hit traces count the camera ray plus every
    extension ray below max_depth, NEE shadow rays at most one per scatter.  max_depth 0 / 1 pin the
    counts exactly; the probe does not change the image."""
    W, H, spp = 24, 16, 3
    cs = scene.compile_scene(cornell((W, H)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = O.OracleScene(cs, nodes, tris, capi)
    r0, w0, _ = orc.render(spp, depth)
    r, w, st, pr = orc.render(spp, depth, probe=True)
    assert np.array_equal(r, r0) and np.array_equal(w, w0)
    assert np.all(pr["flags"] == (capi.PROBE_SEED | capi.PROBE_RAYS))
    ys, xs = np.mgrid[0:H, 0:W]
    draws = _lcg_draws((xs + ys * W).reshape(-1), pr["seed"].reshape(-1), spp * (6 + 6 * depth))
    assert np.all(draws >= 4 * spp) and np.all((draws - 4 * spp) % 2 == 0)
    cl, sh = pr["closest_rays"].reshape(-1), pr["shadow_rays"].reshape(-1)
    scatter_draws = draws - 4 * spp
    assert st["camera_rays"] <= cl.sum() <= st["camera_rays"] + st["extension_rays"]
    assert sh.sum() == st["shadow_rays"]
    if depth == 0:
        assert np.all(cl == spp) and np.all(sh == 0) and np.all(draws == 4 * spp)
    else:
        assert np.all(cl >= spp) and np.all(cl <= spp * max(1, depth))
        assert np.all(6 * (cl - spp) <= scatter_draws) and np.all(sh <= scatter_draws // 6)
        assert sh.sum() > 0
    if depth == 1:
        assert np.all(cl == spp)   # the trace at depth == max_depth adds nothing and is not made


def test_oracle_overlapping_tiles_merge_in_tile_order():
    """Overlapping tiles are merged one after another in tile order (Film::merge_tile under the
    reference's mutex, cpu/integrator.cpp:138-140; the HIP library merges in the same order): the
    same tile listed 8 times on 8 threads is the single render added 8 times, every pixel, every
    run.  An unlocked merge from the worker threads lost updates here (the r1 flaky weights)."""
    cs = scene.compile_scene(cornell((32, 32)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = O.OracleScene(cs, nodes, tris, capi)
    t = (3, 2, 29, 31)
    one, w1, _ = orc.render(2, 5, tiles=[t], n_threads=1)
    acc = np.zeros_like(one)
    for _ in range(8):
        acc = (acc + one).astype(np.float32)
    for _ in range(3):
        r, w, _ = orc.render(2, 5, tiles=[t] * 8, n_threads=8)
        assert np.array_equal(w, 8 * w1) and np.array_equal(r, acc)
    ao1, aw1, _ = orc.render_ao(3, tiles=[t], n_threads=1)
    ao, aw, _ = orc.render_ao(3, tiles=[t] * 8, n_threads=8)
    assert np.array_equal(aw, 8 * aw1) and np.array_equal(ao, 8 * ao1)


def test_oracle_ao_properties():
    """cpu::AmbientOcclusion restated (integrator.cpp:40-87): L per sample is 0 or 1 on all three
    channels, monotone in `occlude` for the same sample streams, 1 for every camera hit when
    occlude <= 0 (t < occlude never holds), and 0 on a camera miss."""
    cs = scene.compile_scene(cornell((24, 16)))
    nodes, tris, _ = capi.build_bvh_host(cs.vertices, cs.indices)
    orc = O.OracleScene(cs, nodes, tris, capi)
    spp = 6
    inf, wi, st = orc.render_ao(spp)
    assert np.all(wi == spp)
    assert np.array_equal(inf[..., 0], inf[..., 1]) and np.array_equal(inf[..., 0], inf[..., 2])
    assert np.array_equal(inf, np.round(inf)) and inf.min() >= 0 and inf.max() <= spp
    near, _, _ = orc.render_ao(spp, occlude=0.25)
    far, _, _ = orc.render_ao(spp, occlude=2.0)
    hitmask, _, s0 = orc.render_ao(spp, occlude=0.0)
    assert np.all(inf <= far) and np.all(far <= near) and np.all(near <= hitmask)
    assert (near > inf).any() and inf.mean() > 0
    assert s0["camera_rays"] == 24 * 16 * spp and s0["shadow_rays"] == hitmask[..., 0].sum()
    assert st["shadow_rays"] == s0["shadow_rays"]
    # exact culling is a traversal detail: same image
    ex, _, _ = orc.render_ao(spp, exact_cull=True)
    assert np.array_equal(ex, inf)
    # a lone quad: nothing can occlude its AO rays, whichever side they leave from
    quad = scene.Mesh(vertices=np.array([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, 5, 0]], np.float32),
                      indices=np.array([[0, 1, 2], [0, 2, 3]], np.int32),
                      normals=np.tile(np.array([0, 0, 1], np.float32), (2, 3)),
                      texcoords=np.zeros((2, 6), np.float32), material_indices=np.zeros(2, np.int32),
                      materials=[scene.DiffuseMaterial(scene.ConstantTexture((0.5, 0.5, 0.5)))])
    qs = scene.compile_scene(scene.Scene(camera=scene.PerspectiveCamera(position=(0, 0, 4), resolution=(12, 8),
                                                                        fov=40), shapes=[quad]))
    qn, qt, _ = capi.build_bvh_host(qs.vertices, qs.indices)
    qo = O.OracleScene(qs, qn, qt, capi)
    r, w, _ = qo.render_ao(3)
    assert np.all(r == 3)


SDL = """
// a scene written in the reference's language (core/parser.cpp:150-363)
let grey = [0.725, 0.71, 0.68]
export light = EmissiveMaterial { color: [17, 12, 4] }
export mesh = AkariMesh {
  path: "MESH",
  materials: [
    DiffuseMaterial { color: [0.63, 0.065, 0.05] },
    DiffuseMaterial { color: [0.14,0.45,0.091] },
    DiffuseMaterial { color: $grey }, DiffuseMaterial { color: $grey }, DiffuseMaterial { color: $grey },
    GlossyMaterial { color: 0.5, roughness: 0.3 },
    MixMaterial { fraction: 0.25, first: DiffuseMaterial { color: $grey }, second: $light },
    $light,
  ]
}
export scene = Scene {
    camera: PerspectiveCamera { fov: 15, position: [0, 1, 9], rotation: [0, -0.5, 0], resolution: [32, 24] },
    integrator: Path { spp: 4, max_depth: 3, tile_size: 16, megakernel: true },
    output: "out.png",
    shapes: [ $mesh ]
}
"""


def test_scene_language(tmp_path):
    (tmp_path / "m.akari").write_text(SDL.replace("MESH", str(CORNELL_MESH)))
    (tmp_path / "top.akari").write_text('import "m.akari" as cbox\nexport scene = $cbox.scene\n')
    sc = scene.load_scene_file(tmp_path / "top.akari")
    assert sc.camera.resolution == (32, 24) and sc.camera.fov == 15.0 and sc.camera.rotation[1] == -0.5
    it = sc.integrator
    assert (it.spp, it.max_depth, it.tile_size, it.wavefront) == (4, 3, 16, False)
    mesh = sc.shapes[0]
    assert mesh.n_tris == 36 and len(mesh.materials) == 8
    assert mesh.materials[7] is mesh.materials[6].second      # $light is one object
    assert not mesh.materials[7].double_sided                # the node ignores double_sided
    assert mesh.materials[0].color.value[1] == float(np.float32(0.065))
    cs = scene.compile_scene(sc)
    # Emissive only at top level counts as a light (scene.cpp:62-66); the Mix child does not
    assert [p for _, p in cs.lights] == [34, 35]
    assert len(cs.materials) == 9


def test_scene_language_errors(tmp_path):
    bad = tmp_path / "bad.akari"
    bad.write_text("export a = [1, 2\n")
    with pytest.raises(scene.SdlError):
        scene.load_scene_file(bad, "a")
    bad.write_text("export a = $nothing\n")
    with pytest.raises(scene.SdlError):
        scene.load_scene_file(bad, "a")
    bad.write_text('import "missing.akari" as m\n')
    with pytest.raises(scene.SdlError):
        scene.load_scene_file(bad, "a")


def test_number_parsing_matches_reference():
    p = scene.SdlParser()
    for src, exp in (("0.725", 0 + 725 / 1000.0), ("-12.5", -12.5), ("17", 17.0), ("0.065", 65 / 1000.0)):
        p.src, p.pos, p.path = src, 0, ROOT
        assert p._number() == exp


def test_soup_generator_matches_pcg():
    v, n, t = capi.generate_soup(1000, seed=42, r=0.01, n_threads=3)
    u = O.pcg(42, 12 * 1000).reshape(1000, 12)
    c = (np.float32(2.0) * u[:, :3] - np.float32(1.0)).astype(np.float32)
    off = ((np.float32(2.0) * u[:, 3:] - np.float32(1.0)) * np.float32(0.01)).astype(np.float32)
    exp = (c[:, None, :] + off.reshape(1000, 3, 3)).astype(np.float32).reshape(-1, 3)
    assert np.array_equal(v, exp)
    v1, _, _ = capi.generate_soup(1000, seed=42, r=0.01, n_threads=1)
    assert np.array_equal(v, v1)
    assert np.array_equal(t[0], np.array([0, 1, 1, 0, 1, 1], np.float32))
    assert np.allclose(np.linalg.norm(n.reshape(-1, 3), axis=1), 1, atol=1e-5)


def test_soup_scene_lights():
    cs = scene.compile_scene(scene.soup_scene(n_tris=100, resolution=(8, 8)))
    assert cs.lights == [(0, 100), (0, 101)]
    v = cs.vertices[cs.indices[100]]
    ng = np.cross(v[1] - v[0], v[2] - v[0])
    assert ng[1] < 0                      # one-sided emitter facing -y (light.h:67)
    # power = |cross| (twice the area: 4) * texcoord area (0.5) * luminance (10), scene.cpp:72-87
    assert np.allclose(cs.power, 4 * 0.5 * 10, rtol=1e-6)


def test_render_scene_fails_loudly_without_gpu(tmp_path):
    """No CPU fallback: the scene renderer goes through the HIP library or raises."""
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from akari_amd import render
    with pytest.raises(capi.AkrError):
        render.render_scene(cornell((8, 8)))


def _f32_fma(a, b, c):
    """f32 fma emulated in f64: exact whenever a * b + c fits 53 bits (always here: 8-bit q or
    255 times a 24-bit float, plus a 24-bit float within 2^29 of it), then one rounding."""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def _f32_fma_exact(a, b, c):
    """f32 fma at any magnitude: the product of two f32 is exact in f64, the sum is rounded to odd in
    f64 (TwoSum gives its error exactly), and a round-to-odd value of 53 bits rounds to 24 bits or
    fewer (a subnormal result) as the exact sum does."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    p, c = np.broadcast_arrays(p, c)
    with np.errstate(all="ignore"):   # an infinite operand or sum: err is NaN and s stands
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where((err != 0) & even, odd, s).astype(np.float32)


def _lean_slot_test(node, slot, o, invd, tmin, lim, fma=_f32_fma, parts=None):
    """kernels.hip visit_wide_lean for one slot, emulated in f32 (vectorised over rays).  `parts`, a
    list, receives every intermediate array."""
    f = np.float32
    meta = int(node["meta"])
    s = np.array([np.float32(2.0 ** (((meta >> (8 * a)) & 0xFF) - 127)) for a in range(3)], np.float32)
    sc = (s[None, :] * invd).astype(f)
    oq = ((node["origin"][None, :].astype(f) - o).astype(f) * invd).astype(f)
    e = fma(fma(f(255.0), np.abs(sc), np.abs(oq)), f(2.0 ** -21), f(2.0 ** -120))
    no, fo = (oq - e).astype(f), (oq + e).astype(f)
    q = [[(int(node["q"][2 * a + hi]) >> (8 * slot)) & 0xFF for hi in (0, 1)] for a in range(3)]
    pos = invd > 0
    qn = np.stack([np.where(pos[:, a], q[a][0], q[a][1]) for a in range(3)], 1).astype(f)
    qf = np.stack([np.where(pos[:, a], q[a][1], q[a][0]) for a in range(3)], 1).astype(f)
    n = fma(qn, sc, no)
    x = fma(qf, sc, fo)
    t = np.maximum(n.max(1), tmin)
    m1 = np.minimum(x.min(1), lim)
    if parts is not None:
        parts += [sc, oq, e, no, fo, n, x]
    return t <= m1, t


def _ref_box_test(lo, hi, o, invd, tmin, tmax, best):
    """The reference intersectAABB (bvh-accelerator.h:89-103) with the tight cull and the
    traversal's cull (t < 0 or t > best), in f32."""
    t0 = ((lo[None, :] - o).astype(np.float32) * invd).astype(np.float32)
    t1 = ((hi[None, :] - o).astype(np.float32) * invd).astype(np.float32)
    m0 = np.minimum(t0, t1).max(1)
    m1 = np.maximum(t0, t1).min(1)
    t = np.maximum(tmin, m0)
    hit = (m0 <= m1) & (t < tmax) & (t <= m1) & ~(t < 0) & ~(t > best)
    return hit, t


def test_lean_slot_test_conservative():
    """The lean slot test passes whenever the reference test of the exact box
    passes, with an entry distance no larger — on every leaf slot of a built wide view, for
    random rays and for rays aimed at each box's corners, edges and faces (grazing), with
    bounded and unbounded intervals."""
    cs = scene.compile_scene(small_soup(3_000))
    _, _, _, wide = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=1, wide=True)
    wn, lv, _ = wide
    rng = np.random.default_rng(5)
    base = random_rays(512, 3, -1.3, 1.3)
    checked = 0
    for ni in range(len(wn)):
        node = wn[ni]
        for k in range(4):
            c = int(node["child"][k])
            if c == 0xFFFFFFFF or not (c & 0x80000000):
                continue
            leaf = lv[c & 0x7FFFFFFF]
            # 48 rays through corner / edge / face points of this box at t = dist
            m = 48
            sel = rng.integers(0, 3, (m, 3))
            tgt = np.where(sel == 0, leaf["lo"], np.where(sel == 1, leaf["hi"], (leaf["lo"] + leaf["hi"]) / 2))
            dd = rng.normal(size=(m, 3)).astype(np.float32)
            dd /= np.linalg.norm(dd, axis=1, keepdims=True).astype(np.float32)
            dist = rng.choice(np.float32([0.01, 0.37, 3.0]), m).astype(np.float32)
            o = np.concatenate([base["o"], (tgt - dd * dist[:, None]).astype(np.float32)]).astype(np.float32)
            d = np.concatenate([base["d"], dd]).astype(np.float32)
            invd = (np.float32(1.0) / d).astype(np.float32)
            nr = o.shape[0]
            tmin = rng.choice(np.float32([0.0, 1e-3, 0.2]), nr).astype(np.float32)
            tmax = rng.choice(np.float32([np.inf, 0.37, 2.0]), nr).astype(np.float32)
            best = rng.choice(np.float32([np.inf, 0.37, 1.0]), nr).astype(np.float32)
            tmaxp = np.nextafter(tmax, np.float32(-np.inf)).astype(np.float32)
            lim = np.minimum(best, tmaxp)
            rh, rt = _ref_box_test(leaf["lo"], leaf["hi"], o, invd, tmin, tmax, best)
            lh, lt = _lean_slot_test(node, k, o, invd, tmin, lim)
            assert np.all(lh[rh]), f"lean test rejects a box the reference enters (node {ni}, slot {k})"
            assert np.all(lt[rh] <= rt[rh])
            checked += int(rh.sum())
    assert checked > 20_000


def test_lean_slot_test_conservative_on_grid_bounds():
    """Adversarial boxes whose exact bounds lie ON the quantization grid (the builder's zero-slack
    case): the lean test's per-axis values differ from the reference's by rounding only, which the
    slack must cover.  Rays graze corners, edges and faces; magnitudes up to 2^20."""
    rng = np.random.default_rng(11)
    f = np.float32
    n_box, m = 12000, 64
    bad = 0
    checked = 0
    for b in range(n_box):
        scale = f(2.0 ** rng.integers(-8, 20))
        org = (rng.uniform(-1, 1, 3) * scale).astype(f)
        e = rng.integers(-20, 12, 3) + int(np.log2(scale))
        s = np.array([f(2.0 ** int(x)) for x in e], f)
        q_lo = rng.integers(0, 128, 3)
        q_hi = q_lo + rng.integers(0, 128, 3)
        lo = (org.astype(np.float64) + q_lo * s.astype(np.float64))
        hi = (org.astype(np.float64) + q_hi * s.astype(np.float64))
        if np.any(lo.astype(f).astype(np.float64) != lo) or np.any(hi.astype(f).astype(np.float64) != hi):
            continue  # keep boxes whose bounds are exactly on the grid
        lo, hi = lo.astype(f), hi.astype(f)
        node = np.zeros((), [("origin", f, 3), ("meta", np.uint32), ("q", np.uint32, 6)])
        node["origin"] = org
        node["meta"] = int(e[0] + 127) | int(e[1] + 127) << 8 | int(e[2] + 127) << 16
        node["q"] = [int(q_lo[0]), int(q_hi[0]), int(q_lo[1]), int(q_hi[1]), int(q_lo[2]), int(q_hi[2])]
        sel = rng.integers(0, 3, (m, 3))
        tgt = np.where(sel == 0, lo, np.where(sel == 1, hi, ((lo + hi) / 2).astype(f))).astype(f)
        d = rng.normal(size=(m, 3)).astype(f)
        d[rng.random((m, 3)) < 0.2] *= f(1e-3)   # steep rays: large |invd|
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f)
        dist = (rng.choice([0.01, 0.5, 7.0], m) * scale).astype(f)
        o = (tgt - d * dist[:, None]).astype(f)
        invd = (f(1.0) / d).astype(f)
        tmin = np.zeros(m, f)
        lim = np.full(m, np.finfo(f).max, f)
        rh, rt = _ref_box_test(lo, hi, o, invd, tmin, np.full(m, np.inf, f), np.full(m, np.inf, f))
        lh, lt = _lean_slot_test(node, 0, o, invd, tmin, lim)
        bad += int(np.sum(rh & ~lh)) + int(np.sum(rh & (lt > rt)))
        checked += int(rh.sum())
    assert checked > 30_000
    assert bad == 0


def test_f32_fma_exact_matches_libm():
    """The exact f32 fma of the stated-bounds test against libm's fmaf, on operands spread over the
    whole exponent range (where the f64 emulation _f32_fma double-rounds) and on halfway cases."""
    import ctypes.util
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    rng = np.random.default_rng(17)
    f = np.float32
    n = 20_000
    mant = lambda: (1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23)) * rng.choice([-1.0, 1.0], n)
    a = (mant() * 2.0 ** rng.integers(-60, 60, n)).astype(f)
    b = (mant() * 2.0 ** rng.integers(-60, 60, n)).astype(f)
    ab = a.astype(np.float64) * b.astype(np.float64)
    # addends from far below the product to far above it, and within a few binades (cancellation)
    c = (-ab * 2.0 ** rng.choice([-60, -30, -25, -24, -23, -1, 0, 1, 23, 24, 25, 40], n) * rng.choice([1.0, -1.0, 1.0 + 2.0 ** -20], n))
    with np.errstate(over="ignore", under="ignore"):
        c = c.astype(f)
    a[:256], b[:256] = f(255.0), (mant()[:256] * 2.0 ** rng.integers(-149, -120, 256)).astype(f)   # subnormal products
    c[:256] = (mant()[:256] * 2.0 ** rng.integers(-149, -120, 256)).astype(f)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies halfway between two f32; an addend of 2^-80 decides the side
    k = 2.0 ** rng.integers(-30, 30, 256)
    a[256:512], b[256:512] = ((1 + 2.0 ** -12) * k).astype(f), f(1 + 2.0 ** -12)
    c[256:512] = (rng.choice([-1.0, 1.0], 256) * 2.0 ** -80 * k).astype(f)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], f)
    got = _f32_fma_exact(a, b, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(_f32_fma(a, b, c) != want) > 0   # the f64 emulation is not exact out here


def _grid_box(rng, org, e):
    """A wide-node frame (origin `org`, steps 2^e) and the tightest f32 box inside one of its grid
    cells' hull [org + q_lo 2^e, org + q_hi 2^e]: the builder's zero-slack case (it quantizes outward
    in real arithmetic).  Returns (node, lo, hi), or None where no f32 lies inside on some axis."""
    from fractions import Fraction
    f = np.float32
    q_lo = rng.integers(0, 128, 3)
    q_hi = q_lo + rng.integers(0, 128, 3)

    def inside(x, up):   # the f32 nearest to x that is >= x (up) or <= x
        v = f(float(x))
        while up and Fraction(float(v)) < x:
            v = np.nextafter(v, f(np.inf))
        while not up and Fraction(float(v)) > x:
            v = np.nextafter(v, f(-np.inf))
        return v
    lo = np.array([inside(Fraction(float(org[a])) + int(q_lo[a]) * Fraction(2) ** int(e[a]), True) for a in range(3)], f)
    hi = np.array([inside(Fraction(float(org[a])) + int(q_hi[a]) * Fraction(2) ** int(e[a]), False) for a in range(3)], f)
    if np.any(lo > hi):
        return None
    node = np.zeros((), [("origin", f, 3), ("meta", np.uint32), ("q", np.uint32, 6)])
    node["origin"] = org
    node["meta"] = int(e[0] + 127) | int(e[1] + 127) << 8 | int(e[2] + 127) << 16
    node["q"] = [int(q_lo[0]), int(q_hi[0]), int(q_lo[1]), int(q_hi[1]), int(q_lo[2]), int(q_hi[2])]
    return node, lo, hi


def _stated_bounds_rays(rng, m, lo, hi, ld_choices, off_exp):
    """m rays aimed at corner / edge / face / inner points of the box: direction components
    +-mantissa * 2^ld, ld drawn per ray from one of `ld_choices` (a (low, high) range shared by the
    axes), the origin so far back that the largest |d| T is about 2^off_exp.  f32 (o, d, T)."""
    f = np.float32
    sel = rng.integers(0, 4, (m, 3))
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    inner = lo.astype(np.float64) + (hi.astype(np.float64) - lo.astype(np.float64)) * rng.random((m, 3))
    tgt = np.where(sel == 0, lo, np.where(sel == 1, hi, np.where(sel == 2, mid, inner)))
    rg = np.array(ld_choices)[rng.integers(0, len(ld_choices), m)]
    ld = rng.integers(rg[:, :1], rg[:, 1:] + 1, (m, 3))
    mant = np.where(rng.random((m, 3)) < 0.3, 1.0, 1.0 + rng.integers(0, 1 << 23, (m, 3)) / float(1 << 23))
    d = (rng.choice([-1.0, 1.0], (m, 3)) * mant * 2.0 ** ld).astype(f)
    T = 2.0 ** (rng.integers(off_exp[0], off_exp[1] + 1, m) - ld.max(1)) * rng.uniform(0.25, 1.0, m)
    with np.errstate(over="ignore", under="ignore"):
        o = (tgt - d.astype(np.float64) * T[:, None]).astype(f)
        T = T.astype(f)
    return o, d, T


# (name, log2 of the frame origin's magnitude (None: the origin is a small multiple of the step), step
#  exponents, per-ray ranges of log2 |d|, log2 of the distance |d| T from the box to the origin)
_STATED_BOUNDS_REGIMES = [
    # frames at the 2^40 gate, origins out to 2^60, all three 1 / d at 2^64: oq and the slot values near 2^124
    ("top", (36, 40), (24, 40), [(-64, -64), (-64, -62), (-64, -40), (-30, 0)], (52, 60)),
    # every scale up to the gate, unit-length-like directions with components down to 2^-64
    ("middle", (-8, 40), None, [(-64, 0), (-12, 0), (-2, 0)], None),
    # steps at the bottom of the exponent range: sc = 2^e / d underflows for |d| > 1
    ("bottom", None, (-126, -112), [(0, 20), (-10, 10), (-64, 0), (0, 0)], None),
]


def test_lean_slot_test_conservative_at_stated_bounds():
    """The lean slot test's claim (kernels.hip, above visit_wide_lean_node) at the bounds it states:
    frame origins and steps up to 2^40, ray origins up to 2^60, |1 / d| up to 2^64, and steps down to
    2^-126 where sc underflows and the 2^-120 term is the slack.  Every fma is exact (_f32_fma_exact).
    For every ray that lean_ok admits: no intermediate is NaN or infinite; where the reference test of
    the exact box accepts, the lean test accepts, with an entry distance no larger."""
    rng = np.random.default_rng(23)
    f = np.float32
    m = 96
    checked, admitted = {}, 0
    for name, org_exp, e_rng, ld_choices, off_exp in _STATED_BOUNDS_REGIMES:
        checked[name] = 0
        for b in range(1500):
            if name == "top":
                e = rng.integers(e_rng[0], e_rng[1] + 1, 3)
                org = np.clip(rng.uniform(-1, 1, 3) * 2.0 ** rng.integers(org_exp[0], org_exp[1] + 1, 3), -2.0 ** 40, 2.0 ** 40).astype(f)
                if b % 8 == 0:
                    org[rng.integers(0, 3)] = f(rng.choice([-1.0, 1.0]) * 2.0 ** 40)
                off = off_exp
            elif name == "middle":
                k = int(rng.integers(org_exp[0], org_exp[1] + 1))
                org = (rng.uniform(-1, 1, 3) * 2.0 ** k).astype(f)
                e = np.minimum(rng.integers(-20, 12, 3) + k, 40)
                top_e = int(e.max()) + 7       # the box is at most 2^(e + 8) wide
                off = (top_e - 8, min(60, top_e + 14))
            else:
                e = rng.integers(e_rng[0], e_rng[1] + 1, 3)
                org = (rng.integers(-1024, 1025, 3) * 2.0 ** e.min()).astype(f)
                off = (int(e.min()), int(e.max()) + 10)
            box = _grid_box(rng, org, e)
            if box is None:
                continue
            node, lo, hi = box
            o, d, T = _stated_bounds_rays(rng, m, lo, hi, ld_choices, off)
            with np.errstate(all="ignore"):
                invd = (f(1.0) / d).astype(f)
                ok = (np.isfinite(o).all(1) & np.isfinite(invd).all(1) & (invd != 0).all(1)
                      & (np.abs(o).max(1) <= f(2.0 ** 60)) & (np.abs(invd).max(1) <= f(2.0 ** 64)))   # lean_ok
                o, invd, T = o[ok], invd[ok], T[ok]
                n = len(o)
                admitted += n
                for tmin, tmax in ((np.zeros(n, f), np.full(n, np.inf, f)), ((T * f(0.5)).astype(f), (T * f(2.0)).astype(f))):
                    fin = np.isfinite(tmax)
                    tmaxp = np.where(fin, np.nextafter(tmax, f(-np.inf)), np.finfo(f).max).astype(f)   # float_below; fminf(best, +inf)
                    rh, rt = _ref_box_test(lo, hi, o, invd, tmin, tmax, np.full(n, np.inf, f))
                    parts = []
                    lh, lt = _lean_slot_test(node, 0, o, invd, tmin, tmaxp, fma=_f32_fma_exact, parts=parts)
                    for p in parts:
                        assert np.isfinite(p).all(), f"{name}: a NaN or infinite intermediate (box {b})"
                    assert np.all(lh[rh]), f"{name}: the lean test rejects a box the reference enters (box {b})"
                    assert np.all(lt[rh] <= rt[rh]), f"{name}: a lean entry distance above the reference's (box {b})"
                    checked[name] += int(rh.sum())
    print(f"lean slot test at its stated bounds: accepted cases checked {checked}, of {admitted} admitted rays")
    assert sum(checked.values()) >= 30_000
    assert min(checked.values()) >= 3_000, checked   # no regime passes on rejections alone


def test_traversal_limit_inputs_on_the_oracle():
    """The conditions test_gpu_trace_limits.py relies on, on the oracle alone (a host-built tree): the
    hit shares of the scaled, far-origin and near-axis batches, on which side of the 2^40 gate each
    scaled wide view lies, which rays lean_ok admits, that every interval variant changes oracle
    answers across its edge, and the share of the far camera's pixels whose paths go on."""
    import helpers as H
    share = lambda h: float((h["gid"] != 0xFFFFFFFF).mean())
    base = random_rays(1 << 14, 2, -1.2, 1.2)
    orcs = {}
    for k in (0, 20, 38, 39, 40):
        cs = scene.compile_scene(H.scaled_soup(k))
        nodes, tris, _, (wn, _, _) = capi.build_bvh_host(cs.vertices, cs.indices, wide=True)
        orcs[k] = orc = O.OracleScene(cs, nodes, tris, capi)
        steps = 2.0 ** (np.stack([(wn["meta"] >> (8 * a)) & 0xFF for a in range(3)]).astype(np.int64).max() - 127)
        max_abs = max(float(np.abs(wn["origin"]).max()), steps)
        assert (max_abs <= 2.0 ** 40) == (k <= 39), (k, max_abs)
        rays = H.scaled_rays(base, k)
        assert H.lean_expected(rays).all()
        for any_hit in (False, True):
            s = share(orc.trace(rays, any_hit=any_hit)[0])
            assert abs(s - 0.8256) < 1e-4, (k, any_hit, s)     # pure scaling: the same share at every k
    for k, want in ((0, (0.61, 0.61)), (38, (0.78, 0.24))):
        for log2_dist, w in zip((59, 61), want):
            rays = H.far_origin_rays(k, log2_dist)
            assert np.all(H.lean_expected(rays) == (log2_dist == 59))
            s = share(orcs[k].trace(rays)[0])
            assert abs(s - w) < 0.01 and s >= 0.2, (k, log2_dist, s)
    for e in (-62, -63, -64, -65, -66):
        rays = H.near_axis_rays(e)
        assert np.all(H.lean_expected(rays) == (e >= -64))
        s = share(orcs[0].trace(rays)[0])
        assert abs(s - 0.8213) < 1e-4, (e, s)
    n = 4096 + 17
    for reason in H.LEAN_REFUSALS:
        for pattern in ("1in64", "alternate", "63in64", "half"):
            mask = H.refusal_mask(n, pattern)
            assert np.array_equal(H.lean_expected(H.refuse_lean(random_rays(n, 7, -1.2, 1.2), mask, reason)), ~mask)
    # intervals that end on a hit
    crays = random_rays(1 << 12, 6, -0.9, 0.9)
    crays["o"][:, 1] += 1.0
    ccs = scene.compile_scene(cornell((24, 24)))
    corc = O.OracleScene(ccs, *capi.build_bvh_host(ccs.vertices, ccs.indices)[:2], capi)
    for orc, rays in ((orcs[0], random_rays(1 << 12, 6, -1.2, 1.2)), (corc, crays)):
        for exact in (False, True):
            oh = orc.trace(rays, exact_cull=exact)[0]
            hit = oh["gid"] != 0xFFFFFFFF
            assert hit.mean() >= 0.5
            variants = H.interval_variants(rays[hit], oh["t"][hit])
            for any_hit in (False, True):
                ans = {v: orc.trace(r, any_hit=any_hit, exact_cull=exact)[0] for v, r in variants.items()}
                ans[None] = orc.trace(rays[hit], any_hit=any_hit, exact_cull=exact)[0]
                for v in variants:
                    other = ans[{"tmax=t+": "tmax=t", "tmin=t-": "tmin=t"}.get(v)]
                    assert np.any((ans[v]["gid"] != other["gid"]) | (ans[v]["t"] != other["t"])), (v, any_hit, exact)
        nf = orc.trace(H.nonfinite_rays((0.0, 1.0, 0.0) if orc is corc else (0.0, 0.0, 0.0)))[0]
        assert (nf["gid"][12:] != 0xFFFFFFFF).all() and (nf["gid"][:12] == 0xFFFFFFFF).all()
    # the far camera: a finite film, and most paths go on past the camera ray
    cs = scene.compile_scene(H.far_camera_soup((24, 24)))
    orc = O.OracleScene(cs, *capi.build_bvh_host(cs.vertices, cs.indices)[:2], capi)
    rad, w, _, probe = orc.render(4, 5, probe=True)
    going = float((probe["closest_rays"] > 4).mean())
    print(f"far camera: {going:.4f} of the pixels trace more than spp closest rays, mean {probe['closest_rays'].mean():.1f} "
          f"closest and {probe['shadow_rays'].mean():.1f} shadow rays")
    assert np.isfinite(rad).all() and rad.mean() > 0 and going >= 0.4


def test_device_trig_matches_libm_on_path_range(tmp_path):
    """The device's fsin/fcos (akr_trig.h: fdlibm-style f64 reduction and kernels) against the C
    library's f64 sin/cos that the oracle uses, both rounded to f32, on every 64th f32 in
    [-2 pi, 2 pi] (the path's arguments: concentric_disk theta, GGX phi).  Run with stride 1 it covers
    all 2.17e9 inputs; that exhaustive run found no difference."""
    import subprocess
    exe = tmp_path / "trig_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
                    f"-I{ROOT / 'akarirender-1_amd' / 'csrc'}", str(ROOT / "tests" / "cpp" / "trig_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "64", "8"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    n, bad = (int(v) for v in re.findall(r"\d+", out.stdout))
    assert n > 30_000_000 and bad == 0
