"""Adaptive sampling on device 0: masked continues, sessions whose slots hold
different counts, the convergence test and the adaptive render.

A slot's samples are one LCG chain, so a slot that received c samples equals the oracle's c-spp render
at that pixel bit for bit, whatever its neighbours received.  Every expectation is therefore built from
whole-frame `orc.render(total, ..., probe=True)` calls of the unchanged oracle, one per (scene, total),
shared by all tests, plus the NumPy f32 restatement of the convergence test in test_adaptive_host.py.
All comparisons are array_equal."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell, slot_pixels, small_soup
from test_adaptive_host import STRIP, replay, strip_errors

pytestmark = pytest.mark.gpu

RAGGED = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 64, 64), (5, 5, 5, 9)]   # ragged, clipped, empty
NO_SESSION = "no render session to continue"
DEPTH = 5

_ORACLES = {}   # scene name -> [nodes, tris, OracleScene, {total: (radiance, weight, seed)}]


def _setup(ctx, name, make):
    """Upload scene `name`; returns (cs, frame) where frame(total) is the oracle's whole-frame
    (radiance [H, W, 3], weight [H, W], final sampler state [H, W]) of a total-spp render."""
    cs = scene.compile_scene(make())
    scene.upload_scene(ctx, cs)
    nodes, tris = ctx.accel_export()
    ent = _ORACLES.get(name)
    if ent is None or not (np.array_equal(ent[0], nodes) and np.array_equal(ent[1], tris)):
        ent = _ORACLES[name] = [nodes, tris, py_oracle.OracleScene(cs, nodes, tris, capi), {}]
    W, H = (int(v) for v in cs.camera.resolution)

    def frame(total):
        if total not in ent[3]:
            out = ent[2].render(total, DEPTH, tiles=[(0, 0, W, H)], probe=True)
            got = (out[0], out[1], np.ascontiguousarray(out[3]["seed"]))
            for a in got:
                a.setflags(write=False)
            assert np.all(got[1] == total)
            ent[3][total] = got
        return ent[3][total]
    return cs, frame


def _slot_film(frame, total, ys, xs):
    """The per-slot film [n, 4] of a uniform total-spp render."""
    rad, w, _ = frame(total)
    return np.concatenate([rad[ys, xs], w[ys, xs][:, None]], axis=1).astype(np.float32)


def _expected(frame, count, ys, xs, W, H):
    """Per-slot film [n, 4] and sampler state [n], and the merged host frame, when slot k holds count[k]
    samples (slots of overlapping tiles add up in the frame, in slot order)."""
    n = len(ys)
    film = np.zeros((n, 4), np.float32)
    seed = np.zeros(n, np.uint32)
    for total in np.unique(count):
        sel = count == total
        film[sel] = _slot_film(frame, int(total), ys[sel], xs[sel])
        seed[sel] = frame(int(total))[2][ys[sel], xs[sel]]
    rad, w = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    np.add.at(rad, (ys, xs), film[:, :3])
    np.add.at(w, (ys, xs), film[:, 3])
    return film, seed, rad, w


def _check(ctx, frame, count, rad, w, ys, xs, W, H, probe=True):
    film, seed, erad, ew = _expected(frame, count, ys, xs, W, H)
    assert np.array_equal(w, ew), f"{np.count_nonzero(w != ew)} weights differ"
    assert np.array_equal(rad, erad), f"{np.count_nonzero(rad != erad)} radiance values differ"
    sampler, sfilm = ctx.render_state_export()
    assert np.array_equal(sfilm, film), "exported film sums differ from the oracle"
    assert np.array_equal(sampler, seed), "exported sampler states differ from the oracle"
    if probe:
        p = ctx.pixel_probe(len(ys))
        assert np.all(p["flags"] & capi.PROBE_SEED)
        assert np.array_equal(p["seed"], seed), "probe sampler states differ from the oracle"
    assert ctx.render_state_spp_range() == (int(count.min()), int(count.max()))
    assert ctx.render_state_info()["spp_done"] == int(count.max())


FORMS = {
    "wavefront": dict(path=0, path_defer=0, path_spec=0),
    "k_path": dict(path=1, path_defer=0, path_spec=0),
    "k_path_defer": dict(path=1, path_defer=1, path_spec=0),
    "k_path_spec": dict(path=1, path_defer=0, path_spec=1),
}


def _set_form(ctx, form, order):
    """Force one render form, with the cost-ordered fetch off or forced on at every spp (as
    test_gpu_progressive.py sets them)."""
    for k, v in FORMS[form].items():
        ctx.set_option(k, v)
    ctx.set_option("path_order", (1 if form == "wavefront" else 2) if order else 0)
    ctx.set_option("path_order_pair", ((1 if form in ("k_path_defer", "k_path_spec") else 3) if order else 0))
    ctx.set_option("path_order_min_spp", 0 if order else 64)
    ctx.set_option("path_order_shift", 0)


def _masks(n):
    last = np.zeros(n, np.uint8)
    last[(n - 1) // STRIP * STRIP:] = 1
    single = np.zeros(n, np.uint8)
    single[n // 3] = 1
    return {"checker": (np.arange(n) % 3 == 0).astype(np.uint8) * 7, "zero": np.zeros(n, np.uint8),
            "ones": np.ones(n, np.uint8), "single": single, "last_short_strip": last}


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("form", list(FORMS))
def test_masked_continue_bit_exact(hip_ctx_factory, form, order):
    W, H = 40, 24
    ys, xs = slot_pixels(RAGGED, W, H)
    n = len(ys)
    assert n % STRIP != 0, "the tile list must end in a short strip"
    with hip_ctx_factory(0) as ctx:
        _set_form(ctx, form, order)
        ctx.set_option("pixel_probe", 1)
        cs, frame = _setup(ctx, "cornell40x24", lambda: cornell((W, H)))
        for name, mask in _masks(n).items():
            ctx.render(3, DEPTH, RAGGED, W, H)
            rad, w = ctx.render_continue_masked(5, mask, W, H)
            if mask.any():
                assert ctx.render_form()["form"] == form, f"{name}: the masked pass ran {ctx.render_form()['form']}"
            count = np.where(mask != 0, 8, 3)
            _check(ctx, frame, count, rad, w, ys, xs, W, H, probe=bool(mask.any()))
            rad, w = ctx.render_continue(2, W, H)   # a uniform continue, from each slot's own count
            _check(ctx, frame, count + 2, rad, w, ys, xs, W, H)


class _DeviceBytes:
    """n bytes of device memory through the HIP runtime the library already loaded."""

    def __init__(self, n):
        self.hip, self.n, self.p = C.CDLL("libamdhip64.so"), n, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(n)) == 0

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert a.size == self.n
        assert self.hip.hipMemcpy(self.p, a.ctypes.data_as(C.c_void_p), C.c_size_t(self.n), 1) == 0   # host to device

    def get(self, dtype):
        out = np.empty(self.n, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.n), 2) == 0  # device to host
        return out.view(dtype)

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def test_masked_continue_device_form(hip_ctx_factory):
    W, H = 40, 24
    ys, xs = slot_pixels(RAGGED, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as ctx:
        cs, frame = _setup(ctx, "cornell40x24", lambda: cornell((W, H)))
        d_mask, d_rad, d_w = _DeviceBytes(n), _DeviceBytes(12 * n), _DeviceBytes(4 * n)
        try:
            mask = _masks(n)["checker"]
            d_mask.put(mask)
            ctx.render_device(3, DEPTH, RAGGED, d_rad.p.value, d_w.p.value)
            d_rad.put(np.full(3 * n, np.nan, np.float32))
            assert ctx.render_continue_masked_device(5, d_mask.p.value, n, d_rad.p.value, d_w.p.value) == n
            ctx.synchronize()
            count = np.where(mask != 0, 8, 3)
            film = _expected(frame, count, ys, xs, W, H)[0]
            assert np.array_equal(d_w.get(np.float32), film[:, 3])
            assert np.array_equal(d_rad.get(np.float32).reshape(-1, 3), film[:, :3])
            with pytest.raises(capi.AkrError, match="the mask has"):
                ctx.render_continue_masked_device(1, d_mask.p.value, n - 1, d_rad.p.value, d_w.p.value)
            assert ctx.render_state_spp_range() == (3, 8)
            # a null mask is refused like the host form's: the session stays, and goes on
            with pytest.raises(capi.AkrError, match="null argument"):
                ctx.render_continue_masked_device(1, 0, n, d_rad.p.value, d_w.p.value)
            assert ctx.render_state_spp_range() == (3, 8)
            assert ctx.render_continue_masked_device(2, d_mask.p.value, n, d_rad.p.value, d_w.p.value) == n
            ctx.synchronize()
            film = _expected(frame, np.where(mask != 0, 10, 3), ys, xs, W, H)[0]
            assert np.array_equal(d_w.get(np.float32), film[:, 3])
            assert np.array_equal(d_rad.get(np.float32).reshape(-1, 3), film[:, :3])
            assert ctx.render_state_spp_range() == (3, 10)
        finally:
            ctx.synchronize()
            for d in (d_mask, d_rad, d_w):
                d.free()


def test_masked_rules(hip_ctx_factory):
    W, H = 40, 24
    ys, xs = slot_pixels(RAGGED, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as ctx:
        cs, frame = _setup(ctx, "cornell40x24", lambda: cornell((W, H)))
        mask = _masks(n)["checker"]
        with pytest.raises(capi.AkrError, match=NO_SESSION):
            ctx.render_continue_masked(1, mask, W, H)
        with pytest.raises(capi.AkrError, match=NO_SESSION):
            ctx.render_state_spp_range()
        ctx.render(3, DEPTH, RAGGED, W, H)
        for wrong in (mask[:-1], np.concatenate([mask, mask[:1]])):
            with pytest.raises(capi.AkrError, match="the mask has"):
                ctx.render_continue_masked(5, wrong, W, H)
        with pytest.raises(capi.AkrError, match="spp must be >= 0"):
            ctx.render_continue_masked(-1, mask, W, H)
        assert ctx.render_state_spp_range() == (3, 3)          # the session stays, and is usable
        rad, w = ctx.render_continue_masked(5, mask, W, H)
        count = np.where(mask != 0, 8, 3)
        _check(ctx, frame, count, rad, w, ys, xs, W, H, probe=False)
        # spp 0 returns the totals
        rad, w = ctx.render_continue_masked(0, np.ones(n, np.uint8), W, H)
        _check(ctx, frame, count, rad, w, ys, xs, W, H, probe=False)
        # a non-uniform export is refused by the import as today: its weights differ from spp
        sampler, film = ctx.render_state_export()
        with pytest.raises(capi.AkrError, match="holds weight"):
            ctx.render_state_import(8, DEPTH, RAGGED, sampler, film)
        with pytest.raises(capi.AkrError, match="holds weight"):
            ctx.render_state_import(3, DEPTH, RAGGED, sampler, film)
        assert ctx.render_state_spp_range() == (3, 8)          # refused imports change nothing
        # the 2^24 cap applies to the largest resulting count
        one = [(4, 4, 6, 5)]
        top = float(1 << 24)
        ctx.render_state_import((1 << 24) - 1, DEPTH, one, np.array([4 + 4 * W, 5 + 4 * W], np.uint32),
                                np.array([[1.0, 2.0, 3.0, top - 1], [1.0, 2.0, 3.0, top - 1]], np.float32))
        with pytest.raises(capi.AkrError, match="exceed 2\\^24"):
            ctx.render_continue_masked(2, np.array([1, 0], np.uint8), W, H)
        assert ctx.render_state_spp_range() == ((1 << 24) - 1, (1 << 24) - 1)
        rad, w = ctx.render_continue_masked(2, np.zeros(2, np.uint8), W, H)   # nothing masked: nothing exceeds
        assert w[4, 4] == top - 1 and w[4, 5] == top - 1
        rad, w = ctx.render_continue_masked(1, np.array([1, 0], np.uint8), W, H)
        assert w[4, 4] == top and w[4, 5] == top - 1
        assert ctx.render_state_spp_range() == ((1 << 24) - 1, 1 << 24)
        with pytest.raises(capi.AkrError, match="exceed 2\\^24"):
            ctx.render_continue_masked(1, np.array([1, 1], np.uint8), W, H)
        rad, w = ctx.render_continue_masked(1, np.array([0, 1], np.uint8), W, H)   # the other slot still has room
        assert w[4, 4] == top and w[4, 5] == top
        # an adaptive render leaves a session; set_camera ends it
        ctx.render_adaptive(8, DEPTH, RAGGED, W, H, 0.0, min_spp=4)
        assert ctx.render_state_info()["spp_done"] == 8
        cam = cs.camera
        ctx.set_camera(cam.position, cam.rotation, cam.fov, cam.resolution)
        for call in (lambda: ctx.render_continue_masked(1, mask, W, H), lambda: ctx.adaptive_error(),
                     lambda: ctx.adaptive_step()):
            with pytest.raises(capi.AkrError, match=NO_SESSION):
                call()


@pytest.mark.parametrize("tiles", [[(0, 0, 96, 54)], [(7, 11, 57, 14)]], ids=["96x54_81_strips", "50x3_short_last_strip"])
def test_metric_matches_restatement(hip_ctx_factory, tiles):
    W, H = 96, 54
    ys, xs = slot_pixels(tiles, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as ctx:
        cs, frame = _setup(ctx, "soup96x54", lambda: small_soup(resolution=(W, H)))
        E = strip_errors(_slot_film(frame, 4, ys, xs), _slot_film(frame, 8, ys, xs))
        assert len(E) == (n + STRIP - 1) // STRIP
        threshold = float(np.median(E))
        stop = E <= np.float32(threshold)
        print(f"{n} slots, {len(E)} strips, E in [{E.min()}, {E.max()}], threshold {threshold}, {stop.sum()} stop")
        assert 0 < stop.sum() < len(E), "the threshold must split the strips"
        rad, w, info = ctx.render_adaptive(8, DEPTH, tiles, W, H, threshold, min_spp=4)
        err, active = ctx.adaptive_error()
        assert err.dtype == np.float32 and np.array_equal(err, E), f"{np.count_nonzero(err != E)} strip errors differ"
        assert np.array_equal(active != 0, ~stop)
        assert np.all(w[ys, xs] == 8) and info["passes"] == 2 and info["strips"] == len(E)
        assert info["strips_at_cap"] == int((~stop).sum()) and info["samples"] == 8 * n


def _replay_case(frame, ys, xs, totals, threshold=None):
    films = {t: _slot_film(frame, t, ys, xs) for t in totals}
    if threshold is None:   # the median strip error of the first test: some strips stop there, some go on
        threshold = float(np.median(strip_errors(films[totals[0]], films[totals[1]])))
    return threshold, replay(films, totals, threshold)


def _check_adaptive(ctx, frame, got, count, err, active, passes, cap, ys, xs, W, H):
    rad, w, info = got
    _check(ctx, frame, count, rad, w, ys, xs, W, H)
    at_cap = int(active.sum()) if count.max() == cap else 0
    assert info == dict(passes=passes, spp_min=int(count.min()), spp_max=int(count.max()), samples=int(count.sum()),
                        strips=len(err), strips_at_cap=at_cap), info
    gerr, gactive = ctx.adaptive_error()
    assert np.array_equal(gerr, err) and np.array_equal(gactive != 0, active)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", ["cornell64_whole", "cornell40x24_ragged"])
def test_adaptive_end_to_end(hip_ctx_factory, case, form):
    if case == "cornell64_whole":
        W, H, tiles = 64, 64, [(0, 0, 64, 64)]
    else:
        W, H, tiles = 40, 24, RAGGED
    ys, xs = slot_pixels(tiles, W, H)
    with hip_ctx_factory(0) as ctx:
        _set_form(ctx, form, form in ("k_path", "k_path_spec"))
        ctx.set_option("pixel_probe", 1)
        cs, frame = _setup(ctx, f"cornell{W}x{H}", lambda: cornell((W, H)))
        # doubling from 4 to the cap 32: the replay on the oracle's films first
        totals = progressive.adaptive_totals(4, 0, 32)
        assert totals == [4, 8, 16, 32]
        threshold, (count, err, active, passes, first_stop) = _replay_case(frame, ys, xs, totals)
        n_strips = len(err)
        print(f"{case}: threshold {threshold}, {first_stop} of {n_strips} strips stop at the first test, "
              f"{int(active.sum())} are still above it at the cap, counts {np.unique(count, return_counts=True)}")
        assert 0 < first_stop < n_strips, "some strips must stop at the first test and some go on"
        assert count.max() == 32, "at least one strip must reach the cap"
        got = ctx.render_adaptive(32, DEPTH, tiles, W, H, threshold, min_spp=4)
        assert ctx.render_form()["form"] == form
        _check_adaptive(ctx, frame, got, count, err, active, passes, 32, ys, xs, W, H)
        # afterwards the session can be continued, masked and uniformly
        if case == "cornell40x24_ragged":
            mask = (np.arange(len(ys)) % 2).astype(np.uint8)
            rad, w = ctx.render_continue_masked(1, mask, W, H)
            _check(ctx, frame, count + mask, rad, w, ys, xs, W, H)
            rad, w = ctx.render_continue(1, W, H)
            _check(ctx, frame, count + mask + 1, rad, w, ys, xs, W, H)
        # passes of 4 to the cap 16
        totals = progressive.adaptive_totals(4, 4, 16)
        threshold, (count, err, active, passes, first_stop) = _replay_case(frame, ys, xs, totals)
        assert 0 < first_stop < n_strips
        got = ctx.render_adaptive(16, DEPTH, tiles, W, H, threshold, min_spp=4, pass_spp=4)
        _check_adaptive(ctx, frame, got, count, err, active, passes, 16, ys, xs, W, H)


def test_adaptive_stepwise_and_device_form(hip_ctx_factory):
    """akr_hip_adaptive_begin / _step give the one-call render's film and info, with the film readable
    between passes; so does progressive.render_adaptive with a per-pass callback, and the device form."""
    W, H, tiles = 40, 24, RAGGED
    ys, xs = slot_pixels(tiles, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        cs, frame = _setup(ctx, "cornell40x24", lambda: cornell((W, H)))
        totals = progressive.adaptive_totals(4, 0, 32)
        threshold, (count, err, active, passes, first_stop) = _replay_case(frame, ys, xs, totals)
        seen = []

        def on_pass(info, rad, w):
            seen.append((info["passes"], info["spp_max"], float(w.sum())))

        got = progressive.render_adaptive(ctx, 32, DEPTH, tiles, W, H, threshold, min_spp=4, on_pass=on_pass)
        _check_adaptive(ctx, frame, got, count, err, active, passes, 32, ys, xs, W, H)
        assert [s[:2] for s in seen] == [(k + 1, t) for k, t in enumerate(totals[:passes])]
        assert seen[0][2] == 4 * n and seen[-1][2] == count.sum()
        # a callback that stops after the second pass: the replay cut at two totals
        c2, e2, a2, p2, _ = replay({t: _slot_film(frame, t, ys, xs) for t in totals[:2]}, totals[:2], threshold)
        rad, w, info = progressive.render_adaptive(ctx, 32, DEPTH, tiles, W, H, threshold, min_spp=4,
                                                   on_pass=lambda info, rad, w: info["passes"] == 2)
        _check(ctx, frame, c2, rad, w, ys, xs, W, H)
        assert info["passes"] == 2 and info["strips_at_cap"] == 0 and info["samples"] == c2.sum()
        # a time budget that is already spent stops after the first pass
        rad, w, info = progressive.render_adaptive(ctx, 32, DEPTH, tiles, W, H, threshold, min_spp=4, time_budget=0.0)
        _check(ctx, frame, np.full(n, 4), rad, w, ys, xs, W, H)
        # a continue that draws samples ends the adaptive run but keeps the session
        ctx.render_continue(1, W, H)
        with pytest.raises(capi.AkrError, match="not an adaptive render in progress"):
            ctx.adaptive_step()
        assert ctx.render_state_spp_range() == (5, 5)
        # the device form
        d_rad, d_w = _DeviceBytes(12 * n), _DeviceBytes(4 * n)
        try:
            npx, info = ctx.render_adaptive_device(32, DEPTH, tiles, d_rad.p.value, d_w.p.value, threshold, min_spp=4)
            ctx.synchronize()
            film = _expected(frame, count, ys, xs, W, H)[0]
            assert npx == n and info["samples"] == count.sum() and info["passes"] == passes
            assert np.array_equal(d_w.get(np.float32), film[:, 3])
            assert np.array_equal(d_rad.get(np.float32).reshape(-1, 3), film[:, :3])
        finally:
            ctx.synchronize()
            d_rad.free()
            d_w.free()


def test_adaptive_edges(hip_ctx_factory):
    W, H, tiles = 40, 24, RAGGED
    ys, xs = slot_pixels(tiles, W, H)
    n = len(ys)
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        cs, frame = _setup(ctx, "cornell40x24", lambda: cornell((W, H)))
        # threshold 0: only strips with E == 0 stop
        totals = progressive.adaptive_totals(4, 0, 16)
        _, (count, err, active, passes, _) = _replay_case(frame, ys, xs, totals, threshold=0.0)
        got = ctx.render_adaptive(16, DEPTH, tiles, W, H, 0.0, min_spp=4)
        _check_adaptive(ctx, frame, got, count, err, active, passes, 16, ys, xs, W, H)
        assert np.array_equal(np.repeat(err == 0, STRIP)[:n], count < 16)
        # threshold +inf: every slot ends with exactly the second total
        got = ctx.render_adaptive(16, DEPTH, tiles, W, H, float("inf"), min_spp=4)
        _, (count, err, active, passes, _) = _replay_case(frame, ys, xs, totals, threshold=np.inf)
        assert np.all(count == 8) and passes == 2 and not active.any()
        _check_adaptive(ctx, frame, got, count, err, active, passes, 16, ys, xs, W, H)
        # a cap equal to (and below) min_spp: a plain render, no test
        for cap, min_spp in ((4, 4), (3, 8)):
            rad, w, info = ctx.render_adaptive(cap, DEPTH, tiles, W, H, 0.0, min_spp=min_spp)
            _check(ctx, frame, np.full(n, cap), rad, w, ys, xs, W, H)
            assert info == dict(passes=1, spp_min=cap, spp_max=cap, samples=cap * n, strips=(n + 63) // 64, strips_at_cap=0)
            with pytest.raises(capi.AkrError, match="ran no convergence test"):
                ctx.adaptive_error()
        # a cap that makes the last pass short: 4, 8, 10
        totals = progressive.adaptive_totals(4, 0, 10)
        assert totals == [4, 8, 10]
        threshold, (count, err, active, passes, first_stop) = _replay_case(frame, ys, xs, totals)
        assert 0 < first_stop < len(err)
        got = ctx.render_adaptive(10, DEPTH, tiles, W, H, threshold, min_spp=4)
        _check_adaptive(ctx, frame, got, count, err, active, passes, 10, ys, xs, W, H)
        # fewer slots than one strip
        small = [(3, 3, 10, 8)]
        sy, sx = slot_pixels(small, W, H)
        assert len(sy) == 35
        totals = progressive.adaptive_totals(4, 0, 16)
        threshold, (count, err, active, passes, _) = _replay_case(frame, sy, sx, totals)
        got = ctx.render_adaptive(16, DEPTH, small, W, H, threshold, min_spp=4)
        _check_adaptive(ctx, frame, got, count, err, active, passes, 16, sy, sx, W, H)
        # refused parameters leave the session alone
        for kw, message in ((dict(threshold=float("nan")), "threshold"), (dict(threshold=-1.0), "threshold"),
                            (dict(threshold=0.1, min_spp=0), "min_spp"), (dict(threshold=0.1, pass_spp=-1), "pass_spp")):
            kw = dict(dict(min_spp=4), **kw)
            with pytest.raises(capi.AkrError, match=message):
                ctx.render_adaptive(16, DEPTH, small, W, H, kw.pop("threshold"), **kw)
        assert ctx.render_state_info()["n_pixels"] == 35


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 16, max_depth: 4, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def _pfm(path, W, H):
    raw = path.read_bytes()
    return np.frombuffer(raw[raw.index(b"-1.0\n") + 5:], np.float32).reshape(H, W, 3)[::-1]


def test_cli_adaptive(tmp_path):
    """--adaptive writes the image and the --spp-map, which equal the library call's film and weights;
    with --checkpoint it exits non-zero with the message."""
    path = tmp_path / "box.akari"
    path.write_text(SDL.format(out=tmp_path / "default.pfm", mesh=CORNELL_MESH))
    code = ("import sys; sys.path[:0] = [%r]; from akari_amd import render; sys.exit(render.main(sys.argv[1:]))"
            % str(ROOT / "akarirender-1_amd"))
    out, spp_map = tmp_path / "image.pfm", tmp_path / "spp.pfm"
    sc = scene.load_scene_file(str(path))
    cs = scene.compile_scene(sc)
    with capi.HipContext(0) as ctx:
        scene.upload_scene(ctx, cs)
        # the threshold: the median strip error of the first test (threshold +inf runs exactly that test)
        ctx.render_adaptive(16, 4, render._tiles(sc, 16), 40, 24, float("inf"), min_spp=4)
        threshold = repr(float(np.median(ctx.adaptive_error()[0])))
        rad, w, info = ctx.render_adaptive(16, 4, render._tiles(sc, 16), 40, 24, float(threshold), min_spp=4)
    r = subprocess.run([sys.executable, "-c", code, str(path), "--adaptive", threshold, "--min-spp", "4", "--out", str(out),
                        "--spp-map", str(spp_map), "--preview"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "pass 1 to 4 spp" in r.stdout
    print(f"CLI adaptive: {info}")
    assert info["spp_min"] < info["spp_max"], "the threshold must leave a non-uniform film"
    got = _pfm(spp_map, 40, 24)
    assert np.array_equal(got[..., 0], w) and np.array_equal(got[..., 1], w) and np.array_equal(got[..., 2], w)
    assert np.array_equal(_pfm(out, 40, 24), rad / w[..., None])
    r = subprocess.run([sys.executable, "-c", code, str(path), "--adaptive", threshold, "--checkpoint",
                        str(tmp_path / "c.npz")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "cannot be combined with --checkpoint" in r.stderr
    assert not (tmp_path / "c.npz").exists()


def test_cpp_adapter_adaptive(tmp_path):
    exe = tmp_path / "adaptive_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "adaptive_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "strips=3" in r.stdout and "errors=3" in r.stdout
