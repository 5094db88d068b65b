"""Host side of adaptive sampling: the schedule, the argument checks, the CLI's
refusals, the NumPy restatement of the convergence test that the GPU tests compare against, and the
C++ adapter's new calls.  No GPU needed."""
import subprocess

import numpy as np
import pytest

from akari_amd import capi, progressive, render
from conftest import CORNELL_MESH, ROOT

f32 = np.float32
STRIP = 64


def strip_errors(prev, film):
    """The convergence test of include/akr_hip.h restated in NumPy f32: prev and film are [n, 4] per-slot
    (r, g, b sums, count) before and after the pass being judged; returns each strip's error E."""
    prev, film = np.asarray(prev, f32), np.asarray(film, f32)
    assert prev.shape == film.shape and prev.dtype == film.dtype == f32
    with np.errstate(all="ignore"):
        m1 = film[:, :3] / film[:, 3:4]
        m0 = prev[:, :3] / prev[:, 3:4]
        d = np.abs(m1[:, 0] - m0[:, 0])
        d = d + np.abs(m1[:, 1] - m0[:, 1])
        d = d + np.abs(m1[:, 2] - m0[:, 2])
        s = m1[:, 0] + m1[:, 1]
        s = s + m1[:, 2]
        e = np.where(s > 0, d / np.sqrt(s), f32(0))
    assert e.dtype == f32
    n = len(e)
    n_strips = (n + STRIP - 1) // STRIP
    tree = np.zeros(n_strips * STRIP, f32)   # absent slots of a short last strip count 0
    tree[:n] = e
    tree = tree.reshape(n_strips, STRIP)
    while tree.shape[1] > 1:                 # adjacent pairs, six levels
        tree = tree[:, 0::2] + tree[:, 1::2]
    slots = np.minimum(STRIP, n - STRIP * np.arange(n_strips)).astype(f32)
    with np.errstate(all="ignore"):
        out = tree[:, 0] / slots
    assert out.dtype == f32
    return out


def replay(films, totals, threshold):
    """The adaptive loop on whole films: films[t] is the [n, 4] per-slot film of a uniform t-spp render,
    totals the counts an active slot passes through.  Returns (count per slot, error per strip, active
    per strip, passes, strips stopped at the first test)."""
    n = len(films[totals[0]])
    n_strips = (n + STRIP - 1) // STRIP
    active = np.ones(n_strips, bool)
    err = np.zeros(n_strips, f32)
    count = np.full(n, totals[0], np.int64)
    passes, first_stop = 1, None
    for before, t in zip(totals, totals[1:]):
        if not active.any():
            break
        count[np.repeat(active, STRIP)[:n]] = t
        passes += 1
        E = strip_errors(films[before], films[t])
        err[active] = E[active]
        still = active & ~(E <= f32(threshold))   # NaN keeps sampling
        if first_stop is None:
            first_stop = int(active.sum() - still.sum())
        active = still
    return count, err, active, passes, first_stop


def test_adaptive_totals():
    at = progressive.adaptive_totals
    assert at(4, 0, 32) == [4, 8, 16, 32]
    assert at(4, 0, 20) == [4, 8, 16, 20]            # the last pass is short
    assert at(4, 4, 16) == [4, 8, 12, 16]
    assert at(4, 5, 16) == [4, 9, 14, 16]
    assert at(16, 0, 16) == [16] and at(16, 0, 7) == [7] and at(1, 0, 0) == [0]
    assert at(1, 0, 5) == [1, 2, 4, 5]
    for bad in ((0, 0, 8), (-1, 0, 8), (4, -1, 8), (4, 0, -1)):
        with pytest.raises(ValueError):
            at(*bad)


def test_adaptive_argument_checks():
    ok = progressive.check_adaptive_args
    ok(0.0, 1, 0, 8)
    ok(float("inf"), 16, 4, 1 << 24)
    with pytest.raises(ValueError, match="threshold"):
        ok(float("nan"), 4, 0, 8)
    with pytest.raises(ValueError, match="threshold"):
        ok(-0.5, 4, 0, 8)
    with pytest.raises(ValueError, match="min_spp"):
        ok(0.1, 0, 0, 8)
    with pytest.raises(ValueError, match="pass_spp"):
        ok(0.1, 4, -2, 8)
    with pytest.raises(ValueError, match="2\\^24"):
        ok(0.1, 4, 0, (1 << 24) + 1)
    # render_adaptive refuses them before it touches the context
    with pytest.raises(ValueError, match="threshold"):
        progressive.render_adaptive(None, 8, 5, [(0, 0, 4, 4)], 4, 4, float("nan"))
    # the structs the bindings pass match the header's layout
    import ctypes as C
    assert C.sizeof(capi.AdaptiveParams) == 16 and C.sizeof(capi.AdaptiveInfo) == 40
    for name in ("akr_hip_render_continue_masked", "akr_hip_render_continue_masked_device",
                 "akr_hip_render_state_spp_range", "akr_hip_render_adaptive", "akr_hip_render_adaptive_device",
                 "akr_hip_adaptive_error", "akr_hip_adaptive_begin", "akr_hip_adaptive_step"):
        assert name in capi.EXPORTS
        assert hasattr(capi.load_library(), name), f"{name} is not exported by the library"


def test_metric_restatement_on_hand_made_films():
    n = 150   # two whole strips and a short one of 22
    zero0 = np.zeros((n, 4), f32)
    zero0[:, 3] = 4
    zero1 = zero0.copy()
    zero1[:, 3] = 8
    assert np.array_equal(strip_errors(zero0, zero1), np.zeros(3, f32))      # a zero film: s is not > 0
    const0 = np.tile(f32([2.0, 4.0, 6.0, 4.0]), (n, 1))
    const1 = np.tile(f32([4.0, 8.0, 12.0, 8.0]), (n, 1))
    assert np.array_equal(strip_errors(const0, const1), np.zeros(3, f32))    # the same means: d is 0
    # a known case: means (1, 1, 1) before, (1.5, 1, 0.5) after in slots 0, 64 and 128 only:
    # d = 0.5 + 0 + 0.5 = 1, s = 3, e = 1 / sqrt(3); E = e / 64, e / 64, e / 22
    prev = np.tile(f32([4.0, 4.0, 4.0, 4.0]), (n, 1))
    film = np.tile(f32([8.0, 8.0, 8.0, 8.0]), (n, 1))
    film[[0, 64, 128], :3] = f32([12.0, 8.0, 4.0])
    e = f32(1.0) / np.sqrt(f32(3.0))
    want = np.array([e / f32(64), e / f32(64), e / f32(22)], f32)
    got = strip_errors(prev, film)
    assert got.dtype == f32 and np.array_equal(got, want)
    # the tree's first level adds neighbours: slots 0 and 1 (64 and 65) give e + e before anything else
    film[[1, 65], :3] = f32([12.0, 8.0, 4.0])
    assert np.array_equal(strip_errors(prev, film)[:2], np.array([(e + e) / f32(64)] * 2, f32))
    # an infinite sum gives e = inf / inf = NaN, which is not <= any threshold: the strip stays active
    nan_film = film.copy()
    nan_film[0, 0] = np.inf
    count, err, active, passes, first_stop = replay({4: prev, 8: nan_film}, [4, 8], np.inf)
    assert np.isnan(err[0]) and active.tolist() == [True, False, False] and first_stop == 2 and passes == 2
    assert np.all(count == 8)


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: {integrator},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def test_cli_adaptive_flag_validation_needs_no_gpu(tmp_path, capsys):
    path = tmp_path / "s.akari"
    ao = tmp_path / "ao.akari"
    path.write_text(SDL.format(integrator="Path { spp: 8, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    ao.write_text(SDL.format(integrator="AO { spp: 4 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            render.main([str(a) for a in argv])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err, err

    refused([path, "--adaptive", "0.1", "--checkpoint", tmp_path / "c.npz"], "cannot be combined with --checkpoint")
    refused([path, "--adaptive", "0.1", "--resume", tmp_path / "c.npz"], "cannot be combined with --checkpoint")
    refused([path, "--adaptive", "-1"], "threshold >= 0")
    refused([path, "--adaptive", "nan"], "threshold >= 0")
    refused([path, "--adaptive", "0.1", "--min-spp", "0"], "at least one sample")
    refused([path, "--adaptive", "0.1", "--gpus", "2"], "render on one GPU")
    refused([path, "--adaptive", "0.1", "--pass-spp", "0"], "at least one sample per pass")
    refused([path, "--spp-map", tmp_path / "m.pfm"], "--spp-map needs --adaptive")
    refused([ao, "--adaptive", "0.1"], "need the Path integrator; the scene's is AOIntegrator")
    assert not (tmp_path / "o.pfm").exists()


def test_adapter_adaptive_calls_compile(tmp_path):
    exe = tmp_path / "adaptive_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "adaptive_demo.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # no argument: nothing touches a device
