"""Host side of multiple importance sampling of lights: the restatement against its
goldens, the power heuristic, the expectation and the variance of the two estimators restated on the CPU, and
the parser, command line and checkpoint.  No GPU needed."""
import json
import multiprocessing as mp
import sys

import numpy as np
import pytest

from akari_amd import progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN
from helpers import cornell
from test_progressive_host import SDL, TILES, _checkpoint

sys.path.insert(0, str(GOLDEN))
import make_env_golden as ME  # noqa: E402
import make_mis_golden as MM  # noqa: E402
import mis_restate as S  # noqa: E402
import ref_restate as R  # noqa: E402

F = np.float32
BLOCK = (10, 10, 14, 14)   # the block the restatement is run on again, as make_path_golden's


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(MM.CONFIGS))
def test_restatement_reproduces_committed_goldens(name):
    """The goldens cannot drift from the restatement: a 4 x 4 block of every configuration, run again."""
    g = np.load(GOLDEN / f"mis_golden_{name}.npz")
    assert json.loads(str(g["configs"])) == [list(c) for c in MM.CONFIGS[name]]
    x0, y0, x1, y1 = BLOCK
    px = [(x, y) for y in range(y0, y1) for x in range(x0, x1)]
    for key, env_on, sp, depth, clamp in MM.CONFIGS[name]:
        sc = R.RefScene(MM.build_scene(name, key, sp))
        env = ME.restated_env(name, sp) if env_on else None
        out, _ = MM.render_pixels(sc, env, px, MM.SPP, depth, clamp, parallel=False)
        sel = (slice(y0, y1), slice(x0, x1))
        assert np.array_equal(bits(out["radiance"]).reshape(4, 4, 3), bits(g[key + "_radiance"][sel])), (name, key)
        assert np.array_equal(out["seed"].reshape(4, 4), g[key + "_seed"][sel]), (name, key)
        assert np.array_equal(out["closest"].reshape(4, 4), g[key + "_closest"][sel]), (name, key)
        assert np.array_equal(out["shadow"].reshape(4, 4), g[key + "_shadow"][sel]), (name, key)
        assert np.all(g[key + "_weight"] == MM.SPP)


def test_golden_set_takes_every_new_branch_and_keeps_seeds_and_counts():
    total = {}
    for name in MM.CONFIGS:
        g = np.load(GOLDEN / f"mis_golden_{name}.npz")
        for k, v in json.loads(str(g["counts"])).items():
            total[k] = total.get(k, 0) + v
        for key, env_on, *_ in MM.CONFIGS[name]:
            old = MM.existing(name, key, env_on)
            if old is not None:   # no draw added or moved, no ray added or removed
                for a, k in zip(old, ("seed", "closest", "shadow")):
                    assert np.array_equal(a, g[f"{key}_{k}"]), (name, key, k)
    assert all(total.get(b, 0) >= 1 for b in MM.REQUIRED_BRANCHES), total


def test_power_weights_sum_to_one():
    """w(a, b) + w(b, a) = 1 to one ulp of 1, on a grid with inf and tiny values; w(a, inf) = 0."""
    grid = [F(v) for v in (1e-38, 1e-30, 1e-12, 1e-3, 0.25, 0.5, 1.0, 2.9005864, 2.9006042, 7.0, 1e3, 1e12, 1e30, 3e38)]
    worst = 0.0
    for a in grid:
        assert S.power_weight(a, F(np.inf)) == 0 and S.power_weight(F(np.inf), a) == 1
        for b in grid:
            wa, wb = S.power_weight(a, b), S.power_weight(b, a)
            assert wa.dtype == np.float32 and 0 <= wa <= 1
            worst = max(worst, abs(float(wa) + float(wb) - 1.0))
    assert worst <= 2.0 ** -23, worst
    assert S.power_weight(F(1.0), F(1.0)) == F(0.5)


# ----------------------------------------------------------------------------- expectation and variance
_G = {}


def _samples(args):
    x, y, mis = args
    out = []
    S.render_pixel(_G["sc"], _G["env"], x, y, _G["spp"], _G["depth"], 0.0, None, mis=mis, samples=out)
    return np.array(out, np.float64)


_BOTH = {}


def both_estimators():
    """`cornell` with its map, 4 x 4 at 4,096 spp, max_depth 3, restated with the switch off and on (about ten
    seconds on 16 cores) -> per-sample radiance [2, 16 pixels, spp, 3], computed once."""
    if not _BOTH:
        sc = R.RefScene(ME.build_scene("cornell", (4, 4)))
        sc._mis_tri_sel = S.tri_select_pdf(sc)
        _G.update(sc=sc, env=ME.restated_env("cornell"), spp=4096, depth=3)
        jobs = [(x, y, mis) for mis in (False, True) for y in range(4) for x in range(4)]
        with mp.get_context("fork").Pool(min(16, mp.cpu_count())) as pool:
            res = pool.map(_samples, jobs, chunksize=1)
        _BOTH["s"] = np.array(res).reshape(2, 16, 4096, 3)
    return _BOTH["s"]


def test_expectation_of_the_two_estimators_agrees():
    """Frame means within 4 standard errors of their difference, every pixel-channel within 5; each
    estimator's variance comes from its own per-sample second moments."""
    s = both_estimators()
    spp = s.shape[2]
    frame = s.mean(axis=(1, 3))                       # [2, spp]: the frame mean of each sample index
    se = np.sqrt(frame[0].var(ddof=1) / spp + frame[1].var(ddof=1) / spp)
    z_frame = (frame[1].mean() - frame[0].mean()) / se
    mean, var = s.mean(axis=2), s.var(axis=2, ddof=1)  # [2, 16, 3]
    se_pc = np.sqrt((var[0] + var[1]) / spp)
    z = (mean[1] - mean[0]) / se_pc
    print(f"frame means {frame[0].mean():.5f} (today) {frame[1].mean():.5f} (mis): {z_frame:+.2f} standard errors; "
          f"largest pixel-channel difference {np.abs(z).max():.2f} standard errors")
    assert abs(z_frame) <= 4, z_frame
    assert np.abs(z).max() <= 5, np.abs(z).max()


def test_variance_with_mis_is_below_todays():
    s = both_estimators()
    var = s.var(axis=2, ddof=1).sum(axis=(1, 2))      # per-pixel variance, summed over the frame
    print(f"per-pixel variance, mis against today's estimator: ratio {var[1] / var[0]:.3f}")
    assert var[1] / var[0] < 1


# ----------------------------------------------------------------------------- parser, command line, checkpoint
def test_parser_reads_mis_in_the_path_node(tmp_path):
    def load(integrator):
        p = tmp_path / "s.akari"
        p.write_text(SDL.format(integrator=integrator, out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
        return scene.load_scene_file(p).integrator
    assert scene.PathIntegrator().mis is False
    assert load("Path { spp: 4, max_depth: 3 }").mis is False
    assert load("Path { spp: 4, max_depth: 3, mis: true }").mis is True
    assert load("Path { spp: 4, mis: false }").mis is False
    with pytest.raises(Exception, match="mis needs true or false"):
        load("Path { spp: 4, mis: 3 }")


def test_checkpoint_fingerprint_carries_the_switch():
    cs = scene.compile_scene(cornell((32, 24)))
    assert progressive.scene_fingerprint(cs, False) == progressive.scene_fingerprint(cs)
    assert progressive.scene_fingerprint(cs, True) != progressive.scene_fingerprint(cs)
    ck = _checkpoint(cs)                               # rendered without the switch
    ck.check(cs, TILES, 32, 24)
    with pytest.raises(progressive.CheckpointError, match="rendered with mis off"):
        ck.check(cs, TILES, 32, 24, mis=True)
    with pytest.raises(progressive.CheckpointError, match="rendered with mis off"):
        ck.restore(None, cs, TILES, mis=True)         # checked before the context is touched
    ck.fingerprint = progressive.scene_fingerprint(cs, True)
    ck.check(cs, TILES, 32, 24, mis=True)
    with pytest.raises(progressive.CheckpointError, match="rendered with mis on"):
        ck.check(cs, TILES, 32, 24)


def test_adapter_set_mis_compiles_and_links(tmp_path):
    import subprocess
    from akari_amd import capi
    from conftest import ROOT
    exe, lib = tmp_path / "mis_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "mis_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # without "run" it touches no device


def test_cli_refusals_need_no_gpu(tmp_path, capsys):
    path, ao = tmp_path / "s.akari", tmp_path / "ao.akari"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    ao.write_text(SDL.format(integrator="AO { spp: 4 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            render.main([str(a) for a in argv])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err, err

    refused([ao, "--mis"], "--mis needs the Path integrator; the scene's is AOIntegrator")
    # a checkpoint of the same scene rendered without the switch is refused before the upload, and the other way
    sc = scene.load_scene_file(path)
    cs = scene.compile_scene(sc)
    tiles = render._tiles(sc, sc.integrator.tile_size)
    for saved, flags, message in ((False, ["--mis"], "rendered with mis off"), (True, [], "rendered with mis on")):
        ck = _checkpoint(cs, tiles=tiles, spp=2)
        ck.max_depth, ck.ray_clamp = 3, float(np.float32(sc.integrator.ray_clamp))
        ck.fingerprint = progressive.scene_fingerprint(cs, saved)
        ck.save(tmp_path / "c.npz")
        refused([path, "--resume", tmp_path / "c.npz", *flags], message)
    assert not (tmp_path / "o.pfm").exists()
