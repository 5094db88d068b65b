"""Host side of option "env_path" (DESIGN.md section 3.17): the option and PathPlanIn::plain_only by a small
g++ program (tests/cpp/env_path_check.cpp), the adapter's call, the command line and the checkpoint
fingerprint.  No GPU needed."""
import subprocess

import numpy as np
import pytest

from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH, ROOT
from helpers import cornell
from test_progressive_host import SDL

CSRC = ROOT / "akarirender-1_amd" / "csrc"


def test_option_and_plain_only_plan(tmp_path):
    exe = tmp_path / "env_path_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "env_path_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 90, r.stdout   # every check ran


def test_adapter_set_env_path_compiles_and_links(tmp_path):
    exe, lib = tmp_path / "env_path_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "env_path_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # without "run" it touches no device


def test_header_and_guide_name_the_switch():
    header = (ROOT / "include" / "akr_hip.h").read_text()
    assert '"env_path"' in header[header.index("int akr_hip_set_option("):header.index("int akr_hip_upload_mesh(")]
    assert "env_path" in (ROOT / "INTEGRATION.md").read_text()
    assert "set_env_path" in (ROOT / "INTEGRATION.md").read_text()


def test_checkpoint_fingerprint_does_not_carry_the_switch():
    """The bits are the same either way, so a checkpoint rendered with one value continues with the other: the
    fingerprint has no parameter for it."""
    import inspect
    assert "env_path" not in inspect.signature(progressive.scene_fingerprint).parameters
    assert "env_path" not in inspect.signature(progressive.Checkpoint.restore).parameters
    assert not any("env_path" in n for n in vars(scene.PathIntegrator()))   # and no scene-file syntax
    cs = scene.compile_scene(cornell((32, 24)))
    assert progressive.scene_fingerprint(cs, False) == progressive.scene_fingerprint(cs)


class FakeContext:
    """Records the options a run sets; renders a black film."""
    made = []

    def __init__(self, device=0):
        self.device, self.options = device, []
        FakeContext.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def close(self):
        pass

    def set_option(self, key, value):
        self.options.append((key, value))

    def render(self, spp, max_depth, tiles, w, h, **kw):
        return np.zeros((h, w, 3), np.float32), np.full((h, w), float(spp), np.float32)


@pytest.fixture()
def fake_device(monkeypatch):
    FakeContext.made = []
    monkeypatch.setattr(capi, "HipContext", FakeContext)
    monkeypatch.setattr(scene, "upload_scene", lambda ctx, cs, **kw: None)
    monkeypatch.setattr(capi, "render_node", lambda ctxs, spp, d, tiles, w, h, **kw: ctxs[0].render(spp, d, tiles, w, h))
    monkeypatch.setattr(progressive, "render_progressive",
                        lambda ctx, spp, d, tiles, w, h, **kw: (*ctx.render(spp, d, tiles, w, h), spp))
    monkeypatch.setattr(progressive, "render_adaptive",
                        lambda ctx, spp, d, tiles, w, h, thr, **kw: (*ctx.render(spp, d, tiles, w, h),
                                                                     dict(spp_min=spp, spp_max=spp, samples=spp * w * h, passes=1)))
    return FakeContext


def switch_values(ctxs):
    return [[v for k, v in c.options if k == "env_path"] for c in ctxs]


@pytest.mark.parametrize("flags,n_ctx", [([], 1), (["--gpus", "2"], 2), (["--pass-spp", "2"], 1), (["--adaptive", "0.1", "--min-spp", "2"], 1)])
def test_cli_sets_the_switch_on_every_context(tmp_path, fake_device, flags, n_ctx):
    """--env-path reaches every context the run renders with, whichever driver runs; without the flag the
    option is set to 0 there; and with no environment in the scene the flag is accepted all the same."""
    path = tmp_path / "s.akari"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    assert scene.load_scene_file(path).environment is None
    for extra, want in ((["--env-path"], 1), ([], 0)):
        fake_device.made = []
        assert render.main([str(path), *flags, *extra]) == 0
        assert len(fake_device.made) == n_ctx
        assert switch_values(fake_device.made) == [[want]] * n_ctx, fake_device.made[0].options
    assert (tmp_path / "o.pfm").exists()


def test_cli_env_path_with_an_environment_file(tmp_path, fake_device):
    from akari_amd import film
    sky = np.full((4, 8, 3), 0.5, np.float32)
    film.write_pfm(tmp_path / "sky.pfm", sky, np.ones(sky.shape[:2], np.float32))
    path = tmp_path / "s.akari"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    assert render.main([str(path), "--env", str(tmp_path / "sky.pfm"), "--env-res", "8", "--env-path"]) == 0
    assert switch_values(fake_device.made) == [[1]]
