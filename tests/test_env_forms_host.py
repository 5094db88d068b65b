"""Host side of option "env_forms" (DESIGN.md section 0.8): the option and what it does to the render plan by
a small g++ program (tests/cpp/env_forms_check.cpp), the adapter's call, the command line, the documents and
the checkpoint fingerprint.  No GPU needed."""
import inspect
import json
import subprocess

import numpy as np
import pytest

from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from helpers import cornell
from test_plan_host import case_line, parse_plan
from test_progressive_host import SDL

CSRC = ROOT / "akarirender-1_amd" / "csrc"


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("env_forms_check") / "env_forms_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "env_forms_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_option_refusals_and_table(check_exe):
    r = subprocess.run([str(check_exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 80, r.stdout   # every check ran


def test_plans_under_an_environment_are_the_pinned_ones(check_exe):
    """With an environment, env_path 1 and env_forms 1 the render builds its PathPlanIn with plain_only false, so
    plan_path() returns the plans committed for renders without an environment, field for field."""
    cases = json.loads((GOLDEN / "path_plan_cases.json").read_text())["cases"]
    assert len(cases) >= 40
    feed = "\n".join(case_line(c) + " env_path=1 env_forms=1" for c in cases) + "\n"
    out = subprocess.run([str(check_exe), "plans"], input=feed, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    kinds = set()
    for c, line in zip(cases, lines):
        plan = parse_plan(line)
        assert plan.pop("plain_only") == 0, c["name"]
        assert plan == c["plan"], (c["name"], c["plan"], plan)
        kinds |= {l["kind"] for l in plan["launch"]}
    assert kinds == {0, 1, 2}   # every form is reached


def test_plans_refuse_a_case_without_the_switches(check_exe):
    out = subprocess.run([str(check_exe), "plans"], input="64 64 16 5 0 0 1 1 8 8 8 256 env_path=1\n", capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 2 and "env_forms=1" in out.stdout
    out = subprocess.run([str(check_exe), "plans"], input="64 64 16 5 0 0 1 1 8 8 8 256 env_path=1 env_forms=2\n",
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "env_forms must be in [0, 1]" in out.stdout


def test_adapter_set_env_forms_compiles_and_links(tmp_path):
    exe, lib = tmp_path / "env_forms_demo", capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "env_forms_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0   # without "run" it touches no device


def test_header_guide_and_readme_name_the_option():
    header = (ROOT / "include" / "akr_hip.h").read_text()
    comment = header[header.index("int akr_hip_set_option("):header.index("int akr_hip_upload_mesh(")]
    assert '"env_forms"' in comment and "only k_path has one" not in comment
    assert "#define AKR_HIP_API_VERSION 3" in header
    guide = (ROOT / "INTEGRATION.md").read_text()
    assert "env_forms" in guide and "set_env_forms" in guide
    readme = (ROOT / "README.md").read_text()
    assert "--env-forms" in readme and "env_forms" in readme
    assert "set_env_forms" in (CSRC / "akari_hip.hpp").read_text()


def test_checkpoint_fingerprint_does_not_carry_the_option():
    assert "env_forms" not in inspect.signature(progressive.scene_fingerprint).parameters
    assert "env_forms" not in inspect.signature(progressive.Checkpoint.restore).parameters
    assert "env_forms" not in inspect.signature(progressive.Checkpoint.capture).parameters
    assert not any("env_forms" in n for n in vars(scene.PathIntegrator()))   # and no scene-file syntax
    cs = scene.compile_scene(cornell((32, 24)))
    assert progressive.scene_fingerprint(cs, False) == progressive.scene_fingerprint(cs)


class RecordingContext:
    """Records the options a run sets; renders a black film."""
    made = []

    def __init__(self, device=0):
        self.device, self.options = device, []
        RecordingContext.made.append(self)

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
def recording_device(monkeypatch):
    RecordingContext.made = []
    monkeypatch.setattr(capi, "HipContext", RecordingContext)
    monkeypatch.setattr(scene, "upload_scene", lambda ctx, cs, **kw: None)
    monkeypatch.setattr(capi, "render_node", lambda ctxs, spp, d, tiles, w, h, **kw: ctxs[0].render(spp, d, tiles, w, h))
    monkeypatch.setattr(progressive, "render_progressive",
                        lambda ctx, spp, d, tiles, w, h, **kw: (*ctx.render(spp, d, tiles, w, h), spp))
    monkeypatch.setattr(progressive, "render_adaptive",
                        lambda ctx, spp, d, tiles, w, h, thr, **kw: (*ctx.render(spp, d, tiles, w, h),
                                                                     dict(spp_min=spp, spp_max=spp, samples=spp * w * h, passes=1)))
    return RecordingContext


def values(ctxs, key):
    return [[v for k, v in c.options if k == key] for c in ctxs]


def scene_file(tmp_path):
    path = tmp_path / "s.akari"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    return path


@pytest.mark.parametrize("flags,n_ctx", [([], 1), (["--gpus", "2"], 2), (["--pass-spp", "2"], 1),
                                         (["--adaptive", "0.1", "--min-spp", "2"], 1)])
def test_cli_sets_the_option_on_every_context(tmp_path, recording_device, flags, n_ctx):
    """--env-forms reaches every context the run renders with, whichever driver runs, --gpus 2 shares included;
    without the flag the option is never set, so the options such a run sets are the ones it set before."""
    path = scene_file(tmp_path)
    assert render.main([str(path), *flags, "--env-path", "--env-forms"]) == 0
    assert len(recording_device.made) == n_ctx
    assert values(recording_device.made, "env_forms") == [[1]] * n_ctx, recording_device.made[0].options
    assert values(recording_device.made, "env_path") == [[1]] * n_ctx
    with_flag = [c.options for c in recording_device.made]
    for extra in (["--env-path"], []):
        recording_device.made = []
        assert render.main([str(path), *flags, *extra]) == 0
        assert len(recording_device.made) == n_ctx
        assert values(recording_device.made, "env_forms") == [[]] * n_ctx, recording_device.made[0].options
        if extra:   # the flag adds its one option and changes no other
            assert [[kv for kv in o if kv[0] != "env_forms"] for o in with_flag] == [c.options for c in recording_device.made]
    assert (tmp_path / "o.pfm").exists()


def test_cli_refuses_env_forms_without_env_path(tmp_path, recording_device, capsys):
    path = scene_file(tmp_path)
    with pytest.raises(SystemExit) as e:
        render.main([str(path), "--env-forms"])
    assert e.value.code not in (0, None)
    assert "--env-forms needs --env-path" in capsys.readouterr().err
    assert recording_device.made == []   # refused before a device is touched
    assert not (tmp_path / "o.pfm").exists()


def test_render_scene_takes_the_option_as_an_argument(recording_device):
    for kw, want in ((dict(env_path=True, env_forms=True), [[1], [1]]), (dict(env_path=True), [[], []]), ({}, [[], []])):
        recording_device.made = []
        render.render_scene(cornell((8, 8)), devices=[0, 1], **kw)
        assert values(recording_device.made, "env_forms") == want
