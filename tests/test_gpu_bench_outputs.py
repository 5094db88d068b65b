"""bench.py on one GPU, plain and --full, on a toy soup: --steps sets the timed steps, the line holds
ms_per_step, a plain run leaves what takes runs of its own to --full, and --dump-outputs writes the
film of the timed render: bit for bit what a caller gets from akr_hip_render of the same scene, tiles
and spp (packed tile order), from identical inputs in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from akari_amd import capi, dist, scene
from conftest import ROOT
from helpers import slot_pixels

TRIS, W, H, TILE, STEPS, FRAME_SPP, DEPTH = 20_000, 96, 54, 32, 3, 4, 5   # 3 steps x 2 spp, 3 x 2 tiles (clipped)
FULL_ONLY = ("roofline", "kernels", "wavefront", "cpu_baseline", "configs")


@pytest.fixture(scope="module")
def expected_film(hip_ctx_factory):
    """The caller's view: one akr_hip_render of the same scene with the benchmark's build parameters."""
    import argparse
    spp = STEPS * -(-FRAME_SPP // STEPS)
    cs = scene.compile_scene(scene.soup_scene(n_tris=TRIS, resolution=(W, H)))
    kw, _ = bench.build_params(argparse.Namespace(leaf=4, sah_isect=4.0, bins=32, builder="sbvh", spatial_budget=0.0),
                               capi, 1)
    tiles = dist.tile_grid(W, H, TILE)
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, cs, **kw)
        rad, w = ctx.render(spp, DEPTH, tiles, W, H)
    ys, xs = slot_pixels(tiles, W, H)
    return spp, rad[ys, xs], w[ys, xs]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "full"])
def test_bench_one_gpu_line_and_dumped_film(mode, expected_film, tmp_path):
    spp, rad, w = expected_film
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, "-u", str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--frame-spp", str(FRAME_SPP), "--tris", str(TRIS), "--width", str(W), "--height", str(H), "--tile",
           str(TILE), "--dump-outputs", str(tmp_path / "out")]
    if mode == "full":   # the legs that render other scenes or run the CPU oracle stay out of a quick test
        cmd += ["--full", "--cpu-baseline", "0", "--side-legs", "0", "--wavefront-spp", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = lines[0]
    assert line["steps"] == STEPS and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["config"]["spp"] == spp and line["config"]["spp_per_step"] * STEPS == spp
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: W * H * spp samples in STEPS steps
    assert line["value"] == pytest.approx(W * H * spp / (line["ms_per_step"] * STEPS * 1e-3) / 1e6, rel=2e-2)
    assert line["full"] is (mode == "full") and line["bvh"]["cached"] is False
    if mode == "plain":
        assert all(line[k] is None for k in FULL_ONLY), {k: line[k] for k in FULL_ONLY}
    else:
        assert line["roofline"]["kernel"] in ("path", "trace_closest") and line["roofline"]["rays_per_sample"]
        assert line["kernels"] and all(v["launches"] >= 1 for v in line["kernels"].values())
    out = tmp_path / "out"
    assert sorted(p.name for p in out.iterdir()) == ["radiance.npy", "weight.npy"]
    got_rad, got_w = np.load(out / "radiance.npy"), np.load(out / "weight.npy")
    assert got_rad.dtype == np.float32 and got_rad.shape == (W * H, 3) and got_w.shape == (W * H,)
    assert np.all(got_w == spp)
    assert got_rad.tobytes() == rad.tobytes() and got_w.tobytes() == w.tobytes()
    assert got_rad.mean() > 0
