"""Host side of progressive rendering (akari_amd/progressive.py, render.py's flags): no GPU needed."""
import numpy as np
import pytest

from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH
from helpers import cornell, mixed_scene

TILES = [(0, 0, 16, 16), (16, 0, 32, 16), (0, 16, 16, 24)]


def _checkpoint(cs, tiles=TILES, spp=3, seed=5):
    rng = np.random.default_rng(seed)
    n = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in tiles)
    film = rng.random((n, 4), dtype=np.float32)
    film[:, 3] = spp
    w, h = cs.camera.resolution
    return progressive.Checkpoint(int(w), int(h), capi.rect_array(tiles), spp, 5, 10.0, 0,
                                  rng.integers(0, 1 << 32, n, dtype=np.uint32), film, progressive.scene_fingerprint(cs))


def test_checkpoint_round_trip(tmp_path):
    cs = scene.compile_scene(cornell((32, 24)))
    ck = _checkpoint(cs)
    path = tmp_path / "a.npz"
    ck.save(path)
    assert [p.name for p in tmp_path.iterdir()] == ["a.npz"], "temporary file left behind"
    back = progressive.Checkpoint.load(path)
    assert (back.width, back.height, back.spp_done, back.max_depth, back.ray_clamp, back.flags) == (32, 24, 3, 5, 10.0, 0)
    assert back.fingerprint == ck.fingerprint and len(ck.fingerprint) == 64
    for k in ("tiles", "sampler", "film"):
        a, b = getattr(ck, k), getattr(back, k)
        assert a.dtype == b.dtype and np.array_equal(a, b)
    back.check(cs, TILES, 32, 24)
    ck.spp_done = 7   # saving again replaces the file whole
    ck.save(path)
    assert progressive.Checkpoint.load(path).spp_done == 7
    with np.load(path) as z:
        assert int(z["version"]) == progressive.Checkpoint.FORMAT_VERSION


def test_checkpoint_rejects_other_scene_resolution_tiles_and_files(tmp_path):
    cs = scene.compile_scene(cornell((32, 24)))
    ck = _checkpoint(cs)
    with pytest.raises(progressive.CheckpointError, match="fingerprint"):
        ck.check(scene.compile_scene(mixed_scene((32, 24))), TILES, 32, 24)
    moved = cornell((32, 24))
    moved.camera.position = (0.0, 1.0, 9.5)
    with pytest.raises(progressive.CheckpointError, match="fingerprint"):
        ck.check(scene.compile_scene(moved), TILES, 32, 24)
    with pytest.raises(progressive.CheckpointError, match="resolution"):
        ck.check(scene.compile_scene(cornell((24, 32))), TILES, 24, 32)
    with pytest.raises(progressive.CheckpointError, match="tile list"):
        ck.check(cs, TILES[:2], 32, 24)
    with pytest.raises(progressive.CheckpointError, match="tile list"):
        ck.check(cs, [TILES[1], TILES[0], TILES[2]], 32, 24)
    # restore() checks before it touches the context
    with pytest.raises(progressive.CheckpointError, match="tile list"):
        ck.restore(None, cs, TILES[:2])
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not a zip")
    with pytest.raises(progressive.CheckpointError, match="not a render checkpoint"):
        progressive.Checkpoint.load(junk)
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(progressive.CheckpointError, match="not a render checkpoint"):
        progressive.Checkpoint.load(tmp_path / "other.npz")
    ck.save(tmp_path / "v.npz")
    with np.load(tmp_path / "v.npz") as z:
        fields = {k: z[k] for k in z.files}
    fields["version"] = np.int32(99)
    np.savez(tmp_path / "v99.npz", **fields)
    with pytest.raises(progressive.CheckpointError, match="format 99"):
        progressive.Checkpoint.load(tmp_path / "v99.npz")
    fields["version"] = np.int32(progressive.Checkpoint.FORMAT_VERSION)
    fields["film"] = fields["film"][:-1]
    np.savez(tmp_path / "short.npz", **fields)
    with pytest.raises(progressive.CheckpointError, match="sampler states"):
        progressive.Checkpoint.load(tmp_path / "short.npz")


def test_schedule_arithmetic():
    pc = progressive.pass_chunks
    assert pc(16, "double") == [1, 1, 2, 4, 8]
    assert pc(21, "double") == [1, 1, 2, 4, 8, 5]            # the last chunk is short
    assert pc(21, "double", first=4) == [4, 4, 8, 5]
    assert pc(10, 4) == [4, 4, 2]
    assert pc(8, 4) == [4, 4]
    assert pc(3, 16) == [3]
    assert pc(0, 4) == [] and pc(0, "double") == []
    assert pc(10, 4, done=3) == [4, 3]                        # a resumed session
    assert pc(20, "double", done=6) == [6, 8]
    assert pc(6, "double", done=6) == []
    for total in (1, 2, 7, 64, 1040):
        for sched in ("double", 1, 3, 16, 2000):
            for done in (0, 1, total // 2):
                chunks = pc(total, sched, done)
                assert sum(chunks) == total - done and all(c > 0 for c in chunks)
                if not isinstance(sched, str):
                    assert all(c == sched for c in chunks[:-1]) and (not chunks or chunks[-1] <= sched)
    for bad in (dict(total=3, schedule=0), dict(total=3, schedule=-2), dict(total=3, schedule="halve"),
                dict(total=3, schedule=2, done=4), dict(total=3, schedule="double", first=0)):
        with pytest.raises(ValueError):
            pc(**bad)


class _FakeCtx:
    """Records the calls render_progressive makes (no device)."""

    def __init__(self, done=None):
        self.calls, self.done = [], done

    def render(self, spp, max_depth, tiles, w, h, ray_clamp=0.0, exact_cull=False):
        self.calls.append(("render", spp))
        self.done = spp
        return np.zeros((h, w, 3), np.float32), np.full((h, w), self.done, np.float32)

    def render_continue(self, spp, w, h):
        self.calls.append(("continue", spp))
        self.done += spp
        return np.zeros((h, w, 3), np.float32), np.full((h, w), self.done, np.float32)

    def render_state_info(self):
        return dict(width=8, height=4, spp_done=self.done)


def test_render_progressive_passes_budget_and_resume():
    ctx, seen = _FakeCtx(), []
    rad, w, done = progressive.render_progressive(ctx, 10, 5, TILES, 8, 4, schedule=4,
                                                  on_pass=lambda d, r, wt: seen.append((d, float(wt[0, 0]))))
    assert ctx.calls == [("render", 4), ("continue", 4), ("continue", 2)] and done == 10 and np.all(w == 10)
    assert seen == [(4, 4.0), (8, 8.0), (10, 10.0)]
    # the budget is tested after each pass: at least one pass, none begun past it
    ticks = iter([0.0, 1.0, 2.5, 99.0])
    ctx = _FakeCtx()
    *_, done = progressive.render_progressive(ctx, 64, 5, TILES, 8, 4, time_budget=2.0, clock=lambda: next(ticks))
    assert ctx.calls == [("render", 1), ("continue", 1)] and done == 2
    ctx = _FakeCtx()
    *_, done = progressive.render_progressive(ctx, 64, 5, TILES, 8, 4, schedule=8, on_pass=lambda d, r, wt: d >= 16)
    assert done == 16                                          # a true return value stops the render
    ctx = _FakeCtx(done=6)                                      # a restored session: only continues
    *_, done = progressive.render_progressive(ctx, 10, 5, TILES, 8, 4, schedule=3, resume=True)
    assert ctx.calls == [("continue", 3), ("continue", 1)] and done == 10
    ctx = _FakeCtx(done=6)
    *_, done = progressive.render_progressive(ctx, 6, 5, TILES, 8, 4, resume=True)
    assert ctx.calls == [("continue", 0)] and done == 6        # nothing to add: the film as it stands
    with pytest.raises(ValueError, match="another resolution"):
        progressive.render_progressive(_FakeCtx(done=6), 10, 5, TILES, 9, 4, resume=True)


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [16, 8] }},
    integrator: {integrator},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey,
                                                       EmissiveMaterial {{ color: [17, 12, 4] }}] }} ]
}}
"""


def test_cli_flag_validation_needs_no_gpu(tmp_path, capsys):
    """Flags that cannot work are refused with a clear message before a device is touched."""
    path = tmp_path / "s.akari"
    ao = tmp_path / "ao.akari"
    path.write_text(SDL.format(integrator="Path { spp: 4, max_depth: 3 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    ao.write_text(SDL.format(integrator="AO { spp: 4 }", out=tmp_path / "o.pfm", mesh=CORNELL_MESH))
    ck = tmp_path / "c.npz"
    ck.write_bytes(b"junk")

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            render.main([str(a) for a in argv])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err, err

    for flag in (["--pass-spp", "2"], ["--preview"], ["--time-budget", "3"], ["--checkpoint", ck], ["--resume", ck]):
        refused([path, "--gpus", "2", *flag], "render on one GPU")
        refused([ao, *flag], "need the Path integrator; the scene's is AOIntegrator")
    refused([path, "--pass-spp", "0"], "at least one sample per pass")
    refused([path, "--time-budget", "0"], "positive number of seconds")
    refused([path, "--time-budget", "nan"], "positive number of seconds")
    refused([path, "--resume", tmp_path / "missing.npz"], "no checkpoint file")
    refused([path, "--resume", ck], "not a render checkpoint")
    # a checkpoint of another scene is refused before the upload, too
    other = _checkpoint(scene.compile_scene(cornell((16, 8))), tiles=[(0, 0, 16, 8)])
    other.save(tmp_path / "other.npz")
    refused([path, "--resume", tmp_path / "other.npz"], "checkpoint")
    assert not (tmp_path / "o.pfm").exists()
