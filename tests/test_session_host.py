"""Host side of the render session: csrc/tile_layout.h (how a tile list becomes film slots) and csrc/session.h
(what a session holds after each call that extends it) are plain C++, checked here through small g++ programs
(tests/cpp/tile_layout_check.cpp, session_check.cpp): the layout against helpers.slot_pixels, the session's
transitions against values written out from the rules in include/akr_hip.h.  No GPU needed."""
import subprocess

import numpy as np
import pytest

from akari_amd import progressive
from conftest import ROOT
from helpers import slot_pixels

CSRC = ROOT / "akarirender-1_amd" / "csrc"
HEADERS = ("tile_layout.h", "session.h")
CAP = 1 << 24


def build(tmp_path_factory, name):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / f"{name}.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def ask(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    replies = out.stdout.splitlines()
    assert len(replies) == len(lines)
    return replies


@pytest.fixture(scope="module")
def layout_exe(tmp_path_factory):
    return build(tmp_path_factory, "tile_layout_check")


@pytest.fixture(scope="module")
def session_exe(tmp_path_factory):
    return build(tmp_path_factory, "session_check")


@pytest.mark.parametrize("header", HEADERS)
def test_header_is_hip_free(header):
    text = (CSRC / header).read_text()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++",
                        "-include", str(CSRC / header), "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-M", "-x", "c++", "-include", str(CSRC / header), "/dev/null"],
                          capture_output=True, text=True, check=True).stdout.lower()
    assert "rocm" not in deps and "hip_runtime" not in deps


# ---- the tile layout
W, H = 7, 5
TILE_LISTS = {
    "inside": [(1, 1, 4, 3)],
    "clipped_left": [(-2, 1, 3, 4)],
    "clipped_top": [(2, -3, 5, 2)],
    "clipped_right": [(5, 1, 9, 4)],
    "clipped_bottom": [(1, 3, 4, 8)],
    "outside": [(7, 0, 10, 5)],
    "zero_area": [(2, 2, 2, 4)],
    "inverted": [(4, 1, 2, 3)],
    "overlapping": [(0, 0, 4, 3), (2, 1, 6, 4)],
    "empty_list": [],
    "first_tile_empty": [(3, 3, 3, 3), (1, 1, 3, 2)],
}


def layout_line(width, height, pixels, tiles):
    return " ".join(str(v) for v in (width, height, int(pixels), len(tiles), *(c for t in tiles for c in t)))


def parse_layout(reply):
    out = {}
    for kv in reply.split():
        k, v = kv.split("=")
        out[k] = v
    tiles = [tuple(int(c) for c in t.split(",")) for t in out["tiles"].split(";") if t]
    px = [int(p, 16) for p in out.get("px", "").split(",") if p]
    frame = [int(p) for p in out.get("frame", "").split(",") if p]
    return int(out["n"]), int(out["alloc"]), tiles, px, frame


def expected_tiles(tiles, width, height):
    """(x0, y0, width, first slot) of every non-empty clipped tile, read off slot_pixels of the tile alone."""
    out, first = [], 0
    for t in tiles:
        ys, xs = slot_pixels([t], width, height)
        if len(ys):
            out.append((int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), first))
            first += len(ys)
    return out


@pytest.mark.parametrize("name", TILE_LISTS)
def test_tile_layout(layout_exe, name):
    tiles = TILE_LISTS[name]
    n, _, got_tiles, px, frame = parse_layout(ask(layout_exe, [layout_line(W, H, True, tiles)])[0])
    ys, xs = slot_pixels(tiles, W, H)
    assert n == len(ys) == len(px)
    assert got_tiles == expected_tiles(tiles, W, H)
    assert np.array_equal(np.array(px, np.int64), xs | (ys << 16))
    assert np.array_equal(np.array(frame, np.int64), xs + ys * W)
    if name in ("outside", "zero_area", "inverted", "empty_list"):
        assert n == 0 and got_tiles == []
    if name == "overlapping":
        assert n == 24 and len(set(px)) < n        # a pixel two tiles cover holds two slots


def test_tile_layout_limit(layout_exe):
    """Fewer than 2^31 slots are laid out, without an allocation per pixel; 2^31 or more are refused."""
    big, row = (0, 0, 65535, 32768), (0, 0, 65535, 1)
    ok, refused, refused_first = ask(layout_exe, [layout_line(65535, 65535, False, [big]),
                                                  layout_line(65535, 65535, False, [big, row]),
                                                  layout_line(65535, 65535, False, [big, big, row])])
    n, alloc, tiles, _, _ = parse_layout(ok)
    assert n == 2_147_450_880 and tiles == [(0, 0, 65535, 0)]
    assert alloc <= 256, "layout_tiles allocates per tile, not per pixel"
    assert refused == refused_first == "error too many pixels in one render call"


# ---- the session
def state(reply):
    result, fields = reply.split(" | ")
    return result, {k: (float(v) if "." in v or "inf" in v else int(v)) for k, v in (kv.split("=") for kv in fields.split())}


def run(exe, lines):
    return [state(r) for r in ask(exe, lines)]


def test_open_and_params(session_exe):
    (r0, s0), (r1, s1), (r2, s2) = run(session_exe, ["params 3", "open 150 3 1", "params 4"])
    assert r0.startswith("error no render session to continue") and s0["valid"] == 0
    assert r1 == "ok" and r2 == "ok 4,5,2.5,1"
    assert s1 == s2 == dict(valid=1, seeded=1, n=150, spp_done=3, max_depth=5, flags=1, ray_clamp=2.5, uniform=1, spp_min=3,
                            n_strips=0, on=0, more=0, some_stopped=0, cap=0, pass_spp=0, total=0, threshold=0, m=0, passes=0,
                            info_min=0, info_max=0, samples=0, strips=0, strips_at_cap=0)


def test_continues(session_exe):
    got = run(session_exe, ["open 150 0 0", "all 0", "all 2",         # a uniform continue; the first samples seed the slots
                            "subset 150 5 0",                          # m == N keeps a uniform session uniform
                            "subset 70 5 0",                           # uniform -> non-uniform: spp_min = the old count
                            "subset 150 2 12", "range 9 14",           # m == N on a non-uniform one: counts added and read back
                            "all 3"])
    assert [r for r, _ in got] == ["ok", "ok", "ok", "ok 00", "ok 01", "ok 02", "ok", "ok"]
    key = lambda s: (s["seeded"], s["uniform"], s["spp_min"], s["spp_done"])
    assert [key(s) for _, s in got] == [(0, 1, 0, 0), (0, 1, 0, 0), (1, 1, 2, 2), (1, 1, 7, 7), (1, 0, 7, 12), (1, 0, 7, 12),
                                        (1, 0, 9, 14), (1, 0, 12, 17)]
    assert all(s["n"] == 150 and s["valid"] == 1 and s["on"] == 0 for _, s in got)


def test_cap(session_exe):
    """2^24 samples per slot are the most a session holds: 2^24 - 1 accepts one more and refuses two, and a
    refused call leaves the session equal to its snapshot."""
    message = f"refused render session: {CAP - 1} + 2 samples per slot exceed 2^24 (the weight is an f32 count)"
    got = run(session_exe, [f"open 150 {CAP - 1} 1", "all 2", "subset 70 2 0", "subset 150 2 0", "all 1",
                            f"open 150 {CAP - 1} 1", "subset 70 1 0",
                            # non-uniform, counts 2^24 - 4 and 2^24 - 1: only the listed slots' largest count decides
                            f"open 150 {CAP - 4} 1", "subset 70 3 0", f"subset 10 2 {CAP - 4}", f"range {CAP - 4} {CAP - 1}",
                            f"subset 10 2 {CAP - 1}", "all 2", "subset 10 1 0"])
    results, states = [r for r, _ in got], [s for _, s in got]
    assert results[:5] == ["ok", message, message, message, "ok"]
    assert states[1] == states[2] == states[3] == states[0] and states[4]["spp_done"] == states[4]["spp_min"] == CAP
    assert results[5:7] == ["ok", "ok 01"] and (states[6]["spp_min"], states[6]["spp_done"]) == (CAP - 1, CAP)
    assert results[7:11] == ["ok", "ok 01", "ok 12", "ok"]
    assert (states[10]["uniform"], states[10]["spp_min"], states[10]["spp_done"]) == (0, CAP - 4, CAP - 1)
    assert results[11:13] == [message, message] and states[11] == states[12] == states[10]
    assert results[13] == "ok 02"        # below the cap nothing is read before the pass


@pytest.mark.parametrize("row", [(4, 0, 32), (4, 0, 20), (4, 4, 16), (4, 5, 16), (16, 0, 16), (16, 0, 7), (1, 0, 0), (1, 0, 5)])
def test_adaptive_pass_sizes(session_exe, row):
    """The totals an always-active slot passes through are progressive.adaptive_totals' (test_adaptive_totals' rows)."""
    min_spp, pass_spp, cap = row
    want = progressive.adaptive_totals(min_spp, pass_spp, cap)
    got = run(session_exe, [f"adaptive 150 {cap} {min_spp} {pass_spp}"] + ["step 150"] * len(want))
    totals = [s["total"] for _, s in got]
    assert totals[:len(want)] == want and got[-1][0] == "ok done" and got[-1][1] == got[-2][1]
    assert [r for r, _ in got[1:-1]] == [f"ok {b - a}" for a, b in zip(want, want[1:])]
    assert [s["more"] for _, s in got[:-1]] == [1] * (len(want) - 1) + [0]
    last = got[-1][1]
    assert (last["passes"], last["samples"], last["spp_done"], last["spp_min"], last["uniform"]) == (len(want), 150 * cap, cap, cap, 1)
    assert last["strips_at_cap"] == (3 if len(want) > 1 else 0)       # counted by the test at the cap only


def test_adaptive_run(session_exe):
    """150 slots are two strips of 64 and one of 22; the cap 10 gives the totals 4, 8, 10.  The first test stops
    one full strip, the second the other, and the short strip is still active at the cap."""
    got = run(session_exe, ["step 1", "open 150 4 1", "step 1", "adaptive 150 10 4 0", "step 86", "step 22", "step 0", "all 1"])
    assert got[0][0].startswith("error no render session") and got[2][0].startswith("error adaptive step: the session is not")
    assert got[2][1] == got[1][1]
    assert [r for r, _ in got[3:]] == ["ok", "ok 4", "ok 2", "ok done", "ok"]
    keys = ("on", "more", "some_stopped", "total", "m", "passes", "info_min", "info_max", "samples", "strips", "strips_at_cap",
            "n_strips", "uniform", "spp_min", "spp_done")
    rows = [tuple(s[k] for k in keys) for _, s in got[3:]]
    assert rows[0] == (1, 1, 0, 4, 150, 1, 4, 4, 600, 3, 0, 3, 1, 4, 4)
    assert rows[1] == (1, 1, 1, 8, 86, 2, 8, 8, 1200, 3, 0, 3, 1, 8, 8)
    assert rows[2] == (1, 0, 1, 10, 22, 3, 8, 10, 1372, 3, 1, 3, 0, 8, 10)
    assert rows[3] == rows[2]
    assert rows[4] == (0, 0, 1, 10, 22, 3, 8, 10, 1372, 3, 1, 3, 0, 9, 11)     # a continue with samples ends the run
    assert got[3][1]["cap"] == 10 and got[3][1]["threshold"] == 0.25
