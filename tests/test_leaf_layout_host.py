"""Host side of the device leaf blob: csrc/leaf_layout.h (offsets, padding, the size check and the
one-triangle flag of a device leaf reference) is plain C++, checked here through a small g++ program
(tests/cpp/leaf_layout_check.cpp) against the layout restated in Python.  No GPU needed."""
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "akarirender-1_amd" / "csrc"
LEAF, ONE, LIMIT = 0x80000000, 1 << 30, 1 << 30


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("leaf_layout_check") / "leaf_layout_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "leaf_layout_check.cpp"), "-o", str(out)], check=True)
    return out


def ask(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    replies = out.stdout.splitlines()
    assert len(replies) == len(lines)
    return replies


def parse(reply):
    head, *pairs = reply.split()[0:2], *reply.split()[2:]
    words, pad = (int(x.split("=")[1]) for x in head)
    return words, pad, [(int(p.split(":")[0]), int(p.split(":")[1], 16)) for p in pairs]


def expected(align, counts):
    """A leaf's record is 2 float4 of header and 3 per triangle, and starts at a multiple of `align`."""
    words, pairs = 0, []
    for c in counts:
        words = (words + align - 1) // align * align
        pairs.append((words, LEAF | (ONE if c == 1 else 0) | words))
        words += 2 + 3 * c
    return words, pairs


def test_header_is_hip_free():
    text = (CSRC / "leaf_layout.h").read_text()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++",
                        "-include", str(CSRC / "leaf_layout.h"), "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["g++", "-std=c++17", "-M", "-x", "c++", "-include", str(CSRC / "leaf_layout.h"), "/dev/null"],
                          capture_output=True, text=True, check=True).stdout.lower()
    assert "rocm" not in deps and "hip_runtime" not in deps


CASES = [[1], [4], [1, 1, 1], [1, 2, 3, 4, 1, 8, 1, 1, 2], [2, 1, 2, 1], [3, 3, 3], [8, 1], []]


@pytest.mark.parametrize("align", [1, 8])
def test_offsets_flags_and_padding(exe, align):
    replies = ask(exe, [" ".join(str(x) for x in [align] + counts) for counts in CASES])
    for counts, reply in zip(CASES, replies):
        words, pad, pairs = parse(reply)
        want_words, want_pairs = expected(align, counts)
        assert (words, pairs) == (want_words, want_pairs), (align, counts, reply)
        # three zero float4 behind the last record: a leaf phase may fetch the second triangle's record
        # with the header of a one-triangle leaf that is the blob's last
        assert pad == 3
        for (off, ref), c in zip(pairs, counts):
            assert off % align == 0 and off < LIMIT
            assert ref & LEAF and ref & (ONE - 1) == off
            assert bool(ref & ONE) == (c == 1)                 # the flag exactly when the count is one
            assert ref < 0xFFFFFFFE                            # neither AKR_CHILD_EMPTY nor the kernels' pop mark
        ends = [off + 2 + 3 * c for (off, _), c in zip(pairs, counts)]
        assert all(e <= nxt for e, (nxt, _) in zip(ends, pairs[1:])) and (not ends or ends[-1] == words)
        if align == 1:
            assert all(e == nxt for e, (nxt, _) in zip(ends, pairs[1:]))    # no gap


def test_the_limit_is_2_to_the_30_float4(exe):
    big = 1 << 20                                    # 3 * 2^20 + 2 float4 per leaf
    per = 3 * big + 2
    fits = (LIMIT - 1) // per                        # 341 leaves end below 2^30, the 342nd does not
    assert fits * per < LIMIT <= (fits + 1) * per
    a = (LIMIT - 4) // 3 // 2                        # two leaves that end exactly at 2^30
    b = (LIMIT - 4) // 3 - a
    assert 4 + 3 * (a + b) == LIMIT
    ok, over, exact, below = ask(exe, [f"1 repeat {fits} {big}", f"1 repeat {fits + 1} {big}", f"1 {a} {b}",
                                       f"1 {a} {b - 1}"])
    words, _, pairs = parse(ok)
    assert words == fits * per and pairs == [((fits - 1) * per, LEAF | (fits - 1) * per)]
    for reply in (over, exact):
        assert reply.startswith("error ") and "30-bit" in reply and "too large" in reply
    words, _, pairs = parse(below)
    assert words == LIMIT - 3 and pairs[1] == (2 + 3 * a, LEAF | (2 + 3 * a))
    # with alignment, the round-up alone may cross the limit
    assert ask(exe, [f"8 {a} {b - 1} 1"])[0].startswith("error ")


def test_which_tree_gets_the_one_triangle_kernel(exe):
    """From 97 % one-triangle leaves (0.97^22 = 0.51: half of the leaf phases of about 22 holders hold no other
    leaf), in integer arithmetic; the benchmark soup's tree does, the Cornell box's (4 of 28) does not."""
    cases = [(0, 0, 0), (1, 1, 1), (97, 100, 1), (96, 100, 0), (969, 1000, 0), (970, 1000, 1), (4, 28, 0),
             (13_716_334, 13_722_927, 1), (2**40 * 97 // 100 + 1, 2**40, 1), (2**40 * 96 // 100, 2**40, 0)]
    replies = ask(exe, [f"pays {a} {b}" for a, b, _ in cases])
    assert [int(r) for r in replies] == [w for _, _, w in cases]
