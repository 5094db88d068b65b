"""Host side of the render form rule and the option table: csrc/path_plan.h and csrc/options.h are plain
C++, so the rule's every branch and every option row are checked here by small g++ programs (tests/cpp)
against rows recorded before the two were pulled out of capi.hip.  No GPU needed."""
import json
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = ROOT / "akarirender-1_amd" / "csrc"
HEADERS = ("akr_path_forms.h", "options.h", "path_plan.h")
INT32_MAX, INT64_MAX = 2**31 - 1, 2**63 - 1


def build(tmp_path_factory, name):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / f"{name}.cpp"),
                    "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return build(tmp_path_factory, "path_plan_check")


@pytest.fixture(scope="module")
def options_exe(tmp_path_factory):
    return build(tmp_path_factory, "options_check")


@pytest.mark.parametrize("header", HEADERS)
def test_header_is_hip_free(header):
    """Each new header compiles alone, with no ROCm directory on the include path."""
    text = (CSRC / header).read_text()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++",
                        "-include", str(CSRC / header), "/dev/null"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "rocm" not in subprocess.run(["g++", "-std=c++17", "-M", "-x", "c++", "-include", str(CSRC / header), "/dev/null"],
                                        capture_output=True, text=True, check=True).stdout.lower()


# ---- the plan
def case_line(c):
    i = c["in"]
    head = [i["N"], i["M"], i["spp"], i["max_depth"], i["cont"], i["subset"], i["n_tris"], i["bvh_dev_bytes"], *i["grid"],
            i["block"]]
    return " ".join([str(x) for x in head] + [f"{k}={v}" for k, v in c["opt"].items()])


def parse_plan(line):
    plan = {}
    for kv in line.split():
        k, v = kv.split("=")
        plan[k] = [int(x) for x in v.split(",")] if "," in v else int(v)
    keys = ("kind", "grid", "list", "order_mode", "prio", "mix", "contrib_lanes")
    plan["launch"] = [dict(zip(keys, plan.pop(k))) for k in ("L0", "L1") if k in plan]
    return plan


def test_plan_cases(plan_exe):
    cases = json.loads((GOLDEN / "path_plan_cases.json").read_text())["cases"]
    assert 40 <= len(cases) <= 70 and len({c["name"] for c in cases}) == len(cases)
    out = subprocess.run([str(plan_exe)], input="\n".join(case_line(c) for c in cases) + "\n", capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    wrong = [(c["name"], c["plan"], parse_plan(l)) for c, l in zip(cases, lines) if parse_plan(l) != c["plan"]]
    assert not wrong, wrong[:3]
    # the recorded rows reach every branch of the rule
    plans = [c["plan"] for c in cases]
    assert {p["last_form"] for p in plans} == {-1, 2, 3, 4}
    assert {tuple(p["gate_forms"]) for p in plans} == {(-1, -1), (2, 3), (2, 4)}
    launches = [l for p in plans for l in p["launch"]]
    assert {l["kind"] for l in launches} == {0, 1, 2} and {l["list"] for l in launches} == {0, 1, 2}
    assert {l["order_mode"] for l in launches} == {0, 1, 2, 3}
    assert {(l["kind"], l["order_mode"]) for l in launches if l["list"] == 2} == {(0, 0), (1, 0), (1, 1), (2, 0)}
    assert any(p["pilot"] and p["path_pilot"] for p in plans) and any(p["want_steps"] and not p["gated"] for p in plans)
    assert any(not p["pilot"] and p["last_ordered"] == 0 for p in plans) and any(p["pilot_rays"] > 0 for p in plans)


def test_plan_rejects_a_bad_option(plan_exe):
    out = subprocess.run([str(plan_exe)], input="64 64 16 5 0 0 1 1 8 8 8 256 path_spec=3\n", capture_output=True, text=True)
    assert out.returncode == 2 and "path_spec must be in [0, 2]" in out.stdout


# ---- the option table
class Table:
    def __init__(self, exe):
        self.p = subprocess.Popen([str(exe)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, cmd, reply=True):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        return self.p.stdout.readline().rstrip("\n") if reply else None

    def rows(self):
        self.ask("table", reply=False)
        rows = []
        while (line := self.p.stdout.readline().strip()) != "end":
            name, kind, lo, hi, default = line.split()
            rows.append(dict(name=name, kind=kind, lo=int(lo), hi=int(hi), default=int(default)))
        return rows

    def close(self):
        self.p.stdin.close()
        assert self.p.wait(timeout=10) == 0


@pytest.fixture()
def table(options_exe):
    t = Table(options_exe)
    yield t
    t.close()


def test_option_rows(table):
    rows = table.rows()
    assert len({r["name"] for r in rows}) == len(rows)
    for r in rows:
        name, lo, hi = r["name"], r["lo"], r["hi"]
        table.ask("reset", reply=False)
        assert table.ask(f"get {name}").split()[0] == str(r["default"])
        if r["kind"] == "flag":
            for v, want in ((0, 0), (1, 1), (7, 1), (-3, 1), (0, 0)):   # non-zero is true
                assert table.ask(f"set {name} {v}") == f"ok {want}"
        elif r["kind"] == "tri":
            for v, want in ((0, "0 0 0"), (1, "1 1 0"), (2, "2 1 1"), (3, "1 1 0"), (-1, "1 1 0"), (0, "0 0 0")):
                assert table.ask(f"set {name} {v}").startswith("ok")
                assert table.ask(f"get {name}") == want      # the value, then its two derived booleans
        elif r["kind"] == "floor":
            assert table.ask(f"set {name} 0") == "ok 0" and table.ask(f"set {name} 77") == "ok 77"
            assert table.ask(f"set {name} {INT32_MAX}") == f"ok {INT32_MAX}"
            assert table.ask(f"set {name} {INT32_MAX + 1}") == f"ok {INT32_MAX}"     # clamped, not refused
            assert table.ask(f"set {name} {INT64_MAX}") == f"ok {INT32_MAX}"
            assert table.ask(f"set {name} -1").startswith(f"error {name} must be")
            assert table.ask(f"get {name}") == str(INT32_MAX)                        # a refusal stores nothing
        elif r["kind"] == "pow2":
            ok = [v for v in range(lo - 2, hi + 3) if table.ask(f"set {name} {v}") == f"ok {v}"]
            assert (name, ok) == ("leaf_align", [1, 2, 4, 8])
            assert table.ask(f"set {name} 3").startswith(f"error {name} must be") and table.ask(f"get {name}") == "8"
        else:
            assert r["kind"] == "range"
            assert table.ask(f"set {name} {lo}") == f"ok {lo}" and table.ask(f"get {name}") == str(lo)
            assert table.ask(f"set {name} {hi}") == f"ok {hi}" and table.ask(f"get {name}") == str(hi)
            assert table.ask(f"set {name} {lo - 1}").startswith(f"error {name} must be")
            if hi < INT64_MAX:
                assert table.ask(f"set {name} {hi + 1}").startswith(f"error {name} must be")
                assert table.ask(f"set {name} {hi + 1}") == f"error {name} must be in [{lo}, {hi}]"
            assert table.ask(f"get {name}") == str(hi)
    assert table.ask("set no_such_option 1") == "error unknown option 'no_such_option'"
    assert table.ask("set  1").startswith("error unknown option '")


def test_options_match_the_record(table):
    """Names, kinds, bounds and defaults against the record taken from akr_hip_set_option before the table
    existed; and every option the public header's comment names has a row."""
    golden = json.loads((GOLDEN / "options.json").read_text())["options"]
    rows = {r["name"]: r for r in table.rows()}
    assert sorted(rows) == sorted(g["name"] for g in golden) and len(golden) == 47
    for g in golden:
        r = rows[g["name"]]
        assert r["default"] == g["default"], g["name"]
        assert r["kind"] == {"set": "pow2"}.get(g["kind"], g["kind"]), g["name"]
        if g["kind"] in ("range", "set", "floor"):
            assert r["lo"] == g["lo"] and r["hi"] == (INT64_MAX if g["hi"] is None else g["hi"]), g["name"]
    header = (ROOT / "include" / "akr_hip.h").read_text()
    comment = header[header.index("/* Options:"):header.index("int akr_hip_set_option(")]
    named = set(re.findall(r'"(\w+)"', comment))
    assert len(named) > 40 and named <= set(rows), named - set(rows)
