"""tools/isa_budget.py on a small hand-written listing (tests/golden/isa_budget_listing.s: two functions,
a loop with a child loop, a few instructions of each class).  No compiler runs."""
import json
import subprocess
import sys

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(ROOT / "tools"))
import isa_budget  # noqa: E402

LISTING = GOLDEN / "isa_budget_listing.s"


def counts(**kw):
    out = dict({c: 0 for c in isa_budget.CLASSES}, saveexec=0, insts=0)
    out.update(kw)
    return out


def test_classes_by_prefix():
    got = {m: isa_budget.classify(m) for m in
           ("v_fma_f32", "v_cmp_lt_i32_e32", "s_and_b64", "s_and_saveexec_b64", "s_bcnt1_i32_b64", "s_cbranch_execz",
            "s_branch", "s_endpgm", "s_setpc_b64", "s_waitcnt", "s_nop", "s_barrier", "s_load_dwordx2",
            "s_buffer_load_dword", "ds_read_b64", "ds_write2st64_b32", "global_load_dwordx4", "scratch_store_dwordx4",
            "buffer_load_dword", "flat_load_dword", "unknown_op")}
    assert got == {"v_fma_f32": "valu", "v_cmp_lt_i32_e32": "valu", "s_and_b64": "salu", "s_and_saveexec_b64": "salu",
                   "s_bcnt1_i32_b64": "salu", "s_cbranch_execz": "branch", "s_branch": "branch", "s_endpgm": "branch",
                   "s_setpc_b64": "branch", "s_waitcnt": "wait", "s_nop": "wait", "s_barrier": "wait",
                   "s_load_dwordx2": "smem", "s_buffer_load_dword": "smem", "ds_read_b64": "lds",
                   "ds_write2st64_b32": "lds", "global_load_dwordx4": "vmem", "scratch_store_dwordx4": "vmem",
                   "buffer_load_dword": "vmem", "flat_load_dword": "vmem", "unknown_op": "other"}


def test_loops_of_the_named_kernel():
    name, body = isa_budget.kernel_body(LISTING.read_text(), "k_toy")
    assert name == "_ZN3akr5k_toyEv"
    loops = isa_budget.budget(body)
    assert set(loops) == {None, "BB0_2", "BB0_4"}
    assert loops[None]["own"] == counts(valu=1, salu=1, branch=2, vmem=1, smem=1, wait=1, insts=7)
    outer, inner = loops["BB0_2"], loops["BB0_4"]
    assert (outer["depth"], outer["parent"]) == (1, None)
    assert (inner["depth"], inner["parent"]) == (2, "BB0_2")
    assert outer["own"] == counts(valu=3, salu=4, branch=3, lds=1, vmem=1, wait=2, saveexec=1, insts=14)
    assert inner["own"] == inner["total"] == counts(valu=2, salu=2, branch=1, lds=1, wait=1, insts=7)
    assert outer["total"] == counts(valu=5, salu=6, branch=4, lds=2, vmem=1, wait=3, saveexec=1, insts=21)


def test_other_kernel_and_missing_kernel():
    name, body = isa_budget.kernel_body(LISTING.read_text(), "k_other")
    loops = isa_budget.budget(body)
    assert set(loops) == {None} and loops[None]["own"] == counts(valu=1, branch=1, insts=2)
    try:
        isa_budget.kernel_body(LISTING.read_text(), "k_absent")
    except SystemExit as e:
        assert "k_absent" in str(e)
    else:
        raise AssertionError("a missing kernel must be an error")


def test_command_line_report_and_json():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), str(LISTING), "k_toy", "--json"],
                         capture_output=True, text=True, check=True).stdout
    d = json.loads(out)
    assert d["kernel"] == "_ZN3akr5k_toyEv" and d["loops"]["BB0_4"]["own"]["insts"] == 7
    text = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), str(LISTING), "k_toy"],
                          capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in text.splitlines()]
    assert ["BB0_4", "d2", "in", "BB0_2", "own", "2", "2", "1", "1", "0", "0", "1", "0", "0", "7"] in rows
