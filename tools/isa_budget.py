"""The instruction budget of a kernel's loops, from a gfx950 assembly listing (hipcc -S with the
Makefile's flags, --cuda-device-only).  The listing's own comments say which loop a block lies in
("Loop Header: Depth=", "Child Loop", "in Loop: Header="); every instruction is counted for the
innermost loop that holds its block, and classified by the prefix of its mnemonic alone:

  valu    v_*                                   salu    s_* not named below
  branch  s_cbranch*, s_branch, s_setpc*,       lds     ds_*
          s_swappc*, s_endpgm                   vmem    global_*, buffer_*, flat_*, scratch_*
  wait    s_waitcnt*, s_nop, s_sleep, s_barrier smem    s_load*, s_buffer_load*
  saveexec: instructions whose mnemonic contains "saveexec" (one per exec-mask save region; they are
  scalar ALU instructions and counted there too)

Per loop it prints its own counts (blocks of that loop that lie in no child loop) and the counts with
its child loops.  Static counts: what one trip issues depends on the branches taken.

Usage: python tools/isa_budget.py <file.s> <kernel symbol substring> [--json]"""
import json
import re
import sys

CLASSES = ("valu", "salu", "branch", "lds", "vmem", "smem", "wait", "other")
_BRANCH = ("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")
_WAIT = ("s_waitcnt", "s_nop", "s_sleep", "s_barrier")
_SMEM = ("s_load", "s_buffer_load")
_VMEM = ("global_", "buffer_", "flat_", "scratch_")


def classify(mnemonic):
    """The unit class of a mnemonic, by prefix."""
    m = mnemonic
    if m.startswith(_BRANCH):
        return "branch"
    if m.startswith(_WAIT):
        return "wait"
    if m.startswith(_SMEM):
        return "smem"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("v_"):
        return "valu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(_VMEM):
        return "vmem"
    return "other"


def kernel_body(text, sym):
    """(symbol, lines) of the first function whose symbol contains `sym`."""
    for m in re.finditer(r"^(_Z\S*|[A-Za-z_][\w.$]*):\s*(;.*)?$", text, re.M):
        if sym in m.group(1) and not m.group(1).startswith(".L"):
            end = text.find(".Lfunc_end", m.end())
            return m.group(1), text[m.end():end if end >= 0 else len(text)].splitlines()
    raise SystemExit(f"no kernel matching {sym}")


_LABEL = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)")
_HEADER = re.compile(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
_CHILD = re.compile(r"Child Loop (BB\d+_\d+) Depth[= ](\d+)")


def budget(lines):
    """{header: {"depth", "parent", "own": counts, "total": counts}} and the counts outside any loop
    (key None).  counts: {class: n, ..., "saveexec": n, "insts": n}."""
    zero = lambda: dict({c: 0 for c in CLASSES}, saveexec=0, insts=0)
    loops = {None: {"depth": 0, "parent": None, "own": zero()}}
    cur = None          # the loop of the block being read
    func = None
    pending = None      # a label whose comment lines are still being read
    for raw in lines:
        s = raw.strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            if m.group(1):
                func = m.group(1).split("_")[0]
                pending = m.group(1)
            else:
                pending = f"{func}_{m.group(2)}" if func else f"BB?_{m.group(2)}"
            cur = None
        if pending is not None and (m or s.startswith(";")):
            h = _HEADER.search(s)
            if h:
                parent = loops.get(pending, {}).get("parent")
                loops.setdefault(pending, {"own": zero()}).update(depth=int(h.group(1)))
                loops[pending].setdefault("parent", parent)
                cur = pending
            p = _PARENT.search(s)
            if p and int(p.group(2)) >= 1:
                # the innermost parent is the last "Parent Loop" line before the header line
                loops.setdefault(pending, {"own": zero()})["parent"] = p.group(1)
            i = _IN_LOOP.search(s)
            if i:
                cur = i.group(1)
                loops.setdefault(cur, {"own": zero(), "parent": None}).setdefault("depth", int(i.group(2)))
            for c in _CHILD.finditer(s):
                loops.setdefault(c.group(1), {"own": zero()}).setdefault("parent", None)
            if m or s.startswith(";"):
                continue
        if s.startswith((";", ".")) or s.endswith(":"):
            continue
        pending = None
        mnem = s.split()[0]
        own = loops[cur]["own"]
        own[classify(mnem)] += 1
        own["insts"] += 1
        if "saveexec" in mnem:
            own["saveexec"] += 1
    # a child loop's parent: the listing names every enclosing loop before the header line, the
    # innermost last; a depth-1 loop has none
    for k, v in loops.items():
        v.setdefault("depth", 0)
        v.setdefault("parent", None)
        if k is not None and v["depth"] <= 1:
            v["parent"] = None
    for k, v in loops.items():
        v["total"] = dict(v["own"])
    for k in sorted((k for k in loops if k is not None), key=lambda k: -loops[k]["depth"]):
        p = loops[k]["parent"]
        if p in loops and p is not None:
            for c, n in loops[k]["total"].items():
                loops[p]["total"][c] += n
    return loops


def report(name, loops):
    cols = CLASSES + ("saveexec", "insts")
    out = [name, "%-22s %5s  %s" % ("loop (header, depth)", "", " ".join("%8s" % c for c in cols))]
    keys = [k for k in loops if k is not None]
    for k in [None] + keys:
        v = loops[k]
        tag = "outside loops" if k is None else "%s d%d%s" % (k, v["depth"], " in " + v["parent"] if v["parent"] else "")
        for kind in ("own", "total"):
            if k is None and kind == "total":
                continue
            out.append("%-22s %5s  %s" % (tag if kind == "own" else "", kind, " ".join("%8d" % v[kind][c] for c in cols)))
    return "\n".join(out)


def main(argv):
    args = [a for a in argv if a != "--json"]
    if len(args) != 2:
        raise SystemExit(__doc__)
    name, body = kernel_body(open(args[0]).read(), args[1])
    loops = budget(body)
    if "--json" in argv:
        print(json.dumps({"kernel": name, "loops": {str(k): v for k, v in loops.items()}}))
    else:
        print(report(name, loops))


if __name__ == "__main__":
    main(sys.argv[1:])
