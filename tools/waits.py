#!/usr/bin/env python3
"""tools/waits.py <file.s> [kernel-name-substring] — where hipcc put the vector-memory waits in each loop of a kernel.

Reads the assembly of one csrc file (hipcc with the Makefile's flags plus `-S --cuda-device-only`) and prints, per
kernel and per loop (a backward branch and its target), the sequence of

    L    a vector load      (global_load_* / buffer_load_*)
    S    a vector store     (global_store_* / buffer_store_*)
    Wn   s_waitcnt vmcnt(n)
    |    s_barrier
    xz   s_cbranch_execz    (a predicated region the wave may skip: a path without whatever is inside)

in program order.  vmcnt on gfx950 counts loads and stores together, in issue order, so a row of a streaming loop that
keeps P loads in flight and stores once per row can wait with vmcnt(2P) at the most; a smaller n means the wave waits for
younger loads, or for its stores, before it touches the row it needs.  No GPU needed.
"""
import re
import sys


def kernels(lines):
    cur, out = None, {}
    for ln in lines:
        m = re.match(r"^(_Z\S*):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            out[cur].append(ln)
    return out


def events(body):
    ev = []
    for ln in body:
        t = ln.strip()
        m = re.match(r"s_waitcnt\s+.*vmcnt\((\d+)\)", t)
        if m:
            ev.append("W" + m.group(1))
        elif re.match(r"(global|buffer)_load", t):
            ev.append("L")
        elif re.match(r"(global|buffer)_store", t):
            ev.append("S")
        elif t.startswith("s_barrier"):
            ev.append("|")
        elif t.startswith("s_cbranch_execz"):
            ev.append("xz")
    return ev


def main(argv):
    if not argv:
        sys.exit(__doc__)
    pat = argv[1] if len(argv) > 1 else ""
    try:
        import subprocess
        demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() or n
    except Exception:  # noqa: BLE001
        demangle = lambda n: n
    for name, body in kernels(open(argv[0]).read().split("\n")).items():
        shown = demangle(name)
        if pat not in name and pat not in shown:
            continue
        labels = {}
        for i, ln in enumerate(body):
            m = re.match(r"^(\.LBB\d+_\d+):", ln)
            if m:
                labels[m.group(1)] = i
        loops = {}
        for i, ln in enumerate(body):
            m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
            if m and labels.get(m.group(1), i) < i:
                a = labels[m.group(1)]
                loops[a] = max(loops.get(a, 0), i)  # one loop per header: its last backward branch
        print("== " + re.sub(r"\(unsigned char const\*.*", "", shown).replace("mi355::(anonymous namespace)::", ""))
        for a, b in sorted(loops.items()):
            ev = events(body[a:b + 1])
            nl, ns = ev.count("L"), ev.count("S")
            if nl + ns:
                print("  lines %6d..%-6d %2d loads %2d stores: %s" % (a, b, nl, ns, " ".join(ev)))


if __name__ == "__main__":
    main(sys.argv[1:])
