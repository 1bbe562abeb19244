"""Compare the gfx950 kernels of two builds of the library (host-only; no GPU needed).

    python tools/isa_diff.py OLD.so NEW.so

For every kernel present in both: whether the AMDGPU metadata (codeobj.FIELDS) is equal, the
instruction counts, and whether the kernel's selected loop is equal -- to the letter ("exact")
and after replacing register numbers, labels and the lane index of v_readlane / v_writelane
(the SGPR spill slot) by placeholders ("norm").  The selected loop is the ADMM run where the
kernel has one: the four-wave kernels' shortest call-free loop with four workgroup barriers,
the two-wave kernels' shortest with three, else the longest call-free loop (k_solve,
k_solve_b; tests/isa_shape.py).  A kernel of OLD that became a function template in NEW (another
symbol, the same name and parameter list) is compared with that instantiation, under its old
symbol.  Exit status 1 if any kernel differs in metadata or in its normalised loop, or is in one
library only.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from isa_shape import LLVM, code_objects, count, instructions, loops, metadata  # noqa: E402

BARRIERS = (("k_solve_w4", 4), ("k_setup_solve_w4", 4), ("k_solve_w2", 3), ("k_setup_solve_w2", 3))


def barriers_of(symbol):
    """Workgroup barriers of the kernel's ADMM loop, or None: the longest call-free loop."""
    for name, nbar in BARRIERS:
        if f"{len(name)}{name}I" in symbol:
            return nbar
    return None


def selected_loop(ins, labels, nbar):
    free = [(lo, hi) for lo, hi in loops(ins, labels) if count(ins, lo, hi, "s_swappc") == 0]
    if nbar is not None:
        free = [t for t in free if count(ins, t[0], t[1], "s_barrier") == nbar]
        pick = min
    else:
        pick = max
    if not free:
        return []
    lo, hi = pick(free, key=lambda t: t[1] - t[0])
    return ins[lo:hi + 1]


def normalise(ins):
    out = []
    for s in ins:
        if s.startswith(("v_readlane", "v_writelane")):
            s = re.sub(r",\s*\d+\s*$", ", N", s)
        s = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[R]", s)
        s = re.sub(r"\b([vsa])\d+\b", r"\1R", s)
        out.append(re.sub(r"\bL\d+\b", "L", s))
    return out


def kernels(lib, workdir):
    """{symbol: (metadata, instruction count, selected loop)} of every kernel in `lib`."""
    os.makedirs(workdir)
    todo = [(co, name, md) for co in code_objects(lib, workdir) for name, md in metadata(co).items()]

    def one(item):
        co, name, md = item
        ins, labels = instructions(co, name)
        return name, (md, len(ins), selected_loop(ins, labels, barriers_of(name)))
    with ThreadPoolExecutor(max_workers=8) as pool:  # (one llvm-objdump per kernel: the time goes there)
        return dict(pool.map(one, todo))


def signature(symbol):
    """`name(parameter types)` of a kernel, demangled, without the template arguments of the
    function itself: what a kernel and the template instantiation it became have in common."""
    tool = os.path.join(LLVM, "llvm-cxxfilt")
    txt = subprocess.run([tool if os.path.exists(tool) else "c++filt", symbol], check=True, capture_output=True,
                         text=True).stdout.strip()
    depth, at = 0, len(txt)
    for i, c in enumerate(txt):  # the parameter list opens at the first "(" outside <...>
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            at = i
            break
    head, params = txt[:at].rstrip(), txt[at:]
    if head.endswith(">"):  # the function's own template arguments
        depth = 0
        for i in range(len(head) - 1, -1, -1):
            depth += (head[i] == ">") - (head[i] == "<")
            if depth == 0:
                head = head[:i]
                break
    return head.split()[-1] + params


def pair_renamed(a, b):
    """A kernel of the old library that became a function template keeps its name and its
    parameter list and changes its symbol: where exactly one kernel of the new library has the
    signature of a kernel found in the old one only, compare the two under the old symbol."""
    new_only = {}
    for name in set(b) - set(a):
        new_only.setdefault(signature(name), []).append(name)
    for name in sorted(set(a) - set(b)):
        hit = new_only.get(signature(name), [])
        if len(hit) == 1:
            b[name] = b.pop(hit[0])


def diff(old, new):
    """Rows (symbol, metadata equal, old count, new count, loop length, exact, norm) and the
    symbols found in one library only."""
    with tempfile.TemporaryDirectory() as d:
        a, b = kernels(old, os.path.join(d, "a")), kernels(new, os.path.join(d, "b"))
    pair_renamed(a, b)
    rows = []
    for name in sorted(set(a) & set(b)):
        (ma, na, la), (mb, nb, lb) = a[name], b[name]
        rows.append((name, ma == mb, na, nb, len(lb), la == lb, normalise(la) == normalise(lb)))
    return rows, sorted(set(a) ^ set(b))


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    rows, only = diff(argv[1], argv[2])
    print(f"{'metadata':9s}{'insns old':>10s}{'new':>7s}{'loop':>6s}  {'exact':6s}{'norm':6s}kernel")
    bad = len(only)
    for name, meq, na, nb, nl, exact, norm in rows:
        yn = lambda v: "equal" if v else "DIFF"  # noqa: E731
        print(f"{yn(meq):9s}{na:10d}{nb:7d}{nl:6d}  {yn(exact):6s}{yn(norm):6s}{name}")
        bad += not (meq and norm)
    for name in only:
        print(f"in one library only: {name}")
    print(f"{len(rows)} kernels in both, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
