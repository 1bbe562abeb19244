#!/usr/bin/env python3
"""CPU only: the plan ladder's table (tests/plan_ladder.py::RUNGS) derived again.  Per rung:
what mpcqp_plan_preview gives for its pattern, and the first seed of 1..20 that meets
plan_ladder.premises -- with the margin condition of the run to convergence, and failing that
the first that meets the rest (converge = False).  Prints one row per rung in RUNGS' form, the
oracle's iteration counts of the run to convergence and the dense restatement's deviation from
the oracle on the fixed-count run.  One process per rung (--jobs)."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
for k in ("MPCQP_VARIANT", "MPCQP_ELIM"):
    os.environ.pop(k, None)


def search(i):
    import plan_ladder as L
    r = L.RUNGS[i]
    fallback, why = None, []
    for seed in range(1, 21):
        b = L.build(r.builder, r.N, seed)
        ok, what, det = L.premises(b)
        if ok:
            return i, seed, True, b, det, why
        why.append(f"seed {seed}: {what}")
        if fallback is None and what.startswith("converge"):  # (the fixed-count run's conditions held)
            fallback = (seed, b, det)
    if fallback is None:
        return i, None, False, None, None, why
    seed, b, det = fallback
    return i, seed, False, b, det, why


def row(i):
    import plan_ladder as L
    r = L.RUNGS[i]
    i, seed, conv, b, det, why = search(i)
    if seed is None:
        return f"{L.rung_id(r)}: no seed\n  " + "\n  ".join(why)
    var, nb, amax, ne = L.preview(b)
    bo, bd = det["fixed"]
    dx, dy = L.deviation(bd.x, bd.y, bo)
    s = (f'    Rung("{r.builder}", {r.N}, {b["n"]}, {b["m"]}, {var}, {nb}, {amax}, {ne}, {seed}, {conv}),'
         f"  # fixed: dense vs oracle x {dx:.1e} y {dy:.1e}, status {bo.status_val.tolist()}")
    if conv:
        s += f"; converge: iterations {det['converge'][0].iter.tolist()}"
    if (var, nb, amax, ne, b["n"], b["m"]) != (r.variant, r.nb, r.amax, r.ne, r.n, r.m):
        s += "  <-- differs from RUNGS"
    if (seed, conv) != (r.seed, r.converge):
        s += f"  <-- RUNGS has seed {r.seed}, converge {r.converge}"
    if why:
        s += "\n        # passed over: " + "; ".join(why)
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    import plan_ladder
    with ProcessPoolExecutor(a.jobs) as ex:
        for line in ex.map(row, range(len(plan_ladder.RUNGS))):
            print(line, flush=True)
