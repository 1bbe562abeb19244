"""BASELINE.json's full-size slack workload (configs[2]: 65536 QPs), every instance checked.

The oracle finishes a few hundred of these instances in seconds, not 65536, so at full size
the check is a size-independent property: each returned (x, y) must satisfy OSQP's own
termination test for status "solved" (OSQP 0.6 check_termination, unscaled residuals):

  dual:   ||P x + q + A'y||_inf <= eps_abs + eps_rel * max(||P x||, ||A'y||, ||q||)
  primal: dist(A x, [l, u])_inf <= ||A x - z||_inf <= eps_abs + eps_rel * max(||A x||, ||z||),
          and with ||z|| <= ||A x|| + ||A x - z||:  dist <= (eps_abs + eps_rel ||A x||) / (1 - eps_rel)

computed on the host from the instance's CSC values with numpy, for the first solve and for
a second solve of moved initial states, which the kernel dispatches longest-previous-first
(the order the timed bench steps run in).  The oracle pins a sample of the same batch.
"""
import numpy as np
import pytest

import pyoracle
from loop_checks import stage_shift as _stage_shift
from osqp_amd import OSQPBatch, mpc
from parity import check_agreement, subset, termination_detail as _termination_holds

pytestmark = pytest.mark.gpu  # (the checker itself is CPU-tested: test_fullsize_checker.py)


def test_cfg3_full_batch_meets_the_termination_test():
    b = mpc.make_batch(3)  # configs[2]: B = 65536
    B = b["Px"].shape[0]
    assert B == 65536
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    h = OSQPBatch()
    h.setup(b["P"], b["q"], b["A"], b["l"], b["u"], Px=b["Px"], Ax=b["Ax"], **s)
    r1 = h.solve()
    assert (r1.status_val == 1).all()
    ok_d, ok_p, fd, fp = _termination_holds(b, r1.x, r1.y)
    assert ok_d.all(), (np.flatnonzero(~ok_d)[:10], fd.max())
    assert ok_p.all(), (np.flatnonzero(~ok_p)[:10], fp.max())
    # a receding-horizon step: initial states moved, bounds updated, solved again (warm,
    # dispatched longest-previous-first from the first solve's iteration counts)
    rng = np.random.default_rng(11)
    l, u = b["l"].copy(), b["u"].copy()
    x0 = -l[:, :5] + rng.uniform(-0.02, 0.02, (B, 5))
    l[:, :5] = -x0
    u[:, :5] = -x0
    h.update(l=l, u=u)
    r2 = h.solve()
    assert (r2.status_val == 1).all()
    b2 = dict(b, l=l, u=u)
    ok_d, ok_p, fd, fp = _termination_holds(b2, r2.x, r2.y)
    assert ok_d.all(), (np.flatnonzero(~ok_d)[:10], fd.max())
    assert ok_p.all(), (np.flatnonzero(~ok_p)[:10], fp.max())
    # the oracle on a sample of the first solve
    idx = np.random.default_rng(1).choice(B, 256, replace=False)
    bo = pyoracle.solve_batch(b["P"], b["A"], b["Px"][idx], b["q"][idx], b["Ax"][idx], b["l"][idx], b["u"][idx],
                              nthreads=16, **s)
    check_agreement("cfg3 B=65536, oracle sample 256", subset(b, idx), r1.x[idx], r1.y[idx], r1.status_val[idx],
                    r1.iter[idx], bo)


def test_cfg5_full_batch_warm_meets_the_termination_test():
    """configs[4] at full size (B = 8192 incremental dynamic QPs, N = 50), as bench.py times
    it: a cold solve, then the solution shifted one stage (the warm start of SURVEY.md §8d
    D2) and the next step's QP -- initial states jittered +-2 % of the D2 ranges, as
    bench.py::bound_sequence -- solved from it, dispatched longest-previous-first from the
    cold solve's iteration counts.  Every instance of both solves: status solved (the oracle
    solves a 512-instance sample of this batch cold and warm with no other status) and OSQP's
    termination test recomputed on the host.  An oracle sample of 128 pins the warm solve's
    iteration counts and du."""
    import bench
    b = mpc.make_batch(5)
    B, N = b["Px"].shape[0], b["N"]
    assert B == 8192
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    h = OSQPBatch()
    h.setup(b["P"], b["q"], b["A"], b["l"], b["u"], Px=b["Px"], Ax=b["Ax"], **s)
    r1 = h.solve()
    assert (r1.status_val == 1).all(), np.unique(r1.status_val, return_counts=True)
    ok_d, ok_p, fd, fp = _termination_holds(b, r1.x, r1.y)
    assert ok_d.all(), (np.flatnonzero(~ok_d)[:10], fd.max())
    assert ok_p.all(), (np.flatnonzero(~ok_p)[:10], fp.max())
    xs, ys = _stage_shift(r1.x, N, 8, 2, 1), _stage_shift(r1.y, N, 8, 2, 2)
    x0 = bench.x0_sequence(b, 2, bench.instance_seed(5, 0))[1]
    l, u = b["l"].copy(), b["u"].copy()
    l[:, :x0.shape[1]] = -x0
    u[:, :x0.shape[1]] = -x0
    h.update(l=l, u=u)
    h.warm_start(x=xs, y=ys)
    r2 = h.solve()
    assert (r2.status_val == 1).all(), np.unique(r2.status_val, return_counts=True)
    assert r2.iter.mean() < r1.iter.mean()
    b2 = dict(b, l=l, u=u)
    ok_d, ok_p, fd, fp = _termination_holds(b2, r2.x, r2.y)
    assert ok_d.all(), (np.flatnonzero(~ok_d)[:10], fd.max())
    assert ok_p.all(), (np.flatnonzero(~ok_p)[:10], fp.max())
    idx = np.random.default_rng(2).choice(B, 128, replace=False)
    bo = pyoracle.solve_batch(b["P"], b["A"], b["Px"][idx], b["q"][idx], b["Ax"][idx], l[idx], u[idx],
                              nthreads=16, x0=xs[idx], y0=ys[idx], **s)
    assert (bo.status_val == 1).all()
    # (warm-started long-horizon solves: the iteration counts may part by one check interval on
    # a few instances -- the reduced KKT's rounding over hundreds of iterations, DESIGN.md §3;
    # each such instance is held to the termination test and the eps bound instead)
    def tight(d):  # the sampled instances' optimum: the oracle from the same warm start at eps 1e-9
        j = idx[d]
        return pyoracle.solve_batch(b["P"], b["A"], b["Px"][j], b["q"][j], b["Ax"][j], l[j], u[j], nthreads=16,
                                    x0=xs[j], y0=ys[j], **dict(s, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)).x
    check_agreement("cfg5 B=8192 warm, oracle sample 128", subset(b2, idx), r2.x[idx], r2.y[idx],
                    r2.status_val[idx], r2.iter[idx], bo, min_match=0.97, tight=tight)
