"""The one-shot cfg-2 kernel on a small batch, against the persisting kernel and the oracle.

The headline instantiation of the fused four-wave kernel (one_shot_form 2, no eliminated columns,
amax <= 5) keeps its S_k^{-1} tiles in a swizzled LDS layout (solve_phases.h::tile_at); the
persisting kernel keeps them row-major.  tests/test_one_shot.py holds the two bit-identical on the
full batch; this test does it on 32 instances chosen to go through every swizzled accessor several
times, and adds the direct check against the oracle that the one-shot kernel lacked:

* the batch: cut from mpc.make_batch(2, B=1024, seed=2000) -- the 8 instances with the highest
  oracle iteration counts and the first 24 of the others.  The oracle (run here, on the host)
  must itself show an instance of 300 iterations or more: three rho updates, so three
  refactorisations into the swizzled tiles, each with its store-back, F_k products and run starts;
* two calls, the second with moved bounds (test_one_shot.py::_inputs), which leaves some
  instances infeasible;
* the one-shot handle's x, y, status and iteration counts are bit-identical to a persisting
  handle's in both calls;
* the first call's one-shot outputs agree with the oracle (tests/parity.py::check_agreement:
  status and iteration counts equal, ||u - u_ref||_inf < 1e-4).
"""
import numpy as np
import pytest

import pyoracle
from osqp_amd import mpc
from parity import check_agreement


def _batch():
    from osqp_amd import _drop_common_zeros
    b = mpc.make_batch(2, B=1024, seed=2000)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    full = pyoracle.solve_batch(P, A, Px, b["q"], Ax, b["l"], b["u"], nthreads=8, **s)
    top = np.argsort(-full.iter, kind="stable")[:8]
    rest = np.setdiff1d(np.arange(1024), top)[:24]
    idx = np.concatenate([top, rest])
    cut = lambda v: np.ascontiguousarray(v[idx]) if np.ndim(v) == 2 else v  # noqa: E731
    bs = dict(b, P=P, A=A, Px=cut(Px), Ax=cut(Ax), q=cut(b["q"]), l=cut(b["l"]), u=cut(b["u"]))
    return bs, s, idx, full


def _out(B, n, m, dev):
    import torch
    return (torch.empty((B, n), dtype=torch.float64, device=dev), torch.empty((B, m), dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


def _same_bits(a, c):
    """Bit-identical, NaN outputs of unsolved instances included; else which instances differ."""
    import torch
    ab, cb = (t.view(torch.int64) if t.dtype == torch.float64 else t for t in (a, c))
    if torch.equal(ab, cb):
        return True
    rows = (ab != cb).reshape(ab.shape[0], -1).any(1).nonzero().flatten().tolist()
    raise AssertionError(f"{len(rows)} instances differ, first {rows[:8]}")


@pytest.mark.gpu
def test_one_shot_small_batch_matches_persisting_and_oracle():
    import torch
    from osqp_amd import DeviceBatch
    bs, s, idx, full = _batch()
    B = idx.size
    assert B == 32
    print("oracle iteration counts of the cut:", full.iter[idx].tolist())
    assert full.iter[idx].max() >= 300, full.iter[idx].max()
    Px, Ax = bs["Px"], bs["Ax"]
    assert Px.shape == (B, bs["P"].nnz) and Ax.shape == (B, bs["A"].nnz)
    bo = pyoracle.solve_batch(bs["P"], bs["A"], Px, bs["q"], Ax, bs["l"], bs["u"], nthreads=4, **s)
    assert np.array_equal(bo.iter, full.iter[idx])

    # the second call's bounds: the first call's, moved (test_one_shot.py::_inputs)
    rng = np.random.default_rng(2001)
    l2, u2 = bs["l"].copy(), bs["u"].copy()
    fin = np.isfinite(l2) & np.isfinite(u2) & (l2 == u2)
    shift = rng.normal(scale=0.05, size=l2.shape)
    l2[fin] += shift[fin]
    u2[fin] += shift[fin]

    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dPx, dAx, dq = t(Px), t(Ax), t(bs["q"])
    bounds = [(t(bs["l"]), t(bs["u"])), (t(l2), t(u2))]
    torch.cuda.synchronize()
    keep, one = DeviceBatch(bs["P"], bs["A"], B, device=0, **s), DeviceBatch(bs["P"], bs["A"], B, device=0, **s)
    assert one.one_shot(True) == 2
    pi = one.plan_info()
    assert pi["variant"] == 17 and pi["amax"] <= 5, pi  # the swizzled instantiation
    first = None
    for call, (l, u) in enumerate(bounds):
        o1, o2 = _out(B, bs["n"], bs["m"], dev), _out(B, bs["n"], bs["m"], dev)
        keep.setup_solve(dPx, dAx, dq, l, u, *o1)
        one.setup_solve(dPx, dAx, dq, l, u, *o2)
        torch.cuda.synchronize()
        st = o1[2].cpu().numpy()
        print(f"call {call}: status counts {dict(zip(*np.unique(st, return_counts=True)))}, "
              f"max iterations {int(o1[3].max())}")
        for a, c in zip(o1, o2):
            assert _same_bits(a, c), (call, np.unique(st, return_counts=True))
        if call == 0:
            first = [v.cpu().numpy() for v in o2]
    check_agreement("cfg2 one-shot, 32 of seed 2000 (8 slowest + 24)", bs, first[0], first[1], first[2], first[3], bo)
