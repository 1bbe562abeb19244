"""The one-shot cfg-2 kernel's new instantiation against the one it replaces and the persisting kernel.

The headline instantiation of the fused four-wave kernel (one_shot_form 2, no eliminated columns,
amax <= 5) issues the loop's phase A and phase B reads earlier and takes the Gauss-Jordan pivot by
v_readlane of the lane that publishes it (solve_wave.hip::solve_w4_body, GL 3; solve_phases.h::
gj_seg SEG 3 / 4); the instantiation it replaces (GL 1) stays in the library and is selected by
MPCQP_ONE_SHOT_LOOP=lds, read when the handle is created.  Neither the sums nor their operands
change, so the three kernels must agree to the bit:

* the batch is tests/test_one_shot_small.py's: 32 instances cut from mpc.make_batch(2, B=1024,
  seed=2000) -- the 8 with the highest oracle iteration counts and the first 24 of the others; the
  host oracle must itself show an instance of 300 iterations or more (three refactorisations);
* per settings variant (the defaults and tests/test_one_shot_passes.py's four): two setup_solve calls,
  the second with moved bounds (some instances infeasible), on a persisting handle, an
  MPCQP_ONE_SHOT_LOOP=lds one-shot handle and a default one-shot handle; x, y, status and iteration
  counts of the default one are bit-identical to both others' in both calls;
* the first call of the default handle agrees with the oracle (tests/parity.py::check_agreement).
"""
import os

import numpy as np
import pytest

import pyoracle
from parity import check_agreement
from test_one_shot_small import _batch, _out, _same_bits

VARIANTS = {
    "defaults": {},
    "max_iter=110": dict(max_iter=110),
    "scaled_termination": dict(scaled_termination=True),
    "check_termination=10": dict(check_termination=10),
    "adaptive_rho=False max_iter=500": dict(adaptive_rho=False, max_iter=500),
}


@pytest.fixture(scope="module")
def cut():
    bs, s, idx, full = _batch()  # (the 1024-instance oracle: once per module)
    assert idx.size == 32
    print("oracle iteration counts of the cut:", full.iter[idx].tolist())
    assert full.iter[idx].max() >= 300, full.iter[idx].max()
    rng = np.random.default_rng(2001)  # the second call's bounds (test_one_shot_small.py)
    l2, u2 = bs["l"].copy(), bs["u"].copy()
    fin = np.isfinite(l2) & np.isfinite(u2) & (l2 == u2)
    shift = rng.normal(scale=0.05, size=l2.shape)
    l2[fin] += shift[fin]
    u2[fin] += shift[fin]
    return bs, s, (l2, u2)


def _one_shot_handle(bs, s, lds):
    """A one-shot handle; lds: created under MPCQP_ONE_SHOT_LOOP=lds (read at creation only)."""
    from osqp_amd import DeviceBatch
    old = os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
    try:
        if lds:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = "lds"
        h = DeviceBatch(bs["P"], bs["A"], 32, device=0, **s)
    finally:
        os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
        if old is not None:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = old
    assert h.one_shot(True) == 2
    pi = h.plan_info()
    assert pi["variant"] == 17 and pi["amax"] <= 5, pi
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(VARIANTS))
def test_wave_loop_matches_lds_loop_persisting_and_oracle(cut, label):
    import torch
    from osqp_amd import DeviceBatch
    bs, s, (l2, u2) = cut
    kw = VARIANTS[label]
    s = dict(s, **kw)
    bo = pyoracle.solve_batch(bs["P"], bs["A"], bs["Px"], bs["q"], bs["Ax"], bs["l"], bs["u"], nthreads=4, **s)
    print(f"oracle, {label}: iterations {bo.iter.tolist()}")
    if not kw:
        assert bo.iter.max() >= 300, bo.iter
    B = 32
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dPx, dAx, dq = t(bs["Px"]), t(bs["Ax"]), t(bs["q"])
    bounds = [(t(bs["l"]), t(bs["u"])), (t(l2), t(u2))]
    torch.cuda.synchronize()
    keep = DeviceBatch(bs["P"], bs["A"], B, device=0, **s)
    lds, wave = _one_shot_handle(bs, s, True), _one_shot_handle(bs, s, False)
    first = None
    for call, (l, u) in enumerate(bounds):
        ok, ol, ow = (_out(B, bs["n"], bs["m"], dev) for _ in range(3))
        keep.setup_solve(dPx, dAx, dq, l, u, *ok)
        lds.setup_solve(dPx, dAx, dq, l, u, *ol)
        wave.setup_solve(dPx, dAx, dq, l, u, *ow)
        torch.cuda.synchronize()
        st = ow[2].cpu().numpy()
        print(f"{label}, call {call}: status counts {dict(zip(*np.unique(st, return_counts=True)))}, "
              f"iterations {ow[3].cpu().tolist()}")
        for a, c, d in zip(ok, ol, ow):
            assert _same_bits(a, d), (label, call, "persisting")
            assert _same_bits(c, d), (label, call, "lds loop")
        if call == 0:
            first = [v.cpu().numpy() for v in ow]
    check_agreement(f"cfg2 one-shot wave loop, {label}", bs, first[0], first[1], first[2], first[3], bo)
