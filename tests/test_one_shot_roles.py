"""The one-shot cfg-2 kernel with its ADMM loop compiled once per wave role, against the kernels it
must equal to the bit.

The headline instantiation of the fused four-wave kernel (one_shot_form 2, no eliminated columns,
amax <= 5) is GL 4 of solve_wave.hip::solve_w4_body: GL 3 with the run's loop compiled four times,
once per wave index (admm_run<W>, solve_w4_run.inc), so that what serves the other waves' roles
leaves each wave's path.  Only control flow on compile-time constants folds: every floating-point
operation that reaches x, y, z, w, rb, tv or xt is the general loop's, operand for operand
(DESIGN.md §21).  The loop it replaces stays in the library as MPCQP_ONE_SHOT_LOOP=wave (GL 3), next
to MPCQP_ONE_SHOT_LOOP=lds (GL 1); both are read when the handle is created.

* the cut: tests/test_one_shot_small.py's 32 instances of mpc.make_batch(2, B=1024, seed=2000); the
  host oracle must show an instance of 300 iterations or more (three refactorisations).  Per
  settings variant of tests/test_one_shot_wave.py, two setup_solve calls (the second with moved
  bounds: some instances infeasible) on four handles -- persisting, lds, wave, default; x, y,
  status and iteration counts of the default one are bit-identical to each of the others' in both
  calls, and its first call agrees with the oracle (tests/parity.py::check_agreement);
* row ownership: which waves own rows changes with m (vanilla layout: m = 9 N + 8, 64 rows per
  wave).  At N = 18 (m = 170) waves 0-2 own rows; at N = 21 (m = 197) and N = 22 (m = 206) wave
  3 does too; N = 20 (m = 188, the cut's) lies between.  plan_ladder's vanilla builder, B = 3;
  N = 18 with the ladder's seed, N = 22 with seed 1, at which the oracle solves all three
  instances (275, 75 and 25 iterations; checked on the host and asserted here).  The default
  handle is bit-identical to the persisting and wave handles and agrees with the oracle.  A
  horizon whose plan does not take one-shot form 2 on the device is skipped with the form it
  took.  On the MI355X that is N = 22's case: it takes form 3 (the G blocks and y no longer fit
  the LDS budget of two workgroups per CU), and so did N = 21 when tried, so on this layout no
  horizon reaches the role loops with wave 3 owning rows; N = 22 stays here for a device or a
  budget where it does.
"""
import os

import numpy as np
import pytest

import plan_ladder as L
import pyoracle
from parity import check_agreement
from test_one_shot_small import _batch, _out, _same_bits
from test_one_shot_wave import VARIANTS

LOOPS = (None, "lds", "wave")  # MPCQP_ONE_SHOT_LOOP at creation (None: the default, GL 4)
HORIZON_SEED = {18: next(r.seed for r in L.RUNGS if (r.builder, r.N) == ("vanilla", 18)), 22: 1}


def _handle(P, A, B, s, loop=None, one_shot=True):
    """A handle created under MPCQP_ONE_SHOT_LOOP=loop (read at creation only); one_shot False:
    the persisting kernel."""
    from osqp_amd import DeviceBatch
    old = os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
    try:
        if loop:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = loop
        h = DeviceBatch(P, A, B, device=0, **s)
    finally:
        os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
        if old is not None:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = old
    return h


def _form(h):
    """(one-shot form, variant, amax) after asking the handle for the one-shot form."""
    form = h.one_shot(True)
    pi = h.plan_info()
    return form, pi["variant"], pi["amax"]


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


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(VARIANTS))
def test_role_loops_match_wave_lds_persisting_and_oracle(cut, label):
    import torch
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
    others = {"persisting": _handle(bs["P"], bs["A"], B, s, one_shot=False)}
    for loop in LOOPS:
        h = _handle(bs["P"], bs["A"], B, s, loop)
        form, variant, amax = _form(h)
        assert form == 2 and variant == 17 and amax <= 5, (loop, form, variant, amax)
        others[loop or "default"] = h
    roles = others.pop("default")
    first = None
    for call, (l, u) in enumerate(bounds):
        outs = {k: _out(B, bs["n"], bs["m"], dev) for k in others}
        o = _out(B, bs["n"], bs["m"], dev)
        for k, h in others.items():
            h.setup_solve(dPx, dAx, dq, l, u, *outs[k])
        roles.setup_solve(dPx, dAx, dq, l, u, *o)
        torch.cuda.synchronize()
        st = o[2].cpu().numpy()
        print(f"{label}, call {call}: status counts {dict(zip(*np.unique(st, return_counts=True)))}, "
              f"iterations {o[3].cpu().tolist()}")
        for k in others:
            for a, d in zip(outs[k], o):
                assert _same_bits(a, d), (label, call, k)
        if call == 0:
            first = [v.cpu().numpy() for v in o]
    check_agreement(f"cfg2 one-shot role loops, {label}", bs, first[0], first[1], first[2], first[3], bo)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [18, 22])
def test_role_loops_at_other_row_ownerships(N):
    import torch
    from osqp_amd import _drop_common_zeros
    b = L.build("vanilla", N, HORIZON_SEED[N])
    assert b["m"] == 9 * N + 8
    s = L.settings(b, "converge")
    bo = L.solve_oracle(b, "converge")
    print(f"N = {N}, m = {b['m']}: oracle status {bo.status_val.tolist()} iterations {bo.iter.tolist()}")
    assert (bo.status_val == 1).all(), bo.status_val
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    dev = torch.device("cuda", 0)
    X = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (Px, Ax, b["q"], b["l"], b["u"])]
    torch.cuda.synchronize()
    roles = _handle(P, A, L.B, s)
    form, variant, amax = _form(roles)
    if form != 2:  # (the form is one_shot_form's: the LDS budget of two workgroups per CU)
        pytest.skip(f"N = {N}: the plan takes one-shot form {form}, not 2 (variant {variant}, amax {amax})")
    assert variant == 17 and amax <= 5, (variant, amax)
    wave = _handle(P, A, L.B, s, "wave")
    assert _form(wave) == (2, 17, amax)
    keep = _handle(P, A, L.B, s, one_shot=False)
    assert keep.plan_info()["variant"] == 17
    ok, ow, o = (_out(L.B, b["n"], b["m"], dev) for _ in range(3))
    keep.setup_solve(*X, *ok)
    wave.setup_solve(*X, *ow)
    roles.setup_solve(*X, *o)
    torch.cuda.synchronize()
    print(f"N = {N}: status {o[2].cpu().tolist()} iterations {o[3].cpu().tolist()}")
    for a, c, d in zip(ok, ow, o):
        assert _same_bits(a, d), (N, "persisting")
        assert _same_bits(c, d), (N, "wave loop")
    x, y, st, it = (v.cpu().numpy() for v in o)
    check_agreement(f"cfg2 one-shot role loops, vanilla N = {N}", b, x, y, st, it, bo)
