"""The one-shot cfg-2 kernel with its factorisation compiled for the headline's plan constants,
against the kernels it must equal to the bit.

The headline instantiation of the fused four-wave kernel (one_shot_form 2, no eliminated columns,
amax = bmax = 5) is GL 5 of solve_wave.hip::solve_w4_body: GL 4 with the out-of-line factorisation
factorize_gq_nl (solve_phases.h::factorize_w4q / gj_q) in place of factorize_gp_nl -- amax, bmax
compile-time constants, the pivot steps compiled once for wave 0 and once for waves 1-3 behind
scalar branches, the F, corner and G products straight-line, one step of lookahead in the pivot
chain.  The floating-point operations, their operands and their order are factorize_w4's, so the
default handle must agree to the bit with an MPCQP_ONE_SHOT_LOOP=roles handle (GL 4, read when the
handle is created) and with a persisting handle.

* the cut: tests/test_one_shot_small.py's 32 instances of mpc.make_batch(2, B=1024, seed=2000)
  (N = 20; it holds the 350-iteration instance).  Per settings variant two setup_solve calls, the
  second with moved bounds (some instances infeasible), on a persisting, a roles and a default
  handle: x, y, status and iteration counts of the default one are bit-identical to the others' in
  both calls, and its first call agrees with the oracle (tests/parity.py::check_agreement).  Under
  adaptive_rho_interval=25 every check may refactor: the oracle shows at least three rho updates
  (refactorisations) on some instance of the two calls (on the second call's bounds; two at most
  on the first's);
* plan_ladder's vanilla builder, B = 3, at N = 18 (the smallest four-block shape: bsize[3] = 3 is
  below amax, so wave 3 has no stage-1 pivot and its corner pivots reach padding rows) and N = 19
  (bsize[3] = 8): default against roles and persisting handles, bit-identical.  A horizon whose plan
  does not take one-shot form 2 on the device is skipped with the form it took;
* a refused factor: one of three N = 20 instances has a diagonal entry of P made negative enough
  that a pivot is not positive.  The instance is refused by status (NaN x, y when the first
  factorisation fails); status and outputs equal the roles and persisting handles'.
"""
import functools

import numpy as np
import pytest

import plan_ladder as L
import pyoracle
from parity import check_agreement
from test_one_shot_roles import _form, _handle
from test_one_shot_small import _batch, _out, _same_bits

VARIANTS = {
    "defaults": {},
    "adaptive_rho_interval=25": dict(adaptive_rho_interval=25),
    "rho=1e-3": dict(rho=1e-3),
    "rho=10": dict(rho=10.0),
    "adaptive_rho=False": dict(adaptive_rho=False),
    "scaling=0": dict(scaling=0),
    "max_iter=110": dict(max_iter=110),
}


@functools.lru_cache(maxsize=None)
def _cut():
    """The 32-instance cut and the second call's bounds (the 1024-instance oracle: once)."""
    bs, s, idx, full = _batch()
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


def _oracle_rho_updates(bs, s, l, u):
    """info.rho_updates per instance under bounds l, u (solve_batch does not return them)."""
    out = []
    for k in range(l.shape[0]):
        P, A = bs["P"].copy(), bs["A"].copy()
        P.data, A.data = bs["Px"][k].copy(), bs["Ax"][k].copy()
        o = pyoracle.OSQP()
        o.setup(P, bs["q"][k], A, l[k], u[k], **s)
        out.append(o.solve().info.rho_updates)
    return out


def _three_handles(P, A, B, s):
    """(persisting, roles, default) handles; the one-shot ones must take form 2 on variant 17 with
    amax = 5 (GL 4 and GL 5 of the headline's shape)."""
    default = _handle(P, A, B, s)
    form, variant, amax = _form(default)
    roles = _handle(P, A, B, s, "roles")
    keep = _handle(P, A, B, s, one_shot=False)
    return keep, roles, default, (form, variant, amax), _form(roles)


@pytest.mark.gpu
@pytest.mark.parametrize("label", list(VARIANTS))
def test_factor_matches_roles_persisting_and_oracle(label):
    import torch
    bs, s, (l2, u2) = _cut()
    kw = VARIANTS[label]
    s = dict(s, **kw)
    bo = pyoracle.solve_batch(bs["P"], bs["A"], bs["Px"], bs["q"], bs["Ax"], bs["l"], bs["u"], nthreads=4, **s)
    print(f"oracle, {label}: iterations {bo.iter.tolist()}")
    if not kw:
        assert bo.iter.max() >= 300, bo.iter
    if label == "adaptive_rho_interval=25":
        ru = [_oracle_rho_updates(bs, s, l, u) for l, u in ((bs["l"], bs["u"]), (l2, u2))]
        print("oracle rho updates, first / second call:", ru)
        assert max(max(r) for r in ru) >= 3, ru
    B = 32
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dPx, dAx, dq = t(bs["Px"]), t(bs["Ax"]), t(bs["q"])
    bounds = [(t(bs["l"]), t(bs["u"])), (t(l2), t(u2))]
    torch.cuda.synchronize()
    keep, roles, default, fd, fr = _three_handles(bs["P"], bs["A"], B, s)
    assert fd == (2, 17, 5) and fr == (2, 17, 5), (fd, fr)
    others = {"persisting": keep, "roles": roles}
    first = None
    for call, (l, u) in enumerate(bounds):
        outs = {k: _out(B, bs["n"], bs["m"], dev) for k in others}
        o = _out(B, bs["n"], bs["m"], dev)
        for k, h in others.items():
            h.setup_solve(dPx, dAx, dq, l, u, *outs[k])
        default.setup_solve(dPx, dAx, dq, l, u, *o)
        torch.cuda.synchronize()
        st = o[2].cpu().numpy()
        print(f"{label}, call {call}: status counts {dict(zip(*np.unique(st, return_counts=True)))}, "
              f"iterations {o[3].cpu().tolist()}")
        for k in others:
            for a, d in zip(outs[k], o):
                assert _same_bits(a, d), (label, call, k)
        if call == 0:
            first = [v.cpu().numpy() for v in o]
    check_agreement(f"cfg2 one-shot factorisation, {label}", bs, first[0], first[1], first[2], first[3], bo)


def _ladder_inputs(b, dev):
    import torch
    from osqp_amd import _drop_common_zeros
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    return P, A, Px, [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (Px, Ax, b["q"], b["l"], b["u"])]


def _run_three(P, A, X, s, n, m, dev, what):
    """One setup_solve on persisting, roles and default handles; the default's outputs, held
    bit-identical to the others'."""
    import torch
    keep, roles, default, fd, fr = _three_handles(P, A, L.B, s)
    if fd[0] != 2:  # (the form is one_shot_form's: the LDS budget of two workgroups per CU)
        pytest.skip(f"{what}: the plan takes one-shot form {fd[0]}, not 2 (variant {fd[1]}, amax {fd[2]})")
    assert fd == (2, 17, 5) and fr == (2, 17, 5), (fd, fr)
    assert keep.plan_info()["variant"] == 17
    ok, orl, o = (_out(L.B, n, m, dev) for _ in range(3))
    keep.setup_solve(*X, *ok)
    roles.setup_solve(*X, *orl)
    default.setup_solve(*X, *o)
    torch.cuda.synchronize()
    print(f"{what}: status {o[2].cpu().tolist()} iterations {o[3].cpu().tolist()}")
    for a, c, d in zip(ok, orl, o):
        assert _same_bits(a, d), (what, "persisting")
        assert _same_bits(c, d), (what, "roles")
    return [v.cpu().numpy() for v in o]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [18, 19])
def test_factor_at_other_block_sizes(N):
    import torch
    b = L.build("vanilla", N, 1)
    assert b["m"] == 9 * N + 8
    dev = torch.device("cuda", 0)
    P, A, _, X = _ladder_inputs(b, dev)
    torch.cuda.synchronize()
    _run_three(P, A, X, L.settings(b, "converge"), b["n"], b["m"], dev, f"vanilla N = {N}")


@pytest.mark.gpu
def test_refused_factor_matches_roles_and_persisting():
    import torch
    b = dict(L.build("vanilla", 20, 1))
    dev = torch.device("cuda", 0)
    from osqp_amd import _drop_common_zeros
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    bad, j = 1, b["n"] // 2  # instance 1, a column of the second block
    rows = P.indices[P.indptr[j]:P.indptr[j + 1]]
    e = int(P.indptr[j] + np.flatnonzero(rows == j)[0])
    Px = Px.copy()
    Px[bad, e] = -1e3  # P + sigma I + rho A'A stays negative there: a pivot <= 0
    b["P"], b["Px"] = P, Px
    P, A, _, X = _ladder_inputs(b, dev)
    torch.cuda.synchronize()
    x, y, st, it = _run_three(P, A, X, L.settings(b, "converge"), b["n"], b["m"], dev, "refused factor, N = 20")
    assert st[bad] != 1, st
    assert np.isnan(x[bad]).all() and np.isnan(y[bad]).all(), (x[bad], y[bad])
    good = [k for k in range(L.B) if k != bad]
    assert np.isfinite(x[good]).all() and np.isfinite(y[good]).all()
