"""The frozen-model closed loop on the device (csrc/mpc_device.hip: k_kin_frozen_tail;
osqp_amd.mpc.kinfrozen_rollout / kinfrozen_tail, osqp_amd.mpc_device.KinematicFrozenMPC) against the
reference's own fixtures of Control/MPC/mpc_kinematics.py:main (tests/golden/make_golden_loops.py):

  kinfrozen_sim_n2.npz, kinfrozen_sim_n3.npz, kinfrozen_sim_n20.npz  three steps of main (numpy
                       seed 0): the initial pred_u / pred_x, each step's inputs, QP, solution
                       (the oracle's, behind the osqp stub) and state after the tail
  kinfrozen_sim_n100.npz  two steps at main's own N = 100
  kinfrozen_run_n20.npz   30 steps at N = 20: plt_states / plt_actions and their sensitivity to
                       the solver tolerance (traj_sens)

What main does (the fixtures decide, not its comments): one linearisation per step, at the
current (x, u) with u the control applied last, on every stage; pred_x takes the solution's
states with no shift; the plant steps with that same linear model.  Its initial rollout advances
the plant state in place (x0 IS x), so the loop starts from pred_x stage N-1.

Whole-run check (test_whole_run_within_solver_tolerance), measured on an MI355X: largest
|device - fixture| per column (x, y, v, yaw, steer, accel) over the 30 rows 2.7e-15, 8.9e-16,
1.3e-14, 7.2e-16, 1.2e-14, 2.6e-13, against traj_sens 4.8e-8, 1.9e-7, 9.4e-9, 8.6e-7, 8.2e-6,
1.9e-7.
"""
import ctypes as C
import json

import numpy as np
import pytest

from loop_checks import (EINVAL, EUNSUPPORTED, check_assembled, check_fixture_step, check_solutions, check_whole_run,
                         dense, dev as _t, host, oracle_batch, oracle_solve, same_csc as _same_csc, sim_qp as _sim_qp)
from osqp_amd import mpc
from osqp_amd.mpc_device import LTVLayout, _bind

L_F, L_R, DT = 1.25, 1.40, 0.02  # main's vehicle (:270-283)
VEH = (L_F, L_R, DT)
W = (mpc.KINFROZEN_Q, mpc.KINFROZEN_QN, mpc.KINFROZEN_R)
BOUNDS = (mpc.KINFROZEN_XMIN, mpc.KINFROZEN_XMAX, mpc.KINFROZEN_UMIN, mpc.KINFROZEN_UMAX)
SETTINGS = dict(polish=False, warm_start=True)  # :195
SIMS = [("kinfrozen_sim_n2.npz", 2), ("kinfrozen_sim_n3.npz", 3), ("kinfrozen_sim_n20.npz", 20),
        ("kinfrozen_sim_n100.npz", 100)]


def _layout(N, **kw):
    return LTVLayout(N, *W, *BOUNDS, mpc.KIN_MASK_A, mpc.KIN_MASK_B, **kw)


def _qp(Ad, Bd, gd, x, Xr, N):
    """mpc (:148-191): the one model on every stage."""
    return mpc.ltv_qp([Ad] * N, [Bd] * N, [gd] * N, x, Xr, *W, N, *BOUNDS)


def _search(path_x, path_y, pred_x):
    """main's reference_search (:39-81: speed 10, yaw 0) on pred_x (N+1, 4)."""
    return mpc.reference_search_paths(path_x[None], path_y[None], None, None, [10.0], pred_x[None], DT)[0]


def _model(x, u):
    return tuple(v[0] for v in mpc.linearise_kinematics(*VEH, x, u))


def loop(x0, u0, pred_u0, path_x, path_y, N, steps, solve):
    """main (:268-461) for one vehicle with `solve(P, q, A, l, u) -> x` always `solved`; the rows."""
    pred_x, x = mpc.kinfrozen_rollout(x0, pred_u0, N, *VEH)
    u = np.asarray(u0, float)
    rows = []
    for _ in range(steps):
        Xr = _search(path_x, path_y, pred_x)
        Ad, Bd, gd = _model(x, u)
        sol = solve(*_qp(Ad, Bd, gd, x, Xr, N))
        row, x, u, pred_x, _ = mpc.kinfrozen_tail(sol, 1, Ad, Bd, gd, x, u, pred_x, N)
        rows.append(row)
    return np.stack(rows)


_oracle_solve = oracle_solve(SETTINGS)


# ----------------------------------------------------------------------- CPU tests --
def test_constants_are_the_loops_own():
    """:381-391, inside the loop: QN ends in 50 (100 before the loop, :353), yaw within +-pi."""
    assert np.array_equal(np.diag(mpc.KINFROZEN_Q), [1.0, 1.0, 5.0, 10.0])
    assert np.array_equal(np.diag(mpc.KINFROZEN_QN), [10.0, 10.0, 50.0, 50.0])
    assert np.array_equal(np.diag(mpc.KINFROZEN_R), [0.1, 0.1])
    assert np.array_equal(mpc.KINFROZEN_UMIN, [-np.deg2rad(15), -3.]) and np.array_equal(mpc.KINFROZEN_UMAX,
                                                                                         [np.deg2rad(15), 1.])
    assert np.array_equal(mpc.KINFROZEN_XMIN, [-np.inf, -np.inf, -100., -np.pi])
    assert np.array_equal(mpc.KINFROZEN_XMAX, [np.inf, np.inf, 100., np.pi])


@pytest.mark.parametrize("name,N", SIMS)
def test_sim_steps_restatements_match_reference(golden, name, N):
    """The captured steps of main: the host restatements reproduce the initial horizon and each
    step from its inputs and solution, and mpc.ltv_qp with the KINFROZEN_* constants and the one
    model on every stage reproduces each step's QP exactly."""
    g = golden(name)
    assert json.loads(str(g["settings"])) == dict(verbose=False, warm_start=True)
    T = g["in_x"].shape[0]
    # initial horizon (:318-329): the index is i, column N stays zero, the plant starts at column N-1
    pu0 = g["init_pred_u"].T
    assert np.array_equal(pu0[N], pu0[N - 1]) and np.array_equal(g["x0"], [0.0, 0.0, 5.0, np.deg2rad(30)])
    px0, x_start = mpc.kinfrozen_rollout(g["x0"], pu0, N, *VEH)
    assert np.array_equal(px0[0], g["x0"]) and not px0[N].any()
    assert np.allclose(px0, g["init_pred_x"].T, rtol=1e-12, atol=1e-12)
    assert np.array_equal(x_start, px0[N - 1]) and np.allclose(x_start, g["x_start"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(g["in_x"][0], g["x_start"]) and np.array_equal(g["in_pred_x"][0], g["init_pred_x"])
    assert np.array_equal(g["in_u"][0], g["u0"])
    if N > 2:  # a rollout under pred_u0[i - 1] would differ
        wrong = mpc.kin_update(*VEH, g["x0"], pu0[0])
        assert not np.allclose(wrong, g["init_pred_x"].T[1], rtol=1e-9, atol=1e-9)
    for t in range(T):
        x, u, pred_x = g["in_x"][t], g["in_u"][t], g["in_pred_x"][t].T       # (4,), (2,), (N+1, 4)
        Xr = _search(g["path_x"], g["path_y"], pred_x)
        assert np.array_equal(Xr, g["in_Xr"][t])
        assert (Xr[1] == -5.0).all() and (Xr[2] == 10.0).all() and (Xr[3] == 0.0).all()
        Ad, Bd, gd = _model(x, u)
        assert np.allclose(Ad, g["in_Ad"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(Bd, g["in_Bd"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(gd, g["in_gd"][t], rtol=1e-13, atol=1e-15)
        P, q, A, l, uu = _qp(g["in_Ad"][t], g["in_Bd"][t], g["in_gd"][t], x, g["in_Xr"][t], N)
        Pr, qr, Ar, lr, ur = _sim_qp(g, t)
        assert _same_csc(P, Pr) and _same_csc(A, Ar)
        assert np.array_equal(dense(P), dense(Pr)) and np.array_equal(dense(A), dense(Ar))
        assert np.array_equal(q, qr) and np.array_equal(l, lr) and np.array_equal(uu, ur)
        row, xn, un, pxn, skipped = mpc.kinfrozen_tail(g["sol"][t], 1, g["in_Ad"][t], g["in_Bd"][t], g["in_gd"][t],
                                                       x, u, pred_x, N)
        assert not skipped
        assert np.allclose(xn, g["out_x"][t], rtol=1e-12, atol=1e-12)
        assert np.array_equal(un, g["out_u"][t]) and np.array_equal(row, g["out_row"][t])   # copies: bit for bit
        assert np.array_equal(pxn, g["out_pred_x"][t].T)
        assert np.array_equal(pxn.ravel(), g["sol"][t][:(N + 1) * 4])          # stage 0 is the solution's
        assert np.array_equal(row[:4], x) and np.array_equal(row[4:], g["sol"][t][(N + 1) * 4:(N + 1) * 4 + 2])
    # consecutive steps chain: a step's output is the next step's input
    assert np.array_equal(g["out_x"][:-1], g["in_x"][1:]) and np.array_equal(g["out_u"][:-1], g["in_u"][1:])
    assert np.array_equal(g["out_pred_x"][:-1], g["in_pred_x"][1:])


def test_host_tail_skips_what_is_not_solved():
    rng = np.random.default_rng(0)
    N = 3
    sol, x, u, pred_x = rng.normal(size=22), rng.normal(size=4), rng.normal(size=2), rng.normal(size=(4, 4))
    Ad, Bd, gd = _model(x, u)
    for status in (2, -2, 7, 0):
        row, xn, un, pxn, skipped = mpc.kinfrozen_tail(sol, status, Ad, Bd, gd, x, u, pred_x, N)
        assert skipped and row is None and xn is x and un is u and pxn is pred_x
    assert not mpc.kinfrozen_tail(sol, 1, Ad, Bd, gd, x, u, pred_x, N)[4]


def test_whole_loop_restatement_matches_reference(golden):
    g = golden("kinfrozen_run_n20.npz")
    rows = loop(g["x0"], g["u0"], g["init_pred_u"].T, g["path_x"], g["path_y"], int(g["N"]), int(g["steps"]),
                _oracle_solve)
    assert rows.shape == g["traj"].shape == (30, 6)
    assert np.allclose(rows, g["traj"], rtol=1e-12, atol=1e-12)
    assert (g["traj_sens"] > 0).all()


def _raw_tail(L, B, sol, status, Ad, Bd, gd, x, u, px, skipped, steps, traj, cap, tlen, ptr):
    return _bind().mpcqp_kin_frozen_tail_device(L._h, B, ptr(sol), None if status is None else ptr(status), ptr(Ad),
                                                ptr(Bd), ptr(gd), ptr(x), ptr(u), ptr(px), ptr(skipped), ptr(steps),
                                                ptr(traj), cap, ptr(tlen), None)


def test_argument_errors():
    from osqp_amd import lib
    from osqp_amd.mpc_device import KinematicFrozenMPC
    z, zi = np.zeros(8), np.zeros(2, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    # the frozen tail handed an nx-6 layout: refused before anything is read or launched
    # (the buffers are host arrays that only have to be non-NULL)
    xmin = np.array([-np.inf, -np.inf, -2 * np.pi, -100., -30., -0.5 * np.pi])
    L6 = LTVLayout(4, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, xmin, -xmin, mpc.KINLTV_UMIN, mpc.KINLTV_UMAX, mpc.DYN_MASK_A,
                   mpc.DYN_MASK_B)
    assert _raw_tail(L6, 1, z, None, z, z, z, z, z, z, zi, zi, z, 0, zi, ptr) == EUNSUPPORTED
    assert b"nx 4" in lib().mpcqp_last_error()
    L4 = _layout(4)
    assert _raw_tail(L4, 1, z, None, z, z, z, z, z, z, zi, zi, z, -1, zi, ptr) == EINVAL
    assert _raw_tail(L4, -1, z, None, z, z, z, z, z, z, zi, zi, z, 0, zi, ptr) == EINVAL
    assert _raw_tail(L4, 1, z, None, z, z, z, z, z, z, zi, zi, z, 0, zi, lambda a: None) == EINVAL
    assert _raw_tail(L4, 0, z, None, z, z, z, z, z, z, zi, zi, z, 0, zi, ptr) == 0        # B = 0: nothing to do
    assert not z.any() and not zi.any()
    px = np.linspace(0, 10, 5)
    with pytest.raises(ValueError):      # checked before anything touches a device
        KinematicFrozenMPC(np.zeros((2, 4)), np.zeros((2, 2)), px, px, N=4, pred_u0=np.zeros((2, 4, 2)))
    with pytest.raises(TypeError, match="no shift"):
        KinematicFrozenMPC(np.zeros((2, 4)), np.zeros((2, 2)), px, px, N=4, shift_warm=True)


# ------------------------------------------------------------------------- GPU tests --
def _tail(L, sol, status, Ad, Bd, gd, x, u, px, skipped, steps, traj, cap, tlen):
    """mpcqp_kin_frozen_tail_device on device tensors, on the null stream; returns the call's code."""
    import torch
    from osqp_amd.mpc_device import _p
    code = _raw_tail(L, x.shape[0], sol, status, Ad, Bd, gd, x, u, px, skipped, steps, traj, cap, tlen, _p)
    torch.cuda.synchronize()
    return code


def _host_case(N, B, seed):
    """B seeded (state, model, solution) cases at horizon N with the host tail's results."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-5, 5, B), rng.uniform(-5, 5, B), rng.uniform(2, 25, B), rng.uniform(-1, 1, B)], 1)
    u = np.stack([np.deg2rad(rng.uniform(-10, 10, B)), rng.uniform(-2, 1, B)], 1)
    Ad0, Bd0, gd0 = mpc.linearise_kinematics(*VEH, x, u)
    sol = rng.uniform(-1, 1, (B, (N + 1) * 4 + N * 2))
    sol[:, 2:(N + 1) * 4:4] += 10.0
    return x, u, Ad0, Bd0, gd0, sol


def _lists(Ad0, Bd0, gd0, N):
    """(B, N, ..) lists as the assembly takes them; only stage 0 may be read by the tail."""
    Ad, Bd, gd = (np.ascontiguousarray(np.repeat(v[:, None], N, 1)) for v in (Ad0, Bd0, gd0))
    Ad[:, 1:] += 1.0; Bd[:, 1:] -= 1.0; gd[:, 1:] += 3.0
    return Ad, Bd, gd


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3, 20])
def test_tail_matches_host(golden, N, B):
    """k_kin_frozen_tail against the fixture's own post-tail state (the captured steps of main take
    the first places of the batch) and, for the seeded rest, against mpc.kinfrozen_tail; the
    record stops at traj_cap (every third vehicle's is already full)."""
    import torch
    x, u, Ad0, Bd0, gd0, sol = _host_case(N, B, 100 * N + B)
    g = golden(f"kinfrozen_sim_n{N}.npz")
    T = min(B, 3)
    x[:T], u[:T], sol[:T] = g["in_x"][:T], g["in_u"][:T], g["sol"][:T]
    Ad0[:T], Bd0[:T], gd0[:T] = g["in_Ad"][:T], g["in_Bd"][:T], g["in_gd"][:T]
    want = [mpc.kinfrozen_tail(sol[b], 1, Ad0[b], Bd0[b], gd0[b], x[b], u[b], None, N) for b in range(B)]
    rows, xn, un, pxn = (np.stack([w[i] for w in want]) for i in range(4))
    xn[:T], un[:T], pxn[:T], rows[:T] = g["out_x"][:T], g["out_u"][:T], g["out_pred_x"][:T].transpose(0, 2, 1), \
        g["out_row"][:T]
    Ad, Bd, gd = _lists(Ad0, Bd0, gd0, N)
    cap = 2
    tlen0 = np.array([0, 1, 2], np.int32)[np.arange(B) % 3]
    rng = np.random.default_rng(1)
    traj0 = rng.normal(size=(B, cap, 6))
    xd, ud, px = _t(x), _t(u), _t(rng.normal(size=(B, N + 1, 4)))
    skipped, steps = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2))
    traj, tlen = _t(traj0), _t(tlen0, torch.int32)
    L = _layout(N)
    assert _tail(L, _t(sol), None, _t(Ad), _t(Bd), _t(gd), xd, ud, px, skipped, steps, traj, cap, tlen) == 0
    assert np.allclose(xd.cpu().numpy(), xn, rtol=1e-12, atol=1e-12)
    assert np.array_equal(ud.cpu().numpy(), un)
    assert np.array_equal(px.cpu().numpy(), pxn)                               # copies: bit for bit
    assert np.array_equal(px.cpu().numpy().reshape(B, -1), sol[:, :(N + 1) * 4])
    want_traj = traj0.copy()
    room = tlen0 < cap
    want_traj[room, tlen0[room]] = rows[room]
    assert np.array_equal(traj.cpu().numpy(), want_traj)                       # a full record is not written
    assert np.array_equal(tlen.cpu().numpy(), np.minimum(tlen0 + 1, cap))
    assert (steps == 1).all() and not skipped.any()


@pytest.mark.gpu
def test_skip_rule_at_the_entry_point():
    """A crafted status vector: every vehicle whose status is not 1 (solved inaccurate 2, max
    iterations -2, an unknown 7) keeps all its state bit for bit and counts one skip; the
    others equal an all-solved call."""
    import torch
    N, B = 5, 130
    x, u, Ad0, Bd0, gd0, sol = _host_case(N, B, 9)
    Ad, Bd, gd = _lists(Ad0, Bd0, gd0, N)
    status = np.array([1, 2, -2, 7, 1, 1, -2], np.int32)[np.arange(B) % 7]
    ok = status == 1
    L = _layout(N)
    rng = np.random.default_rng(3)
    px0, traj0 = rng.normal(size=(B, N + 1, 4)), rng.normal(size=(B, 3, 6))

    def run(st):
        s = dict(x=_t(x), u=_t(u), px=_t(px0), traj=_t(traj0),
                 skipped=torch.zeros(B, dtype=torch.int32, device="cuda"),
                 steps=torch.full((B,), 4, dtype=torch.int32, device="cuda"),
                 tlen=torch.ones(B, dtype=torch.int32, device="cuda"))
        assert _tail(L, _t(sol), None if st is None else _t(st, torch.int32), _t(Ad), _t(Bd), _t(gd), s["x"], s["u"],
                     s["px"], s["skipped"], s["steps"], s["traj"], 3, s["tlen"]) == 0
        return {k: v.cpu().numpy() for k, v in s.items()}

    got, ref = run(status), run(None)
    for k, before in (("x", x), ("u", u), ("px", px0), ("traj", traj0)):
        assert np.array_equal(got[k][~ok], before[~ok]), k
        assert np.array_equal(got[k][ok], ref[k][ok]), k
        assert not np.array_equal(ref[k][~ok], before[~ok]), k
    assert np.array_equal(got["skipped"], (~ok).astype(np.int32)) and not ref["skipped"].any()
    assert np.array_equal(got["steps"], 4 + ok) and (ref["steps"] == 5).all()
    assert np.array_equal(got["tlen"], 1 + ok) and (ref["tlen"] == 2).all()


def _starts(B, N):
    """Distinct starts beside main's path (y = -5) and a seeded initial pred_u (the script's noise)."""
    x0 = np.zeros((B, 4))
    x0[:, 0] = np.linspace(0.0, 40.0, B)
    x0[:, 1] = -5.0 + np.array([5.0, 1.0, -2.0, 3.5, -4.0, 2.0])[np.arange(B) % 6]
    x0[:, 2] = np.array([5.0, 12.0, 8.0, 15.0, 10.0, 18.0])[np.arange(B) % 6]
    x0[:, 3] = np.deg2rad([30.0, 4.0, -3.0, -6.0, 8.0, 1.0])[np.arange(B) % 6]
    u0 = np.tile([0.0, 0.01], (B, 1)); u0[1::2, 0] = np.deg2rad(1.0)
    rng = np.random.default_rng(7)
    pred_u0 = u0[:, None] + rng.normal(0.0, [np.deg2rad(1), 0.1], (B, N + 1, 2))
    pred_u0[:, N] = pred_u0[:, N - 1]
    return x0, u0, pred_u0


def _main_path():
    px = np.linspace(-10, 100, 200)
    return px, px * 0.0 - 5.0


def _state(ctl):
    return tuple(v.cpu().numpy() for v in (ctl.x, ctl.u, ctl.pred_x))


def _check_step(ctl, before, N, status, Ppat, Apat, Px):
    """One step of the class against the host restatement fed the device's own state, the oracle
    on that QP, and the host tail of the device's own solution."""
    x, u, pred_x = before
    px, py = ctl.path_x.cpu().numpy(), ctl.path_y.cpu().numpy()
    B = x.shape[0]
    last, sol = host(ctl)
    for b in range(B):
        Xr = _search(px, py, pred_x[b])
        assert np.array_equal(last["Xr"][b], Xr)
        Ad, Bd, gd = _model(x[b], u[b])
        assert last["Ad"][b].shape == (N, 4, 4)                               # the one model on every stage
        assert all(np.array_equal(last[k][b], np.repeat(last[k][b][:1], N, 0)) for k in ("Ad", "Bd", "gd"))
        check_assembled(last, b, Ad[None], Bd[None], gd[None], _qp(Ad, Bd, gd, x[b], Xr, N), Apat)
    ro = oracle_batch(last, status, Ppat, Apat, Px, SETTINGS)
    check_solutions(sol, ro.x, slice((N + 1) * 4, None))
    for b in range(B):
        row, xn, un, pxn, _ = mpc.kinfrozen_tail(sol[b], 1, last["Ad"][b, 0], last["Bd"][b, 0], last["gd"][b, 0], x[b],
                                                 u[b], pred_x[b], N)
        assert np.allclose(ctl.x[b].cpu().numpy(), xn, rtol=1e-13, atol=1e-13)
        assert np.array_equal(ctl.u[b].cpu().numpy(), un)
        assert np.array_equal(ctl.pred_x[b].cpu().numpy(), pxn)
    return ro


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 20])
def test_closed_loop_matches_host_restatement(N):
    from osqp_amd.mpc_device import KinematicFrozenMPC
    B, steps = 6, 4
    x0, u0, pred_u0 = _starts(B, N)
    px, py = _main_path()
    ctl = KinematicFrozenMPC(x0, u0, px, py, N=N, pred_u0=pred_u0, traj_cap=3)
    print(f"plan_info N={N}:", ctl.solver.plan_info())
    for b in range(B):
        wx, xs = mpc.kinfrozen_rollout(x0[b], pred_u0[b], N, *VEH)
        assert np.allclose(ctl.pred_x[b].cpu().numpy(), wx, rtol=1e-12, atol=1e-12)
        assert np.allclose(ctl.x[b].cpu().numpy(), xs, rtol=1e-12, atol=1e-12) and not ctl.pred_x[b, N].any()
    assert np.array_equal(ctl.u.cpu().numpy(), u0)
    P, Apat, _, _ = ctl.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    rows = []
    n_iter_match = 0
    for _ in range(steps):
        before = _state(ctl)
        status, iters = ctl.step()
        ro = _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, Px)
        n_iter_match += int((iters.cpu().numpy() == ro.iter).sum())
        rows.append(np.concatenate([before[0], ctl.u.cpu().numpy()], 1))
    assert n_iter_match >= 0.9 * B * steps
    assert (ctl.steps_taken.cpu().numpy() == steps).all() and not ctl.skipped.any()
    # trajectory cap: rows beyond traj_cap are dropped
    traj, tlen = ctl.trajectories()
    assert traj.shape == (B, 3, 6) and np.array_equal(tlen, np.full(B, 3))
    assert np.array_equal(traj, np.stack(rows[:3], 1))
    # the default pred_u0 is u0 in every stage
    dflt = KinematicFrozenMPC(x0[:2], u0[:2], px, py, N=N)
    wx, xs = mpc.kinfrozen_rollout(x0[1], np.tile(u0[1], (N + 1, 1)), N, *VEH)
    assert np.allclose(dflt.pred_x[1].cpu().numpy(), wx, rtol=1e-12, atol=1e-12)
    assert np.allclose(dflt.x[1].cpu().numpy(), xs, rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_one_step_at_the_shipped_horizon(golden):
    """N = 100 (main's own), B = 2: vehicle 0 is the fixture's first step, vehicle 1 its second
    (state and horizon set from the fixture)."""
    from osqp_amd.mpc_device import KinematicFrozenMPC
    g = golden("kinfrozen_sim_n100.npz")
    N = 100
    ctl = KinematicFrozenMPC(np.tile(g["x0"], (2, 1)), np.tile(g["u0"], (2, 1)), g["path_x"], g["path_y"],
                             pred_u0=np.tile(g["init_pred_u"].T, (2, 1, 1)))
    assert ctl.N == N
    info = ctl.solver.plan_info()
    print("plan_info N=100:", info)
    assert info["lds_bytes_solve"] <= 160 * 1024
    assert np.allclose(ctl.pred_x[0].cpu().numpy(), g["in_pred_x"][0].T, rtol=1e-12, atol=1e-12)
    assert np.allclose(ctl.x[0].cpu().numpy(), g["in_x"][0], rtol=1e-12, atol=1e-12)
    ctl.x[1] = _t(g["in_x"][1]); ctl.u[1] = _t(g["in_u"][1]); ctl.pred_x[1] = _t(g["in_pred_x"][1].T)
    P, Apat, _, _ = ctl.layout.pattern()
    before = _state(ctl)
    status, iters = ctl.step()
    _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, np.tile(P.data, (2, 1)))
    check_fixture_step(ctl, g, Apat, slice((N + 1) * 4, None))
    print("iters", iters.cpu().numpy(), "fixture", g["sol_iter"])


@pytest.mark.gpu
def test_skip_rule_at_the_class():
    """max_iter = 10: no solve ends `solved`, so nothing moves and every step counts as skipped."""
    from osqp_amd.mpc_device import KinematicFrozenMPC
    x0, u0, pred_u0 = _starts(3, 10)
    px, py = _main_path()
    ctl = KinematicFrozenMPC(x0, u0, px, py, N=10, pred_u0=pred_u0, traj_cap=4, max_iter=10)
    before = _state(ctl)
    for _ in range(3):
        status, _ = ctl.step()
        assert (status.cpu().numpy() != 1).all()
    after = _state(ctl)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(ctl.u.cpu().numpy(), u0)
    assert (ctl.steps_taken.cpu().numpy() == 0).all() and (ctl.skipped.cpu().numpy() == 3).all()
    traj, tlen = ctl.trajectories()
    assert not traj.any() and not tlen.any()


@pytest.mark.gpu
def test_whole_run_within_solver_tolerance(golden):
    """The 30-step run of kinfrozen_run_n20.npz on the device: rounding inside ADMM must move the
    trajectory less than the solver tolerance does (traj_sens: the same run of the reference with
    the oracle at eps 1e-6 against eps 1e-3).  Two copies of the vehicle stay identical."""
    from osqp_amd.mpc_device import KinematicFrozenMPC
    g = golden("kinfrozen_run_n20.npz")
    steps = int(g["steps"])
    ctl = KinematicFrozenMPC(np.tile(g["x0"], (2, 1)), np.tile(g["u0"], (2, 1)), g["path_x"], g["path_y"],
                             N=int(g["N"]), pred_u0=np.tile(g["init_pred_u"].T, (2, 1, 1)), traj_cap=steps + 2)
    status, _ = ctl.run(steps)
    traj, tlen = ctl.trajectories()
    assert np.array_equal(tlen, [steps, steps]) and not ctl.skipped.any() and (status.cpu().numpy() == 1).all()
    check_whole_run(traj, steps, g)
