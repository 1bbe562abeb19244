"""The path bank and the lane-change closed loop on the device (csrc/mpc_device.hip:
k_kin_reference_paths, k_lane_tail; osqp_amd.mpc.reference_search_paths / lane_tail / lane_path_id,
osqp_amd.mpc_device.reference_search_paths / LaneChangeMPC) against the reference's own fixtures of
Control/MPC/mpc_increment_kinematics_pred_matrix.py:main (tests/golden/make_golden_loops.py):

  lane_sim_n2.npz, lane_sim_n3.npz, lane_sim_n10.npz  three steps of main with sim_time = 10, one
                       on each side of each path switch (paths 0, 1, 0): inputs, QP, solution
                       (the oracle's, behind the osqp stub), state after the tail
  lane_sim_n40.npz     two steps at main's own N = 40
  lane_run_n10.npz     60 steps at N = 10, switches after steps 10 and 30: plt_states /
                       plt_actions and their sensitivity to the solver tolerance (traj_sens)

The host restatements are checked against the fixtures on CPU, the device kernels on the GPU.

Whole-run check (test_whole_run_within_solver_tolerance), measured on an MI355X: largest
|device - fixture| per column (x, y, v, yaw, steer, accel) over the 60 rows 1.6e-11, 2.8e-11,
4.4e-13, 6.1e-12, 2.0e-12, 1.3e-11, against traj_sens 2.0e-1, 4.4e-1, 4.0e-3, 6.9e-2, 2.9e-2,
1.6e-2.
"""
import ctypes as C
import json

import numpy as np
import pytest

from loop_checks import (EINVAL, EUNSUPPORTED, check_assembled, check_fixture_step, check_solutions, check_whole_run,
                         dense, dev as _t, host, oracle_batch, oracle_solve, same_csc as _same_csc, sim_qp as _sim_qp,
                         stage_shift as _stage_shift)
from osqp_amd import mpc
from osqp_amd.mpc_device import IncrementalLayout, KinVehicle, _bind

L_F, L_R, DT = 1.25, 1.40, 0.02  # main's vehicle (:283-296)
VEH = (L_F, L_R, DT)
W = (mpc.LANE_Q, mpc.LANE_QN, mpc.LANE_R)
BOUNDS = (mpc.LANE_XMIN_T, mpc.LANE_XMAX_T, mpc.LANE_DUMIN, -mpc.LANE_DUMIN)
SETTINGS = dict(polish=False, warm_start=False)  # :242
SIMS = [("lane_sim_n2.npz", 2), ("lane_sim_n3.npz", 3), ("lane_sim_n10.npz", 10), ("lane_sim_n40.npz", 40)]


def _layout(N, **kw):
    return IncrementalLayout(N, *W, *BOUNDS, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B, **kw)


def _qp(Ad, Bd, gd, xt, Xr, N):
    return mpc.incremental_qp(list(Ad), list(Bd), list(gd), xt, Xr, *W, N, *BOUNDS)


def _search(paths_x, paths_y, path_id, pred):
    """main's reference_search (:41-83: speed 10, yaw 0) for one vehicle on path `path_id`."""
    return mpc.reference_search_paths(paths_x, paths_y, None, [path_id], [10.0], pred[None], DT)[0]


def lin_rollout(x0, u0, N):
    """Initial horizon (:350-368): the linearised model rolled forward with zero increments."""
    xt = np.concatenate([x0, u0])
    pred = [xt]
    for _ in range(N):
        Ad, Bd, gd = (v[0] for v in mpc.linearise_kinematics(*VEH, xt[:4], xt[4:]))
        xt = np.concatenate([Ad @ xt[:4] + Bd @ xt[4:] + gd, xt[4:]])
        pred.append(xt)
    return np.stack(pred)


def loop(x0, u0, path_x, paths_y, switch_steps, paths_of, N, steps, solve):
    """main (:281-476) for one vehicle with `solve(P, q, A, l, u) -> x`; the recorded rows."""
    paths_x = np.tile(path_x, (len(paths_y), 1))
    xt, pred, step = np.concatenate([x0, u0]), lin_rollout(x0, u0, N), 0
    pid = int(mpc.lane_path_id(step, switch_steps, paths_of))
    rows = []
    for _ in range(steps):
        Xr = _search(paths_x, paths_y, pid, pred)
        Ad, Bd, gd = mpc.linearise_kinematics(*VEH, pred[:N, :4], pred[:N, 4:])
        sol = solve(*_qp(Ad, Bd, gd, xt, Xr, N))
        row, xt, pred, _, step, pid = mpc.lane_tail(sol, Ad[0], Bd[0], gd[0], xt, step, N, *VEH, switch_steps, paths_of)
        rows.append(row)
    return np.stack(rows)


_oracle_solve = oracle_solve(SETTINGS)


# ----------------------------------------------------------------------- CPU tests --
def test_constants_are_the_scripts():
    """:302-312 against KIN_*: only Q differs."""
    assert np.array_equal(np.diag(mpc.LANE_Q), [50.0, 50.0, 10.0, 50.0])
    assert np.array_equal(np.diag(mpc.LANE_QN), [1000.0, 1000.0, 100.0, 1000.0])
    assert np.array_equal(np.diag(mpc.LANE_R), [100.0, 100.0])
    assert np.array_equal(mpc.LANE_DUMIN, [-np.deg2rad(0.5), -0.5])
    assert np.array_equal(mpc.LANE_XMIN_T, [-np.inf, -np.inf, -100., -2 * np.pi, -np.deg2rad(15), -3.])
    assert np.array_equal(mpc.LANE_XMAX_T, [np.inf, np.inf, 100., 2 * np.pi, np.deg2rad(15), 1.])
    for a, b in ((mpc.LANE_QN, mpc.KIN_QN), (mpc.LANE_R, mpc.KIN_R), (mpc.LANE_DUMIN, mpc.KIN_DUMIN),
                 (mpc.LANE_XMIN_T, mpc.KIN_XMIN_T), (mpc.LANE_XMAX_T, mpc.KIN_XMAX_T)):
        assert np.array_equal(a, b)
    assert not np.array_equal(mpc.LANE_Q, mpc.KIN_Q)
    assert (mpc.LANE_SWITCH_STEPS, mpc.LANE_PATHS_OF) == ((50, 150), (0, 1, 0))


@pytest.mark.parametrize("name,N", SIMS)
def test_sim_steps_restatements_match_reference(golden, name, N):
    """The captured steps of main: the host restatements reproduce each step from its inputs and
    solution, and mpc.incremental_qp with the LANE_* constants reproduces each step's QP exactly."""
    g = golden(name)
    assert json.loads(str(g["settings"])) == dict(verbose=True, polish=False, warm_start=False)
    T = g["in_xt"].shape[0]
    paths_x = np.tile(g["path_x"], (2, 1))
    assert np.allclose(lin_rollout(g["in_xt"][0, :4], g["in_xt"][0, 4:], N), g["in_pred"][0].T, rtol=1e-12, atol=1e-12)
    assert not g["in_pdu"][0].any()
    assert g["in_path_id"].tolist() == [0, 1, 0][:T]
    assert np.array_equal(mpc.lane_path_id(np.arange(T), g["switch_steps"], g["paths_of"]), g["in_path_id"])
    for t in range(T):
        pred, pdu = g["in_pred"][t].T, g["in_pdu"][t].T                    # (N+1, 6), (N+1, 2)
        Xr = _search(paths_x, g["paths_y"], g["in_path_id"][t], pred)
        assert np.array_equal(Xr, g["in_Xr"][t])
        assert (Xr[1] == 4.0 * g["in_path_id"][t]).all() and (Xr[2] == 10.0).all() and (Xr[3] == 0.0).all()
        Ad, Bd, gd = mpc.linearise_kinematics(*VEH, pred[:N, :4], pred[:N, 4:])
        assert np.allclose(Ad, g["in_Ad"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(Bd, g["in_Bd"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(gd, g["in_gd"][t], rtol=1e-13, atol=1e-15)
        P, q, A, l, u = _qp(g["in_Ad"][t], g["in_Bd"][t], g["in_gd"][t], g["in_xt"][t], g["in_Xr"][t], N)
        Pr, qr, Ar, lr, ur = _sim_qp(g, t)
        assert _same_csc(P, Pr) and _same_csc(A, Ar)
        assert np.array_equal(dense(P), dense(Pr)) and np.array_equal(dense(A), dense(Ar))
        assert np.array_equal(q, qr) and np.array_equal(l, lr) and np.array_equal(u, ur)
        row, xt, px, pu, step, pid = mpc.lane_tail(g["sol"][t], g["in_Ad"][t][0], g["in_Bd"][t][0], g["in_gd"][t][0],
                                                   g["in_xt"][t], t, N, *VEH, g["switch_steps"], g["paths_of"])
        assert np.array_equal(row, g["in_xt"][t]) and np.array_equal(row, g["out_row"][t])   # copies: bit for bit
        assert np.allclose(xt, g["out_xt"][t], rtol=1e-12, atol=1e-12)
        assert np.array_equal(xt[4:], g["out_xt"][t][4:])
        assert np.allclose(px, g["out_pred"][t].T, rtol=1e-12, atol=1e-12)
        assert np.array_equal(px[1:N], g["out_pred"][t].T[1:N]) and np.array_equal(px[N, 4:], g["out_pred"][t].T[N, 4:])
        assert np.array_equal(pu, g["out_pdu"][t].T)
        assert step == t + 1 and (t + 1 >= T or pid == g["in_path_id"][t + 1])
    # consecutive steps chain: a step's output is the next step's input
    assert np.array_equal(g["out_xt"][:-1], g["in_xt"][1:]) and np.array_equal(g["out_pred"][:-1], g["in_pred"][1:])
    assert np.array_equal(g["out_pdu"][:-1], g["in_pdu"][1:])


def test_path_schedule_is_strict():
    """The script's `if i > ...`: a step exactly at a threshold is still on the old path."""
    assert mpc.lane_path_id([0, 50, 51, 150, 151, 999]).tolist() == [0, 0, 1, 1, 0, 0]
    assert mpc.lane_path_id([3, 4, 5], (3, 4), (2, 0, 1)).tolist() == [2, 0, 1]
    assert mpc.lane_path_id([7], (), (3,)).tolist() == [3]
    g = np.zeros(4 * 6 + 3 * 2)
    Ad, Bd, gd = (v[0] for v in mpc.linearise_kinematics(*VEH, np.array([0, 0, 10.0, 0]), np.zeros(2)))
    for step, want in ((48, 0), (49, 0), (50, 1), (148, 1), (149, 1), (150, 0)):   # the tail counts first
        _, _, _, _, s1, pid = mpc.lane_tail(g, Ad, Bd, gd, np.zeros(6), step, 3, *VEH)
        assert (s1, pid) == (step + 1, want)


def test_whole_loop_restatement_matches_reference(golden):
    g = golden("lane_run_n10.npz")
    rows = loop(g["x0"], g["u0"], g["path_x"], g["paths_y"], g["switch_steps"], g["paths_of"], int(g["N"]),
                int(g["steps"]), _oracle_solve)
    assert rows.shape == g["traj"].shape == (60, 6)
    assert np.allclose(rows, g["traj"], rtol=1e-12, atol=1e-12)
    assert (g["traj_sens"] > 0).all()
    assert np.array_equal(mpc.lane_path_id(np.arange(60), g["switch_steps"], g["paths_of"]), g["path_id"])


def test_reference_search_paths_holds_the_last_segment_and_clamps():
    px = np.linspace(0.0, 10.0, 11)
    paths_x, paths_y = np.stack([px, px]), np.stack([0 * px, 0 * px + 4])
    pred = np.zeros((4, 4, 6)); pred[:, :, 2] = 30.0
    pred[:, 0, 0] = [2.2, 2.2, 10.4, 2.2]
    Xr = mpc.reference_search_paths(paths_x, paths_y, None, [0, 1, 1, 9], [10.0, 11.0, 12.0, 13.0], pred, 0.05)
    assert np.array_equal(Xr[0, 0], [4.0, 6.0, 7.0, 9.0]) and (Xr[0, 1] == 0).all() and (Xr[1, 1] == 4).all()
    assert (Xr[2, 0] == 9.0).all() and (Xr[2, 1] == 4).all()             # the start of the last segment, held
    assert np.array_equal(Xr[3], Xr[1] + np.array([0, 0, 2.0, 0])[:, None])  # id 9 clamped to path 1
    assert np.array_equal(Xr[:, 2], np.repeat([[10.0], [11.0], [12.0], [13.0]], 4, 1)) and not Xr[:, 3].any()


def _raw_lane_tail(L, B, sol, Ad, Bd, gd, xt, pred, pdu, sw, paths_of, step, pid, traj, cap, tlen, ptr, nsw=None):
    hp = lambda a: C.c_void_p(a.ctypes.data)
    return _bind().mpcqp_lane_tail_device(L._h, C.byref(KinVehicle()), B, ptr(sol), ptr(Ad), ptr(Bd), ptr(gd), ptr(xt),
                                          ptr(pred), ptr(pdu), len(sw) if nsw is None else nsw, hp(sw), hp(paths_of),
                                          ptr(step), ptr(pid), ptr(traj), cap, ptr(tlen), None)


def test_argument_errors():
    from osqp_amd import lib
    from osqp_amd.mpc_device import LaneChangeMPC
    z, zi = np.zeros(8), np.zeros(2, np.int32)
    sw, po = np.zeros(9, np.int32), np.zeros(10, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    # refused before anything is read or launched (the buffers are host arrays that only have to be non-NULL)
    L6 = IncrementalLayout(4, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                           -mpc.DYN_DUMIN)
    assert _raw_lane_tail(L6, 1, z, z, z, z, z, z, z, sw[:2], po[:3], zi, zi, z, 0, zi, ptr) == EUNSUPPORTED
    assert b"nx 4" in lib().mpcqp_last_error()
    L4 = _layout(4)
    assert _raw_lane_tail(L4, 1, z, z, z, z, z, z, z, sw, po, zi, zi, z, 0, zi, ptr) == EUNSUPPORTED   # nsw 9
    assert b"nsw" in lib().mpcqp_last_error()
    assert _raw_lane_tail(L4, 1, z, z, z, z, z, z, z, sw, po, zi, zi, z, 0, zi, ptr, nsw=-1) == EINVAL
    assert _raw_lane_tail(L4, 1, z, z, z, z, z, z, z, sw[:2], po[:3], zi, zi, z, -1, zi, ptr) == EINVAL
    null = lambda a: None
    assert _raw_lane_tail(L4, 1, z, z, z, z, z, z, z, sw[:2], po[:3], zi, zi, z, 0, zi, null) == EINVAL
    assert not z.any() and not zi.any()
    f = _bind().mpcqp_kin_reference_search_paths_device
    assert f(1, 3, 6, 0, 5, ptr(z), ptr(z), None, None, ptr(z), ptr(z), 0.02, ptr(z), 0, None) == EINVAL   # npaths 0
    assert f(1, 3, 6, 1, 1, ptr(z), ptr(z), None, None, ptr(z), ptr(z), 0.02, ptr(z), 0, None) == EINVAL   # npath 1
    assert f(1, 3, 6, 1, 5, ptr(z), ptr(z), None, None, None, ptr(z), 0.02, ptr(z), 0, None) == EINVAL     # set_speed
    assert f(0, 3, 6, 1, 5, ptr(z), ptr(z), None, None, ptr(z), ptr(z), 0.02, ptr(z), 0, None) == 0        # B = 0
    # the class: the schedule is checked before anything touches a device
    px = np.linspace(0, 10, 5)
    for kw in (dict(paths_of=(0, 1)), dict(paths_of=(0, 2, 0)), dict(paths_of=(0, -1, 0)),
               dict(switch_steps=tuple(range(9)), paths_of=(0,) * 10)):
        with pytest.raises(ValueError):
            LaneChangeMPC(np.zeros((1, 4)), np.zeros((1, 2)), px, np.stack([px, px]), N=4, **kw)
    with pytest.raises(ValueError):
        LaneChangeMPC(np.zeros((1, 4)), np.zeros((1, 2)), px, np.zeros((2, 4)), N=4)


# ------------------------------------------------------------------------- GPU tests --
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 130])
def test_paths_search_matches_host(B):
    """Two paths with vehicles on both (and ids outside the bank, clamped); the last vehicle's
    nearest point is its path's last, so the last segment is held (B = 130: a full 128-thread
    block plus a partial one).  One path and path_id = NULL: the one-path entry point's bits."""
    import torch
    from osqp_amd.mpc_device import reference_search_kin, reference_search_paths
    N, npt = 10, 60
    rng = np.random.default_rng(40 + B)
    px = np.linspace(-10.0, 100.0, npt)
    paths_x = np.stack([px, px + 0.3 * np.sin(px / 9.0)])
    paths_y = np.stack([0.0 * px, 4.0 + 0.5 * np.sin(px / 7.0)])
    paths_yaw = np.stack([0.01 + 0 * px, 0.05 * np.cos(px / 7.0)])
    pid = np.array([0, 1, 1, 0, -3, 7, 2, 1], np.int32)[np.arange(B) % 8]
    pred = np.zeros((B, N + 1, 6))
    pred[:, 0, 0] = rng.uniform(-12, 90, B); pred[:, 0, 1] = rng.uniform(-3, 7, B)
    pred[:, :, 2] = rng.uniform(0, 40, (B, N + 1)) * np.where(np.arange(B) % 5 == 3, -1, 1)[:, None]
    pred[-1, 0, :2] = 100.4, 1.0
    speed = rng.uniform(5, 25, B)
    args = (_t(paths_x), _t(paths_y))
    for yaw in (paths_yaw, None):
        got = reference_search_paths(*args, None if yaw is None else _t(yaw), _t(pid, torch.int32), _t(speed),
                                     _t(pred), DT).cpu().numpy()
        want = mpc.reference_search_paths(paths_x, paths_y, yaw, pid, speed, pred, DT)
        assert np.array_equal(got, want)
    p_last = min(max(int(pid[-1]), 0), 1)
    assert (got[-1, 0] == paths_x[p_last, npt - 2]).all()
    if B > 1:
        on0 = (got[:, 1] == 0.0).all(1)
        assert on0.any() and (~on0).any()                   # vehicles on both paths in one batch
    # path_id NULL = path 0 for everyone; with one path: the existing entry point bit for bit
    one = reference_search_paths(_t(paths_x[1:]), _t(paths_y[1:]), _t(paths_yaw[1:]), None, _t(speed), _t(pred), DT)
    old = reference_search_kin(_t(paths_x[1]), _t(paths_y[1]), _t(paths_yaw[1]), _t(speed), _t(pred), DT)
    assert torch.equal(one, old)
    two = reference_search_paths(*args, _t(paths_yaw), None, _t(speed), _t(pred), DT)
    assert torch.equal(two, reference_search_kin(_t(paths_x[0]), _t(paths_y[0]), _t(paths_yaw[0]), _t(speed), _t(pred),
                                                 DT))


SW, PATHS_OF = np.array([5, 9], np.int32), np.array([0, 1, 2], np.int32)


def _host_case(N, B, seed):
    """B seeded (state, stage-0 model, solution, step) cases at horizon N with the host tail's results."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-5, 5, B), rng.uniform(-5, 5, B), rng.uniform(2, 25, B), rng.uniform(-1, 1, B)], 1)
    u = np.stack([np.deg2rad(rng.uniform(-10, 10, B)), rng.uniform(-2, 1, B)], 1)
    Ad, Bd, gd = mpc.linearise_kinematics(*VEH, x, u)
    Ad, Bd, gd = (np.ascontiguousarray(np.repeat(v[:, None], N, 1)) for v in (Ad, Bd, gd))
    Ad[:, 1:] += 1.0                                # only stage 0 may be read
    sol = rng.uniform(-1, 1, (B, (N + 1) * 6 + N * 2))
    sol[:, 2:(N + 1) * 6:6] += 10.0
    # a step exactly at and just past each threshold once the tail has counted: 4 -> 5, 5 -> 6, 8 -> 9, 9 -> 10
    step = np.array([4, 5, 8, 9, 0, 20], np.int32)[np.arange(B) % 6]
    return np.concatenate([x, u], 1), Ad, Bd, gd, sol, step


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3, 10])
def test_tail_matches_host(golden, N, B):
    """k_lane_tail against the fixture's own post-tail state (the captured steps of main take the
    first places of the batch) and, for the seeded rest, against mpc.lane_tail; the record stops at
    traj_cap (every third vehicle's is already full)."""
    import torch
    from osqp_amd.mpc_device import _p
    xt, Ad, Bd, gd, sol, step = _host_case(N, B, 100 * N + B)
    g = golden(f"lane_sim_n{N}.npz")
    T = min(B, 3)
    xt[:T], sol[:T] = g["in_xt"][:T], g["sol"][:T]
    Ad[:T], Bd[:T], gd[:T] = g["in_Ad"][:T], g["in_Bd"][:T], g["in_gd"][:T]
    want = [mpc.lane_tail(sol[b], Ad[b, 0], Bd[b, 0], gd[b, 0], xt[b], step[b], N, *VEH, SW, PATHS_OF)
            for b in range(B)]
    rows, xn, pxn, pun = (np.stack([w[i] for w in want]) for i in range(4))
    xn[:T], pxn[:T] = g["out_xt"][:T], g["out_pred"][:T].transpose(0, 2, 1)
    pun[:T] = g["out_pdu"][:T].transpose(0, 2, 1)
    cap = 2
    tlen0 = np.array([0, 1, 2], np.int32)[np.arange(B) % 3]
    rng = np.random.default_rng(1)
    traj0 = rng.normal(size=(B, cap, 6))
    xd, pred, pdu = _t(xt), _t(rng.normal(size=(B, N + 1, 6))), _t(rng.normal(size=(B, N + 1, 2)))
    sd, pid = _t(step, torch.int32), torch.full((B,), -1, dtype=torch.int32, device="cuda")
    traj, tlen = _t(traj0), _t(tlen0, torch.int32)
    L = _layout(N)
    assert _raw_lane_tail(L, B, _t(sol), _t(Ad), _t(Bd), _t(gd), xd, pred, pdu, SW, PATHS_OF, sd, pid, traj,
                          cap, tlen, _p) == 0
    torch.cuda.synchronize()
    assert np.allclose(xd.cpu().numpy(), xn, rtol=1e-12, atol=1e-12)
    assert np.allclose(pred.cpu().numpy(), pxn, rtol=1e-12, atol=1e-12)
    assert np.array_equal(pred[:, 1:N].cpu().numpy(), pxn[:, 1:N])           # copies: bit for bit
    assert np.array_equal(pdu.cpu().numpy(), pun)
    assert np.array_equal(sd.cpu().numpy(), step + 1)
    assert np.array_equal(pid.cpu().numpy(), mpc.lane_path_id(step + 1, SW, PATHS_OF))
    assert np.array_equal(pid.cpu().numpy(), [w[5] for w in want])
    want_traj = traj0.copy()
    room = tlen0 < cap
    want_traj[room, tlen0[room]] = rows[room]
    assert np.array_equal(traj.cpu().numpy(), want_traj)                     # a full record is not written
    assert np.array_equal(tlen.cpu().numpy(), np.minimum(tlen0 + 1, cap))
    assert np.array_equal(rows, xt)


def _starts(B):
    """Distinct starts beside the two lanes (y = 0 and y = 4)."""
    x0 = np.zeros((B, 4))
    x0[:, 0] = np.linspace(0.0, 40.0, B)
    x0[:, 1] = np.array([0.0, 1.0, -2.0, 3.5, 4.0, 2.0])[np.arange(B) % 6]
    x0[:, 2] = np.array([20.0, 12.0, 8.0, 15.0, 10.0, 18.0])[np.arange(B) % 6]
    x0[:, 3] = np.deg2rad([0.0, 4.0, -3.0, -6.0, 8.0, 1.0])[np.arange(B) % 6]
    u0 = np.tile([0.0, 0.01], (B, 1)); u0[1::2, 0] = np.deg2rad(1.0)
    return x0, u0


def _lanes():
    px = np.linspace(-10, 100, 200)
    return px, np.stack([px * 0.0, px * 0.0 + 4])


def _state(ctl):
    return tuple(v.cpu().numpy() for v in (ctl.xt, ctl.pred, ctl.pdu, ctl.steps, ctl.path_id))


def _check_step(ctl, before, N, status, Ppat, Apat, Px, settings=SETTINGS, warm=None):
    """One step of the class against the host restatement fed the device's own state, the oracle
    on that QP, and the host tail of the device's own solution."""
    xt, pred, pdu, steps, pid = before
    paths_x, paths_y = ctl.paths_x.cpu().numpy(), ctl.paths_y.cpu().numpy()
    B = xt.shape[0]
    last, sol = host(ctl)
    for b in range(B):
        Xr = _search(paths_x, paths_y, pid[b], pred[b])
        assert np.array_equal(last["Xr"][b], Xr)
        Ad, Bd, gd = mpc.linearise_kinematics(*VEH, pred[b, :N, :4], pred[b, :N, 4:])
        check_assembled(last, b, Ad, Bd, gd, _qp(Ad, Bd, gd, xt[b], Xr, N), Apat)
    ro = oracle_batch(last, status, Ppat, Apat, Px, settings, warm)
    if warm is None:
        check_solutions(sol, ro.x, slice((N + 1) * 6, None))
    for b in range(B):
        row, xn, pxn, pun, s1, p1 = mpc.lane_tail(sol[b], last["Ad"][b, 0], last["Bd"][b, 0], last["gd"][b, 0], xt[b],
                                                  steps[b], N, *VEH, ctl.switch_steps, ctl.paths_of)
        assert np.allclose(ctl.xt[b].cpu().numpy(), xn, rtol=1e-13, atol=1e-13)
        assert np.allclose(ctl.pred[b].cpu().numpy(), pxn, rtol=1e-10, atol=1e-10)
        assert np.array_equal(ctl.pdu[b].cpu().numpy(), pun)
        assert (int(ctl.steps[b]), int(ctl.path_id[b])) == (s1, p1)
    return ro


@pytest.mark.gpu
@pytest.mark.parametrize("N", [10, 40])
def test_closed_loop_matches_host_restatement(N):
    """B = 6 distinct starts, 4 steps on the script's own schedule with step0 placing half the batch
    before the first switch (steps 48..51: the fourth is on path 1) and half before the second."""
    from osqp_amd.mpc_device import LaneChangeMPC
    B, steps = 6, 4
    x0, u0 = _starts(B)
    px, paths_y = _lanes()
    step0 = np.array([48, 148, 48, 148, 48, 148], np.int32)
    ctl = LaneChangeMPC(x0, u0, px, paths_y, N=N, step0=step0, traj_cap=3)
    print(f"plan_info N={N}:", ctl.solver.plan_info())
    for b in range(B):
        assert np.allclose(ctl.pred[b].cpu().numpy(), lin_rollout(x0[b], u0[b], N), rtol=1e-12, atol=1e-12)
    assert not ctl.pdu.any() and np.array_equal(ctl.path_id.cpu().numpy(), [0, 1] * 3)
    P, Apat, _, _ = ctl.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    rows, ids = [], []
    n_iter_match = 0
    for _ in range(steps):
        before = _state(ctl)
        status, iters = ctl.step()
        ro = _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, Px)
        n_iter_match += int((iters.cpu().numpy() == ro.iter).sum())
        rows.append(before[0]); ids.append(before[4])
    assert n_iter_match >= 0.9 * B * steps
    assert np.array_equal(np.stack(ids), [[0, 1] * 3] * 3 + [[1, 0] * 3])    # the switch fell inside the run
    assert np.array_equal(ctl.steps.cpu().numpy(), step0 + steps)
    # trajectory cap: rows beyond traj_cap are dropped
    traj, tlen = ctl.trajectories()
    assert traj.shape == (B, 3, 6) and np.array_equal(tlen, np.full(B, 3))
    assert np.array_equal(traj, np.stack(rows[:3], 1))


@pytest.mark.gpu
def test_one_step_at_the_shipped_horizon(golden):
    """N = 40 (main's own), B = 2: vehicle 0 is the fixture's first step (path 0), vehicle 1 its
    second (path 1; state and horizon set from the fixture)."""
    from osqp_amd.mpc_device import LaneChangeMPC
    g = golden("lane_sim_n40.npz")
    N = 40
    x0, u0 = g["in_xt"][0, :4], g["in_xt"][0, 4:]
    ctl = LaneChangeMPC(np.tile(x0, (2, 1)), np.tile(u0, (2, 1)), g["path_x"], g["paths_y"],
                        switch_steps=g["switch_steps"], paths_of=g["paths_of"], step0=[0, 1])
    assert ctl.N == N and np.array_equal(ctl.path_id.cpu().numpy(), g["in_path_id"])
    info = ctl.solver.plan_info()
    print("plan_info N=40:", info)
    assert info["lds_bytes_solve"] <= 160 * 1024
    assert np.allclose(ctl.pred[0].cpu().numpy(), g["in_pred"][0].T, rtol=1e-12, atol=1e-12)
    ctl.xt[1] = _t(g["in_xt"][1]); ctl.pred[1] = _t(g["in_pred"][1].T); ctl.pdu[1] = _t(g["in_pdu"][1].T)
    P, Apat, _, _ = ctl.layout.pattern()
    before = _state(ctl)
    status, iters = ctl.step()
    _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, np.tile(P.data, (2, 1)))
    assert np.array_equal(ctl.last["Xr"].cpu().numpy(), g["in_Xr"][:2])
    check_fixture_step(ctl, g, Apat, slice((N + 1) * 6, None))
    print("iters", iters.cpu().numpy(), "fixture", g["sol_iter"])


@pytest.mark.gpu
def test_whole_run_within_solver_tolerance(golden):
    """The 60-step run of lane_run_n10.npz (both lane changes inside it) on the device: rounding
    inside ADMM must move the trajectory less than the solver tolerance does (traj_sens: the same
    run of the reference with the oracle at eps 1e-6 against eps 1e-3).  Two copies of the vehicle
    stay identical."""
    from osqp_amd.mpc_device import LaneChangeMPC
    g = golden("lane_run_n10.npz")
    steps = int(g["steps"])
    ctl = LaneChangeMPC(np.tile(g["x0"], (2, 1)), np.tile(g["u0"], (2, 1)), g["path_x"], g["paths_y"], N=int(g["N"]),
                        switch_steps=g["switch_steps"], paths_of=g["paths_of"], traj_cap=steps + 2)
    status, _ = ctl.run(steps)
    traj, tlen = ctl.trajectories()
    assert np.array_equal(tlen, [steps, steps]) and (status.cpu().numpy() == 1).all()
    assert np.array_equal(ctl.steps.cpu().numpy(), [steps, steps]) and not ctl.path_id.any()
    check_whole_run(traj, steps, g)


@pytest.mark.gpu
def test_shift_warm_matches_oracle():
    """shift_warm=True (an extension): every step's solve starts from the previous solution shifted
    one stage; the oracle, warm-started from the same shifted iterates on the step's QP, ends with
    the same statuses (and the same increments where the iterations agree)."""
    from osqp_amd.mpc_device import LaneChangeMPC
    B, N, steps = 6, 10, 3
    x0, u0 = _starts(B)
    px, paths_y = _lanes()
    ctl = LaneChangeMPC(x0, u0, px, paths_y, N=N, step0=np.full(B, 49, np.int32), shift_warm=True)
    P, Apat, _, _ = ctl.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    du = slice((N + 1) * 6, None)
    match, prev = 0, None
    for _ in range(steps):
        before = _state(ctl)
        status, iters = ctl.step()
        ws = None if prev is None else dict(x0=_stage_shift(prev[0], N, 6, 2, 1), y0=_stage_shift(prev[1], N, 6, 2, 2))
        ro = _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, Px, settings=dict(polish=False), warm=ws or {})
        x = ctl.sol.cpu().numpy()
        same = ro.iter == iters.cpu().numpy()
        match += int(same.sum())
        assert np.abs(x[same][:, du] - ro.x[same][:, du]).max() < 1e-4
        prev = (x, ctl.y.cpu().numpy())
    assert match >= 0.9 * B * steps
