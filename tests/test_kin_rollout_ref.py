"""What tests/test_kin_rollout_device.py's three-step central differences and its skipped vehicle
rest on, confirmed with the CPU oracle: from the points of tests/test_mpc_vjp_ref.py
and their eight neighbours at h = 1e-3, three steps of both kinematic closed loops -- every stage of
the predicted horizon linearised, the layout's QP, the oracle's solve, mpc.kin_incr_shift /
mpc.kin_ltv_shift -- end on the same row classes at every point of every step; on the interior
points no inequality row is active, on the active point the same ones are.  And the LTV instance
that starts at v = 150 is primal infeasible, which is the skipped vehicle of the device test."""
import numpy as np
import pytest

import pyoracle
import qp_adjoint_ref as ref
import test_mpc_vjp_ref as cpu
from osqp_amd import canonical_data, mpc

H_LOOP = 1e-3
T_LOOP = 3
VEH = (cpu.LF, cpu.LR, cpu.DT)
X0_INFEASIBLE = np.array([0.3, 0.2, 150.0, 0.05])    # v beyond the state box (KINLTV_XMAX[2] = 100)
LOOP_CASES = {
    # kind, x0, u0, an inequality row is active
    "incr interior": ("incr",) + cpu.INCR_CASES["interior steer"][:2] + (False,),
    "incr active": ("incr",) + cpu.INCR_CASES["active accel"][:2] + (True,),
    "ltv": ("ltv", cpu.X0_LTV, cpu.U0_LTV, False),
}


def kin_loop_points(x0, h=H_LOOP):
    """x0 and its central-difference neighbours in each of the four states: (9, 4)."""
    return np.concatenate([[x0]] + [[x0 + s * h * e] for e in np.eye(4) for s in (1.0, -1.0)])


def kin_loop_references(N, T):
    """The reference of step t: test_mpc_vjp_ref's, its X row moved on by 0.2 per step."""
    out = []
    for t in range(T):
        Xr = cpu.ltv_reference(N)
        Xr[0] += 0.2 * t
        out.append(Xr)
    return out


def step_qp(kind, N, x0, hor, Xr):
    """One step's QP from the state and the predicted horizon, canonical, bounds clipped; and stage 0
    of the linearisation."""
    if kind == "incr":
        Ad, Bd, gd = mpc.linearise_kinematics(*VEH, hor[:N, :4], hor[:N, 4:])
        P, q, A, l, u = mpc.incremental_qp(list(Ad), list(Bd), list(gd), x0, Xr, mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, N,
                                           mpc.KIN_XMIN_T, mpc.KIN_XMAX_T, mpc.KIN_DUMIN, -mpc.KIN_DUMIN)
    else:
        Ad, Bd, gd = mpc.linearise_kinematics(*VEH, hor[0][:N], hor[1][:N])
        P, q, A, l, u = mpc.ltv_qp(list(Ad), list(Bd), list(gd), x0, Xr, mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R, N,
                                   mpc.KINLTV_XMIN, mpc.KINLTV_XMAX, mpc.KINLTV_UMIN, mpc.KINLTV_UMAX)
    P, A = canonical_data(P, A)
    return (P, q, A, np.maximum(l, -1e30), np.minimum(u, 1e30)), (Ad[0], Bd[0], gd[0])


def loop_classes(kind, N, x0, u0, refs):
    """The row classes and the first inputs of each of len(refs) closed-loop steps from (x0, u0), the
    horizon starting as (x0, u0) on every stage."""
    if kind == "incr":
        state = np.concatenate([x0, u0])
        hor = np.tile(state, (N + 1, 1))
    else:
        state, hor = x0, (np.tile(x0, (N + 1, 1)), np.tile(u0, (N + 1, 1)))
    classes, first = [], []
    for Xr in refs:
        qp, (A0, B0, g0) = step_qp(kind, N, state, hor, Xr)
        r = cpu._solve(*qp)
        classes.append(ref.row_classes(qp[2], qp[3], qp[4], r.x, r.y))
        first.append(r.x[(N + 1) * (6 if kind == "incr" else 4):][:2].copy())
        if kind == "incr":
            state, hor, _ = mpc.kin_incr_shift(VEH, N, r.x, A0, B0, g0, state)
        else:
            state, _, px, pu = mpc.kin_ltv_shift(VEH, N, r.x, A0, B0, g0, state)
            hor = (px, pu)
    return classes, first


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_three_steps_keep_their_row_classes(case, N):
    kind, x0, u0, active = LOOP_CASES[case]
    refs = kin_loop_references(N, T_LOOP)
    runs = [loop_classes(kind, N, p, u0, refs) for p in kin_loop_points(x0)]
    for t in range(T_LOOP):
        first = runs[0][0][t]
        on = (first == 1) | (first == 2)
        for k, (classes, _) in enumerate(runs):
            assert np.array_equal(classes[t], first), f"step {t + 1}: point {k} ends on other row classes"
        if not active:
            assert not on.any(), f"step {t + 1}: an inequality row is active"
        else:
            # the steer increment of the first stage sits on its bound, and as many rows are active as stages
            assert on.sum() == N and abs(abs(runs[0][1][t][0]) + mpc.KIN_DUMIN[0]) < 1e-8, (t, on.sum())


@pytest.mark.parametrize("N", [2, 3])
def test_the_fast_ltv_instance_is_primal_infeasible(N):
    qp, _ = step_qp("ltv", N, X0_INFEASIBLE, (np.tile(X0_INFEASIBLE, (N + 1, 1)), np.tile(cpu.U0_LTV, (N + 1, 1))),
                    cpu.ltv_reference(N))
    o = pyoracle.OSQP()
    o.setup(*qp, **cpu.SET)
    r = o.solve()
    print(f"ltv N={N} from v = 150: {r.info.status} after {r.info.iter} iterations")
    assert r.info.status == "primal infeasible" and r.info.status_val == -3
