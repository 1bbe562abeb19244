"""What tests/test_rollout_device.py's three-step central differences rest on, confirmed with the
CPU oracle: from the interior point of tests/test_dyn_vjp_ref.py and its twelve
neighbours at h = 1e-3, three steps of the dynamic closed loop -- every stage of the predicted
horizon linearised, mpc_increment's QP, the oracle's solve, mpc.incr_shift -- end on the same row
classes at every point of every step, and no inequality row is active."""
import numpy as np

import qp_adjoint_ref as ref
import test_dyn_vjp_ref as dyn
import test_mpc_vjp_ref as cpu
from osqp_amd import canonical_data, mpc

H_LOOP = 1e-3
T_LOOP = 3


def loop_points(x0, h=H_LOOP):
    """x0 and its central-difference neighbours in each of the six states: (13, 6)."""
    return np.concatenate([[x0]] + [[x0 + s * h * e] for e in np.eye(6) for s in (1.0, -1.0)])


def loop_references(N, T):
    """The reference of step t: test_dyn_vjp_ref's, its X row moved on by 0.5 per step."""
    out = []
    for t in range(T):
        Xr = dyn.dyn_reference(N)
        Xr[0] += 0.5 * t
        out.append(Xr)
    return out


def test_three_steps_keep_their_row_classes():
    N = 3
    refs = loop_references(N, T_LOOP)
    classes = []
    for x0 in loop_points(dyn.X0_INTERIOR):
        xt = np.concatenate([x0, dyn.U0])
        pred = np.tile(xt, (N + 1, 1))
        mine = []
        for t in range(T_LOOP):
            Ad, Bd, gd = mpc.linearise_dynamics(dyn.VEH, pred[:N, :6], pred[:N, 6:])
            P, q, A, l, u = mpc.incremental_qp(list(Ad), list(Bd), list(gd), xt, refs[t], mpc.DYN_Q, mpc.DYN_QN,
                                               mpc.DYN_R, N, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                                               -mpc.DYN_DUMIN)
            P, A = canonical_data(P, A)
            l, u = np.maximum(l, -1e30), np.minimum(u, 1e30)
            r = cpu._solve(P, q, A, l, u)
            mine.append(ref.row_classes(A, l, u, r.x, r.y))
            xt, pred, _ = mpc.incr_shift(dyn.VEH, N, r.x, Ad[0], Bd[0], gd[0], xt)
        classes.append(mine)
    for t in range(T_LOOP):
        first = classes[0][t]
        assert not ((first == 1) | (first == 2)).any(), f"step {t + 1}: an inequality row is active"
        for k, mine in enumerate(classes):
            assert np.array_equal(mine[t], first), f"step {t + 1}: point {k} ends on other row classes"
