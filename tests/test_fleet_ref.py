"""The host statements of osqp_amd.mpc for cars other than the one every earlier fixture was
captured with, and what tests/test_fleet_device.py's closed loops rest on (CPU only).

  - mpc.linearise_dynamics, mpc.linearise_kinematics and the two terminal steps (the Euler step
    inside mpc.incr_shift, mpc.kin_update) against the reference's own outputs for the three cars
    of tests/golden/make_golden_fleet.py, within the bars tests/test_mpc_device.py holds
    linearise.npz to: rtol 1e-13 / atol 1e-15, gd rtol 1e-12 / atol 1e-13;
  - mpc.per_vehicle over a batch is the single-vehicle statements, stacked, bit for bit;
  - the premise of the device loops, as tests/test_rollout_ref.py and tests/test_kin_rollout_ref.py
    state theirs: three oracle-solved steps of the dynamic, the kinematic incremental and the
    kinematic LTV loop for the three cars at N in {2, 3} all end `solved` with no inequality row
    active, and the three cars' final states are pairwise different.
"""
import numpy as np
import pytest

import fleet_cases as fc
import qp_adjoint_ref as ref
import test_dyn_vjp_ref as dyn
import test_kin_rollout_ref as kin
import test_mpc_vjp_ref as cpu
import test_rollout_ref as roll
from osqp_amd import canonical_data, mpc

T_LOOP = 3
BAR = dict(rtol=1e-13, atol=1e-15)
BAR_GD = dict(rtol=1e-12, atol=1e-13)


def _worst(got, want, rtol, atol):
    """The largest |got - want| / (atol + rtol |want|): np.allclose holds iff it is <= 1."""
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def test_the_fixtures_are_the_cars_of_the_tests(golden):
    g, k = golden("linearise_fleet.npz"), golden("kin_linearise_fleet.npz")
    assert list(g["cars"]) == list(fc.CARS) == list(k["cars"]) == list(golden("update_fleet.npz")["cars"])
    for c, car in enumerate(fc.CARS):
        assert list(g["params"][c]) == [fc.CARS[car][f] for f in
                                        ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")] + [fc.DT_DYN]
        assert tuple(k["params"][c]) == fc.wheelbase(car)
    assert float(g["turning_circle"]) == fc.TURNING_CIRCLE
    assert np.array_equal(g["x"], golden("linearise.npz")["x"]) and np.array_equal(k["x"], golden("kin_linearise.npz")["x"])
    assert np.array_equal(g["Ad"][0], golden("linearise.npz")["Ad"])       # the default car is the old fixture's


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_dynamic_linearisation_matches_the_reference(golden, c, car):
    g = golden("linearise_fleet.npz")
    Ad, Bd, gd = mpc.linearise_dynamics(fc.params(car), g["x"], g["u"])
    print(f"{car}: Ad {_worst(Ad, g['Ad'][c], **BAR):.3f} Bd {_worst(Bd, g['Bd'][c], **BAR):.3f} "
          f"gd {_worst(gd, g['gd'][c], **BAR_GD):.3f} of the bar")
    assert np.allclose(Ad, g["Ad"][c], **BAR)
    assert np.allclose(Bd, g["Bd"][c], **BAR)
    assert np.allclose(gd, g["gd"][c], **BAR_GD)


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_kinematic_linearisation_matches_the_reference(golden, c, car):
    g = golden("kin_linearise_fleet.npz")
    Ad, Bd, gd = mpc.linearise_kinematics(*fc.wheelbase(car), g["x"], g["u"])
    print(f"{car}: Ad {_worst(Ad, g['Ad'][c], **BAR):.3f} Bd {_worst(Bd, g['Bd'][c], **BAR):.3f} "
          f"gd {_worst(gd, g['gd'][c], **BAR_GD):.3f} of the bar")
    assert np.allclose(Ad, g["Ad"][c], **BAR)
    assert np.allclose(Bd, g["Bd"][c], **BAR)
    assert np.allclose(gd, g["gd"][c], **BAR_GD)


def terminal_step(veh, x, u):
    """The Euler step mpc.incr_shift forms pred[N] with, for a batch of (x, u): N = 2, the solution
    zero but for x_N = x and the input part of x~_{N-1} = u."""
    M, N = x.shape[0], 2
    sol = np.zeros((M, (N + 1) * 8 + N * 2))
    sol[:, N * 8:N * 8 + 6] = x
    sol[:, (N - 1) * 8 + 6:(N - 1) * 8 + 8] = u
    zero = np.zeros((M, 6))
    _, pred, _ = mpc.incr_shift(veh, N, sol, np.tile(np.eye(6), (M, 1, 1)), np.zeros((M, 6, 2)), zero, np.zeros((M, 8)))
    return pred[:, N, :6]


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_terminal_steps_match_the_reference(golden, c, car):
    g = golden("update_fleet.npz")
    xe = terminal_step(fc.params(car), g["dyn_x"], g["dyn_u"])
    xk = mpc.kin_update(*fc.wheelbase(car), g["kin_x"], g["kin_u"])
    print(f"{car}: dynamic {_worst(xe, g['dyn_next'][c], **BAR):.3f} kinematic {_worst(xk, g['kin_next'][c], **BAR):.3f} "
          f"of the bar")
    assert np.allclose(xe, g["dyn_next"][c], **BAR)
    assert np.allclose(xk, g["kin_next"][c], **BAR)


def test_per_vehicle_is_the_single_vehicle_statements_stacked(golden):
    g, k = golden("linearise.npz"), golden("kin_linearise.npz")
    cars = [fc.ORDER[b % 3] for b in range(7)]
    x, u = g["x"][:7], g["u"][:7]
    got = mpc.per_vehicle(mpc.linearise_dynamics, [fc.params(c) for c in cars], x, u)
    for b, car in enumerate(cars):
        want = mpc.linearise_dynamics(fc.params(car), x[b:b + 1], u[b:b + 1])
        for a, w in zip(got, want):
            assert np.array_equal(a[b:b + 1], w)
    assert [a.shape for a in got] == [(7, 6, 6), (7, 6, 2), (7, 6)]
    # leading arguments as a tuple, one result, a None among the batched arguments, a keyword for all
    xk, uk = k["x"][:7], k["u"][:7]
    got = mpc.per_vehicle(mpc.kin_update, [fc.wheelbase(c) for c in cars], xk, uk)
    assert got.shape == (7, 4)
    for b, car in enumerate(cars):
        assert np.array_equal(got[b], mpc.kin_update(*fc.wheelbase(car), xk[b], uk[b]))
    w = np.arange(28.0).reshape(7, 4)
    got = mpc.per_vehicle(lambda l_f, l_r, dt, x, u, w, none, scale: scale * mpc.kin_update_vjp(l_f, l_r, dt, x, u, w)[0]
                          + (0.0 if none is None else 1.0), [fc.wheelbase(c) for c in cars], xk, uk, w, None, scale=2.0)
    for b, car in enumerate(cars):
        assert np.array_equal(got[b], 2.0 * mpc.kin_update_vjp(*fc.wheelbase(car), xk[b], uk[b], w[b])[0])


def _solve_step(qp):
    r = cpu._solve(*qp)                                            # asserts `solved`
    cls = ref.row_classes(qp[2], qp[3], qp[4], r.x, r.y)
    assert not ((cls == 1) | (cls == 2)).any(), "an inequality row is active"
    return r


@pytest.mark.parametrize("N", [2, 3])
def test_dynamic_loop_premise(N):
    """Three steps from test_dyn_vjp_ref.X0_INTERIOR with test_rollout_ref.loop_references."""
    refs = roll.loop_references(N, T_LOOP)
    final = {}
    for car in fc.CARS:
        veh = fc.params(car)
        xt = np.concatenate([dyn.X0_INTERIOR, dyn.U0])
        pred = np.tile(xt, (N + 1, 1))
        for t in range(T_LOOP):
            Ad, Bd, gd = mpc.linearise_dynamics(veh, pred[:N, :6], pred[:N, 6:])
            P, q, A, l, u = mpc.incremental_qp(list(Ad), list(Bd), list(gd), xt, refs[t], mpc.DYN_Q, mpc.DYN_QN,
                                               mpc.DYN_R, N, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                                               -mpc.DYN_DUMIN)
            P, A = canonical_data(P, A)
            r = _solve_step((P, q, A, np.maximum(l, -1e30), np.minimum(u, 1e30)))
            xt, pred, _ = mpc.incr_shift(veh, N, r.x, Ad[0], Bd[0], gd[0], xt)
        final[car] = xt
    _pairwise_different(final)


def _pairwise_different(final):
    cars = list(final)
    for i, a in enumerate(cars):
        for b in cars[i + 1:]:
            gap = np.abs(final[a] - final[b]).max()
            print(f"{a} vs {b}: final states differ by {gap:.3e}")
            assert gap > 0.0, (a, b)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("case", ["incr interior", "ltv"])
def test_kinematic_loop_premise(case, N, monkeypatch):
    """Three steps of test_kin_rollout_ref's two interior loops (INCR_CASES["interior steer"], X0_LTV)
    with each car's wheelbase in place of that module's VEH."""
    kind, x0, u0, _ = kin.LOOP_CASES[case]
    refs = kin.kin_loop_references(N, T_LOOP)
    final = {}
    for car in fc.CARS:
        monkeypatch.setattr(kin, "VEH", fc.wheelbase(car))
        if kind == "incr":
            state = np.concatenate([x0, u0])
            hor = np.tile(state, (N + 1, 1))
        else:
            state, hor = x0, (np.tile(x0, (N + 1, 1)), np.tile(u0, (N + 1, 1)))
        for Xr in refs:
            qp, (A0, B0, g0) = kin.step_qp(kind, N, state, hor, Xr)
            r = _solve_step(qp)
            if kind == "incr":
                state, hor, _ = mpc.kin_incr_shift(kin.VEH, N, r.x, A0, B0, g0, state)
            else:
                state, _, px, pu = mpc.kin_ltv_shift(kin.VEH, N, r.x, A0, B0, g0, state)
                hor = (px, pu)
        final[car] = state
    _pairwise_different(final)
