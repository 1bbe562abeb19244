"""The host statements of the parameter gradients (CPU only) against central
differences of the REFERENCE's own outputs, recorded by tests/golden/make_golden_param_grad.py with
each constructor argument moved up and down by a relative step h and 2h:

  mpc.linearise_dynamics_pvjp, mpc.euler_step_pvjp     chained through mpc.vehicle_constants_vjp
  mpc.linearise_kinematics_pvjp, mpc.kin_update_pvjp   (the kinematic struct derives nothing)

for the three cars of the fleet fixtures, at points outside the low-speed guard and in each of its
two regions for both signs of vx, under random normal cotangents.

The measure is §17's on the SCALED gradient s_a = p_a dL/dp_a (so that m = 1300 and C_roll = 0.015
compare): per (car, point), max_a |s_a - fd_a| / max_a |s_a|, with fd_a = (L(p_a (1 + h)) -
L(p_a (1 - h))) / (2 h).  The bars are ten times the largest value measured (§17's rule,
6.36e-10 -> 6.4e-9), the quotients at h and 2h must agree under the same bar, and inside the guard
the zero pattern of the statement is the zero pattern of the differences, exactly.

Measured (h = 1e-5): see MEASURED below and DESIGN.md §25.
"""
import numpy as np
import pytest

import fleet_cases as fc
from osqp_amd import mpc

# Per statement, the larger of the two figures measured over the three cars: the deviation at h
# (2.11e-10, 5.36e-9, 1.06e-9, 9.26e-9) and the distance between the quotients at h and 2h (3.91e-10,
# 6.38e-9, 9.09e-10, 1.21e-8).  The terminal steps' are larger because their outputs are states of
# size 1 .. 25 moved by dt times a force: the differences lose eps |x| / (h |dx/dp|) to rounding.
MEASURED = {"linearise_dynamics": 3.91e-10, "euler_step": 6.38e-9, "linearise_kinematics": 1.06e-9,
            "kin_update": 1.21e-8}
BAR = {k: 10.0 * v for k, v in MEASURED.items()}
GUARD = (4, 5, 6, 7)  # make_golden_param_grad.DYN_POINTS: vx 0.1, 0.4, -0.2, -0.45


@pytest.fixture(scope="module")
def fx(golden):
    return golden("param_grad.npz")


def _cotangents(seed, P, nx):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, nx, nx)), rng.standard_normal((P, nx, 2)), rng.standard_normal((P, nx)), \
        rng.standard_normal((P, nx))


def _quotients(outs, cots, steps):
    """outs: [(argument, step, direction, point, ...)] -> fd (step, point, argument), scaled:
    (L+ - L-) / (2 h), L = sum of output * cotangent per point."""
    L = sum((o * c[None, None, None]).reshape(o.shape[:4] + (-1,)).sum(-1) for o, c in zip(outs, cots))
    return np.moveaxis((L[:, :, 0] - L[:, :, 1]) / (2.0 * steps[None, :, None]), 0, 2)


def _deviation(s, fd):
    """per point: max_a |s_a - fd_a| / max_a |s_a|"""
    return np.abs(s - fd).max(-1) / np.abs(s).max(-1)


def _check(name, car, s, fd, guard=()):
    dev = _deviation(s, fd[0])
    dev2 = _deviation(fd[1], fd[0])
    print(f"{name} {car}: deviation at h {dev.max():.3e}, quotients h vs 2h {dev2.max():.3e}, bar {BAR[name]:.1e}")
    for p in guard:
        print(f"  guard point {p}: zero pattern {(s[p] == 0).astype(int)} differences {(fd[0][p] == 0).astype(int)}")
    assert (np.abs(s).max(-1) > 0).all()
    assert dev.max() <= BAR[name]
    assert dev2.max() <= BAR[name]
    for p in guard:
        assert np.array_equal(s[p] == 0, fd[0][p] == 0) and np.array_equal(s[p] == 0, fd[1][p] == 0), p


def test_the_fixture_is_the_cars_and_points_of_the_fleet_fixtures(fx, golden):
    assert list(fx["cars"]) == list(fc.CARS)
    for c, car in enumerate(fc.CARS):
        assert list(fx["params"][c]) == [fc.CARS[car][f] for f in
                                         ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")] + [fc.DT_DYN]
        assert tuple(fx["kin_params"][c]) == fc.wheelbase(car)
    x = golden("linearise.npz")["x"]
    assert all((fx["dyn_x"][i] == x).all(1).any() for i in range(8))
    vx = fx["dyn_x"][:, 3]
    assert (np.abs(vx[:4]) > 0.5).all() and list(np.abs(vx[list(GUARD)]) < 0.3) == [True, False, True, False]
    assert list(np.sign(vx[list(GUARD)])) == [1, 1, -1, -1]
    assert fx["steps"][1] == 2 * fx["steps"][0]


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_dynamic_linearisation_gradient_matches_differences_of_the_reference(fx, c, car):
    x, u, p = fx["dyn_x"], fx["dyn_u"], fx["params"][c]
    gAd, gBd, ggd, _ = _cotangents(11 + c, len(x), 6)
    gK = mpc.linearise_dynamics_pvjp(fc.params(car), x[:, None], u[:, None], gAd[:, None], gBd[:, None], ggd[:, None])
    s = mpc.vehicle_constants_vjp(np.broadcast_to(p, (len(x), 9)), gK) * p
    fd = _quotients([fx["dyn_Ad"][c], fx["dyn_Bd"][c], fx["dyn_gd"][c]], [gAd, gBd, ggd], fx["steps"])
    _check("linearise_dynamics", car, s, fd, GUARD)


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_euler_step_gradient_matches_differences_of_the_reference(fx, c, car):
    x, u, p = fx["dyn_x"], fx["dyn_u"], fx["params"][c]
    w = _cotangents(23 + c, len(x), 6)[3]
    gK = mpc.euler_step_pvjp(fc.params(car), x, u, w)
    s = mpc.vehicle_constants_vjp(np.broadcast_to(p, (len(x), 9)), gK) * p
    fd = _quotients([fx["dyn_next"][c]], [w], fx["steps"])
    _check("euler_step", car, s, fd, GUARD)


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_kinematic_linearisation_gradient_matches_differences_of_the_reference(fx, c, car):
    x, u, p = fx["kin_x"], fx["kin_u"], fx["kin_params"][c]
    gAd, gBd, ggd, _ = _cotangents(37 + c, len(x), 4)
    s = mpc.linearise_kinematics_pvjp(*p, x[:, None], u[:, None], gAd[:, None], gBd[:, None], ggd[:, None]) * p
    _check("linearise_kinematics", car, s,
           _quotients([fx["kin_Ad"][c], fx["kin_Bd"][c], fx["kin_gd"][c]], [gAd, gBd, ggd], fx["steps"]))


@pytest.mark.parametrize("c,car", list(enumerate(fc.CARS)))
def test_kinematic_update_gradient_matches_differences_of_the_reference(fx, c, car):
    x, u, p = fx["kin_x"], fx["kin_u"], fx["kin_params"][c]
    w = _cotangents(37 + c, len(x), 4)[3]
    s = mpc.kin_update_pvjp(*p, x, u, w) * p
    _check("kin_update", car, s, _quotients([fx["kin_next"][c]], [w], fx["steps"]))


def test_stage_sum_and_masks_of_the_statements():
    """The stage axis is summed in stage order; None cotangents are zero; a mode that is not 0 gives
    a zero row; per_vehicle stacks the single-vehicle statement."""
    rng = np.random.default_rng(5)
    x, u = rng.standard_normal((2, 3, 6)), 0.2 * rng.standard_normal((2, 3, 2))
    x[..., 3] = [[8.0, -6.0, 0.4], [0.1, 12.0, -0.2]]
    gAd, gBd, ggd = rng.standard_normal((2, 3, 6, 6)), rng.standard_normal((2, 3, 6, 2)), rng.standard_normal((2, 3, 6))
    veh = fc.params("small")
    g = mpc.linearise_dynamics_pvjp(veh, x, u, gAd, gBd, ggd)
    per = mpc.linearise_dynamics_pvjp(veh, x.reshape(6, 1, 6), u.reshape(6, 1, 2), gAd.reshape(6, 1, 6, 6),
                                      gBd.reshape(6, 1, 6, 2), ggd.reshape(6, 1, 6)).reshape(2, 3, 13)
    assert np.array_equal(g, (per[:, 0] + per[:, 1]) + per[:, 2])
    parts = [mpc.linearise_dynamics_pvjp(veh, x, u, *(c if i == j else None for j, c in enumerate((gAd, gBd, ggd))))
             for i in range(3)]
    assert np.allclose(g, sum(parts), rtol=1e-12, atol=1e-12)
    assert not mpc.linearise_dynamics_pvjp(veh, x, u).any()
    w = rng.standard_normal((2, 6))
    e = mpc.euler_step_pvjp(veh, x[:, 0], u[:, 0], w)
    assert np.array_equal(mpc.euler_step_pvjp(veh, x[:, 0], u[:, 0], w, mode=np.array([0, 1]))[0], e[0])
    assert not mpc.euler_step_pvjp(veh, x[:, 0], u[:, 0], w, mode=np.array([0, 1]))[1].any()
    cars = [fc.params(c) for c in ("van", "small")]
    both = mpc.per_vehicle(mpc.linearise_dynamics_pvjp, cars, x, u, gAd, gBd, ggd)
    assert both.shape == (2, 13) and np.array_equal(both[1], g[1])
    xk, uk, wk = rng.standard_normal((2, 4)), 0.2 * rng.standard_normal((2, 2)), rng.standard_normal((2, 4))
    k = mpc.kin_update_pvjp(1.2, 1.3, 0.02, xk, uk, wk, mode=np.array([2, 0]))
    assert not k[0].any() and k[1].any() and k[1, 0] == k[1, 1]


def test_vehicle_constants_are_the_forward_and_their_vjp_its_differences():
    """mpc.vehicle_constants is model_constants of VehicleParams; its VJP against central
    differences of itself (h = 1e-6; the derivation is smooth: bar 1e-8 of the row's largest)."""
    rng = np.random.default_rng(9)
    for car in fc.CARS:
        p = np.array([fc.CARS[car][f] for f in ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")] +
                     [fc.DT_DYN])
        k = np.array(mpc.vehicle_constants(list(p)), float)
        assert np.allclose(k, mpc.model_constants(fc.params(car)), rtol=4e-16, atol=0)
        gk = rng.standard_normal(13)
        g = mpc.vehicle_constants_vjp(p, gk) * p
        fd = np.empty(9)
        for a in range(9):
            up, dn = p.copy(), p.copy()
            up[a] *= 1 + 1e-6
            dn[a] *= 1 - 1e-6
            fd[a] = (np.dot(gk, np.array(mpc.vehicle_constants(list(up)), float)) -
                     np.dot(gk, np.array(mpc.vehicle_constants(list(dn)), float))) / 2e-6
        print(f"{car}: {np.abs(g - fd).max() / np.abs(g).max():.3e}")
        assert np.abs(g - fd).max() <= 1e-8 * np.abs(g).max()
