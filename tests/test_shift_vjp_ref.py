"""osqp_amd.mpc.incr_shift and incr_shift_vjp, the numpy statements of k_incr_shift and
k_tail_vjp<DynamicIncrTail>: the forward against the reference's own three steps
(tests/golden/dyn_main_n30.npz), the VJP against central differences of the forward.

The tail of the loop is linear or bilinear in everything but the six inputs of the terminal Euler
step (x_N's yaw, vx, vy, r and u_{N-1}), so there a central difference with a step of order 1 is
exact up to rounding: tests/test_mpc_vjp_ref.py's argument, measure and bar (BAR_LINEAR, of the
contraction's largest term).  The six are differenced with h = 1e-6 in tests/test_dyn_vjp_ref.py's
way -- outputs differenced entry by entry before they are contracted, the divisor the step the two
points really are apart, the deviation over the row's largest gradient -- against that file's
BAR_LIN = 6.4e-9: the same f, one derivative lower.  The terminal X and Y are drawn in +-5 rather
than that file's +-50: here they are part of the differenced output (x + dt f), and the rounding
of an entry of size 50 over 2 h, 7e-15 / 2e-6 = 3.5e-9, would by itself be half the bar; at 5 (and
|vx| <= 15) it is 9e-16 / 2e-6 = 4.5e-10.
Measured: linear part 6.5e-15 (N 2) and 1.0e-14 (N 3), Euler inputs 6.5e-10 (N 2) and 5.9e-10
(N 3; in the guard 7.2e-11 and 2.9e-11).
"""
import numpy as np
import pytest

import test_dyn_vjp_ref as dyn
from osqp_amd import mpc
from test_mpc_vjp_ref import BAR_LINEAR

VEH = dyn.VEH
H_EULER = dyn.H_LIN
BAR_EULER = dyn.BAR_LIN
NXA = 8
# x_N's yaw, vx, vy, r and u_{N-1}: the terminal Euler step's inputs, as (stage relative to N, entry)
EULER_INPUTS = [(0, 2), (0, 3), (0, 4), (0, 5), (-1, 6), (-1, 7)]


def shift_case(rng, B, N):
    """B vehicles' inputs of incr_shift: solutions whose states are test_dyn_vjp_ref's sample (X, Y of
    every stage in +-5), every fourth terminal state in the low-speed guard (both regions, both
    signs), and a random stage-0 model and state."""
    x, u = dyn.sample(rng, B * (N + 1))
    x[:, :2] = rng.uniform(-5, 5, (B * (N + 1), 2))
    X = np.concatenate([x, u], 1).reshape(B, N + 1, NXA)
    slow = np.arange(B) % 4 == 0
    X[slow, N, 3] = dyn.guard_speeds(rng, int(slow.sum()))
    if B >= 12:
        X[0, N, 3], X[4, N, 3], X[8, N, 3] = 0.2, -0.4, -0.1     # each region whatever the draw
        X[1, N, 3], X[2, N, 3] = -7.0, 6.0                        # and both signs outside
    D = rng.uniform(-0.03, 0.03, (B, N, 2))
    sol = np.concatenate([X.reshape(B, -1), D.reshape(B, -1)], 1)
    Ad0 = np.eye(6) + 0.05 * rng.standard_normal((B, 6, 6))
    Bd0 = 0.05 * rng.standard_normal((B, 6, 2))
    gd0 = 0.05 * rng.standard_normal((B, 6))
    xt = np.concatenate(dyn.sample(rng, B), 1)
    return dict(sol=sol, Ad0=Ad0, Bd0=Bd0, gd0=gd0, xt=xt)


def shift_cotangents(rng, B, N):
    return rng.standard_normal((B, NXA)), rng.standard_normal((B, N + 1, NXA)), rng.standard_normal((B, N + 1, 2))


def copied_entries_are_exact(N, gsol, gpred, gpdu, gu0=None):
    """What the forward only copies: g x~_k = gpred[k-1] (2 <= k <= N; X, Y and the inputs of x~_N
    take gpred[N]'s as well), x~_0 and x~_1 nothing (but x~_{N-1}'s inputs, the Euler step's
    control), g du_k = gpdu[k-1], du_{N-1} the three of its copies added in the output's order."""
    B = gsol.shape[0]
    gX, gD = gsol[:, :(N + 1) * NXA].reshape(B, N + 1, NXA), gsol[:, (N + 1) * NXA:].reshape(B, N, 2)
    ok = not gX[:, 0].any() and not gX[:, 1, :6].any() and (N == 2 or not gX[:, 1, 6:].any())
    ok = ok and np.array_equal(gX[:, 2:N, :6], gpred[:, 1:N - 1, :6])
    ok = ok and np.array_equal(gX[:, 2:N - 1, 6:], gpred[:, 1:N - 2, 6:])
    ok = ok and np.array_equal(gX[:, N, [0, 1, 6, 7]], gpred[:, N - 1][:, [0, 1, 6, 7]] + gpred[:, N][:, [0, 1, 6, 7]])
    ok = ok and np.array_equal(gD[:, 1:N - 1], gpdu[:, 0:N - 2])
    ok = ok and np.array_equal(gD[:, N - 1], (gpdu[:, N - 2] + gpdu[:, N - 1]) + gpdu[:, N])
    return bool(ok and (gu0 is None or np.array_equal(gD[:, 0], gu0)))


def euler_zero_pattern_is_exact(N, sol, gsol, gpred):
    """The Euler step gives vy, r of x_N and steer of u_{N-1} nothing for |vx_N| < 0.5 and vx nothing
    for |vx_N| < 0.3: those entries of gsol are their copies' cotangents alone."""
    B = sol.shape[0]
    gX = gsol[:, :(N + 1) * NXA].reshape(B, N + 1, NXA)
    vx = np.abs(sol[:, N * NXA + 3])
    lat, lon = vx < 0.5, vx < 0.3
    before = gpred[:, N - 2, 6] if N >= 3 else np.zeros(B)       # x~_{N-1} is itself a copy's source for N >= 3
    return bool(np.array_equal(gX[lat, N, 4:6], gpred[lat, N - 1, 4:6]) and np.array_equal(gX[lon, N, 3], gpred[lon, N - 1, 3])
                and np.array_equal(gX[lat, N - 1, 6], before[lat])
                and (gX[~lat, N, 4:6] != gpred[~lat, N - 1, 4:6]).all() and (gX[~lon, N, 3] != gpred[~lon, N - 1, 3]).all())


def test_incr_shift_matches_the_reference_steps(golden):
    """Three steps of mpc_dynamics.main as the reference ran them, at the tolerances
    test_main_steps_on_device_match_reference holds the kernel to."""
    g = golden("dyn_main_n30.npz")
    N = 30
    xt, pred, pdu = mpc.incr_shift(VEH, N, g["sol"], g["in_Ad"][:, 0], g["in_Bd"][:, 0], g["in_gd"][:, 0], g["in_xt"])
    assert np.allclose(xt, g["out_xt"], rtol=1e-14, atol=1e-14)
    assert np.allclose(pred, g["out_pred"].transpose(0, 2, 1), rtol=1e-12, atol=1e-12)
    assert np.array_equal(pdu, g["out_pdu"].transpose(0, 2, 1))
    # one vehicle without a batch axis
    one = mpc.incr_shift(VEH, N, g["sol"][1], g["in_Ad"][1, 0], g["in_Bd"][1, 0], g["in_gd"][1, 0], g["in_xt"][1])
    assert all(np.array_equal(a, b[1]) for a, b in zip(one, (xt, pred, pdu)))


@pytest.mark.parametrize("N", [2, 3])
def test_incr_shift_vjp_matches_central_differences(N):
    rng = np.random.default_rng(40 + N)
    B = 16
    d = shift_case(rng, B, N)
    cots = shift_cotangents(rng, B, N)
    vxN = d["sol"][:, N * NXA + 3]
    assert (np.abs(vxN) < 0.3).sum() >= 2 and ((np.abs(vxN) > 0.3) & (np.abs(vxN) < 0.5)).sum() >= 1
    assert (vxN < -0.5).sum() >= 2 and (vxN > 0.5).sum() >= 2
    gsol, gAd0, gBd0, ggd0, gxt = mpc.incr_shift_vjp(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["xt"], *cots)
    grads = dict(sol=gsol, Ad0=gAd0, Bd0=gBd0, gd0=ggd0, xt=gxt)
    assert all(np.isfinite(g).all() for g in grads.values())
    assert copied_entries_are_exact(N, gsol, cots[1], cots[2], gu0=gxt[:, 6:])
    assert euler_zero_pattern_is_exact(N, d["sol"], gsol, cots[1])
    euler_cols = [(N + s) * NXA + i for s, i in EULER_INPUTS]

    def outputs(e):
        return np.concatenate([o.reshape(B, -1) for o in mpc.incr_shift(VEH, N, **e)], 1)

    c = np.concatenate([g.reshape(B, -1) for g in cots], 1)
    # everything the tail is linear in, one input array at a time, a random step of order 1
    worst = 0.0
    for key, grad in grads.items():
        dirn = rng.standard_normal(d[key].shape)
        if key == "sol":
            dirn[:, euler_cols] = 0.0
        diff = (outputs(dict(d, **{key: d[key] + dirn})) - outputs(dict(d, **{key: d[key] - dirn}))) / 2.0
        terms = c * diff
        fd, an = terms.sum(1), (grad * dirn).reshape(B, -1).sum(1)
        dev = (np.abs(fd - an) / np.abs(terms).max(1)).max()
        worst = max(worst, dev)
        print(f"incr_shift vjp N={N} {key}: deviation {dev:.2e}")
        assert np.abs(terms).max(1).all(), key
        assert dev < BAR_LINEAR, key
    print(f"measured incr_shift vjp N={N} linear part: {worst:.2e}, bar {BAR_LINEAR:.1e}")
    # the Euler step's six inputs, h = 1e-6
    fd = np.zeros((B, 6))
    for k, col in enumerate(euler_cols):
        e = np.zeros(d["sol"].shape[1])
        e[col] = H_EULER
        sp, sm = d["sol"] + e, d["sol"] - e
        fd[:, k] = (c * (outputs(dict(d, sol=sp)) - outputs(dict(d, sol=sm)))).sum(1) / (sp - sm).sum(1)
    an = gsol[:, euler_cols]
    dev = np.abs(fd - an) / np.abs(an).max(1)[:, None]
    slow = np.abs(vxN) < 0.5
    print(f"measured incr_shift vjp N={N} Euler inputs: per column {dev.max(0)}, worst {dev.max():.2e} (in the guard "
          f"{dev[slow].max():.2e}, vx < 0 {dev[vxN < 0].max():.2e}), bar {BAR_EULER:.1e}")
    assert dev.max() < BAR_EULER


def test_incr_shift_vjp_none_is_a_zero_cotangent():
    rng = np.random.default_rng(3)
    N, B = 3, 8
    d = shift_case(rng, B, N)
    cots = shift_cotangents(rng, B, N)
    full = mpc.incr_shift_vjp(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["xt"], *cots)
    parts = [mpc.incr_shift_vjp(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["xt"],
                                *[c if i == k else None for i, c in enumerate(cots)]) for k in range(3)]
    for j, f in enumerate(full):
        assert np.allclose(sum(p[j] for p in parts), f, rtol=0, atol=1e-13 * np.abs(f).max())
    # only gpdu: nothing reaches the model, the state or the predicted states
    assert not any(parts[2][j].any() for j in (1, 2, 3, 4)) and not parts[2][0][:, :(N + 1) * NXA].any()
    # leading axes are free
    one = mpc.incr_shift_vjp(VEH, N, d["sol"][2], d["Ad0"][2], d["Bd0"][2], d["xt"][2], *[c[2] for c in cots])
    assert all(np.array_equal(a, f[2]) for a, f in zip(one, full))
