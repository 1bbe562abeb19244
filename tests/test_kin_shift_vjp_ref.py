"""osqp_amd.mpc.kin_incr_shift / kin_ltv_shift and their VJPs, the numpy statements of the two
kinematic tails (kin_incr_step_shift under k_kin_shift and k_lane_tail; k_kin_ltv_shift) and of
k_tail_vjp<KinIncrTail> / <KinLtvTail>: the forwards against the reference's own
steps (tests/golden/kin_sim_n40.npz, kinltv_sim_n3.npz) and against mpc.lane_tail, the VJPs against
central differences of the forwards, the masks' copies and zeros exactly.

Both tails are linear or bilinear in everything but the six inputs of the terminal
update_kinematics_model step -- x~_N's own six entries for the incremental tail, (S_N, U_{N-1}) for
the LTV one -- so there a central difference with a step of order 1 is exact up to rounding
(tests/test_mpc_vjp_ref.py's BAR_LINEAR, of the contraction's largest term).  The six are differenced
with h = 1e-6 as tests/test_shift_vjp_ref.py does it, against BAR_LIN = 1e-7 of
tests/test_mpc_vjp_ref.py: the same h on the same model.
"""
import numpy as np
import pytest

from osqp_amd import mpc
from test_mpc_vjp_ref import BAR_LIN, BAR_LINEAR, DT, LF, LR

VEH = (LF, LR, DT)
H_UPDATE = 1e-6
TOL = dict(rtol=1e-12, atol=1e-12)     # tests/test_kin_device.py's, for kin_sim_n40.npz


def kin_modes(B, kind):
    """Every fourth vehicle untouched (mode 1); for the incremental tail every fifth, where not that,
    stopped on this step (mode 2)."""
    b = np.arange(B)
    mode = np.where(b % 4 == 0, 1, 0)
    if kind == "incr":
        mode = np.where((b % 5 == 0) & (mode == 0), 2, mode)
    return mode.astype(np.int32)


def kin_case(rng, B, N, kind):
    """B vehicles' inputs of a kinematic tail: solutions whose states are (X, Y in +-5, v in 2..12 or
    reversing, yaw in +-1) with inputs (steer +-0.25, accel +-1), a random stage-0 model, the state
    before the step and the previous horizon (what a vehicle in mode 1 keeps)."""
    nxa = 6 if kind == "incr" else 4
    M = B * (N + 1)
    v = rng.uniform(2, 12, M) * np.where(rng.uniform(size=M) < 0.2, -1.0, 1.0)
    x = np.stack([rng.uniform(-5, 5, M), rng.uniform(-5, 5, M), v, rng.uniform(-1, 1, M)], 1)
    u = np.stack([rng.uniform(-0.25, 0.25, M), rng.uniform(-1, 1, M)], 1)
    if kind == "incr":
        X = np.concatenate([x, u], 1).reshape(B, N + 1, 6)
        D = rng.uniform(-0.03, 0.03, (B, N, 2))
    else:
        X, D = x.reshape(B, N + 1, 4), u[:B * N].reshape(B, N, 2)
    d = dict(sol=np.concatenate([X.reshape(B, -1), D.reshape(B, -1)], 1),
             Ad0=np.eye(4) + 0.05 * rng.standard_normal((B, 4, 4)), Bd0=0.05 * rng.standard_normal((B, 4, 2)),
             gd0=0.05 * rng.standard_normal((B, 4)), x=rng.standard_normal((B, nxa)))
    if kind == "incr":
        d.update(pred=rng.standard_normal((B, N + 1, 6)), pdu=rng.standard_normal((B, N + 1, 2)))
    else:
        d.update(u=rng.standard_normal((B, 2)), pred_x=rng.standard_normal((B, N + 1, 4)),
                 pred_u=rng.standard_normal((B, N + 1, 2)))
    return d


def kin_cotangents(rng, B, N, kind):
    if kind == "incr":
        shapes = [(B, 6), (B, N + 1, 6), (B, N + 1, 2)]
    else:
        shapes = [(B, 4), (B, 2), (B, N + 1, 4), (B, N + 1, 2)]
    return [rng.standard_normal(s) for s in shapes]


def forward(kind, N, d, mode=None):
    if kind == "incr":
        return mpc.kin_incr_shift(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["gd0"], d["x"], mode, d["pred"], d["pdu"])
    return mpc.kin_ltv_shift(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["gd0"], d["x"], mode, d["u"], d["pred_x"],
                             d["pred_u"])


def vjp(kind, N, d, cots, mode=None):
    """(gsol, gAd0, gBd0, ggd0, g state before) of the host statement."""
    fn = mpc.kin_incr_shift_vjp if kind == "incr" else mpc.kin_ltv_shift_vjp
    return fn(VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["x"], *cots, mode=mode)


def update_columns(kind, N):
    """The columns of sol that are the terminal update's six inputs."""
    if kind == "incr":
        return [N * 6 + i for i in range(6)]
    return [N * 4 + i for i in range(4)] + [(N + 1) * 4 + (N - 1) * 2 + j for j in range(2)]


def split(kind, N, gsol):
    nxa, B = (6 if kind == "incr" else 4), gsol.shape[0]
    return gsol[:, :(N + 1) * nxa].reshape(B, N + 1, nxa), gsol[:, (N + 1) * nxa:].reshape(B, N, 2)


def masks_are_exact(kind, N, mode, cots, g):
    """What the masks promise, bit for bit: a mode-1 vehicle gets zero in gsol and the model outputs and
    its state's cotangent back; a mode-2 vehicle the unpacked solution's copies."""
    gsol, gA, gB, gg, gxb = g
    gX, gD = split(kind, N, gsol)
    gstate = cots[0]
    gpred, gpdu = (cots[1], cots[2]) if kind == "incr" else (cots[2], cots[3])
    m1, m2 = mode == 1, mode == 2
    ok = not gsol[m1].any() and np.array_equal(gxb[mode != 0], gstate[mode != 0])
    ok = ok and not gA[mode != 0].any() and not gB[mode != 0].any() and not gg[mode != 0].any()
    if m2.any():
        ok = ok and np.array_equal(gX[m2], gpred[m2]) and np.array_equal(gD[m2, :N - 1], gpdu[m2, :N - 1])
        ok = ok and np.array_equal(gD[m2, N - 1], gpdu[m2, N - 1] + gpdu[m2, N])
    return bool(ok)


def copies_are_exact(kind, N, mode, cots, g):
    """What a stepped vehicle's tail only copies: stages 0 and 1 of the states get nothing (but U_1 at
    N = 2), stage k (2 <= k < N) takes the cotangent of stage k-1, input k that of k-1, the last input
    its three copies in the output's order; ggd0 is w; the first input's cotangent is g u."""
    gsol, gA, gB, gg, gxb = g
    gX, gD = split(kind, N, gsol)
    s = mode == 0
    if kind == "incr":
        gxt, gpred, gpdu = cots
        w = gxt + gpred[:, 0]
        ok = np.array_equal(gD[s, 0], gxb[s, 4:]) and np.array_equal(gg[s], w[s, :4])
        ok = ok and np.array_equal(gD[s, N - 1], (gpdu[s, N - 2] + gpdu[s, N - 1]) + gpdu[s, N])
    else:
        gx, gu, gpred, gpdu = cots
        ok = np.array_equal(gg[s], (gx + gpred[:, 0])[s])
    ok = ok and not gX[s, 0].any() and not gX[s, 1].any() and np.array_equal(gX[s, 2:N], gpred[s, 1:N - 1])
    ok = ok and np.array_equal(gD[s, 1:N - 1], gpdu[s, 0:N - 2])
    return bool(ok)


# ------------------------------------------------------------------------- forwards --
def test_kin_incr_shift_matches_lane_tail_and_the_reference_steps(golden):
    g = golden("kin_sim_n40.npz")
    N = 40
    xt, pred, pdu = mpc.kin_incr_shift(VEH, N, g["sol"], g["in_Ad"][:, 0], g["in_Bd"][:, 0], g["in_gd"][:, 0],
                                       g["in_xt"])
    assert np.allclose(xt, g["out_xt"], **TOL) and np.allclose(pred, g["out_pred"].transpose(0, 2, 1), **TOL)
    assert np.allclose(pdu, g["out_pdu"].transpose(0, 2, 1), **TOL)
    for t in range(g["sol"].shape[0]):
        _, lx, lp, ld, _, _ = mpc.lane_tail(g["sol"][t], g["in_Ad"][t][0], g["in_Bd"][t][0], g["in_gd"][t][0],
                                            g["in_xt"][t], 0, N, *VEH)
        # lane_tail's plant step is numpy's matrix product, kin_incr_shift's the kernel's association
        assert np.allclose(xt[t], lx, **TOL) and np.allclose(pred[t], lp, **TOL) and np.array_equal(pdu[t], ld)
        assert np.array_equal(pred[t, 1:], lp[1:])
    # one vehicle without a batch axis
    one = mpc.kin_incr_shift(VEH, N, g["sol"][1], g["in_Ad"][1, 0], g["in_Bd"][1, 0], g["in_gd"][1, 0], g["in_xt"][1])
    assert all(np.array_equal(a, b[1]) for a, b in zip(one, (xt, pred, pdu)))


def test_kin_ltv_shift_matches_the_reference_steps(golden):
    g = golden("kinltv_sim_n3.npz")
    N = 3
    x, u, px, pu = mpc.kin_ltv_shift(VEH, N, g["sol"], g["in_Ad"][:, 0], g["in_Bd"][:, 0], g["in_gd"][:, 0], g["in_x"])
    assert np.allclose(x, g["out_x"], **TOL) and np.array_equal(u, g["sol"][:, (N + 1) * 4:(N + 1) * 4 + 2])
    assert np.allclose(px, g["out_pred_x"].transpose(0, 2, 1), **TOL)
    assert np.allclose(pu, g["out_pred_u"].transpose(0, 2, 1), **TOL)


@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_masked_forwards_keep_what_they_should(kind):
    rng = np.random.default_rng(7)
    N, B = 3, 20
    d, mode = kin_case(rng, B, N, kind), kin_modes(B, kind)
    out, plain = forward(kind, N, d, mode), forward(kind, N, d)
    keep = (d["x"], d["pred"], d["pdu"]) if kind == "incr" else (d["x"], d["u"], d["pred_x"], d["pred_u"])
    for o, p, k in zip(out, plain, keep):
        assert np.array_equal(o[mode == 1], k[mode == 1]) and np.array_equal(o[mode == 0], p[mode == 0])
    if kind == "incr":
        m2 = mode == 2
        X, D = split(kind, N, d["sol"])
        assert m2.any() and np.array_equal(out[0][m2], d["x"][m2]) and np.array_equal(out[1][m2], X[m2])
        assert np.array_equal(out[2][m2, :N], D[m2]) and np.array_equal(out[2][m2, N], D[m2, N - 1])


# ----------------------------------------------------------------------------- VJPs --
def test_kin_update_vjp_matches_central_differences():
    rng = np.random.default_rng(12)
    n, h = 64, H_UPDATE
    d = kin_case(rng, n, 1, "incr")
    z = d["sol"][:, :6]
    w = rng.standard_normal((n, 4))
    gx, gu = mpc.kin_update_vjp(*VEH, z[:, :4], z[:, 4:], w)
    an = np.concatenate([gx, gu], 1)
    assert np.array_equal(gx[:, :2], w[:, :2])
    for c in range(6):
        e = np.zeros(6)
        e[c] = h
        zp, zm = z + e, z - e
        fd = (w * (mpc.kin_update(*VEH, zp[:, :4], zp[:, 4:]) - mpc.kin_update(*VEH, zm[:, :4], zm[:, 4:]))).sum(1) \
            / (zp - zm).sum(1)
        dev = (np.abs(fd - an[:, c]) / np.abs(an).max(1)).max()
        print(f"kin_update vjp input {c}: deviation {dev:.2e}")
        assert dev < BAR_LIN


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_tail_vjp_matches_central_differences(kind, N):
    rng = np.random.default_rng(50 + N)
    B = 16
    d = kin_case(rng, B, N, kind)
    cots = kin_cotangents(rng, B, N, kind)
    g = vjp(kind, N, d, cots)
    grads = dict(sol=g[0], Ad0=g[1], Bd0=g[2], gd0=g[3], x=g[4])
    assert all(np.isfinite(v).all() for v in grads.values())
    zero = np.zeros(B, np.int32)
    assert copies_are_exact(kind, N, zero, cots, g)
    cols = update_columns(kind, N)

    def outputs(e):
        return np.concatenate([o.reshape(B, -1) for o in forward(kind, N, e)], 1)

    c = np.concatenate([v.reshape(B, -1) for v in cots], 1)
    worst = 0.0
    for key, grad in grads.items():
        dirn = rng.standard_normal(d[key].shape)
        if key == "sol":
            dirn[:, cols] = 0.0
        diff = (outputs(dict(d, **{key: d[key] + dirn})) - outputs(dict(d, **{key: d[key] - dirn}))) / 2.0
        terms = c * diff
        fd, an = terms.sum(1), (grad * dirn).reshape(B, -1).sum(1)
        dev = (np.abs(fd - an) / np.abs(terms).max(1)).max()
        worst = max(worst, dev)
        print(f"{kind} tail vjp N={N} {key}: deviation {dev:.2e}")
        assert np.abs(terms).max(1).all(), key
        assert dev < BAR_LINEAR, key
    print(f"measured {kind} tail vjp N={N} linear part: {worst:.2e}, bar {BAR_LINEAR:.1e}")
    fd = np.zeros((B, 6))
    for k, col in enumerate(cols):
        e = np.zeros(d["sol"].shape[1])
        e[col] = H_UPDATE
        sp, sm = d["sol"] + e, d["sol"] - e
        fd[:, k] = (c * (outputs(dict(d, sol=sp)) - outputs(dict(d, sol=sm)))).sum(1) / (sp - sm).sum(1)
    an = g[0][:, cols]
    dev = np.abs(fd - an) / np.abs(an).max(1)[:, None]
    print(f"measured {kind} tail vjp N={N} update inputs: per column {dev.max(0)}, worst {dev.max():.2e}, "
          f"bar {BAR_LIN:.1e}")
    assert dev.max() < BAR_LIN


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_masked_vehicles_copy_and_zero_exactly(kind, N):
    rng = np.random.default_rng(60 + N)
    B = 16
    d, mode = kin_case(rng, B, N, kind), kin_modes(B, kind)
    cots = kin_cotangents(rng, B, N, kind)
    g, plain = vjp(kind, N, d, cots, mode), vjp(kind, N, d, cots)
    assert (mode == 1).sum() == 4 and ((mode == 2).sum() == 3) == (kind == "incr")
    assert masks_are_exact(kind, N, mode, cots, g) and copies_are_exact(kind, N, mode, cots, g)
    # a stepped vehicle is not touched by its neighbours' masks
    assert all(np.array_equal(a[mode == 0], p[mode == 0]) for a, p in zip(g, plain))
    # and the masked forwards have exactly these transposes: the outputs of a mode-1 vehicle do not move
    # with sol or the model, those of a mode-2 vehicle are copies of sol
    c = np.concatenate([v.reshape(B, -1) for v in cots], 1)

    def outputs(e):
        return np.concatenate([o.reshape(B, -1) for o in forward(kind, N, e, mode)], 1)

    off = mode != 0
    for key, grad in (("sol", g[0]), ("Ad0", g[1]), ("Bd0", g[2]), ("gd0", g[3]), ("x", g[4])):
        dirn = rng.standard_normal(d[key].shape)
        diff = (outputs(dict(d, **{key: d[key] + dirn})) - outputs(dict(d, **{key: d[key] - dirn}))) / 2.0
        terms = (c * diff)[off]
        fd, an = terms.sum(1), (grad * dirn).reshape(B, -1).sum(1)[off]
        scale = np.maximum(np.abs(terms).max(1), 1e-300)
        assert (np.abs(fd - an) / scale).max() < BAR_LINEAR, key
        assert not an[np.abs(terms).max(1) == 0].any(), key


@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_none_is_a_zero_cotangent(kind):
    rng = np.random.default_rng(4)
    N, B = 3, 8
    d, mode = kin_case(rng, B, N, kind), kin_modes(B, kind)
    cots = kin_cotangents(rng, B, N, kind)
    full = vjp(kind, N, d, cots, mode)
    parts = [vjp(kind, N, d, [c if i == k else None for i, c in enumerate(cots)], mode) for k in range(len(cots))]
    for j, f in enumerate(full):
        assert np.allclose(sum(p[j] for p in parts), f, rtol=0, atol=1e-13 * np.abs(f).max())
    one = vjp(kind, N, {k: v[2] for k, v in d.items()}, [c[2] for c in cots], mode[2])
    assert all(np.array_equal(a, f[2]) for a, f in zip(one, full))
