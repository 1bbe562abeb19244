"""The dynamic bicycle's linearisation differentiated on the device (include/mpcqp.h, DESIGN.md
§17): k_linearise_vjp against its numpy statement, torch_mpc.linearise_dynamics against the entry
point it wraps, MPCLayer over the dynamic model against the CPU chain of tests/test_dyn_vjp_ref.py
at the device's own solution, and two closed-loop steps of mpc_dynamics.main's loop -- plant step
and shift in plain torch between two MPCLayers -- against central differences of the same device
computation.

Bars: BAR_LIN and BAR_CHAIN are ten times the deviation measured on the MI355X, max |a - b| /
max |b| per output array; the closed loop's rule and bar are those of
test_mpc_gain_matches_finite_differences (h = 1e-3, 1e-8 / h * 10 = 1e-4 of the largest derivative).
"""
import numpy as np
import pytest

import test_dyn_vjp_ref as dyn
import test_mpc_vjp_ref as cpu
from osqp_amd import mpc
from test_mpc_vjp_device import INCR_ADJOINT, TIGHT, Arena, _bits, _dev, _rel

pytestmark = pytest.mark.gpu

BAR_LIN = 1.5e-14          # measured: 1.42e-15 (B 130, N 2, without gAd; all three cotangents: <= 7.7e-16)
BAR_CHAIN = 1.2e-13        # measured: interior 1.13e-14, steer active 1.06e-14
BAR_LOOP = 1e-4
N_CHAIN = 3


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _vehicle():
    from osqp_amd.mpc_device import Vehicle
    veh = Vehicle()
    assert (veh.m, veh.l_f, veh.l_r, veh.dt) == (dyn.VEH.m, dyn.VEH.l_f, dyn.VEH.l_r, dyn.VEH.dt)
    return veh


def _points(rng, B, N):
    """(B, N) points of test_dyn_vjp_ref's sample, every fourth moved into the low-speed guard (both
    of its regions, both signs)."""
    x, u = dyn.sample(rng, B * N)
    slow = np.arange(B * N) % 4 == 0
    x[slow, 3] = dyn.guard_speeds(rng, int(slow.sum()))
    if B * N >= 8:
        x[0, 3], x[4, 3] = 0.2, -0.4                             # one of each region whatever the draw
    return x.reshape(B, N, 6), u.reshape(B, N, 2)


def _zero_pattern_is_exact(x, gx, gu, full=True):
    """X, Y never; vy, r, steer not for |vx| < 0.5; vx not for |vx| < 0.3.  full: with all three
    cotangents present everything else is not zero."""
    vx = np.abs(x[..., 3])
    zeros = (not gx[..., :2].any() and not gx[..., 4:][vx < 0.5].any() and not gu[..., 0][vx < 0.5].any()
             and not gx[..., 3][vx < 0.3].any())
    rest = (gx[..., 3][vx >= 0.3].all() and gx[..., 4:][vx >= 0.5].all() and gu[..., 0][vx >= 0.5].all()
            and gx[..., 2].all() and gu[..., 1].all())
    return zeros and (rest or not full)


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3])
def test_linearise_vjp_matches_the_host_statement(torch, B, N):
    from osqp_amd.mpc_device import linearise_vjp
    veh = _vehicle()
    rng = np.random.default_rng(60 + B + N)
    x, u = _points(rng, B, N)
    cots = dyn.cotangents(rng, (B, N))
    wx, wu = mpc.linearise_dynamics_vjp(dyn.VEH, x, u, *cots)
    tx, tu, tc = _dev(torch, x), _dev(torch, u), [_dev(torch, c) for c in cots]
    shapes = dict(gx=(B, N, 6), gu=(B, N, 2))
    arena, arena2 = Arena(torch, shapes), Arena(torch, shapes)
    linearise_vjp(veh, tx, tu, *tc, out=(arena.view["gx"], arena.view["gu"]))
    linearise_vjp(veh, tx, tu, *tc, out=(arena2.view["gx"], arena2.view["gu"]))
    torch.cuda.synchronize()
    assert arena.guards_intact() and arena2.guards_intact()
    gx, gu = arena.view["gx"].cpu().numpy(), arena.view["gu"].cpu().numpy()
    assert np.isfinite(gx).all() and np.isfinite(gu).all()
    assert _zero_pattern_is_exact(x, gx, gu) and _zero_pattern_is_exact(x, wx, wu)
    dev = dict(gx=_rel(gx, wx), gu=_rel(gu, wu))
    print(f"measured linearise vjp B={B} N={N}: gx {dev['gx']:.3e} gu {dev['gu']:.3e}")
    # two identical calls return identical bits
    assert _bits(arena2.view["gx"].cpu().numpy(), gx) and _bits(arena2.view["gu"].cpu().numpy(), gu)
    # each cotangent None in turn: the host statement's, and a zero tensor's bit for bit
    worst = max(dev.values())
    for k in range(3):
        some = [c if i != k else None for i, c in enumerate(tc)]
        zero = [c if i != k else torch.zeros_like(c) for i, c in enumerate(tc)]
        sx, su = linearise_vjp(veh, tx, tu, *some)
        zx, zu = linearise_vjp(veh, tx, tu, *zero)
        ex, eu = mpc.linearise_dynamics_vjp(dyn.VEH, x, u, *[c if i != k else None for i, c in enumerate(cots)])
        torch.cuda.synchronize()
        sx, su = sx.cpu().numpy(), su.cpu().numpy()
        assert _bits(sx, zx.cpu().numpy()) and _bits(su, zu.cpu().numpy())
        assert _zero_pattern_is_exact(x, sx, su, full=False)
        d = max(_rel(sx, ex), _rel(su, eu))
        print(f"measured linearise vjp B={B} N={N} without cotangent {k}: {d:.3e}")
        worst = max(worst, d)
    # one (x, u) for every stage (stage stride 0): the outputs stay dense, per stage
    xs, us = tx[:, :1].expand(B, N, 6), tu[:, :1].expand(B, N, 2)
    arena3 = Arena(torch, shapes)
    linearise_vjp(veh, xs, us, *tc, out=(arena3.view["gx"], arena3.view["gu"]))
    torch.cuda.synchronize()
    ex, eu = mpc.linearise_dynamics_vjp(dyn.VEH, np.repeat(x[:, :1], N, 1), np.repeat(u[:, :1], N, 1), *cots)
    d = max(_rel(arena3.view["gx"].cpu().numpy(), ex), _rel(arena3.view["gu"].cpu().numpy(), eu))
    print(f"measured linearise vjp B={B} N={N} stage stride 0: {d:.3e}")
    worst = max(worst, d)
    assert arena3.guards_intact()
    # 2-D inputs drop the stage axis
    fx, fu = linearise_vjp(veh, tx[:, 0], tu[:, 0], tc[0][:, 0].contiguous(), tc[1][:, 0].contiguous(),
                           tc[2][:, 0].contiguous())
    f3 = linearise_vjp(veh, tx[:, :1], tu[:, :1], tc[0][:, :1].contiguous(), tc[1][:, :1].contiguous(),
                       tc[2][:, :1].contiguous())
    torch.cuda.synchronize()
    assert fx.shape == (B, 6) and torch.equal(fx, f3[0][:, 0]) and torch.equal(fu, f3[1][:, 0])
    print(f"measured linearise vjp B={B} N={N}: worst {worst:.3e}, bar {BAR_LIN:.1e}")
    assert worst < BAR_LIN


def test_linearise_vjp_refuses_bad_inputs(torch):
    from osqp_amd.mpc_device import linearise_vjp
    veh = _vehicle()
    x, u = torch.zeros((2, 3, 6), dtype=torch.float64, device="cuda:0"), torch.zeros((2, 3, 2), dtype=torch.float64,
                                                                                    device="cuda:0")
    g = torch.zeros((2, 3, 6, 6), dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError):
        linearise_vjp(veh, x[..., :4], u, None, None, None)
    with pytest.raises(ValueError):
        linearise_vjp(veh, x.float(), u, None, None, None)
    with pytest.raises(ValueError):
        linearise_vjp(veh, x.transpose(1, 2).contiguous().transpose(1, 2), u, None, None, None)
    with pytest.raises(ValueError):
        linearise_vjp(veh, x, u, g[:, :2], None, None)
    with pytest.raises(ValueError):
        linearise_vjp(veh, x, u, g.float(), None, None)
    with pytest.raises(ValueError):
        linearise_vjp(veh, x, u, None, g, None)


def test_torch_linearise_dynamics_is_wired_to_the_vjp(torch):
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import linearise, linearise_vjp
    veh = _vehicle()
    rng = np.random.default_rng(71)
    B, N = 5, 3
    x, u = _points(rng, B, N)
    tx, tu = _dev(torch, x).requires_grad_(True), _dev(torch, u).requires_grad_(True)
    outs = tm.linearise_dynamics(veh, tx, tu)
    for o, w in zip(outs, linearise(veh, tx.detach(), tu.detach())):
        assert torch.equal(o, w)
    cots = [_dev(torch, c) for c in dyn.cotangents(rng, (B, N))]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    gx, gu = linearise_vjp(veh, tx.detach(), tu.detach(), *cots)
    assert torch.equal(tx.grad, gx) and torch.equal(tu.grad, gu)
    # only gd has a cotangent, only x requires a gradient
    ox, ou = _dev(torch, x).requires_grad_(True), _dev(torch, u)
    (g1,) = torch.autograd.grad((tm.linearise_dynamics(veh, ox, ou)[2] * cots[2]).sum(), [ox])
    assert torch.equal(g1, linearise_vjp(veh, ox.detach(), ou, None, None, cots[2])[0])
    # a stride-0 expand over the stages: the stage sum
    sx, su = _dev(torch, x[:, 0]).requires_grad_(True), _dev(torch, u[:, 0]).requires_grad_(True)
    outs = tm.linearise_dynamics(veh, sx[:, None, :].expand(B, N, 6), su[:, None, :].expand(B, N, 2))
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    gx, gu = linearise_vjp(veh, sx.detach()[:, None, :].expand(B, N, 6), su.detach()[:, None, :].expand(B, N, 2), *cots)
    assert torch.allclose(sx.grad, gx.sum(1), rtol=1e-14, atol=0) and torch.allclose(su.grad, gu.sum(1), rtol=1e-14,
                                                                                      atol=0)


# ----------------------------------------------------------------------- end to end --
PERT = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [1.0, -0.5, 0.7, 0.3, -0.8, 0.6], [-0.6, 1.0, -1.0, 0.5, 0.9, -0.4],
                 [0.4, 0.8, 0.9, -1.0, 0.3, 1.0], [-1.0, -0.9, 0.2, -0.7, -1.0, -0.9]])
POINTS = {
    # x0, the entry of du_0 that is the loss, the scale of PERT, the stages whose steer-increment row
    # is active in the step from x0 (the oracle's, tests/test_dyn_vjp_ref.py)
    "interior": (dyn.X0_INTERIOR, 0, 1e-4, ()),
    "steer active": (dyn.X0_ACTIVE, 1, 1e-3, (0, 2)),
}


def _layout(N):
    from osqp_amd.mpc_device import IncrementalLayout
    lay = IncrementalLayout(N, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                            -mpc.DYN_DUMIN)
    assert (lay.nx, lay.nu, lay.nxa, lay.nnzA) == (dyn.NX, dyn.NU, dyn.NXA, dyn.expected_nnz_A(N))
    return lay


def _classes(torch, layer, n):
    """row classes of every instance of the layer's last solve"""
    g = layer.qp.batch.adjoint(torch.zeros((layer.B, n), dtype=torch.float64, device="cuda:0"), None)
    layer.qp.batch.synchronize()
    return g.act.cpu().numpy()


@pytest.mark.parametrize("point", list(POINTS))
def test_mpc_layer_over_the_dynamic_model(torch, point):
    """MPCLayer on B = 5 states around the point: du_0[j].sum() backward to x0 through
    linearise_dynamics expanded to every stage, against the CPU chain at the device's own (x, y)."""
    from osqp_amd import torch_mpc as tm
    x0b, j, scale, active = POINTS[point]
    N, B, veh = N_CHAIN, len(PERT), _vehicle()
    lay = _layout(N)
    x0s = x0b + scale * PERT
    Xr = dyn.dyn_reference(N)
    layer = tm.MPCLayer(lay, B, strict=False, **dict(TIGHT, warm_start=True, **INCR_ADJOINT))
    tx = _dev(torch, x0s).requires_grad_(True)
    tu = _dev(torch, np.tile(dyn.U0, (B, 1)))
    Ad, Bd, gd = tm.linearise_dynamics(veh, tx[:, None, :].expand(B, N, 6), tu[:, None, :].expand(B, N, 2))
    X, U, y = layer(Ad, Bd, gd, torch.cat([tx, tu], dim=1), _dev(torch, np.tile(Xr, (B, 1, 1))))
    U[:, 0, j].sum().backward()
    torch.cuda.synchronize()
    print(f"{point}: status {layer.status.tolist()} iters {layer.iters.tolist()} astat {layer.astat.tolist()} "
          f"ares {layer.ares.flatten().tolist()}")
    assert (layer.status == 1).all() and (layer.astat == 1).all()
    gx0 = tx.grad.cpu().numpy()
    xs = torch.cat([X.reshape(B, -1), U.reshape(B, -1)], dim=1).detach().cpu().numpy()
    ys = y.detach().cpu().numpy()
    seed = np.zeros(lay.n)
    seed[dyn.seed_of(N, 0, j)] = 1.0
    worst = 0.0
    for b in range(B):
        P, q, A, l, u, _ = dyn.chain_problem(N, x0s[b], dyn.U0)
        a, frozen, total, _ = dyn.chain_gradients(N, x0s[b], dyn.U0, P, A, l, u, xs[b], ys[b], seed)
        on = np.flatnonzero((a.act == 1) | (a.act == 2))
        assert np.array_equal(on, dyn.steer_rows(N)[list(active)]), (b, on)
        d = _rel(gx0[b], total)
        worst = max(worst, d)
        print(f"{point}[{b}]: d du_0[{j}] / d x0 device {gx0[b]} chain {total} (frozen {frozen}) deviation {d:.3e}")
        # the frozen gain is another number: yaw, vy, r
        assert (np.abs(gx0[b] - frozen)[[2, 4, 5]] > 100 * cpu.BAR_CHAIN * np.abs(total).max()).all()
    print(f"measured e2e dyn {point} x0: {worst:.3e}, bar {BAR_CHAIN:.1e}")
    assert worst < BAR_CHAIN


def _two_steps(torch, tm, veh, layers, tx, tu, Xr1, Xr2, j, qdiag=None):
    """Two steps of mpc_dynamics.main's loop from (tx, tu): step 1 linearised at (x0, u0) on every
    stage; u = u0 + du_0, x1 = Ad_0 x0 + Bd_0 u + gd_0; the next horizon is (x1, u) and stages 2..N
    of the solution; step 2 linearised per stage there, its reference shifted by one.  Returns step
    2's du_0[j] per instance."""
    Bn, N = tx.shape[0], layers[0].layout.N
    weights = None if qdiag is None else (torch.diag(qdiag), None, None)
    Ad, Bd, gd = tm.linearise_dynamics(veh, tx[:, None, :].expand(Bn, N, 6), tu[:, None, :].expand(Bn, N, 2))
    X1, U1, _ = layers[0](Ad, Bd, gd, torch.cat([tx, tu], dim=1), Xr1, weights=weights)
    u = tu + U1[:, 0]
    x1 = (Ad[:, 0] @ tx[:, :, None])[:, :, 0] + (Bd[:, 0] @ u[:, :, None])[:, :, 0] + gd[:, 0]
    xt1 = torch.cat([x1, u], dim=1)
    horizon = torch.cat([xt1[:, None, :], X1[:, 2:N + 1]], dim=1)          # (Bn, N, 8): distinct points
    Ad2, Bd2, gd2 = tm.linearise_dynamics(veh, horizon[:, :, :6], horizon[:, :, 6:])
    X2, U2, _ = layers[1](Ad2, Bd2, gd2, xt1, Xr2, weights=weights)
    return U2[:, 0, j]


@pytest.mark.parametrize("point", list(POINTS))
def test_two_closed_loop_steps(torch, point):
    """d (step 2's du_0[j]) / d x0 from one backward through two MPCLayers, the plant step and the
    shift, against central differences (h = 1e-3 in each state; the perturbed copies ride in the
    same batch) of the same device computation: 1e-4 of the largest derivative.  And d loss / d
    diag Q, the loss summed over that batch, against central differences with H_Q = 1e-3 in the
    weight.  Row classes are equal at every point of both steps: no active row on the interior
    point, two steer-increment rows in either step on the other.
    Measured on the MI355X, of the largest derivative: x0 5.6e-6 (interior; the issue's own 1e-3 against
    1e-4 quotients differ by 6e-6, the truncation of h = 1e-3) and 2.9e-8 (steer active), diag Q
    2.0e-9 and 7.3e-9."""
    from osqp_amd import torch_mpc as tm
    x0b, j, _, active = POINTS[point]
    N, veh, h = N_CHAIN, _vehicle(), 1e-3
    lay = _layout(N)
    pts = np.concatenate([[x0b]] + [[x0b + s * h * e] for e in np.eye(6) for s in (1.0, -1.0)])
    Bn = len(pts)
    Xr1 = _dev(torch, np.tile(dyn.dyn_reference(N), (Bn, 1, 1)))
    shifted = dyn.dyn_reference(N)
    shifted[0] += 0.5
    Xr2 = _dev(torch, np.tile(shifted, (Bn, 1, 1)))
    settings = dict(TIGHT, warm_start=True, **INCR_ADJOINT)
    layers = [tm.MPCLayer(lay, Bn, **settings) for _ in range(2)]
    tx, tu = _dev(torch, pts).requires_grad_(True), _dev(torch, np.tile(dyn.U0, (Bn, 1)))
    qdiag = _dev(torch, np.diag(mpc.DYN_Q)).requires_grad_(True)
    out = _two_steps(torch, tm, veh, layers, tx, tu, Xr1, Xr2, j, qdiag)
    (gx,) = torch.autograd.grad(out[0], [tx], retain_graph=True)
    (gq,) = torch.autograd.grad(out.sum(), [qdiag])
    torch.cuda.synchronize()
    for k, layer in enumerate(layers):
        print(f"{point} step {k + 1}: status {layer.status.tolist()} iters {layer.iters.tolist()} "
              f"astat {layer.astat.tolist()}")
        assert (layer.status == 1).all() and (layer.astat == 1).all()
    acts = [_classes(torch, layer, lay.n) for layer in layers]
    for k, act in enumerate(acts):
        assert (act == act[0]).all(), f"{point}: the active set changes within the steps of step {k + 1}"
        on = np.flatnonzero((act[0] == 1) | (act[0] == 2))
        print(f"{point} step {k + 1}: active inequality rows {on}")
        assert len(on) == len(active) and np.isin(on, dyn.steer_rows(N)).all(), (k, on)
    assert np.array_equal(np.flatnonzero((acts[0][0] == 1) | (acts[0][0] == 2)), dyn.steer_rows(N)[list(active)])
    gx, val = gx.cpu().numpy(), out.detach().cpu().numpy()
    assert not gx[1:].any()
    fd = (val[1::2] - val[2::2]) / (2 * h)
    dev = np.abs(fd - gx[0]).max() / np.abs(fd).max()
    print(f"{point}: d du_0[{j}](step 2) / d x0: fd {fd} backward {gx[0]} deviation {dev:.2e}")
    # the weights: forward runs alone, the two layers reused
    fdl = [tm.MPCLayer(lay, Bn, **settings) for _ in range(2)]
    fq = np.zeros(6)
    for i in range(6):
        vals = []
        for s in (1.0, -1.0):
            qd = np.diag(mpc.DYN_Q).copy()
            qd[i] += s * cpu.H_Q
            with torch.no_grad():
                v = _two_steps(torch, tm, veh, fdl, tx.detach(), tu, Xr1, Xr2, j, _dev(torch, qd))
            torch.cuda.synchronize()
            assert all((layer.status == 1).all() for layer in fdl)
            for k, layer in enumerate(fdl):
                assert (_classes(torch, layer, lay.n) == acts[k][0]).all(), f"{point}: Q[{i}] moves the active set"
            vals.append(v.sum().item())
        fq[i] = (vals[0] - vals[1]) / (2 * cpu.H_Q)
    gq = gq.cpu().numpy()
    dev_q = np.abs(fq - gq).max() / np.abs(fq).max()
    print(f"{point}: d loss / d diag Q: fd {fq} backward {gq} deviation {dev_q:.2e}")
    assert dev < BAR_LOOP
    assert dev_q < BAR_LOOP
