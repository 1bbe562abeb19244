"""The kinematic closed loops differentiated on one solver handle (include/mpcqp.h):
k_tail_vjp<KinIncrTail> and <KinLtvTail> against their numpy statements, masks included; the torch
tails against the wrappers; torch_mpc.KinematicRollout / KinematicLTVRollout -- forward against
KinematicMPC / KinematicLTVMPC, the masks end to end, backward against a chain of two recording
MPCLayers with the torch tail between them and against central differences.

Bars: BAR_KIN_SHIFT and BAR_KIN_ROLL are ten times the deviation measured on the MI355X, max |a - b| /
max |b| per array (the project's rule); BAR_LOOP is
tests/test_dyn_vjp_device.py's (h = 1e-3: 1e-8 / h * 10 = 1e-4 of the largest derivative).  Copies,
zeros and everything the solution record promises are held bit for bit.
"""
import numpy as np
import pytest

import test_kin_rollout_ref as loop
import test_kin_shift_vjp_ref as ks
import test_mpc_vjp_ref as cpu
from osqp_amd import mpc
from test_dyn_vjp_device import BAR_LOOP
from test_mpc_vjp_device import E2E, INCR_ADJOINT, PERT, TIGHT, Arena, _bits, _dev, _mpc_layout, _rel

pytestmark = pytest.mark.gpu

# measured: ltv 2.22e-16 (B 1, N 3, without gx; B 130: 2.18e-16), incr 1.79e-16 (B 130, N 2); the deviation
# sits in gsol's terminal rows and the state's cotangent -- the sum order and FMA contraction of
# kin_update_vjp, Ad0' w and Bd0' w --; gAd0, gBd0: 0; the stop-rule call 7.5e-17
BAR_KIN_SHIFT = 2.3e-15
# measured against the chain through one MPCLayer(record=True): d control / d x0 0 on all three cases (the
# same kernels on the same bits), d loss / d diag Q 1.55e-16 (incr interior), 1.47e-16 (incr active),
# 1.1e-19 (ltv): the weight sums run in another order (per instance, then over the batch)
BAR_KIN_ROLL = 1.6e-15
SETTINGS = {"incr": dict(TIGHT, **INCR_ADJOINT), "ltv": dict(TIGHT)}   # warm start off: both sides solve cold
CASES = {
    # kind, x0, u0, the entry of the first control that is the loss, the scale of PERT
    "incr interior": ("incr",) + E2E["incr interior"][2:6],
    "incr active": ("incr",) + E2E["incr active"][2:6],
    "ltv": ("ltv",) + E2E["ltv N=3"][2:6],
}
N_CHAIN = 3


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _veh():
    from osqp_amd.mpc_device import KinVehicle
    veh = KinVehicle()
    assert (veh.l_f, veh.l_r, veh.dt) == ks.VEH
    return veh


def _idev(torch, a):
    return _dev(torch, np.asarray(a), torch.int32)


# ------------------------------------------------------------------ the tails' VJPs --
def _tail_device_inputs(torch, rng, d, B, N):
    """The host case as the device takes it: (B, N, ..) models whose stage 0 is the case's (the other
    stages, which nothing may read, are noise)."""
    Ad, Bd, gd = rng.standard_normal((B, N, 4, 4)), rng.standard_normal((B, N, 4, 2)), rng.standard_normal((B, N, 4))
    Ad[:, 0], Bd[:, 0], gd[:, 0] = d["Ad0"], d["Bd0"], d["gd0"]
    t = {k: _dev(torch, v) for k, v in d.items() if k not in ("Ad0", "Bd0", "gd0")}
    t.update(Ad=_dev(torch, Ad), Bd=_dev(torch, Bd), gd=_dev(torch, gd))
    return t


def _stop_rule_inputs(torch, d, mode, N):
    """Xr, finish_cnt and done that put each vehicle of the incremental tail into its mode: a mode-2
    vehicle stands 0.1 from its first reference point with the count at 15, the others 10 away."""
    B = len(mode)
    Xr = np.zeros((B, 4, N + 1))
    Xr[:, 0, 0] = d["x"][:, 0] + np.where(mode == 2, 0.1, 10.0)
    Xr[:, 1, 0] = d["x"][:, 1]
    return _dev(torch, Xr), _idev(torch, np.where(mode == 2, 15, 3)), _idev(torch, mode == 1)


def _forward_device(torch, kind, lay, veh, t, d, mode, N):
    """The functional forward with the masks produced by the loop's own rules; returns (outputs, mode)."""
    from osqp_amd import mpc_device as md
    if kind == "incr":
        Xr, cnt, done = _stop_rule_inputs(torch, d, mode, N)
        out = md.kin_shift(lay, veh, t["sol"], t["Ad"], t["Bd"], t["gd"], Xr, t["x"], t["pred"], t["pdu"], cnt, done)
        assert torch.equal(out[3], cnt + _idev(torch, mode == 2)) and torch.equal(out[4], _idev(torch, mode != 0))
        return out[:3], out[5]
    status = _idev(torch, np.where(mode == 1, -3, 1))
    out = md.kin_ltv_shift(lay, veh, t["sol"], status, t["Ad"], t["Bd"], t["gd"], t["x"], t["u"], t["pred_x"],
                           t["pred_u"])
    return out[:4], out[4]


def _vjp_device(kind, lay, veh, t, mode, cots, **kw):
    from osqp_amd import mpc_device as md
    fn = md.kin_shift_vjp if kind == "incr" else md.kin_ltv_shift_vjp
    return fn(lay, veh, t["sol"], t["Ad"], t["Bd"], t["x"], mode, *cots, **kw)


def _names(kind):
    from osqp_amd import mpc_device as md
    return md.SHIFT_VJP_OUTPUTS if kind == "incr" else md.KIN_LTV_SHIFT_VJP_OUTPUTS


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_tail_vjp_kernel_matches_the_host_statement(torch, kind, N, B):
    """Measured on the MI355X (max |a - b| / max |b| per array, the worst of every variant below):
    incr B 1: 8.89e-17 (N 2), 1.26e-17 (N 3); B 130: 1.79e-16 (N 2), 1.35e-16 (N 3);
    ltv B 1: 1.28e-16 (N 2), 2.22e-16 (N 3); B 130: 1.41e-16 (N 2), 2.18e-16 (N 3)."""
    veh, (lay, _) = _veh(), _mpc_layout(kind, N)
    rng = np.random.default_rng(90 + B + N)
    d, cots = ks.kin_case(rng, B, N, kind), ks.kin_cotangents(rng, B, N, kind)
    mode = ks.kin_modes(B, kind) if B > 1 else np.zeros(1, np.int32)
    t = _tail_device_inputs(torch, rng, d, B, N)
    tc = [_dev(torch, c) for c in cots]
    # the functional forward: the host statement's values and the modes, nothing written in place
    keep = {k: v.clone() for k, v in t.items()}
    outs, tmode = _forward_device(torch, kind, lay, veh, t, d, mode, N)
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], keep[k]) for k in t)
    assert np.array_equal(tmode.cpu().numpy(), mode) and tmode.dtype == torch.int32
    for o, h in zip(outs, ks.forward(kind, N, d, mode)):
        assert np.allclose(o.cpu().numpy(), h, rtol=1e-12, atol=1e-12)
        assert np.array_equal(o.cpu().numpy()[mode != 0], h[mode != 0])          # what a mask keeps is a copy
    # the VJP
    names = _names(kind)
    host = dict(zip(names, ks.vjp(kind, N, d, cots, mode)))
    shapes = {k: (B,) + v.shape[1:] for k, v in host.items()}
    arena, arena2 = Arena(torch, shapes), Arena(torch, shapes)
    for a in (arena, arena2):
        o = _vjp_device(kind, lay, veh, t, tmode, tc, out=a.view)
    torch.cuda.synchronize()
    assert arena.guards_intact() and arena2.guards_intact()
    got = {k: arena.view[k].cpu().numpy() for k in names}
    assert all(np.isfinite(v).all() for v in got.values())
    assert all(_bits(arena2.view[k].cpu().numpy(), got[k]) for k in names)     # a repeat returns the same bits
    g = [got[k] for k in names]
    assert ks.masks_are_exact(kind, N, mode, cots, g) and ks.copies_are_exact(kind, N, mode, cots, g)
    assert _bits(got["ggd0"], host["ggd0"])
    # the caller's part: the previous horizon's cotangent passes where the vehicle was left untouched
    prev = ("gpred_prev", "gpdu_prev") if kind == "incr" else ("gu_prev", "gpred_x_prev", "gpred_u_prev")
    for k, c in zip(prev, cots[1:]):
        want = np.where((mode == 1).reshape((-1,) + (1,) * (c.ndim - 1)), c, 0.0)
        assert _bits(getattr(o, k).cpu().numpy(), want), k
    assert all(getattr(_vjp_device(kind, lay, veh, t, tmode, [None] * len(tc)), k) is None for k in prev)
    worst = 0.0
    for k in names:
        dev = _rel(got[k], host[k])
        worst = max(worst, dev)
        print(f"measured {kind} tail vjp B={B} N={N} {k}: {dev:.3e}")
    # mode NULL is mode 0 everywhere
    if B > 1:
        plain = _vjp_device(kind, lay, veh, t, None, tc)
        zeros = _vjp_device(kind, lay, veh, t, torch.zeros_like(tmode), tc)
        hp = dict(zip(names, ks.vjp(kind, N, d, cots)))
        for k in names:
            assert torch.equal(getattr(plain, k), getattr(zeros, k)), k
            worst = max(worst, _rel(getattr(plain, k).cpu().numpy(), hp[k]))
    # each cotangent None in turn: the host statement's, and a zero tensor's bit for bit
    for i in range(len(tc)):
        some = [c if j != i else None for j, c in enumerate(tc)]
        zero = [c if j != i else torch.zeros_like(c) for j, c in enumerate(tc)]
        s, z = _vjp_device(kind, lay, veh, t, tmode, some), _vjp_device(kind, lay, veh, t, tmode, zero)
        e = dict(zip(names, ks.vjp(kind, N, d, [c if j != i else None for j, c in enumerate(cots)], mode)))
        torch.cuda.synchronize()
        for k in names:
            sk = getattr(s, k).cpu().numpy()
            assert _bits(sk, getattr(z, k).cpu().numpy()), (i, k)
            dev = _rel(sk, e[k]) if np.abs(e[k]).max() > 0 else float(np.abs(sk).max())
            worst = max(worst, dev)
        print(f"measured {kind} tail vjp B={B} N={N} without cotangent {i}: worst so far {worst:.3e}")
    # each output left out in turn: its buffer keeps the sentinels, the others their bits
    for k in names:
        a = Arena(torch, shapes)
        o = _vjp_device(kind, lay, veh, t, tmode, tc, want=[w for w in names if w != k],
                        out={w: v for w, v in a.view.items() if w != k})
        torch.cuda.synchronize()
        assert getattr(o, k) is None and a.untouched(k) and a.guards_intact()
        assert all(_bits(a.view[w].cpu().numpy(), got[w]) for w in names if w != k)
    print(f"measured {kind} tail vjp B={B} N={N}: worst {worst:.3e}, bar {BAR_KIN_SHIFT:.1e}")
    assert worst < BAR_KIN_SHIFT


@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_torch_tails_are_wired_to_the_vjps(torch, kind):
    from osqp_amd import torch_mpc as tm
    veh, N, B = _veh(), 3, 9
    lay, _ = _mpc_layout(kind, N)
    rng = np.random.default_rng(93)
    d, mode = ks.kin_case(rng, B, N, kind), ks.kin_modes(B, kind)
    t = _tail_device_inputs(torch, rng, d, B, N)
    ins = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    if kind == "incr":
        Xr, cnt, done = _stop_rule_inputs(torch, d, mode, N)
        outs = tm.kin_shift(lay, veh, ins["sol"], ins["Ad"], ins["Bd"], ins["gd"], Xr, ins["x"], ins["pred"],
                            ins["pdu"], cnt, done)
        diff, tmode, prev = outs[:3], outs[5], dict(pred="gpred_prev", pdu="gpdu_prev")
    else:
        status = _idev(torch, np.where(mode == 1, -3, 1))
        outs = tm.kin_ltv_shift(lay, veh, ins["sol"], status, ins["Ad"], ins["Bd"], ins["gd"], ins["x"], ins["u"],
                                ins["pred_x"], ins["pred_u"])
        diff, tmode, prev = outs[:4], outs[4], dict(u="gu_prev", pred_x="gpred_x_prev", pred_u="gpred_u_prev")
    want, wmode = _forward_device(torch, kind, lay, veh, t, d, mode, N)
    assert torch.equal(tmode, wmode) and all(torch.equal(o, w) for o, w in zip(diff, want))
    assert not tmode.requires_grad
    tc = [_dev(torch, c) for c in ks.kin_cotangents(rng, B, N, kind)]
    sum((o * c).sum() for o, c in zip(diff, tc)).backward()
    g = _vjp_device(kind, lay, veh, t, tmode, tc)
    names = _names(kind)
    assert torch.equal(ins["sol"].grad, g.gsol) and torch.equal(ins["x"].grad, getattr(g, names[4]))
    for k, w in (("Ad", g.gAd0), ("Bd", g.gBd0), ("gd", g.ggd0)):
        assert torch.equal(ins[k].grad[:, 0], w) and not ins[k].grad[:, 1:].any()
    for k, name in prev.items():
        gk = ins[k].grad.cpu().numpy()
        assert torch.equal(ins[k].grad, getattr(g, name)) and gk[mode == 1].all() and not gk[mode != 1].any()
    # only the last cotangent is there, only sol requires a gradient
    sol = t["sol"].clone().requires_grad_(True)
    if kind == "incr":
        out = tm.kin_shift(lay, veh, sol, t["Ad"], t["Bd"], t["gd"], Xr, t["x"], t["pred"], t["pdu"], cnt, done)[2]
    else:
        out = tm.kin_ltv_shift(lay, veh, sol, status, t["Ad"], t["Bd"], t["gd"], t["x"], t["u"], t["pred_x"],
                               t["pred_u"])[3]
    (g1,) = torch.autograd.grad((out * tc[-1]).sum(), [sol])
    only = _vjp_device(kind, lay, veh, t, tmode, [None] * (len(tc) - 1) + [tc[-1]], want=["gsol"])
    assert torch.equal(g1, only.gsol)


def test_stop_rule_makes_mode_two(torch):
    """One torch_mpc.kin_shift call with finish_cnt = 15 on a vehicle within 0.5 of Xr[:, 0]: the stop rule
    fires, mode is 2, and the backward is the host statement's within the kernel's bar."""
    from osqp_amd import torch_mpc as tm
    veh, N, B = _veh(), 3, 4
    lay, _ = _mpc_layout("incr", N)
    rng = np.random.default_rng(94)
    d = ks.kin_case(rng, B, N, "incr")
    t = _tail_device_inputs(torch, rng, d, B, N)
    Xr = np.zeros((B, 4, N + 1))
    Xr[:, 0, 0], Xr[:, 1, 0] = d["x"][:, 0] + [0.3, 0.3, 0.3, 0.6], d["x"][:, 1] + [0.0, 0.39, 0.0, 0.0]
    cnt, done = _idev(torch, [15, 15, 14, 15]), _idev(torch, [0, 0, 0, 0])
    ins = {k: t[k].clone().requires_grad_(True) for k in ("sol", "x")}
    xt1, pred1, pdu1, cnt1, done1, mode = tm.kin_shift(lay, veh, ins["sol"], t["Ad"], t["Bd"], t["gd"], _dev(torch, Xr),
                                                       ins["x"], t["pred"], t["pdu"], cnt, done)
    assert mode.tolist() == [2, 2, 0, 0] and done1.tolist() == [1, 1, 0, 0] and cnt1.tolist() == [16, 16, 15, 15]
    hx, hp, hd = ks.forward("incr", N, d, np.array(mode.tolist()))
    assert np.array_equal(xt1.detach().cpu().numpy()[:2], d["x"][:2])
    assert np.array_equal(pred1.detach().cpu().numpy()[:2], hp[:2]) and np.array_equal(pdu1.detach().cpu().numpy(), hd)
    cots = ks.kin_cotangents(rng, B, N, "incr")
    sum((o * _dev(torch, c)).sum() for o, c in zip((xt1, pred1, pdu1), cots)).backward()
    host = ks.vjp("incr", N, d, cots, np.array(mode.tolist()))
    gsol, gx = ins["sol"].grad.cpu().numpy(), ins["x"].grad.cpu().numpy()
    assert _bits(gsol[:2], host[0][:2]) and _bits(gx[:2], cots[0][:2])       # mode 2 is copies and one addition
    dev = max(_rel(gsol, host[0]), _rel(gx, host[4]))
    print(f"measured stop rule: backward against the host statement {dev:.3e}, bar {BAR_KIN_SHIFT:.1e}")
    assert dev < BAR_KIN_SHIFT


# ------------------------------------------------------------------ forward: the closed loops --
@pytest.mark.parametrize("warm", [False, True])
def test_kinematic_rollout_forward_is_kinematic_mpc(torch, golden, warm):
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import KinematicMPC
    g = golden("kin_sim_n40.npz")
    N, B, T = 3, 3, 3
    x0 = g["x0"][None] + np.array([[0.0] * 4, [0.3, -0.2, -0.5, 0.02], [-0.2, 0.4, 1.0, -0.03]])
    u0 = np.tile([0.0, 0.01], (B, 1))
    ref = KinematicMPC(x0, u0, g["path_x"], g["path_y"], g["path_yaw"], N=N, warm_start=warm)
    torch.cuda.synchronize()
    xt0, pred0 = ref.xt.clone(), ref.pred.clone()
    roll = tm.KinematicRollout(ref.layout, B, ref.veh, warm_start=warm, polish=False)
    XT, DU0, pred_T = roll(xt0, pred0, T, path=(ref.path_x, ref.path_y, ref.path_yaw))
    assert XT.shape == (B, T + 1, 6) and DU0.shape == (B, T, 2) and pred_T.shape == (B, N + 1, 6)
    assert torch.equal(XT[:, 0], xt0)
    for t in range(T):
        status, iters = ref.step()
        torch.cuda.synchronize()
        assert torch.equal(XT[:, t + 1], ref.xt), f"step {t + 1}"
        assert torch.equal(roll.status[t], status) and torch.equal(roll.iters[t], iters)
        assert torch.equal(DU0[:, t], ref.sol[:, (N + 1) * 6:(N + 1) * 6 + 2])
        assert torch.equal(roll.done[t], ref.done)
    assert torch.equal(pred_T, ref.pred) and not roll.mode.any()
    assert roll.tape_doubles_per_instance() == 6 + (N + 1) * 6 + ref.layout.n + roll.batch.record_width
    print(f"kinematic rollout forward warm={warm}: iterations {roll.iters.tolist()}")


@pytest.mark.parametrize("warm", [False, True])
def test_ltv_rollout_forward_is_kinematic_ltv_mpc(torch, golden, warm):
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import KinematicLTVMPC
    g = golden("kinltv_sim_n3.npz")
    N, B, T = 3, 3, 3
    x0 = g["x0"][None] + np.array([[0.0] * 4, [0.3, -0.2, -0.5, 0.02], [-0.2, 0.4, 1.0, -0.03]])
    u0 = np.tile(g["u0"], (B, 1))
    ref = KinematicLTVMPC(x0, u0, g["path_x"], g["path_y"], N=N, shift_warm=warm)
    torch.cuda.synchronize()
    start = [v.clone() for v in (ref.x, ref.u, ref.pred_x, ref.pred_u)]
    roll = tm.KinematicLTVRollout(ref.layout, B, ref.veh, warm_start=warm, polish=False)
    X, U, px_T, pu_T = roll(*start, T, path=(ref.path_x, ref.path_y))
    assert X.shape == (B, T + 1, 4) and U.shape == (B, T + 1, 2)
    assert torch.equal(X[:, 0], start[0]) and torch.equal(U[:, 0], start[1])
    for t in range(T):
        status, iters = ref.step()
        torch.cuda.synchronize()
        assert torch.equal(X[:, t + 1], ref.x) and torch.equal(U[:, t + 1], ref.u), f"step {t + 1}"
        assert torch.equal(roll.status[t], status) and torch.equal(roll.iters[t], iters)
        assert torch.equal(U[:, t + 1], ref.sol[:, (N + 1) * 4:(N + 1) * 4 + 2])
    assert torch.equal(px_T, ref.pred_x) and torch.equal(pu_T, ref.pred_u)
    assert (roll.status == 1).all() and not roll.mode.any() and not ref.skipped.any()
    print(f"ltv rollout forward warm={warm}: iterations {roll.iters.tolist()}")


# ------------------------------------------------------------------ the skipped vehicle --
def _ltv_leaves(torch, x0s, u0, N):
    Bn = len(x0s)
    x0 = _dev(torch, x0s).requires_grad_(True)
    tu = _dev(torch, np.tile(u0, (Bn, 1))).requires_grad_(True)
    px = _dev(torch, np.tile(x0s[:, None, :], (1, N + 1, 1))).requires_grad_(True)
    pu = _dev(torch, np.tile(u0, (Bn, N + 1, 1))).requires_grad_(True)
    return [x0, tu, px, pu]


def test_ltv_rollout_passes_a_skipped_vehicle_through(torch):
    """B = 3 with the primal infeasible instance of tests/test_kin_rollout_ref.py in the middle: its
    state and horizon stay bit for bit, its gradients are identities, strict=True does not raise, and
    the other two instances' gradients are those of a B = 2 rollout without it, bit for bit."""
    from osqp_amd import torch_mpc as tm
    N, T, veh = 3, 3, _veh()
    lay, Qw = _mpc_layout("ltv", N)
    x0s = np.stack([cpu.X0_LTV, loop.X0_INFEASIBLE, cpu.X0_LTV + 1e-2 * PERT[1]])
    refs = loop.kin_loop_references(N, T)
    rng = np.random.default_rng(95)
    cots = [rng.standard_normal(s) for s in ((3, T + 1, 4), (3, T + 1, 2), (3, N + 1, 4), (3, N + 1, 2))]

    def run(keep):
        Bn = len(keep)
        roll = tm.KinematicLTVRollout(lay, Bn, veh, **SETTINGS["ltv"])
        leaves = _ltv_leaves(torch, x0s[keep], cpu.U0_LTV, N)
        qdiag = _dev(torch, np.diag(Qw)).requires_grad_(True)
        Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
        outs = roll(*leaves, T, Xr=Xr, weights=(torch.diag(qdiag), None, None))
        sum((o * _dev(torch, c[keep])).sum() for o, c in zip(outs, cots)).backward()
        torch.cuda.synchronize()
        return roll, leaves, [o.detach().cpu().numpy() for o in outs], [v.grad.cpu().numpy() for v in leaves + [qdiag]]

    roll, leaves, outs, grads = run([0, 1, 2])
    assert roll.status[:, 1].tolist() == [-3] * T and (roll.status[:, [0, 2]] == 1).all()
    assert roll.mode[:, 1].tolist() == [1] * T and not roll.mode[:, [0, 2]].any()
    assert (roll.astat[:, [0, 2]] == 1).all()
    X, U, px, pu = outs
    start = [v.detach().cpu().numpy() for v in leaves]
    assert all(_bits(X[1, t], start[0][1]) and _bits(U[1, t], start[1][1]) for t in range(T + 1))
    assert _bits(px[1], start[2][1]) and _bits(pu[1], start[3][1])
    # identities: d x_T / d x0 = I and so on through the pass-through; every X[1, t] and U[1, t] is x0[1], u0[1]
    for got, c in ((grads[0][1], cots[0][1]), (grads[1][1], cots[1][1])):
        acc = c[T]
        for t in reversed(range(T)):                              # the backward's own order of accumulation
            acc = acc + c[t]
        assert _bits(got, acc)
    assert _bits(grads[2][1], cots[2][1]) and _bits(grads[3][1], cots[3][1])
    (gX,) = torch.autograd.grad(roll(*leaves, T, Xr=torch.stack([_dev(torch, np.tile(r, (3, 1, 1))) for r in refs]))[0]
                                [1, T, 2], [leaves[0]])
    assert gX.cpu().numpy().tolist() == [[0.0] * 4, [0.0, 0.0, 1.0, 0.0], [0.0] * 4]
    # the other two against the rollout without it
    roll2, _, outs2, grads2 = run([0, 2])
    assert all(_bits(a[[0, 2]], b) for a, b in zip(outs, outs2))
    for a, b, k in zip(grads[:4], grads2[:4], ("x0", "u0", "pred_x0", "pred_u0")):
        assert _bits(a[[0, 2]], b), k
    assert _bits(grads[4], grads2[4]) and grads[4].all()


# ------------------------------------------------------------------ backward: the layer chain --
def _chain_case(case):
    kind, x0b, u0, j, scale = CASES[case]
    return kind, x0b + scale * PERT, u0, j


def _start(torch, kind, tx, u0, N):
    """The loop's start from the leaf tx: the state, and the horizon = the start on every stage."""
    Bn = tx.shape[0]
    tu = _dev(torch, np.tile(u0, (Bn, 1)))
    if kind == "incr":
        xt = torch.cat([tx, tu], dim=1)
        return (xt,), (xt[:, None, :].expand(Bn, N + 1, 6),)
    return (tx, tu), (tx[:, None, :].expand(Bn, N + 1, 4), tu[:, None, :].expand(Bn, N + 1, 2))


def _chain_two_steps(torch, tm, veh, layer, kind, tx, u0, Xr1, Xr2, j, qdiag):
    """Two steps through one recording MPCLayer with the torch tail between them; step 2's first control
    [j] per instance."""
    lay = layer.layout
    Bn, N = tx.shape[0], lay.N
    weights = (torch.diag(qdiag), None, None)
    state, hor = _start(torch, kind, tx, u0, N)
    for step, Xr in enumerate((Xr1, Xr2)):
        if kind == "incr":
            xs, us = hor[0][:, :N, :4], hor[0][:, :N, 4:]
        else:
            xs, us = hor[0][:, :N], hor[1][:, :N]
        Ad, Bd, gd = tm.linearise_kinematics(veh, xs, us)
        X, U, _ = layer(Ad, Bd, gd, state[0], Xr, weights=weights)
        if step == 1:
            return U[:, 0, j]
        sol = torch.cat([X.reshape(Bn, -1), U.reshape(Bn, -1)], dim=1)
        if kind == "incr":
            pdu = torch.zeros((Bn, N + 1, 2), dtype=torch.float64, device=tx.device)
            xt, pred, _, _, _, mode = tm.kin_shift(lay, veh, sol, Ad, Bd, gd, Xr, state[0], hor[0], pdu)
            state, hor = (xt,), (pred,)
        else:
            x, u, px, pu, mode = tm.kin_ltv_shift(lay, veh, sol, None, Ad, Bd, gd, *state, *hor)
            state, hor = (x, u), (px, pu)
        assert not mode.any()


def _rollout_two_grads(torch, roll, kind, pts, u0, refs, j, T, qdiag_np):
    """The T-th step's first control [j], d (instance 0's) / d x0 and d (the batch's sum) / d diag Q."""
    Bn, N = len(pts), roll.N
    tx = _dev(torch, pts).requires_grad_(True)
    qdiag = _dev(torch, qdiag_np).requires_grad_(True)
    Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
    state, hor = _start(torch, kind, tx, u0, N)
    outs = roll(*state, *hor, T, Xr=Xr, weights=(torch.diag(qdiag), None, None))
    out = outs[1][:, T - 1, j] if kind == "incr" else outs[1][:, T, j]
    (gx,) = torch.autograd.grad(out[0], [tx], retain_graph=True)
    (gq,) = torch.autograd.grad(out.sum(), [qdiag])
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), gx.cpu().numpy(), gq.cpu().numpy()


def _rollout_class(tm, kind):
    return tm.KinematicRollout if kind == "incr" else tm.KinematicLTVRollout


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_backward_matches_the_layer_chain(torch, case):
    """T = 2 against a chain of two steps through MPCLayer(record=True) with torch_mpc.kin_shift /
    kin_ltv_shift between them: the same kernels in the same order, so step 2's control is equal bit for
    bit; the gradients differ by the order of the weight sums.  Measured on the MI355X: BAR_KIN_ROLL's
    comment."""
    from osqp_amd import torch_mpc as tm
    kind, pts, u0, j = _chain_case(case)
    veh, N, Bn = _veh(), N_CHAIN, len(pts)
    lay, Qw = _mpc_layout(kind, N)
    refs = loop.kin_loop_references(N, 2)
    layer = tm.MPCLayer(lay, Bn, record=True, **SETTINGS[kind])
    tx = _dev(torch, pts).requires_grad_(True)
    qdiag = _dev(torch, np.diag(Qw)).requires_grad_(True)
    Xr1, Xr2 = (_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs)
    out = _chain_two_steps(torch, tm, veh, layer, kind, tx, u0, Xr1, Xr2, j, qdiag)
    (cgx,) = torch.autograd.grad(out[0], [tx], retain_graph=True)
    (cgq,) = torch.autograd.grad(out.sum(), [qdiag])
    torch.cuda.synchronize()
    assert (layer.status == 1).all() and (layer.astat == 1).all()
    cval, cgx, cgq = out.detach().cpu().numpy(), cgx.cpu().numpy(), cgq.cpu().numpy()
    roll = _rollout_class(tm, kind)(lay, Bn, veh, **SETTINGS[kind])
    val, gx, gq = _rollout_two_grads(torch, roll, kind, pts, u0, refs, j, 2, np.diag(Qw))
    assert (roll.status == 1).all() and (roll.astat == 1).all() and not roll.mode.any()
    assert roll.act.shape == (2, Bn, lay.m) and roll.ares.shape == (2, Bn)
    assert _bits(val, cval), "step 2's control differs from the chain's"
    assert not gx[1:].any() and gx[0].any() and gq.any()            # the instances are independent
    dx, dq = _rel(gx[0], cgx[0]), _rel(gq, cgq)
    print(f"measured kin rollout {case}: d control / d x0 {dx:.3e} (rollout {gx[0]} chain {cgx[0]}), "
          f"d loss / d diag Q {dq:.3e} (rollout {gq} chain {cgq}), bar {BAR_KIN_ROLL:.1e}")
    assert dx < BAR_KIN_ROLL and dq < BAR_KIN_ROLL


# ------------------------------------------------------------------ backward: central differences --
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("case", list(loop.LOOP_CASES))
def test_rollout_three_steps_match_central_differences(torch, case, N):
    """T = 3 on the points of tests/test_kin_rollout_ref.py (the row classes stay equal over the nine
    points for three steps): d (step 3's first control [j]) / d x0 against central differences with
    h = 1e-3, the perturbed copies in the same batch.  Measured on the MI355X, of the largest derivative:
    incr interior 1.18e-6 (N 2) and 3.53e-6 (N 3), incr active 3.9e-9 and 8.0e-9, ltv 2.1e-8 and 4.1e-8."""
    from osqp_amd import torch_mpc as tm
    kind, x0b, u0, active = loop.LOOP_CASES[case]
    j = 1 if active else 0
    veh, T, h = _veh(), loop.T_LOOP, loop.H_LOOP
    lay, Qw = _mpc_layout(kind, N)
    pts = loop.kin_loop_points(x0b, h)
    roll = _rollout_class(tm, kind)(lay, len(pts), veh, **SETTINGS[kind])
    val, gx, _ = _rollout_two_grads(torch, roll, kind, pts, u0, loop.kin_loop_references(N, T), j, T, np.diag(Qw))
    assert (roll.status == 1).all() and (roll.astat == 1).all() and not roll.mode.any()
    act = roll.act.cpu().numpy()
    assert (act == act[:, :1]).all(), "the row classes change within the step"
    assert ((act == 1) | (act == 2)).any() == active
    fd = (val[1::2] - val[2::2]) / (2 * h)
    dev = np.abs(fd - gx[0]).max() / np.abs(fd).max()
    print(f"measured kin rollout T=3 {case} N={N}: d control[{j}](step 3) / d x0: fd {fd} backward {gx[0]} "
          f"deviation {dev:.2e}")
    assert dev < BAR_LOOP


# ------------------------------------------------------------------ two rollouts alive --
@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_two_rollouts_alive_at_once(torch, kind):
    from osqp_amd import torch_mpc as tm
    veh, N = _veh(), N_CHAIN
    lay, Qw = _mpc_layout(kind, N)
    cases = [_chain_case(c)[1:] for c in CASES if CASES[c][0] == kind]
    if len(cases) == 1:                                      # the LTV layout has one point: move it
        pts, u0, j = cases[0]
        cases.append((pts + np.array([0.05, -0.02, 0.3, 0.01]), u0, j))
    roll = _rollout_class(tm, kind)(lay, len(cases[0][0]), veh, **SETTINGS[kind])
    refs = loop.kin_loop_references(N, 2)
    alone = [_rollout_two_grads(torch, roll, kind, pts, u0, refs, j, 2, np.diag(Qw)) for pts, u0, j in cases]
    assert not _bits(alone[0][1], alone[1][1])
    # both forwards, then both backwards, the first rollout's last
    live = []
    for pts, u0, j in cases:
        Bn = len(pts)
        tx = _dev(torch, pts).requires_grad_(True)
        qdiag = _dev(torch, np.diag(Qw)).requires_grad_(True)
        Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
        state, hor = _start(torch, kind, tx, u0, N)
        outs = roll(*state, *hor, 2, Xr=Xr, weights=(torch.diag(qdiag), None, None))
        live.append((outs[1][:, 1, j] if kind == "incr" else outs[1][:, 2, j], tx, qdiag))
    for k in (1, 0):
        out, tx, qdiag = live[k]
        (gx,) = torch.autograd.grad(out[0], [tx], retain_graph=True)
        (gq,) = torch.autograd.grad(out.sum(), [qdiag])
        torch.cuda.synchronize()
        assert _bits(out.detach().cpu().numpy(), alone[k][0])
        assert _bits(gx.cpu().numpy(), alone[k][1]) and _bits(gq.cpu().numpy(), alone[k][2]), f"rollout {k}"
