"""Gradients with respect to the vehicle parameters on the device (include/mpcqp.h):
the four *_pvjp kernels against their numpy statements (osqp_amd.mpc), a fleet of copies against
B = 1 calls, torch_mpc.fleet's backward against the mpc_device calls chained through constants_vjp,
and d loss / d params of the three rollouts against central differences with the perturbed cars in
the same batch.

Bars.  BAR_KERNEL: ten times the largest deviation measured on the MI355X, max |a - b| / max |b| per
array (the project's rule); the figures are in its comment.  BAR_LOOP is
tests/test_dyn_vjp_device.py's 1e-4 rule, here on the scaled gradient p dL/dp with a relative step
h = 1e-3 (1e-8 / h * 10).  Copies, zeros, masks and repeats are held bit for bit.
"""
import numpy as np
import pytest

import fleet_cases as fc
import test_dyn_vjp_ref as dyn
import test_kin_rollout_ref as kloop
import test_kin_shift_vjp_ref as ks
import test_rollout_ref as loop
import test_shift_vjp_ref as shift
from osqp_amd import mpc
from test_dyn_vjp_device import BAR_LOOP, POINTS, _layout, _points
from test_kin_rollout_device import SETTINGS as KIN_SETTINGS
from test_kin_rollout_device import _idev, _stop_rule_inputs, _tail_device_inputs
from test_mpc_vjp_device import Arena, _bits, _dev, _mpc_layout, _rel
from test_rollout_device import SETTINGS as DYN_SETTINGS
from test_rollout_device import _shift_device_inputs

pytestmark = pytest.mark.gpu

# measured on the first device run (MI355X), the largest over every case of this file's kernel tests
# (max |a - b| / max |b| per array): linearise_pvjp 1.28e-15 (B 3, N 2, three cars, without gBd),
# kin_linearise_pvjp 1.54e-15 (B 3, N 50, three cars, without ggd), euler_step_pvjp 2.2e-16,
# kin_update_pvjp 4.7e-16: §17's 1.4e-15, the stage sum running in the statement's own order
BAR_KERNEL = 1.6e-14
H_REL = 1e-3
FIELDS = ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------ fleets of the tests --
def _cars(B, which):
    """B car names: the three cars in turn, or B copies of the small one."""
    return [fc.ORDER[b % 3] if which == "cars" else "small" for b in range(B)]


def _dyn_fleet(md, names):
    return md.Fleet([md.Vehicle(dt=fc.DT_DYN, **fc.CARS[c]) for c in names])


def _kin_fleet(md, names):
    return md.KinFleet([md.KinVehicle(*fc.wheelbase(c)) for c in names])


def _per_car(names, statement, lead, *batched, **kw):
    """A single-vehicle host statement over the batch, one call per distinct car; lead(car): the
    statement's leading arguments."""
    out = None
    for car in sorted(set(names)):
        idx = np.array([n == car for n in names])
        part = statement(*lead(car), *(None if a is None else a[idx] for a in batched), **kw)
        if out is None:
            out = np.zeros((len(names),) + part.shape[1:])
        out[idx] = part
    return out


DYN = dict(nx=6, nk=13, lead=lambda car: (fc.params(car),), fleet=_dyn_fleet, lin=mpc.linearise_dynamics_pvjp,
           step=mpc.euler_step_pvjp, dev_lin="linearise_pvjp", dev_step="euler_step_pvjp")
KIN = dict(nx=4, nk=3, lead=fc.wheelbase, fleet=_kin_fleet, lin=mpc.linearise_kinematics_pvjp,
           step=mpc.kin_update_pvjp, dev_lin="kin_linearise_pvjp", dev_step="kin_update_pvjp")
MODELS = dict(dyn=DYN, kin=KIN)


def _lin_points(rng, model, B, N):
    """(B, N) points, every fourth in the low-speed guard (the dynamic model's), and cotangents."""
    if model == "dyn":
        x, u = _points(rng, B, N)
    else:
        x = rng.standard_normal((B, N, 4)) * [3.0, 3.0, 5.0, 1.5] + [0.0, 0.0, 10.0, 0.0]
        u = rng.standard_normal((B, N, 2)) * [0.15, 1.0]
    nx = MODELS[model]["nx"]
    return x, u, [rng.standard_normal((B, N, nx, nx)), rng.standard_normal((B, N, nx, 2)),
                  rng.standard_normal((B, N, nx))]


# ------------------------------------------------------------------ the linearisations' kernels --
@pytest.mark.parametrize("which", ["cars", "copies"])
@pytest.mark.parametrize("N", [2, 3, 50])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("model", ["dyn", "kin"])
def test_linearise_pvjp_matches_the_host_statement(torch, model, B, N, which):
    from osqp_amd import mpc_device as md
    M = MODELS[model]
    fn, nk = getattr(md, M["dev_lin"]), M["nk"]
    rng = np.random.default_rng(500 + 7 * B + N)
    names = _cars(B, which)
    fleet = M["fleet"](md, names)
    x, u, cots = _lin_points(rng, model, B, N)
    want = _per_car(names, M["lin"], M["lead"], x, u, *cots)
    tx, tu, tc = _dev(torch, x), _dev(torch, u), [_dev(torch, c) for c in cots]
    a1, a2 = Arena(torch, dict(gK=(B, nk))), Arena(torch, dict(gK=(B, nk)))
    fn(fleet, tx, tu, *tc, out=a1.view["gK"])
    fn(fleet, tx, tu, *tc, out=a2.view["gK"])
    torch.cuda.synchronize()
    assert a1.guards_intact() and a2.guards_intact()
    gK = a1.view["gK"].cpu().numpy()
    assert np.isfinite(gK).all() and gK.any()
    assert _bits(a2.view["gK"].cpu().numpy(), gK), "a repeated call returns other bits"
    assert np.array_equal(gK == 0, want == 0), "the zero pattern differs from the statement's"
    worst = _rel(gK, want)
    print(f"measured {M['dev_lin']} B={B} N={N} {which}: {worst:.3e}")
    # each cotangent None in turn: the host statement's, and a zero tensor's bit for bit
    for k in range(3):
        some = [c if i != k else None for i, c in enumerate(tc)]
        zero = [c if i != k else torch.zeros_like(c) for i, c in enumerate(tc)]
        s, z = fn(fleet, tx, tu, *some), fn(fleet, tx, tu, *zero)
        e = _per_car(names, M["lin"], M["lead"], x, u, *[c if i != k else None for i, c in enumerate(cots)])
        torch.cuda.synchronize()
        assert _bits(s.cpu().numpy(), z.cpu().numpy())
        d = _rel(s.cpu().numpy(), e)
        print(f"measured {M['dev_lin']} B={B} N={N} {which} without cotangent {k}: {d:.3e}")
        worst = max(worst, d)
    assert not fn(fleet, tx, tu, None, None, None).any()
    # one (x, u) for every stage (stage stride 0)
    a3 = Arena(torch, dict(gK=(B, nk)))
    fn(fleet, tx[:, :1].expand(B, N, M["nx"]), tu[:, :1].expand(B, N, 2), *tc, out=a3.view["gK"])
    torch.cuda.synchronize()
    e = _per_car(names, M["lin"], M["lead"], np.repeat(x[:, :1], N, 1), np.repeat(u[:, :1], N, 1), *cots)
    d = _rel(a3.view["gK"].cpu().numpy(), e)
    print(f"measured {M['dev_lin']} B={B} N={N} {which} stage stride 0: {d:.3e}")
    worst = max(worst, d)
    assert a3.guards_intact()
    # a fleet of copies: row b is a B = 1 call's, bit for bit
    if which == "copies":
        one = M["fleet"](md, names[:1])
        for b in sorted({0, B // 2, B - 1}):
            g1 = fn(one, tx[b:b + 1], tu[b:b + 1], *[c[b:b + 1].contiguous() for c in tc])
            assert _bits(g1.cpu().numpy()[0], gK[b]), b
    print(f"measured {M['dev_lin']} B={B} N={N} {which}: worst {worst:.3e}, bar {BAR_KERNEL:.1e}")
    assert worst < BAR_KERNEL


# ------------------------------------------------------------------ the terminal steps' kernels --
@pytest.mark.parametrize("which", ["cars", "copies"])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("model", ["dyn", "kin"])
def test_terminal_step_pvjp_matches_the_host_statement(torch, model, B, which):
    from osqp_amd import mpc_device as md
    M = MODELS[model]
    fn, nk, nx = getattr(md, M["dev_step"]), M["nk"], M["nx"]
    rng = np.random.default_rng(900 + B)
    names = _cars(B, which)
    fleet = M["fleet"](md, names)
    x, u, _ = _lin_points(rng, model, B, 1)
    x, u, w = x[:, 0], u[:, 0], rng.standard_normal((B, nx))
    mode = (np.arange(B) % 3 == 1).astype(np.int32) * (1 + (np.arange(B) % 2))      # 0, 1 or 2
    # the point as views into one wider buffer, as the tails' solutions are
    buf = _dev(torch, rng.standard_normal((B, nx + 9)))
    buf[:, 2:2 + nx], buf[:, 5 + nx:7 + nx] = _dev(torch, x), _dev(torch, u)
    vx, vu, tw, tmode = buf[:, 2:2 + nx], buf[:, 5 + nx:7 + nx], _dev(torch, w), _idev(torch, mode)
    a1, a2 = Arena(torch, dict(gK=(B, nk))), Arena(torch, dict(gK=(B, nk)))
    fn(fleet, vx, vu, tw, out=a1.view["gK"])
    fn(fleet, vx, vu, tw, out=a2.view["gK"])
    masked = fn(fleet, vx, vu, tw, tmode)
    torch.cuda.synchronize()
    assert a1.guards_intact() and a2.guards_intact()
    gK, masked = a1.view["gK"].cpu().numpy(), masked.cpu().numpy()
    want = _per_car(names, M["step"], M["lead"], x, u, w)
    assert _bits(a2.view["gK"].cpu().numpy(), gK), "a repeated call returns other bits"
    assert np.array_equal(gK == 0, want == 0), "the zero pattern differs from the statement's"
    if model == "dyn":   # vx in (0, 0.5): the tyres carry no force, nothing reaches l_f, l_r, Iz or the tyre constants
        slow = (x[:, 3] > 0) & (x[:, 3] < 0.5)
        assert not gK[slow][:, [1, 2, 3, 7, 8, 9, 10, 11, 12]].any() and gK[slow][:, [0, 4, 5, 6]].all()
    assert _bits(masked[mode == 0], gK[mode == 0]) and not masked[mode != 0].any()
    assert np.array_equal(masked == 0, _per_car(names, M["step"], M["lead"], x, u, w, mode) == 0)
    assert not fn(fleet, vx, vu, None).any()
    if which == "copies":
        one = M["fleet"](md, names[:1])
        for b in sorted({0, B // 2, B - 1}):
            g1 = fn(one, vx[b:b + 1], vu[b:b + 1], tw[b:b + 1])
            assert _bits(g1.cpu().numpy()[0], gK[b]), b
    d = _rel(gK, want)
    print(f"measured {M['dev_step']} B={B} {which}: {d:.3e}, bar {BAR_KERNEL:.1e}")
    assert d < BAR_KERNEL


def test_wrappers_refuse_bad_inputs(torch):
    from osqp_amd import mpc_device as md
    f = _dyn_fleet(md, _cars(2, "cars"))
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    x, u = z(2, 3, 6), z(2, 3, 2)
    with pytest.raises(TypeError, match="fleet form only"):
        md.linearise_pvjp(md.Vehicle(), x, u, None, None, None)
    with pytest.raises(TypeError):
        md.kin_linearise_pvjp(f, z(2, 3, 4), u, None, None, None)
    with pytest.raises(ValueError, match="fleet of 2"):
        md.linearise_pvjp(f, z(3, 3, 6), z(3, 3, 2), None, None, None)
    with pytest.raises(ValueError):
        md.linearise_pvjp(f, x.float(), u, None, None, None)
    with pytest.raises(ValueError):
        md.linearise_pvjp(f, x, u, z(2, 3, 6, 2), None, None)
    with pytest.raises(ValueError):
        md.linearise_pvjp(f, x, u, None, None, None, out=z(2, 9))
    with pytest.raises(Exception, match="N <= 256"):
        md.linearise_pvjp(f, z(2, 257, 6), z(2, 257, 2), None, None, None)
    with pytest.raises(ValueError):
        md.euler_step_pvjp(f, z(2, 4), z(2, 2), None)
    with pytest.raises(ValueError):
        md.euler_step_pvjp(f, z(2, 6), z(2, 2), z(2, 4))
    with pytest.raises(ValueError):
        md.euler_step_pvjp(f, z(2, 6), z(2, 2), None, mode=torch.zeros(2, dtype=torch.int64, device="cuda:0"))


# ------------------------------------------------------------------ torch_mpc.fleet --
def _dyn_params(names):
    return np.array([[fc.CARS[c][k] for k in FIELDS] + [fc.DT_DYN] for c in names])


def _kin_params(names):
    return np.array([fc.wheelbase(c) for c in names])


@pytest.mark.parametrize("model", ["dyn", "kin"])
def test_torch_linearise_backward_is_the_pvjp_chained(torch, model):
    from osqp_amd import mpc_device as md, torch_mpc as tm
    M = MODELS[model]
    B, N = 5, 3
    rng = np.random.default_rng(71)
    names = _cars(B, "cars")
    x, u, cots = _lin_points(rng, model, B, N)
    p = _dev(torch, (_dyn_params if model == "dyn" else _kin_params)(names)).requires_grad_(True)
    pf = tm.fleet(p)
    table = M["fleet"](md, names)
    assert isinstance(pf.table, type(table)) and len(pf) == B and pf.dt == table.dt
    tx, tu, tc = _dev(torch, x).requires_grad_(True), _dev(torch, u), [_dev(torch, c) for c in cots]
    lin, fwd, vjp = ((tm.linearise_dynamics, md.linearise, md.linearise_vjp) if model == "dyn" else
                     (tm.linearise_kinematics, md.linearise_kinematics, md.linearise_kinematics_vjp))
    outs = lin(pf, tx, tu)
    for o, w in zip(outs, fwd(table, tx.detach(), tu)):
        assert torch.equal(o, w)
    sum((o * c).sum() for o, c in zip(outs, tc)).backward()
    gK = getattr(md, M["dev_lin"])(table, tx.detach(), tu, *tc)
    assert p.grad.shape == p.shape and p.grad.device == p.device
    assert _bits(p.grad.cpu().numpy(), table.constants_vjp(gK))
    assert torch.equal(tx.grad, vjp(table, tx.detach(), tu, *tc)[0])
    # a plain fleet or struct: the same outputs, and no params to ask a gradient for
    for o, w in zip(lin(table, tx.detach(), tu), outs):
        assert torch.equal(o, w)
    # only gd has a cotangent; params on the host get their gradient there
    ph = torch.tensor((_dyn_params if model == "dyn" else _kin_params)(names), requires_grad=True)
    (g1,) = torch.autograd.grad((lin(tm.fleet(ph), tx.detach(), tu)[2] * tc[2]).sum(), [ph])
    assert not g1.is_cuda and _bits(g1.numpy(), table.constants_vjp(
        getattr(md, M["dev_lin"])(table, tx.detach(), tu, None, None, tc[2])))
    with pytest.raises(ValueError):
        tm.fleet(p[:, :2])


def test_torch_incr_shift_backward_is_the_terminal_pvjp_chained(torch):
    from osqp_amd import mpc_device as md, torch_mpc as tm
    N, B = 3, 5
    lay = _layout(N)
    rng = np.random.default_rng(91)
    d = shift.shift_case(rng, B, N)
    t = _shift_device_inputs(torch, rng, d, B, N)
    names = _cars(B, "cars")
    p = _dev(torch, _dyn_params(names)).requires_grad_(True)
    pf, table = tm.fleet(p), _dyn_fleet(md, names)
    sol = t["sol"].clone().requires_grad_(True)
    outs = tm.incr_shift(lay, pf, sol, t["Ad"], t["Bd"], t["gd"], t["xt"])
    for o, w in zip(outs, md.incr_shift(lay, table, t["sol"], t["Ad"], t["Bd"], t["gd"], t["xt"])):
        assert torch.equal(o, w)
    tc = [_dev(torch, c) for c in shift.shift_cotangents(rng, B, N)]
    sum((o * c).sum() for o, c in zip(outs, tc)).backward()
    s = t["sol"]
    gK = md.euler_step_pvjp(table, s[:, N * 8:N * 8 + 6], s[:, (N - 1) * 8 + 6:N * 8], tc[1][:, N, :6].contiguous())
    assert gK.any() and _bits(p.grad.cpu().numpy(), table.constants_vjp(gK))
    assert torch.equal(sol.grad, md.incr_shift_vjp(lay, table, s, t["Ad"], t["Bd"], t["xt"], *tc, want=["gsol"]).gsol)
    # the statement at the same views
    want = _per_car(names, mpc.euler_step_pvjp, DYN["lead"], d["sol"][:, N * 8:N * 8 + 6],
                    d["sol"][:, (N - 1) * 8 + 6:N * 8], tc[1][:, N, :6].cpu().numpy())
    assert _rel(gK.cpu().numpy(), want) < BAR_KERNEL


@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_torch_kinematic_tails_backward_is_the_terminal_pvjp_chained(torch, kind):
    from osqp_amd import mpc_device as md, torch_mpc as tm
    N, B = 3, 9
    lay, _ = _mpc_layout(kind, N)
    rng = np.random.default_rng(93)
    d, mode = ks.kin_case(rng, B, N, kind), ks.kin_modes(B, kind)
    t = _tail_device_inputs(torch, rng, d, B, N)
    names = ["default"] * B   # the case's stop rule and status are drawn for ks.VEH, the default car
    p = _dev(torch, _kin_params(names)).requires_grad_(True)
    pf, table = tm.fleet(p), _kin_fleet(md, names)
    tc = [_dev(torch, c) for c in ks.kin_cotangents(rng, B, N, kind)]
    s = t["sol"]
    if kind == "incr":
        Xr, cnt, done = _stop_rule_inputs(torch, d, mode, N)
        outs = tm.kin_shift(lay, pf, s, t["Ad"], t["Bd"], t["gd"], Xr, t["x"], t["pred"], t["pdu"], cnt, done)
        diff, tmode = outs[:3], outs[5]
        xs, us, w = s[:, N * 6:N * 6 + 4], s[:, N * 6 + 4:N * 6 + 6], tc[1][:, N, :4].contiguous()
    else:
        status = _idev(torch, np.where(mode == 1, -3, 1))
        outs = tm.kin_ltv_shift(lay, pf, s, status, t["Ad"], t["Bd"], t["gd"], t["x"], t["u"], t["pred_x"],
                                t["pred_u"])
        diff, tmode = outs[:4], outs[4]
        o = (N + 1) * 4 + (N - 1) * 2
        xs, us, w = s[:, N * 4:N * 4 + 4], s[:, o:o + 2], tc[2][:, N].contiguous()
    assert np.array_equal(tmode.cpu().numpy(), mode)
    sum((o * c).sum() for o, c in zip(diff, tc)).backward()
    gK = md.kin_update_pvjp(table, xs, us, w, tmode)
    g = gK.cpu().numpy()
    assert g[mode == 0].any(1).all() and not g[mode != 0].any()
    assert _bits(p.grad.cpu().numpy(), g)                           # the kinematic chain is the identity


# ------------------------------------------------------------------ end to end --
def _perturbed(p0, args):
    """p0 and, per argument of `args`, p0 with it moved up and down by the relative step H_REL."""
    rows = [p0]
    for a in args:
        for s in (1.0, -1.0):
            q = p0.copy()
            q[a] *= 1.0 + s * H_REL
            rows.append(q)
    return np.array(rows)


def _against_differences(label, val, g, p0, args, must):
    """val (1 + 2 len(args),) the loss per car, g (9,) or (3,) the backward's row 0: the scaled
    measure over `args`, and the entries `must` well above the bar."""
    fd = (val[1::2] - val[2::2]) / (2 * H_REL)
    s = (g * p0)[list(args)]
    dev = np.abs(fd - s).max() / np.abs(s).max()
    print(f"measured {label}: scaled d loss / d params fd {fd} backward {s} deviation {dev:.2e}, bar {BAR_LOOP:.0e}")
    assert dev < BAR_LOOP
    for a in must:
        assert abs(g[a] * p0[a]) > 100 * BAR_LOOP * np.abs(s).max(), (a, g * p0)


# test_dyn_vjp_device's two points drive nearly straight (slip angles below 3e-3 rad), so the lateral
# tyre forces hardly act there; the third is the interior point cornering: vy 0.3 and r -0.1 load both
# axles (slip angles -0.018 rad front, -0.044 rad rear at vx 9.9), and its loss is the steer increment,
# the channel the lateral forces act on.  The tyre entries are asserted there.
LOOP_POINTS = {k: v[:2] for k, v in POINTS.items()}
LOOP_POINTS["cornering"] = (dyn.X0_INTERIOR + np.array([0.0, 0.0, 0.0, 0.0, 0.28, -0.11]), 0)
TYRE = (7, 9, 10, 12)   # B_f, D_f, B_r, D_r of the table's order (C_f, C_r are the number 1.30: no chain)


@pytest.mark.parametrize("point", list(LOOP_POINTS))
def test_dynamic_rollout_params_match_central_differences(torch, point):
    """T = 2, N = 3: d (step 2's du_0[j]) / d params of car 0 against the perturbed cars of the same
    batch.  dt is left out of the comparison: a fleet has one dt (mpcqp_fleet_create), so it cannot
    be moved per car; its kernels' dt entries are held to the statements above and those to the
    reference's differences (tests/test_param_grad_ref.py).

    A zero gradient cannot pass: m and l_f are above 100 bars of the row's largest at every point;
    a tyre constant lives in the table's coordinates, so its entry is measured by what it alone
    contributes to the compared row through the chain (zeroing it would move the row by that), and
    at the cornering point each of B_f, D_f, B_r, D_r contributes more than 100 bars."""
    from osqp_amd import torch_mpc as tm
    x0b, j = LOOP_POINTS[point]
    N, T, args = 3, 2, tuple(range(8))
    p0 = _dyn_params(["default"])[0]
    rows = _perturbed(p0, args)
    Bn = len(rows)
    p = _dev(torch, rows).requires_grad_(True)
    roll = tm.DynamicRollout(_layout(N), Bn, tm.fleet(p), **DYN_SETTINGS)
    xt0 = _dev(torch, np.tile(np.concatenate([x0b, dyn.U0]), (Bn, 1)))
    Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in loop.loop_references(N, T)])
    _, DU0, _ = roll(xt0, xt0[:, None, :].expand(Bn, N + 1, 8).contiguous(), T, Xr=Xr)
    out = DU0[:, T - 1, j]
    out[0].backward()
    torch.cuda.synchronize()
    assert (roll.status == 1).all() and (roll.astat == 1).all()
    act = roll.act.cpu().numpy()
    assert (act == act[:, :1]).all(), "the row classes change within the step"
    g = p.grad.cpu().numpy()
    assert not g[1:].any()                                        # the cars are independent
    _against_differences(f"DynamicRollout {point}", out.detach().cpu().numpy(), g[0], p0, args, must=(0, 1))
    gK = roll.gK.cpu().numpy()
    alone = np.zeros((len(TYRE),) + gK.shape)
    for i, c in enumerate(TYRE):
        alone[i, 0, c] = gK[0, c]
    foot = np.array([np.abs(roll.veh.constants_vjp(a)[0] * p0)[list(args)].max() for a in alone])
    foot /= np.abs(g[0] * p0)[list(args)].max()
    print(f"measured DynamicRollout {point}: B_f, D_f, B_r, D_r alone in the compared row {foot}")
    if point == "cornering":
        assert (foot > 100 * BAR_LOOP).all(), foot


@pytest.mark.parametrize("case,N", [("incr interior", 3), ("ltv", 2)])
def test_kinematic_rollouts_params_match_central_differences(torch, case, N):
    """KinematicRollout at T = 2, N = 3 and KinematicLTVRollout at T = 2, N = 2: d (step 2's first
    control [0]) / d (l_f, l_r) of car 0 against the perturbed cars of the same batch (dt: see the
    dynamic test)."""
    from osqp_amd import torch_mpc as tm
    kind, x0b, u0, _ = kloop.LOOP_CASES[case]
    T, args = 2, (0, 1)
    p0 = _kin_params(["default"])[0]
    rows = _perturbed(p0, args)
    Bn = len(rows)
    p = _dev(torch, rows).requires_grad_(True)
    lay, _ = _mpc_layout(kind, N)
    cls = tm.KinematicRollout if kind == "incr" else tm.KinematicLTVRollout
    roll = cls(lay, Bn, tm.fleet(p), **KIN_SETTINGS[kind])
    tx, tu = _dev(torch, np.tile(x0b, (Bn, 1))), _dev(torch, np.tile(u0, (Bn, 1)))
    Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in kloop.kin_loop_references(N, T)])
    if kind == "incr":
        xt = torch.cat([tx, tu], dim=1)
        outs = roll(xt, xt[:, None, :].expand(Bn, N + 1, 6).contiguous(), T, Xr=Xr)
        out = outs[1][:, T - 1, 0]
    else:
        outs = roll(tx, tu, tx[:, None, :].expand(Bn, N + 1, 4).contiguous(),
                    tu[:, None, :].expand(Bn, N + 1, 2).contiguous(), T, Xr=Xr)
        out = outs[1][:, T, 0]
    out[0].backward()
    torch.cuda.synchronize()
    assert (roll.status == 1).all() and (roll.astat == 1).all() and not roll.mode.any()
    act = roll.act.cpu().numpy()
    assert (act == act[:, :1]).all(), "the row classes change within the step"
    g = p.grad.cpu().numpy()
    assert not g[1:].any() and g[0, 0] == g[0, 1]                 # only the wheelbase enters
    _against_differences(f"{cls.__name__} N={N}", out.detach().cpu().numpy(), g[0], p0, args, must=(0, 1))
