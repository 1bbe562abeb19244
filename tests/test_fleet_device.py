"""A fleet of different vehicles in one batch (include/mpcqp.h), on the device.

Every `_fleet` entry point, through its Python function: the B-vehicle call with a fleet returns the
bits of the B uniform calls with veh[b] on vehicle b alone, stacked; a fleet of B copies of one car
returns the bits of the uniform B-vehicle call; a repeated call returns the same bits.  B = 3 (the cars
of tests/fleet_cases.py, the default not first) and B = 130 (a sweep of m and l_f that crosses a
128-thread block), N in {2, 3}.  The tails' inputs are those of tests/test_rollout_device.py and
tests/test_kin_rollout_device.py: modes 1 and 2 on every fourth / fifth vehicle, each cotangent NULL
and outputs left out.  The fleet linearisations against the reference's own outputs for the three cars
(tests/golden/make_golden_fleet.py) hold the constants the device derives to the reference for cars
other than the default.  The closed loops and the differentiable rollouts with the three-car fleet
against three B = 1 runs.  Everything is compared bit for bit but d loss / d diag Q of a rollout, whose
sum over the batch runs in another order: BAR_KIN_ROLL of tests/test_kin_rollout_device.py (1.6e-15).
"""
import numpy as np
import pytest

import fleet_cases as fc
import test_dyn_vjp_ref as dyn
import test_kin_rollout_ref as kloop
import test_kin_shift_vjp_ref as ks
import test_mpc_vjp_ref as cpu
import test_rollout_ref as loop
import test_shift_vjp_ref as shift
from osqp_amd import mpc
from test_dyn_vjp_device import _layout as _dyn_layout
from test_kin_rollout_device import BAR_KIN_ROLL, SETTINGS as KIN_SETTINGS, _stop_rule_inputs, _tail_device_inputs
from test_mpc_vjp_device import _dev, _mpc_layout, _rel
from test_rollout_device import SETTINGS as DYN_SETTINGS, _shift_device_inputs

pytestmark = pytest.mark.gpu
SHAPES = ["cars", "sweep"]                     # B = 3, B = 130
BAR = dict(rtol=1e-13, atol=1e-15)             # tests/test_mpc_device.py's, for linearise.npz
BAR_GD = dict(rtol=1e-12, atol=1e-13)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def md():
    from osqp_amd import mpc_device
    return mpc_device


def _sources(md, model, which):
    """(the B structs, their fleet, the fleet class) of a shape."""
    if model == "dyn":
        structs = fc.vehicles(md, which)
        return structs, md.Fleet(structs), md.Fleet
    structs = fc.kin_vehicles(md, which)
    return structs, md.KinFleet(structs), md.KinFleet


def _cut(t, sl):
    """The batch slice of a dict of tensors / lists of tensors / None / anything else."""
    def one(v):
        if isinstance(v, (list, tuple)):
            return [one(w) for w in v]
        return v[sl].contiguous() if hasattr(v, "shape") else v
    return {k: one(v) for k, v in t.items()}


def _same(torch, a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), i
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), f"output {i} differs"


def check_entry_point(torch, md, model, which, op, t, reads=True):
    """The three properties of the module docstring for op(veh, inputs) -> list of tensors.  reads: the
    outputs of vehicle 1 (which every mask of the tails leaves in mode 0) depend on its constants."""
    structs, fleet, cls = _sources(md, model, which)
    B = len(structs)
    got = op(fleet, t)
    again = op(fleet, t)
    torch.cuda.synchronize()
    assert all(g is None or bool(torch.isfinite(g.double()).all()) for g in got)
    _same(torch, got, again)                                                  # a repeat returns the same bits
    alone = [op(structs[b], _cut(t, slice(b, b + 1))) for b in range(B)]
    stacked = [None if alone[0][i] is None else torch.cat([a[i] for a in alone]) for i in range(len(got))]
    _same(torch, got, stacked)                                                # vehicle b uses entry b
    for b in {0, B - 1}:                                                      # B copies of one car: the uniform call
        _same(torch, op(cls([structs[b]] * B), t), op(structs[b], t))
    if reads:  # and the cars do differ: some output of vehicle 1 moves when its constants are vehicle 2's
        other = op(structs[2], _cut(t, slice(1, 2)))
        assert any(a is not None and not torch.equal(a, o) for a, o in zip(alone[1], other)), "the constants are not read"


# ------------------------------------------------------------------ the linearisations --
def _lin_points(torch, golden, name, B, N, nx):
    """B * N of the fixture's 48 points (the guard's among them), cycled, as (B, N, nx) / (B, N, 2)."""
    g = golden(name)
    idx = (np.arange(B * N) * 7) % 48
    return _dev(torch, g["x"][idx].reshape(B, N, nx)), _dev(torch, g["u"][idx].reshape(B, N, 2))


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("which", SHAPES)
@pytest.mark.parametrize("model", ["dyn", "kin"])
def test_linearise_fleet(torch, md, golden, model, which, N):
    nx, name, fwd, vjp = (6, "linearise.npz", md.linearise, md.linearise_vjp) if model == "dyn" else \
        (4, "kin_linearise.npz", md.linearise_kinematics, md.linearise_kinematics_vjp)
    B = 3 if which == "cars" else fc.B_SWEEP
    x, u = _lin_points(torch, golden, name, B, N, nx)
    rng = np.random.default_rng(300 + B + N)
    cots = [_dev(torch, rng.standard_normal(s)) for s in ((B, N, nx, nx), (B, N, nx, 2), (B, N, nx))]
    check_entry_point(torch, md, model, which, lambda veh, t: list(fwd(veh, t["x"], t["u"])), dict(x=x, u=u))
    # a stage stride of 0 (one point for every stage), as KinematicFrozenMPC linearises
    check_entry_point(torch, md, model, which,
                      lambda veh, t: list(fwd(veh, t["x"][:, :1].expand(-1, N, nx), t["u"][:, :1].expand(-1, N, 2))),
                      dict(x=x, u=u))
    for drop in (None, 0, 2):                                                 # each cotangent may be NULL
        given = [c if i != drop else None for i, c in enumerate(cots)]
        check_entry_point(torch, md, model, which, lambda veh, t: list(vjp(veh, t["x"], t["u"], *t["cots"])),
                          dict(x=x, u=u, cots=given), reads=drop is None)


@pytest.mark.parametrize("model", ["dyn", "kin"])
def test_fleet_linearisation_matches_the_reference(torch, md, golden, model):
    """The three cars in one call at the fixture's 48 points, within the bars linearise.npz is held to."""
    g = golden("linearise_fleet.npz" if model == "dyn" else "kin_linearise_fleet.npz")
    cars = list(g["cars"])
    order = [cars.index(c) for c in fc.ORDER]
    _, fleet, _ = _sources(md, model, "cars")
    nx = 6 if model == "dyn" else 4
    x = _dev(torch, np.tile(g["x"], (3, 1, 1)))
    u = _dev(torch, np.tile(g["u"], (3, 1, 1)))
    Ad, Bd, gd = ((md.linearise if model == "dyn" else md.linearise_kinematics)(fleet, x, u))
    assert Ad.shape == (3, 48, nx, nx)
    for got, name, bar in ((Ad, "Ad", BAR), (Bd, "Bd", BAR), (gd, "gd", BAR_GD)):
        want = g[name][order]
        worst = (np.abs(got.cpu().numpy() - want) / (bar["atol"] + bar["rtol"] * np.abs(want))).max()
        print(f"measured {model} fleet linearisation {name}: {worst:.3f} of the bar")
        assert np.allclose(got.cpu().numpy(), want, **bar), name
    assert not np.array_equal(g["Ad"][order[0]], g["Ad"][order[1]])


# ------------------------------------------------------------------ the tails --
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("which", SHAPES)
def test_incr_shift_fleet(torch, md, which, N):
    B, lay = (3 if which == "cars" else fc.B_SWEEP), _dyn_layout(N)
    rng = np.random.default_rng(310 + B + N)
    d, cots = shift.shift_case(rng, B, N), shift.shift_cotangents(rng, B, N)
    t = _shift_device_inputs(torch, rng, d, B, N)
    check_entry_point(torch, md, "dyn", which,
                      lambda veh, t: list(md.incr_shift(lay, veh, t["sol"], t["Ad"], t["Bd"], t["gd"], t["xt"])), t)
    tc = [_dev(torch, c) for c in cots]
    names = md.SHIFT_VJP_OUTPUTS

    def vjp(want):
        def op(veh, t):
            o = md.incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *t["cots"], want=want)
            return [getattr(o, k) for k in names]
        return op
    for drop, want in ((None, None), (0, None), (1, None), (2, None), (None, ["gsol"]), (None, list(names[1:]))):
        check_entry_point(torch, md, "dyn", which, vjp(want),
                          dict(t, cots=[c if i != drop else None for i, c in enumerate(tc)]),
                          reads=drop is None and want is None)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("which", SHAPES)
@pytest.mark.parametrize("kind", ["incr", "ltv"])
def test_kinematic_tails_fleet(torch, md, kind, which, N):
    """kin_shift / kin_ltv_shift with the masks produced by the loops' own rules (a mode-2 vehicle meets the
    stop rule on this step, a mode-1 vehicle was done / is not `solved`), and their VJPs."""
    B, (lay, _) = (3 if which == "cars" else fc.B_SWEEP), _mpc_layout(kind, N)
    rng = np.random.default_rng(320 + B + N)
    d, cots = ks.kin_case(rng, B, N, kind), ks.kin_cotangents(rng, B, N, kind)
    mode = ks.kin_modes(B, kind)
    t = _tail_device_inputs(torch, rng, d, B, N)
    tmode = _dev(torch, mode, torch.int32)
    if kind == "incr":
        Xr, cnt, done = _stop_rule_inputs(torch, d, mode, N)
        t.update(Xr=Xr, cnt=cnt, done=done)

        def fwd(veh, t):
            return list(md.kin_shift(lay, veh, t["sol"], t["Ad"], t["Bd"], t["gd"], t["Xr"], t["x"], t["pred"], t["pdu"],
                                     t["cnt"], t["done"]))
        assert np.array_equal(fwd(_sources(md, "kin", which)[1], t)[5].cpu().numpy(), mode)
    else:
        t.update(status=_dev(torch, np.where(mode == 1, -3, 1), torch.int32))

        def fwd(veh, t):
            return list(md.kin_ltv_shift(lay, veh, t["sol"], t["status"], t["Ad"], t["Bd"], t["gd"], t["x"], t["u"],
                                         t["pred_x"], t["pred_u"]))
    check_entry_point(torch, md, "kin", which, fwd, t)
    names = md.SHIFT_VJP_OUTPUTS if kind == "incr" else md.KIN_LTV_SHIFT_VJP_OUTPUTS
    fn = md.kin_shift_vjp if kind == "incr" else md.kin_ltv_shift_vjp
    prev = ("gpred_prev", "gpdu_prev") if kind == "incr" else ("gu_prev", "gpred_x_prev", "gpred_u_prev")
    tc = [_dev(torch, c) for c in cots]

    def vjp(want):
        def op(veh, t):
            o = fn(lay, veh, t["sol"], t["Ad"], t["Bd"], t["x"], t["mode"], *t["cots"], want=want)
            return [getattr(o, k) for k in names + prev]
        return op
    variants = [(None, None, tmode), (None, None, None), (None, ["gsol"], tmode), (None, list(names[1:]), tmode)] + \
        [(i, None, tmode) for i in range(len(tc))]
    for drop, want, m in variants:                          # mode NULL, outputs left out, each cotangent NULL
        check_entry_point(torch, md, "kin", which, vjp(want),
                          dict(t, mode=m, cots=[c if i != drop else None for i, c in enumerate(tc)]),
                          reads=drop is None and want is None)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("which", SHAPES)
def test_kin_rollout_fleet(torch, md, golden, which, N):
    B = 3 if which == "cars" else fc.B_SWEEP
    x, u = _lin_points(torch, golden, "kin_linearise.npz", B, 1, 4)
    check_entry_point(torch, md, "kin", which, lambda veh, t: list(md.rollout_kin(veh, t["x"], t["u"], N)),
                      dict(x=x[:, 0].contiguous(), u=u[:, 0].contiguous()))


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("which", SHAPES)
def test_lane_tail_fleet(torch, md, which, N):
    """mpcqp_lane_tail(_fleet)_device has no functional wrapper: called as LaneChangeMPC calls it, on
    copies, with a trajectory record and vehicles on both sides of the schedule's first switch."""
    B, (lay, _) = (3 if which == "cars" else fc.B_SWEEP), _mpc_layout("incr", N)
    rng = np.random.default_rng(330 + B + N)
    d = ks.kin_case(rng, B, N, "incr")
    t = _tail_device_inputs(torch, rng, d, B, N)
    t.update(step=_dev(torch, 48 + np.arange(B) % 5, torch.int32))
    sw, po = np.array(mpc.LANE_SWITCH_STEPS, np.int32), np.array(mpc.LANE_PATHS_OF, np.int32)

    def op(veh, t):
        Bn = t["sol"].shape[0]
        xt, pred, pdu, step = (t[k].clone() for k in ("x", "pred", "pdu", "step"))
        pid = torch.full((Bn,), -7, dtype=torch.int32, device=xt.device)
        traj = torch.zeros((Bn, 2, 6), dtype=torch.float64, device=xt.device)
        tlen = torch.zeros(Bn, dtype=torch.int32, device=xt.device)
        fn, v = md._entry("lane_tail", veh, Bn)
        md._check(fn(lay._h, v, Bn, md._p(t["sol"]), md._p(t["Ad"]), md._p(t["Bd"]), md._p(t["gd"]), md._p(xt),
                     md._p(pred), md._p(pdu), sw.size, md._np_ptr(sw), md._np_ptr(po), md._p(step), md._p(pid),
                     md._p(traj), 2, md._p(tlen), md._stream(torch, xt.device)), "lane_tail")
        return [xt, pred, pdu, step, pid, traj, tlen]
    check_entry_point(torch, md, "kin", which, op, t)
    pid = op(_sources(md, "kin", which)[1], t)[4].cpu().numpy()
    assert set(pid.tolist()) == {0, 1}                                 # both sides of the switch at step 50


# ------------------------------------------------------------------ fleet size --
def test_a_fleet_of_another_size_is_refused(torch, md, golden):
    structs, fleet, _ = _sources(md, "kin", "cars")
    x, u = _lin_points(torch, golden, "kin_linearise.npz", 2, 2, 4)
    with pytest.raises(ValueError, match="fleet of 3"):
        md.linearise_kinematics(fleet, x, u)
    with pytest.raises(ValueError, match="fleet of 3"):
        md.rollout_kin(fleet, x[:, 0].contiguous(), u[:, 0].contiguous(), 2)
    px = np.linspace(-10, 100, 200)
    with pytest.raises(ValueError, match="fleet of 3"):
        md.KinematicLTVMPC(np.zeros((2, 4)), np.zeros((2, 2)), px, px * 0.0, N=3, veh=fleet)
    from osqp_amd import torch_mpc as tm
    with pytest.raises(ValueError, match="fleet of 3"):
        tm.KinematicLTVRollout(_mpc_layout("ltv", 3)[0], 2, fleet)
    L = md._bind()
    out = [torch.zeros(2 * 2 * 16, dtype=torch.float64, device=x.device) for _ in range(3)]
    rc = L.mpcqp_kin_linearise_fleet_device(fleet._h, 2, 2, md._p(x), x.stride(0), x.stride(1), md._p(u), u.stride(0),
                                            u.stride(1), md._p(out[0]), md._p(out[1]), md._p(out[2]), 0,
                                            md._stream(torch, x.device))
    torch.cuda.synchronize()
    assert rc == 1 and b"fleet's size 3" in L.mpcqp_last_error() and not any(o.any() for o in out)


# ------------------------------------------------------------------ the closed loops --
def _loop_state(ctl, names):
    return [getattr(ctl, k).clone() for k in names]


def _closed_loop_against_singles(torch, build, names, nxa, steps):
    """build(sl, veh_of) -> a loop over the batch slice sl, veh_of(fleet or list of structs) its vehicle;
    names: the state tensors to compare.  The fleet's loop against three B = 1 loops."""
    fleet_loop, singles = build(slice(0, 3), None), [build(slice(b, b + 1), b) for b in range(3)]
    for step in range(steps):
        st, it = fleet_loop.step()
        torch.cuda.synchronize()
        got = _loop_state(fleet_loop, names) + [st.clone(), it.clone(), fleet_loop.sol.clone()]
        for b, one in enumerate(singles):
            s1, i1 = one.step()
            torch.cuda.synchronize()
            want = _loop_state(one, names) + [s1, i1, one.sol]
            for k, g, w in zip(list(names) + ["status", "iters", "sol"], got, want):
                assert torch.equal(g[b:b + 1], w), f"step {step + 1}, vehicle {b}: {k} differs"
        print(f"step {step + 1}: status {st.tolist()} iters {it.tolist()}")
        assert (st == 1).all(), f"step {step + 1}: status {st.tolist()}"
    states = getattr(fleet_loop, names[0]).cpu().numpy()
    assert not np.array_equal(states[0], states[1]) and not np.array_equal(states[1], states[2])
    return fleet_loop


@pytest.mark.parametrize("N", [2, 3])
def test_dynamic_mpc_with_a_fleet(torch, md, golden, N):
    g = golden("dyn_main_n30.npz")
    structs, fleet, _ = _sources(md, "dyn", "cars")
    x0 = g["in_xt"][0][None, :6] + np.array([[0.0] * 6, [0.3, -0.2, 0.02, -0.5, 0.01, 0.0], [-0.2, 0.4, -0.03, 1.0, 0.0, 0.01]])
    u0 = np.tile(g["in_xt"][0][6:], (3, 1))

    def build(sl, b):
        return md.DynamicMPC(x0[sl], u0[sl], g["path_x"], g["path_y"], N=N, veh=fleet if b is None else structs[b])
    _closed_loop_against_singles(torch, build, ("xt", "pred", "pdu"), 8, 3)


@pytest.mark.parametrize("N", [2, 3])
def test_kinematic_mpc_with_a_fleet(torch, md, golden, N):
    g = golden("kin_sim_n40.npz")
    structs, fleet, _ = _sources(md, "kin", "cars")
    x0 = g["x0"][None] + np.array([[0.0] * 4, [0.3, -0.2, -0.5, 0.02], [-0.2, 0.4, 1.0, -0.03]])
    u0 = np.tile([0.0, 0.01], (3, 1))

    def build(sl, b):
        return md.KinematicMPC(x0[sl], u0[sl], g["path_x"], g["path_y"], g["path_yaw"], N=N, traj_cap=3,
                               veh=fleet if b is None else structs[b])
    ctl = _closed_loop_against_singles(torch, build, ("xt", "pred", "pdu", "finish_cnt", "done", "traj", "traj_len"), 6, 3)
    assert ctl.traj_len.tolist() == [3, 3, 3]


@pytest.mark.parametrize("N", [2, 3])
def test_kinematic_ltv_mpc_with_a_fleet(torch, md, golden, N):
    g = golden("kinltv_sim_n3.npz")
    structs, fleet, _ = _sources(md, "kin", "cars")
    x0 = g["x0"][None] + np.array([[0.0] * 4, [0.3, -0.2, -0.5, 0.02], [-0.2, 0.4, 1.0, -0.03]])
    u0 = np.tile(g["u0"], (3, 1))

    def build(sl, b):
        return md.KinematicLTVMPC(x0[sl], u0[sl], g["path_x"], g["path_y"], N=N, traj_cap=3,
                                  veh=fleet if b is None else structs[b])
    ctl = _closed_loop_against_singles(torch, build, ("x", "u", "pred_x", "pred_u", "skipped", "steps_taken", "traj",
                                                      "traj_len"), 4, 3)
    assert not ctl.skipped.any()


@pytest.mark.parametrize("N", [2, 3])
def test_lane_change_mpc_with_a_fleet(torch, md, N):
    from test_lane_device import _lanes, _starts
    structs, fleet, _ = _sources(md, "kin", "cars")
    (x0, u0), (px, paths_y) = _starts(3), _lanes()
    step0 = np.array([49, 50, 10], np.int32)

    def build(sl, b):
        return md.LaneChangeMPC(x0[sl], u0[sl], px, paths_y, N=N, step0=step0[sl], traj_cap=2,
                                veh=fleet if b is None else structs[b])
    _closed_loop_against_singles(torch, build, ("xt", "pred", "pdu", "steps", "path_id", "traj", "traj_len"), 6, 1)


@pytest.mark.parametrize("N", [2, 3])
def test_kinematic_frozen_mpc_with_a_fleet(torch, md, N):
    """The host-side initial rollout runs per vehicle (mpc.per_vehicle): the B = 1 loops' own."""
    from test_kinfrozen_device import _main_path, _starts
    structs, fleet, _ = _sources(md, "kin", "cars")
    (x0, u0, pred_u0), (px, py) = _starts(3, N), _main_path()

    def build(sl, b):
        return md.KinematicFrozenMPC(x0[sl], u0[sl], px, py, N=N, pred_u0=pred_u0[sl], traj_cap=2,
                                     veh=fleet if b is None else structs[b])
    fleet_loop = build(slice(0, 3), None)
    for b in range(3):
        one = build(slice(b, b + 1), b)
        assert torch.equal(fleet_loop.pred_x[b:b + 1], one.pred_x) and torch.equal(fleet_loop.x[b:b + 1], one.x)
    _closed_loop_against_singles(torch, build, ("x", "u", "pred_x", "skipped", "steps_taken", "traj", "traj_len"), 4, 1)


# ------------------------------------------------------------------ the differentiable rollouts --
def _rollout_run(torch, make, Bn, starts, refs, T, qdiag_np, out_of, cot):
    """Outputs and gradients of a T-step rollout from `starts` (leaves) with the given references."""
    leaves = [_dev(torch, s).requires_grad_(True) for s in starts]
    qdiag = _dev(torch, qdiag_np).requires_grad_(True)
    Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
    roll = make(Bn)
    outs = out_of(roll, leaves, T, Xr, (torch.diag(qdiag), None, None))
    sum((o * _dev(torch, c)).sum() for o, c in zip(outs, cot)).backward()
    torch.cuda.synchronize()
    assert (roll.status == 1).all() and (roll.astat == 1).all(), (roll.status.tolist(), roll.astat.tolist())
    return [o.detach() for o in outs], [v.grad for v in leaves], qdiag.grad.cpu().numpy()


def _rollout_against_singles(torch, make_of, starts, refs, T, qdiag_np, out_of, cots, label):
    structs, fleet = make_of["structs"], make_of["fleet"]
    outs, grads, gq = _rollout_run(torch, lambda Bn: make_of["make"](Bn, fleet), 3, starts, refs, T, qdiag_np, out_of, cots)
    total = np.zeros_like(gq)
    for b in range(3):
        o1, g1, q1 = _rollout_run(torch, lambda Bn: make_of["make"](Bn, structs[b]), 1, [s[b:b + 1] for s in starts],
                                  refs, T, qdiag_np, out_of, [c[b:b + 1] for c in cots])
        for k, (a, w) in enumerate(zip(outs, o1)):
            assert torch.equal(a[b:b + 1], w), f"{label}: vehicle {b}, output {k} differs"
        for k, (a, w) in enumerate(zip(grads, g1)):
            assert torch.equal(a[b:b + 1], w), f"{label}: vehicle {b}, gradient of leaf {k} differs"
        total = total + q1
    dq = _rel(gq, total)
    print(f"measured {label}: d loss / d diag Q against the three rollouts' sum {dq:.3e}, bar {BAR_KIN_ROLL:.1e}")
    assert gq.any() and dq < BAR_KIN_ROLL
    assert not torch.equal(outs[0][0], outs[0][1]) and not torch.equal(outs[0][1], outs[0][2])


def test_dynamic_rollout_with_a_fleet(torch, md):
    from osqp_amd import torch_mpc as tm
    N, T = 3, 3
    structs, fleet, _ = _sources(md, "dyn", "cars")
    lay = _dyn_layout(N)
    xt0 = np.tile(np.concatenate([dyn.X0_INTERIOR, dyn.U0]), (3, 1))
    rng = np.random.default_rng(340)
    cots = [rng.standard_normal(s) for s in ((3, T + 1, 8), (3, T, 2), (3, N + 1, 8))]

    def out_of(roll, leaves, T, Xr, weights):
        xt = leaves[0]
        return roll(xt, xt[:, None, :].expand(xt.shape[0], N + 1, 8), T, Xr=Xr, weights=weights)
    _rollout_against_singles(torch, dict(structs=structs, fleet=fleet,
                                         make=lambda Bn, veh: tm.DynamicRollout(lay, Bn, veh, **DYN_SETTINGS)),
                             [xt0], loop.loop_references(N, T), T, np.diag(mpc.DYN_Q), out_of, cots, "dynamic rollout")


def test_kinematic_rollout_with_a_fleet(torch, md):
    from osqp_amd import torch_mpc as tm
    N, T = 3, 3
    structs, fleet, _ = _sources(md, "kin", "cars")
    lay, Qw = _mpc_layout("incr", N)
    x0, u0 = cpu.INCR_CASES["interior steer"][:2]
    xt0 = np.tile(np.concatenate([x0, u0]), (3, 1))
    rng = np.random.default_rng(341)
    cots = [rng.standard_normal(s) for s in ((3, T + 1, 6), (3, T, 2), (3, N + 1, 6))]

    def out_of(roll, leaves, T, Xr, weights):
        xt = leaves[0]
        return roll(xt, xt[:, None, :].expand(xt.shape[0], N + 1, 6), T, Xr=Xr, weights=weights)
    _rollout_against_singles(torch, dict(structs=structs, fleet=fleet,
                                         make=lambda Bn, veh: tm.KinematicRollout(lay, Bn, veh, **KIN_SETTINGS["incr"])),
                             [xt0], kloop.kin_loop_references(N, T), T, np.diag(Qw), out_of, cots, "kinematic rollout")
