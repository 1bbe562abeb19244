"""Closed-loop rollouts differentiated on one solver handle (include/mpcqp.h): the
solution record's round trip, QPLayer(record=True), k_tail_vjp<DynamicIncrTail> against its numpy statement,
and torch_mpc.DynamicRollout -- forward against DynamicMPC, backward against the chain of
MPCLayers of tests/test_dyn_vjp_device.py and against central differences.

Bars: BAR_SHIFT and BAR_ROLL are ten times the deviation measured on the MI355X, max |a - b| /
max |b| per array; BAR_LOOP is tests/test_dyn_vjp_device.py's (h = 1e-3, 1e-4 of the largest
derivative).  Everything the record promises is held bit for bit.
"""
import numpy as np
import pytest

import test_dyn_vjp_ref as dyn
import test_rollout_ref as loop
import test_shift_vjp_ref as shift
from osqp_amd import mpc
from test_dyn_vjp_device import BAR_LOOP, N_CHAIN, PERT, POINTS, _layout, _two_steps, _vehicle
from test_mpc_vjp_device import GUARD, INCR_ADJOINT, SENTINEL, TIGHT, Arena, _bits, _dev, _rel

pytestmark = pytest.mark.gpu

BAR_SHIFT = 1.9e-15        # measured: 1.89e-16 (B 130, N 3, without gpdu; B 1: 1.31e-16; the model outputs: 0)
# measured: d du_0 / d xt0 5.1e-16 and 1.2e-16, d loss / d diag Q 3.05e-14 (interior) and 1.29e-14 (steer
# active).  The two sides do not start step 2 from the same bits: the chain's plant step is torch's
# matrix product, the rollout's k_incr_shift, and step 2's du_0 already differs by 7.4e-15 and 9.4e-15
# of its size; the weight sums also run in another order (per instance, then over the batch).
BAR_ROLL = 3.1e-13
SETTINGS = dict(TIGHT, warm_start=True, **INCR_ADJOINT)
ADJ_FIELDS = ("rx", "ry", "gq", "gl", "gu", "gPx", "gAx", "ares")


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ------------------------------------------------------------------ the shift's VJP --
def _shift_device_inputs(torch, rng, d, B, N):
    """The host case as the device takes it: (B, N, ..) models whose stage 0 is the case's (the other
    stages, which nothing may read, are noise)."""
    Ad, Bd, gd = rng.standard_normal((B, N, 6, 6)), rng.standard_normal((B, N, 6, 2)), rng.standard_normal((B, N, 6))
    Ad[:, 0], Bd[:, 0], gd[:, 0] = d["Ad0"], d["Bd0"], d["gd0"]
    return {k: _dev(torch, v) for k, v in dict(sol=d["sol"], Ad=Ad, Bd=Bd, gd=gd, xt=d["xt"]).items()}


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3])
def test_shift_vjp_kernel_matches_the_host_statement(torch, B, N):
    """Measured on the MI355X (max |a - b| / max |b| per array, the worst of every variant below):
    B 1: 1.31e-16 (N 2), 1.03e-16 (N 3); B 130: 1.17e-16 (N 2), 1.89e-16 (N 3)."""
    from osqp_amd.mpc_device import SHIFT_VJP_OUTPUTS, incr_shift, incr_shift_vjp
    veh, lay = _vehicle(), _layout(N)
    rng = np.random.default_rng(80 + B + N)
    d = shift.shift_case(rng, B, N)
    cots = shift.shift_cotangents(rng, B, N)
    t = _shift_device_inputs(torch, rng, d, B, N)
    tc = [_dev(torch, c) for c in cots]
    # the functional forward: the host statement's values, nothing written in place
    keep = {k: v.clone() for k, v in t.items()}
    xt1, pred1, pdu1 = incr_shift(lay, veh, t["sol"], t["Ad"], t["Bd"], t["gd"], t["xt"])
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], keep[k]) for k in t)
    hx, hp, hd = mpc.incr_shift(dyn.VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["gd0"], d["xt"])
    assert np.allclose(xt1.cpu().numpy(), hx, rtol=1e-14, atol=1e-14)
    assert np.allclose(pred1.cpu().numpy(), hp, rtol=1e-12, atol=1e-12) and np.array_equal(pdu1.cpu().numpy(), hd)
    # the VJP
    host = dict(zip(SHIFT_VJP_OUTPUTS, mpc.incr_shift_vjp(dyn.VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["xt"], *cots)))
    shapes = dict(gsol=(B, lay.n), gAd0=(B, 6, 6), gBd0=(B, 6, 2), ggd0=(B, 6), gxt=(B, 8))
    arena, arena2 = Arena(torch, shapes), Arena(torch, shapes)
    for a in (arena, arena2):
        incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *tc, out=a.view)
    torch.cuda.synchronize()
    assert arena.guards_intact() and arena2.guards_intact()
    got = {k: arena.view[k].cpu().numpy() for k in shapes}
    assert all(np.isfinite(v).all() for v in got.values())
    assert all(_bits(arena2.view[k].cpu().numpy(), got[k]) for k in shapes)   # a repeat returns the same bits
    assert shift.copied_entries_are_exact(N, got["gsol"], cots[1], cots[2], gu0=got["gxt"][:, 6:])
    assert shift.euler_zero_pattern_is_exact(N, d["sol"], got["gsol"], cots[1])
    assert _bits(got["ggd0"], host["ggd0"])
    worst = 0.0
    for k in shapes:
        dev = _rel(got[k], host[k])
        worst = max(worst, dev)
        print(f"measured shift vjp B={B} N={N} {k}: {dev:.3e}")
    # each cotangent None in turn: the host statement's, and a zero tensor's bit for bit
    for i in range(3):
        some = [c if j != i else None for j, c in enumerate(tc)]
        zero = [c if j != i else torch.zeros_like(c) for j, c in enumerate(tc)]
        s = incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *some)
        z = incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *zero)
        e = dict(zip(SHIFT_VJP_OUTPUTS, mpc.incr_shift_vjp(dyn.VEH, N, d["sol"], d["Ad0"], d["Bd0"], d["xt"],
                                                           *[c if j != i else None for j, c in enumerate(cots)])))
        torch.cuda.synchronize()
        for k in shapes:
            sk = getattr(s, k).cpu().numpy()
            assert np.array_equal(sk, getattr(z, k).cpu().numpy()), (i, k)
            dev = _rel(sk, e[k]) if np.abs(e[k]).max() > 0 else float(np.abs(sk).max())
            worst = max(worst, dev)
        print(f"measured shift vjp B={B} N={N} without cotangent {i}: worst so far {worst:.3e}")
    # each output left out in turn: its buffer keeps the sentinels, the others their bits
    for k in shapes:
        a = Arena(torch, shapes)
        o = incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *tc, want=[w for w in shapes if w != k],
                           out={w: v for w, v in a.view.items() if w != k})
        torch.cuda.synchronize()
        assert getattr(o, k) is None and a.untouched(k) and a.guards_intact()
        assert all(_bits(a.view[w].cpu().numpy(), got[w]) for w in shapes if w != k)
    print(f"measured shift vjp B={B} N={N}: worst {worst:.3e}, bar {BAR_SHIFT:.1e}")
    assert worst < BAR_SHIFT


def test_torch_incr_shift_is_wired_to_the_vjp(torch):
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import incr_shift, incr_shift_vjp
    veh, N, B = _vehicle(), 3, 5
    lay = _layout(N)
    rng = np.random.default_rng(91)
    d = shift.shift_case(rng, B, N)
    t = _shift_device_inputs(torch, rng, d, B, N)
    ins = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    outs = tm.incr_shift(lay, veh, ins["sol"], ins["Ad"], ins["Bd"], ins["gd"], ins["xt"])
    for o, w in zip(outs, incr_shift(lay, veh, t["sol"], t["Ad"], t["Bd"], t["gd"], t["xt"])):
        assert torch.equal(o, w)
    tc = [_dev(torch, c) for c in shift.shift_cotangents(rng, B, N)]
    sum((o * c).sum() for o, c in zip(outs, tc)).backward()
    g = incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], *tc)
    assert torch.equal(ins["sol"].grad, g.gsol) and torch.equal(ins["xt"].grad, g.gxt)
    for k, w in (("Ad", g.gAd0), ("Bd", g.gBd0), ("gd", g.ggd0)):
        assert torch.equal(ins[k].grad[:, 0], w) and not ins[k].grad[:, 1:].any()
    # only pdu has a cotangent, only sol requires a gradient
    sol = t["sol"].clone().requires_grad_(True)
    (g1,) = torch.autograd.grad((tm.incr_shift(lay, veh, sol, t["Ad"], t["Bd"], t["gd"], t["xt"])[2] * tc[2]).sum(), [sol])
    assert torch.equal(g1, incr_shift_vjp(lay, veh, t["sol"], t["Ad"], t["Bd"], t["xt"], None, None, tc[2],
                                          want=["gsol"]).gsol)


# ------------------------------------------------------------------ the solution record --
def _dyn_problem(torch, lay, veh, x0s, Xr):
    """The device QP of one step from the states x0s, linearised there on every stage: (Px, Ax, q, l, u)."""
    from osqp_amd.mpc_device import linearise
    B, N = len(x0s), lay.N
    tx, tu = _dev(torch, x0s), _dev(torch, np.tile(dyn.U0, (B, 1)))
    Ad, Bd, gd = linearise(veh, tx[:, None, :].expand(B, N, 6), tu[:, None, :].expand(B, N, 2))
    Ax, q, l, u = lay.assemble(Ad, Bd, gd, torch.cat([tx, tu], dim=1), _dev(torch, np.tile(Xr, (B, 1, 1))))
    Px = _dev(torch, np.tile(lay.pattern()[0].data, (B, 1)))
    return Px, Ax, q, l, u


def _solve(torch, db, data):
    x = torch.empty((db.B, db.n), dtype=torch.float64, device="cuda:0")
    y = torch.empty((db.B, db.m), dtype=torch.float64, device="cuda:0")
    st = torch.empty(db.B, dtype=torch.int32, device="cuda:0")
    it = torch.empty(db.B, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    db.setup(*data)
    db.solve(x, y, st, it)
    db.synchronize()
    return st.cpu().numpy()


def _adjoint(torch, db, gx, gy):
    torch.cuda.synchronize()
    g = db.adjoint(gx, gy)
    db.synchronize()
    out = {k: getattr(g, k).cpu().numpy() for k in ADJ_FIELDS}
    out.update(act=g.act.cpu().numpy(), astat=g.astat.cpu().numpy())
    return out


def _record_round_trip(torch, db, first, other, label):
    """solve `first`, adjoint with a dense seed, save; set up and solve `other` on the same handle;
    set up `first`, load, adjoint: every output bit for bit.  Returns (status, the two adjoints)."""
    rng = np.random.default_rng(17)
    gx, gy = _dev(torch, rng.standard_normal((db.B, db.n))), _dev(torch, rng.standard_normal((db.B, db.m)))
    st = _solve(torch, db, first)
    g1 = _adjoint(torch, db, gx, gy)
    W = db.record_width
    assert W == db.n + 2 * db.m + 1
    full = torch.full((db.B * W + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda:0")
    rec = full[GUARD:GUARD + db.B * W].view(db.B, W)
    db.save_solution(rec)
    db.synchronize()
    assert bool((full[:GUARD] == SENTINEL).all()) and bool((full[-GUARD:] == SENTINEL).all())
    r = rec.cpu().numpy()
    assert np.isfinite(r).all() and np.array_equal(r[:, -1], st.astype(float))
    st2 = _solve(torch, db, other)
    g_other = _adjoint(torch, db, gx, gy)
    torch.cuda.synchronize()
    db.setup(*first)
    db.load_solution(rec)
    g2 = _adjoint(torch, db, gx, gy)
    for k in ADJ_FIELDS:
        assert _bits(g1[k], g2[k]), f"{label}: {k} differs after the round trip"
    assert np.array_equal(g1["act"], g2["act"]) and np.array_equal(g1["astat"], g2["astat"])
    print(f"{label}: status {st.tolist()} / other {st2.tolist()}, astat {g1['astat'].tolist()}, "
          f"max ares {g1['ares'].max():.2e}")
    return st, g1, g_other


@pytest.mark.parametrize("point", list(POINTS))
def test_record_round_trip_on_the_dynamic_layout(torch, point):
    from osqp_amd import DeviceBatch
    x0b, _, scale, _ = POINTS[point]
    N, B, veh = N_CHAIN, len(PERT), _vehicle()
    lay = _layout(N)
    P, A, _, _ = lay.pattern()
    first = _dyn_problem(torch, lay, veh, x0b + scale * PERT, dyn.dyn_reference(N))
    moved = dyn.dyn_reference(N)
    moved[0] += 0.3
    other = _dyn_problem(torch, lay, veh, x0b + 0.01 + scale * PERT[::-1], moved)
    db = DeviceBatch(P, A, B, **SETTINGS)
    st, g1, g_other = _record_round_trip(torch, db, first, other, f"record {point}")
    assert (st == 1).all() and (g1["astat"] == 1).all()
    assert not _bits(g1["gq"], g_other["gq"])                      # the batch in between is another one
    # stopped at max_iter = 5: the record carries the status, the adjoint after the load is not run
    short = DeviceBatch(P, A, B, **dict(SETTINGS, max_iter=5, polish=False))
    st, g1, _ = _record_round_trip(torch, short, first, other, f"record {point} max_iter 5")
    assert (st != 1).all() and not g1["astat"].any()
    assert not any(g1[k].any() for k in ADJ_FIELDS) and not g1["act"].any()


def test_record_round_trip_on_cfg2(torch):
    """cfg 2 (the vanilla lateral layout, B = 8).  Its plan eliminates nothing, so save and load make
    no plan move here; the slack layout below does."""
    from osqp_amd import DeviceBatch, canonical_data
    b = mpc.make_batch(2, 8)
    P, A = canonical_data(b["P"], b["A"])
    first = [_dev(torch, b[k]) for k in ("Px", "Ax", "q", "l", "u")]
    other = [first[0], first[1], first[2] * 1.05, first[3], first[4]]
    db = DeviceBatch(P, A, 8, warm_start=True, **dict(TIGHT, polish=False))
    st, g1, _ = _record_round_trip(torch, db, first, other, "record cfg 2")
    assert (st == 1).all() and (g1["astat"] == 1).all()
    print(f"record cfg 2: plan {db.plan_info()}")


def test_record_round_trip_through_the_replan(torch):
    """The slack layout (cfg 3): its plan eliminates the slack columns, the first adjoint moves the
    handle to the plain plan, and the record is saved and loaded there.  K is singular on this
    layout (astat -1); what comes back is still the same bits."""
    from osqp_amd import DeviceBatch, canonical_data
    b = mpc.make_batch(3, 4)
    P, A = canonical_data(b["P"], b["A"])
    first = [_dev(torch, b[k]) for k in ("Px", "Ax", "q", "l", "u")]
    other = [first[0], first[1], first[2] * 1.05, first[3], first[4]]
    db = DeviceBatch(P, A, 4, **b["settings"])
    assert db.plan_info()["n_eliminated"] > 0
    st, g1, _ = _record_round_trip(torch, db, first, other, "record cfg 3")
    assert db.plan_info()["n_eliminated"] == 0 and (st == 1).all()
    # a handle still on the eliminated plan: save and load make the move themselves
    fresh = DeviceBatch(P, A, 4, **b["settings"])
    _solve(torch, fresh, first)
    rec = fresh.save_solution()
    assert fresh.plan_info()["n_eliminated"] == 0
    late = DeviceBatch(P, A, 4, **b["settings"])
    torch.cuda.synchronize()
    late.setup(*first)
    late.load_solution(rec)
    assert late.plan_info()["n_eliminated"] == 0
    gx = _dev(torch, np.random.default_rng(17).standard_normal((4, db.n)))
    ga, gb = _adjoint(torch, fresh, gx, None), _adjoint(torch, late, gx, None)
    for k in ADJ_FIELDS:
        assert _bits(ga[k], gb[k]), k
    assert np.array_equal(ga["act"], gb["act"]) and np.array_equal(ga["astat"], gb["astat"])


def test_record_refusals(torch):
    from osqp_amd import DeviceBatch, canonical_data
    b = mpc.make_batch(2, 8)
    P, A = canonical_data(b["P"], b["A"])
    data = [_dev(torch, b[k]) for k in ("Px", "Ax", "q", "l", "u")]
    db = DeviceBatch(P, A, 8, warm_start=True, **dict(TIGHT, polish=False))
    rec = torch.zeros((8, db.record_width), dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError, match="no setup"):
        db.load_solution(rec)
    with pytest.raises(ValueError, match="no solve"):
        db.save_solution(rec)
    torch.cuda.synchronize()
    db.setup(*data)
    with pytest.raises(ValueError, match="no solve"):
        db.save_solution(rec)
    with pytest.raises(ValueError, match="record"):
        db.load_solution(rec[:, :-1].contiguous())
    assert db.one_shot(True) > 0
    db.setup_solve(*data)
    db.synchronize()
    with pytest.raises(ValueError, match="one-shot"):
        db.save_solution(rec)
    with pytest.raises(ValueError, match="one-shot"):
        db.load_solution(rec)
    assert not rec.any()


# ------------------------------------------------------------------ QPLayer(record=True) --
def _two_step_case(torch, point):
    x0b, j, _, _ = POINTS[point]
    N = N_CHAIN
    pts = loop.loop_points(x0b)
    Bn = len(pts)
    Xr1, Xr2 = (_dev(torch, np.tile(r, (Bn, 1, 1))) for r in loop.loop_references(N, 2))
    return pts, Bn, j, Xr1, Xr2


def _chain_gradients(torch, tm, veh, layers, pts, Xr1, Xr2, j):
    """test_two_closed_loop_steps's two gradients of step 2's du_0[j] through _two_steps."""
    tx, tu = _dev(torch, pts).requires_grad_(True), _dev(torch, np.tile(dyn.U0, (len(pts), 1)))
    qdiag = _dev(torch, np.diag(mpc.DYN_Q)).requires_grad_(True)
    out = _two_steps(torch, tm, veh, layers, tx, tu, Xr1, Xr2, j, qdiag)
    (gx,) = torch.autograd.grad(out[0], [tx], retain_graph=True)
    (gq,) = torch.autograd.grad(out.sum(), [qdiag])
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), gx.cpu().numpy(), gq.cpu().numpy()


@pytest.fixture(scope="module")
def chain(torch):
    """The chain of two MPCLayers on both points, computed once."""
    from osqp_amd import torch_mpc as tm
    veh, lay, out = _vehicle(), _layout(N_CHAIN), {}
    for point in POINTS:
        pts, Bn, j, Xr1, Xr2 = _two_step_case(torch, point)
        layers = [tm.MPCLayer(lay, Bn, **SETTINGS) for _ in range(2)]
        out[point] = _chain_gradients(torch, tm, veh, layers, pts, Xr1, Xr2, j)
        assert all((layer.status == 1).all() and (layer.astat == 1).all() for layer in layers)
    return out


@pytest.mark.parametrize("point", list(POINTS))
def test_one_recording_layer_serves_both_steps(torch, chain, point):
    from osqp_amd import torch_mpc as tm
    veh, lay = _vehicle(), _layout(N_CHAIN)
    pts, Bn, j, Xr1, Xr2 = _two_step_case(torch, point)
    one = tm.MPCLayer(lay, Bn, record=True, **SETTINGS)
    val, gx, gq = _chain_gradients(torch, tm, veh, [one, one], pts, Xr1, Xr2, j)
    assert _bits(val, chain[point][0]) and _bits(gx, chain[point][1]) and _bits(gq, chain[point][2])
    # the default layer holds one solve: the backward of step 1 after step 2's forward raises
    plain = tm.MPCLayer(lay, Bn, **SETTINGS)
    with pytest.raises(RuntimeError, match="another forward"):
        _chain_gradients(torch, tm, veh, [plain, plain], pts, Xr1, Xr2, j)


# ------------------------------------------------------------------ DynamicRollout --
@pytest.mark.parametrize("warm", [False, True])
def test_rollout_forward_is_dynamic_mpc(torch, golden, warm):
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import DynamicMPC
    g = golden("dyn_main_n30.npz")
    N, B, T = 3, 3, 3
    x0 = g["in_xt"][0][None, :6] + np.array([[0.0] * 6, [0.3, -0.2, 0.02, -0.5, 0.01, 0.0], [-0.2, 0.4, -0.03, 1.0, 0.0, 0.01]])
    u0 = np.tile(g["in_xt"][0][6:], (B, 1))
    ref = DynamicMPC(x0, u0, g["path_x"], g["path_y"], N=N, warm_start=warm)
    torch.cuda.synchronize()
    xt0, pred0 = ref.xt.clone(), ref.pred.clone()
    roll = tm.DynamicRollout(ref.layout, B, ref.veh, warm_start=warm)
    XT, DU0, pred_T = roll(xt0, pred0, T, path=(ref.path_x, ref.path_y))
    assert XT.shape == (B, T + 1, 8) and DU0.shape == (B, T, 2) and pred_T.shape == (B, N + 1, 8)
    assert torch.equal(XT[:, 0], xt0)
    for t in range(T):
        status, iters = ref.step()
        torch.cuda.synchronize()
        assert torch.equal(XT[:, t + 1], ref.xt), f"step {t + 1}"
        assert torch.equal(roll.status[t], status) and torch.equal(roll.iters[t], iters)
        assert torch.equal(DU0[:, t], ref.sol[:, (N + 1) * 8:(N + 1) * 8 + 2])
    assert torch.equal(pred_T, ref.pred)
    print(f"rollout forward warm={warm}: iterations {roll.iters.tolist()}")


def _rollout_gradients(torch, roll, pts, refs, j, T, qdiag_np=None):
    """d DU0[0, T-1, j] / d xt0 and d DU0[:, T-1, j].sum() / d diag Q of a T-step rollout from pred0 = xt0
    on every stage."""
    Bn, N = len(pts), roll.N
    xt0 = _dev(torch, np.concatenate([pts, np.tile(dyn.U0, (Bn, 1))], 1)).requires_grad_(True)
    qdiag = _dev(torch, np.diag(mpc.DYN_Q) if qdiag_np is None else qdiag_np).requires_grad_(True)
    Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
    XT, DU0, _ = roll(xt0, xt0[:, None, :].expand(Bn, N + 1, 8), T, Xr=Xr, weights=(torch.diag(qdiag), None, None))
    out = DU0[:, T - 1, j]
    (gx,) = torch.autograd.grad(out[0], [xt0], retain_graph=True)
    (gq,) = torch.autograd.grad(out.sum(), [qdiag])
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), gx.cpu().numpy(), gq.cpu().numpy()


@pytest.mark.parametrize("point", list(POINTS))
def test_rollout_backward_matches_the_layer_chain(torch, chain, point):
    """T = 2 from pred0 = xt0 on every stage with the two given references is exactly _two_steps:
    one handle instead of two.  Measured on the MI355X: BAR_ROLL's comment."""
    from osqp_amd import torch_mpc as tm
    veh, lay = _vehicle(), _layout(N_CHAIN)
    pts, Bn, j, _, _ = _two_step_case(torch, point)
    roll = tm.DynamicRollout(lay, Bn, veh, **SETTINGS)
    val, gx, gq = _rollout_gradients(torch, roll, pts, loop.loop_references(N_CHAIN, 2), j, 2)
    cval, cgx, cgq = chain[point]
    assert (roll.status == 1).all() and (roll.astat == 1).all()
    assert roll.act.shape == (2, Bn, lay.m) and roll.ares.shape == (2, Bn)
    # (the chain's plant step is torch's matrix product, the rollout's k_incr_shift: step 2 starts from
    # states that differ by rounding)
    print(f"measured rollout {point}: step 2's du_0[{j}] against the chain's {_rel(val, cval):.3e}")
    assert not gx[1:].any()                                       # the instances are independent
    dx, dq = _rel(gx[0, :6], cgx[0]), _rel(gq, cgq)
    print(f"measured rollout {point}: d du_0 / d xt0 {dx:.3e} (rollout {gx[0, :6]} chain {cgx[0]}), "
          f"d loss / d diag Q {dq:.3e}, bar {BAR_ROLL:.1e}")
    assert dx < BAR_ROLL and dq < BAR_ROLL


def test_rollout_three_steps_match_central_differences(torch):
    """T = 3 on the interior point (tests/test_rollout_ref.py: the row classes stay equal over the
    13 points for three steps, no inequality row active): d DU0[0, 2, j] / d x0 against central
    differences with h = 1e-3, the perturbed copies in the same batch.  Measured on the MI355X: 9.9e-6
    of the largest derivative (the truncation of h = 1e-3, as in test_two_closed_loop_steps)."""
    from osqp_amd import torch_mpc as tm
    x0b, j, _, _ = POINTS["interior"]
    veh, lay, T, h = _vehicle(), _layout(N_CHAIN), loop.T_LOOP, loop.H_LOOP
    pts = loop.loop_points(x0b, h)
    roll = tm.DynamicRollout(lay, len(pts), veh, **SETTINGS)
    val, gx, _ = _rollout_gradients(torch, roll, pts, loop.loop_references(N_CHAIN, T), j, T)
    assert (roll.status == 1).all() and (roll.astat == 1).all()
    act = roll.act.cpu().numpy()
    assert (act == act[:, :1]).all(), "the row classes change within the step"
    assert not ((act == 1) | (act == 2)).any()
    fd = (val[1::2] - val[2::2]) / (2 * h)
    dev = np.abs(fd - gx[0, :6]).max() / np.abs(fd).max()
    print(f"measured rollout T=3: d du_0[{j}](step 3) / d x0: fd {fd} backward {gx[0, :6]} deviation {dev:.2e}")
    assert dev < BAR_LOOP


def test_two_rollouts_alive_at_once(torch):
    from osqp_amd import torch_mpc as tm
    veh, lay = _vehicle(), _layout(N_CHAIN)
    cases = []
    for point in POINTS:
        pts, Bn, j, _, _ = _two_step_case(torch, point)
        cases.append((pts, j))
    roll = tm.DynamicRollout(lay, len(cases[0][0]), veh, **SETTINGS)
    refs = loop.loop_references(N_CHAIN, 2)
    alone = [_rollout_gradients(torch, roll, pts, refs, j, 2) for pts, j in cases]
    # both forwards, then both backwards, the first rollout's last
    live = []
    for pts, j in cases:
        Bn = len(pts)
        xt0 = _dev(torch, np.concatenate([pts, np.tile(dyn.U0, (Bn, 1))], 1)).requires_grad_(True)
        qdiag = _dev(torch, np.diag(mpc.DYN_Q)).requires_grad_(True)
        Xr = torch.stack([_dev(torch, np.tile(r, (Bn, 1, 1))) for r in refs])
        _, DU0, _ = roll(xt0, xt0[:, None, :].expand(Bn, N_CHAIN + 1, 8), 2, Xr=Xr, weights=(torch.diag(qdiag), None, None))
        live.append((DU0[:, 1, j], xt0, qdiag))
    for k in (1, 0):
        out, xt0, qdiag = live[k]
        (gx,) = torch.autograd.grad(out[0], [xt0], retain_graph=True)
        (gq,) = torch.autograd.grad(out.sum(), [qdiag])
        torch.cuda.synchronize()
        assert _bits(out.detach().cpu().numpy(), alone[k][0])
        assert _bits(gx.cpu().numpy(), alone[k][1]) and _bits(gq.cpu().numpy(), alone[k][2]), f"rollout {k}"


def test_rollout_strict_and_masking(torch):
    """An instance whose solve stops at max_iter has astat 0 at that step: strict raises, strict=False
    gives it zero gradients and leaves it out of the weight sums."""
    from osqp_amd import torch_mpc as tm
    veh, lay = _vehicle(), _layout(N_CHAIN)
    pts, Bn, j, _, _ = _two_step_case(torch, "interior")
    refs = loop.loop_references(N_CHAIN, 2)
    short = dict(SETTINGS, max_iter=5, polish=False)
    with pytest.raises(RuntimeError, match="no reliable gradient"):
        _rollout_gradients(torch, tm.DynamicRollout(lay, Bn, veh, **short), pts, refs, j, 2)
    roll = tm.DynamicRollout(lay, Bn, veh, strict=False, **short)
    _, gx, gq = _rollout_gradients(torch, roll, pts, refs, j, 2)
    assert (roll.status != 1).all() and not roll.astat.any()
    assert not gx.any() and not gq.any()
