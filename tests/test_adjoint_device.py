"""The device adjoint (mpcqp_adjoint_device / _batch, adjoint.hip::k_adjoint) against the dense
numpy statement of tests/qp_adjoint_ref.py, evaluated at the device's own (x, y): the comparison
isolates the linear solve (tests/test_adjoint_ref.py checks the statement itself against finite
differences).  Deviations are max |a - b| / max |b| per output array, the largest over the
arrays and instances of a case; DESIGN.md ("Gradients of the solution") records what one run on
the MI355X gave, and each bar below is 10x that, never looser than 1e-6.
"""
import json

import numpy as np
import pytest

import osqp_amd
import qp_adjoint_ref as ref
from osqp_amd import OSQP, DeviceBatch, OSQPBatch, canonical_data, mpc
from test_oracle import osqp_demo_problem

pytestmark = pytest.mark.gpu

TIGHT = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=100000, verbose=False)
FIELDS = ("rx", "ry", "gq", "gl", "gu", "gPx", "gAx")
# bars: 10x the largest deviation recorded on the MI355X (demo 2.7e-16, cfg 2
# 2.5e-12, the long plans 7.9e-13), never looser than 1e-6
BAR_DEMO = 3e-15
BAR_CFG2 = 2.5e-11
BAR_LONG = 8e-12
# ares against the helper's residual of the returned (r_x, r_y) on the scaled system (OSQP's
# scaling restated in numpy): equal where the residual is the solve's error, within this factor
# where both are rounding noise, which is what they are below RES_FLOOR (measured)
RES_FACTOR = 10.0  # (measured ratios: 0.986 .. 1.000)
RES_FLOOR = 1e-14


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).to("cuda:0").contiguous()


class _Batch:
    """A DeviceBatch set up and solved once (torch tensors in, numpy views out)."""

    def __init__(self, torch, P, A, Px, Ax, q, l, u, **settings):
        self.torch = torch
        self.P, self.A = canonical_data(P, A)
        self.Px, self.Ax, self.q, self.l, self.u = (np.asarray(v, float) for v in (Px, Ax, q, l, u))
        B = self.q.shape[0]
        self.B, self.n, self.m = B, self.P.shape[0], self.A.shape[0]
        self.db = DeviceBatch(self.P, self.A, B, **settings)
        self.t = [_dev(torch, v) for v in (self.Px, self.Ax, self.q, self.l, self.u)]
        torch.cuda.synchronize()
        self.db.setup(*self.t)

    def solve(self):
        torch = self.torch
        x = torch.empty((self.B, self.n), dtype=torch.float64, device="cuda:0")
        y = torch.empty((self.B, self.m), dtype=torch.float64, device="cuda:0")
        st = torch.empty(self.B, dtype=torch.int32, device="cuda:0")
        it = torch.empty(self.B, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        self.db.solve(x, y, st, it)
        self.db.synchronize()
        return x.cpu().numpy(), y.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()

    def adjoint(self, gx, gy):
        torch = self.torch
        tgx = None if gx is None else _dev(torch, gx)
        tgy = None if gy is None else _dev(torch, gy)
        torch.cuda.synchronize()
        g = self.db.adjoint(tgx, tgy)
        self.db.synchronize()
        return g

    def instance(self, i):
        P, A = self.P.copy(), self.A.copy()
        P.data, A.data = self.Px[i].copy(), self.Ax[i].copy()
        return P, A


def _np(g):
    return {k: getattr(g, k).cpu().numpy() for k in FIELDS + ("act", "ares", "astat")}


def _compare(bt, x, y, gx, gy, g, label, where=None):
    """Largest deviation of the device outputs from the helper over the instances in `where`,
    the helper's residual of the device's (r_x, r_y) per instance, and the class check."""
    worst, hres = 0.0, []
    for i in range(bt.B):
        P, A = bt.instance(i)
        gxi = None if gx is None else gx[i]
        gyi = None if gy is None else gy[i]
        h = ref.adjoint(P, A, bt.l[i], bt.u[i], x[i], y[i], gxi, gyi)
        assert np.array_equal(g["act"][i], h.act), (label, i, np.flatnonzero(g["act"][i] != h.act))
        hres.append(np.atleast_1d(ref.residual(P, A, h.act, g["rx"][i], g["ry"][i], gxi, gyi,
                                               scaling=ref.ruiz_scaling(P, bt.q[i], A))))
        if where is not None and not where[i]:
            continue
        floor = 1e-6 * max(np.abs(getattr(h, k)).max() for k in FIELDS)
        for k in FIELDS:
            d = ref.rel_dev(g[k][i], getattr(h, k), floor)
            if d > 1e-9:
                print(f"{label}[{i}] {k}: deviation {d:.2e} (cond K {h.cond:.1e})")
            worst = max(worst, d)
    print(f"{label}: largest deviation {worst:.3e}")
    return worst, np.array(hres)


def _check_ares(label, ares, hres):
    a, h = np.maximum(ares, RES_FLOOR), np.maximum(hres.reshape(ares.shape), RES_FLOOR)
    print(f"{label}: ares {ares.min():.2e}..{ares.max():.2e}, helper's residual {hres.min():.2e}..{hres.max():.2e}, "
          f"ratio {np.min(a / h):.2e}..{np.max(a / h):.2e}")
    assert np.all(a / h < RES_FACTOR) and np.all(h / a < RES_FACTOR), (label, ares, hres)


# ---------------------------------------------------------------- 1: the demo problem --
def test_demo_problem_through_osqp_adjoint():
    P, q, A, l, u = osqp_demo_problem()[:5]
    d = OSQP()
    d.setup(P, q, A, l, u, polish=True, **TIGHT)
    r = d.solve()
    assert r.info.status == "solved"
    gx, gy = np.array([1.0, -0.5]), np.array([0.25, 3.0, -1.0])
    gP, gq, gA, gl, gu = d.adjoint(gx, gy)
    info = d.adjoint_info
    h = ref.adjoint(P, A, l, u, r.x, r.y, gx, gy)
    assert info.astat == 1 and info.ares < 1e-8
    assert np.array_equal(info.act, h.act) and h.act.tolist() == [3, 0, 2]
    assert gP.shape == (2, 2) and gA.shape == (3, 2)
    Pc, Ac = canonical_data(P, A)
    assert np.array_equal(gP.indices, Pc.indices) and np.array_equal(gA.indices, Ac.indices)
    got = dict(rx=info.rx, ry=info.ry, gq=gq, gl=gl, gu=gu, gPx=gP.data, gAx=gA.data)
    floor = 1e-6 * max(np.abs(getattr(h, k)).max() for k in FIELDS)
    worst = max(ref.rel_dev(got[k], getattr(h, k), floor) for k in FIELDS)
    print(f"demo: largest deviation {worst:.3e}, ares {info.ares:.2e}")
    assert worst < BAR_DEMO
    # one seed alone, and the argument checks that need a handle
    _, _, _, _, gu2 = d.adjoint(gx=gx)
    h2 = ref.adjoint(P, A, l, u, r.x, r.y, gx)
    assert ref.rel_dev(gu2, h2.gu, floor) < BAR_DEMO and ref.rel_dev(d.adjoint_info.rx, h2.rx, floor) < BAR_DEMO
    with pytest.raises(ValueError):
        d.adjoint()
    L, hp = osqp_amd.lib(), d._b._h.ptr
    buf = np.ones(2)
    assert L.mpcqp_adjoint_batch(hp, 0, osqp_amd._dp(buf), *([None] * 11)) == 1   # nrhs < 1
    assert L.mpcqp_adjoint_batch(hp, 1, None, None, *([None] * 10)) == 1          # both seeds NULL
    fresh = OSQP()
    fresh.setup(P, q, A, l, u, **TIGHT)
    with pytest.raises(ValueError, match="no solve"):
        fresh.adjoint(gx=gx)


def test_entries_dropped_from_the_pattern_get_their_gradient():
    """Stored zeros of the user's P and A (dropped from the device pattern, as OSQPBatch.setup
    drops entries zero in every instance) come back in gP / gA on the user's patterns."""
    import scipy.sparse as sp
    P, q, A, l, u = osqp_demo_problem()[:5]
    Pz = sp.csc_matrix((np.array([4.0, 0.0, 2.0]), np.array([0, 0, 1]), np.array([0, 1, 3])), shape=(2, 2))
    Az = sp.csc_matrix((np.array([1.0, 1.0, 0.0, 1.0, 0.0, 1.0]), np.array([0, 1, 2, 0, 1, 2]), np.array([0, 3, 6])),
                       shape=(3, 2))
    assert (Az != A).nnz == 0 and Az.nnz == 6 and Pz.nnz == 3   # (P: the demo's without its coupling)
    u = np.array([1.0, 0.7, 0.6])                                # (x_2 at its bound, as in the demo)
    d = OSQP()
    d.setup(Pz, q, Az, l, u, polish=True, **TIGHT)
    r = d.solve()
    gx, gy = np.array([1.0, -0.5]), np.array([0.25, 3.0, -1.0])
    gP, _, gA, _, _ = d.adjoint(gx, gy)
    assert d.adjoint_info.astat == 1
    h = ref.adjoint(Pz, Az, l, u, r.x, r.y, gx, gy)
    assert gA.nnz == 6 and np.array_equal(gA.indices, Az.indices) and gP.nnz == 3
    floor = 1e-6 * max(np.abs(getattr(h, k)).max() for k in FIELDS)
    assert ref.rel_dev(gA.data, h.gAx, floor) < BAR_DEMO and ref.rel_dev(gP.data, h.gPx, floor) < BAR_DEMO
    assert abs(h.gAx[2]) > 1e-3 and abs(h.gPx[1]) > 1e-3  # stored zeros with a gradient of their own


def test_adjoint_batch_over_shards(monkeypatch):
    """mpcqp_adjoint_batch on a handle cut into shards (MPCQP_SPLIT, read at setup): the same
    bits as on one shard, each shard's slice in its place."""
    b = mpc.make_batch(2, 5)
    rng = np.random.default_rng(5)
    gx, gy = rng.standard_normal((5, 2, b["n"])), rng.standard_normal((5, 2, b["m"]))
    outs = []
    for split in ("1", "2"):
        monkeypatch.setenv("MPCQP_SPLIT", split)
        d = OSQPBatch()
        d.setup(b["P"], b["q"], b["A"], b["l"], b["u"], Px=b["Px"], Ax=b["Ax"], warm_start=True, **TIGHT)
        assert d.plan_info()["n_devices"] == int(split)
        assert (d.solve().status_val == 1).all()
        outs.append(d.adjoint(gx, gy))
    assert (outs[0].astat == 1).all()
    for k in FIELDS + ("act", "ares", "astat"):
        assert np.array_equal(getattr(outs[0], k), getattr(outs[1], k)), k
    one = d.adjoint(gx[:, 1], None)  # a 2-D seed: nrhs = 1, the axis dropped
    assert one.gq.shape == (5, b["n"]) and one.ares.shape == (5,)


# ------------------------------------------------------- 2, 4: cfg 2 through DeviceBatch --
@pytest.fixture(scope="module")
def cfg2(torch):
    b = mpc.make_batch(2, 8)
    bt = _Batch(torch, b["P"], b["A"], b["Px"], b["Ax"], b["q"], b["l"], b["u"], warm_start=True, **TIGHT)
    assert bt.db.plan_info()["nb"] == 4
    x, y, st, it = bt.solve()
    assert (st == 1).all()
    rng = np.random.default_rng(7)
    gx = np.zeros((bt.B, 2, bt.n))
    gx[:, 0, b["u_slice"].start] = 1.0
    gx[:, 1] = rng.standard_normal((bt.B, bt.n))
    gy = np.zeros((bt.B, 2, bt.m))
    gy[:, 1] = rng.standard_normal((bt.B, bt.m))
    return dict(b=b, bt=bt, x=x, y=y, st=st, it=it, gx=gx, gy=gy, u0=b["u_slice"].start)


def test_cfg2_two_seeds_match_the_helper(torch, cfg2):
    bt, x, y, gx, gy = (cfg2[k] for k in ("bt", "x", "y", "gx", "gy"))
    g1 = bt.adjoint(gx, gy)
    g = _np(g1)
    assert g["rx"].shape == (8, 2, bt.n) and g["gAx"].shape == (8, 2, bt.A.nnz) and g["ares"].shape == (8, 2)
    worst, hres = _compare(bt, x, y, gx, gy, g, "cfg2")
    assert (g["astat"] == 1).all() and (g["ares"] < 1e-8).all()
    assert worst < BAR_CFG2
    _check_ares("cfg2", g["ares"], hres)
    # the same call again: identical bits
    g2 = _np(bt.adjoint(gx, gy))
    for k in g:
        assert np.array_equal(g[k], g2[k]), k
    # a following solve: as on a handle that never called adjoint (the factor is marked stale,
    # nothing else is touched)
    b = cfg2["b"]
    other = _Batch(torch, b["P"], b["A"], b["Px"], b["Ax"], b["q"], b["l"], b["u"], warm_start=True, **TIGHT)
    x0, _, st0, it0 = other.solve()
    assert np.array_equal(x0, x) and np.array_equal(it0, cfg2["it"])
    xa, ya, sta, ita = bt.solve()
    xb, yb, stb, itb = other.solve()
    assert np.array_equal(sta, stb) and np.array_equal(ita, itb)
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)


def test_unsolved_instances_get_zeros(torch, cfg2):
    b = cfg2["b"]
    bt = _Batch(torch, b["P"], b["A"], b["Px"], b["Ax"], b["q"], b["l"], b["u"], warm_start=True,
                **dict(TIGHT, max_iter=5))
    _, _, st, _ = bt.solve()
    assert (st != 1).all()
    g = _np(bt.adjoint(cfg2["gx"], cfg2["gy"]))
    assert (g["astat"] == 0).all()
    for k in FIELDS + ("act", "ares"):
        assert not g[k].any(), k


# ------------------------------------------------------------------ 3: long plans --
def _golden_batch(torch, golden, name, B=2, **extra):
    g = golden(name)
    s = dict(json.loads(str(g["settings"])), **TIGHT)
    s.update(extra)
    rep = lambda v: np.tile(np.asarray(v, float), (B, 1))
    P, A = canonical_data(g["P"], g["A"])
    return _Batch(torch, P, A, rep(P.data), rep(A.data), rep(g["q"]), rep(np.maximum(g["l"], -1e30)),
                  rep(np.minimum(g["u"], 1e30)), **s)


# (delta, polish_refine_iter) at which the fixture's adjoint solve reaches astat = 1 on the MI355X
# (DESIGN.md): None = the defaults (1e-6, 3) already do
LONG = {"dyn_ltv_n30.npz": (1e-5, 10), "kin_incr_n40.npz": (1e-4, 30), "kin_ltv_n40.npz": None}


@pytest.mark.parametrize("name", list(LONG))
def test_long_plans_report_their_residual(torch, golden, name):
    """Plans of 8 and 11 blocks (the register-sweep and the 512-thread kernels' plans).  With
    the default delta = 1e-6 and 3 refinement steps the eliminated factorisation is too
    inaccurate on dyn_ltv_n30 and kin_incr_n40 (the device's polish is rejected on both as well,
    where the oracle's LDL' polish is accepted): ares says so and astat is -1; with the larger
    delta of LONG the same call reaches rounding level and matches the helper."""
    bt = _golden_batch(torch, golden, name)
    x, y, st, _ = bt.solve()
    assert (st == 1).all()
    rng = np.random.default_rng(11)
    gx = rng.standard_normal((bt.B, bt.n))
    gy = rng.standard_normal((bt.B, bt.m))

    def check(label):
        g = _np(bt.adjoint(gx, gy))
        assert g["rx"].shape == (bt.B, bt.n) and g["ares"].shape == (bt.B,)
        ok = g["astat"] == 1
        worst, hres = _compare(bt, x, y, gx, gy, g, label, where=ok)
        print(f"{label}: ares {g['ares']}, astat {g['astat']}")
        assert np.isin(g["astat"], (1, -1)).all() and np.array_equal(ok, g["ares"] < 1e-8)
        _check_ares(label, g["ares"], hres)
        assert worst < BAR_LONG
        return g

    g = check(name)
    if name.startswith("kin_incr"):
        bt.db.update_settings(polish_refine_iter=30)  # more refinement steps: the residual does not grow
        g30 = _np(bt.adjoint(gx, gy))
        print(f"{name}: ares with 30 refinement steps {g30['ares']}")
        assert (g30["ares"] <= g["ares"]).all()
    if LONG[name] is None:
        assert (g["astat"] == 1).all()
    else:
        bt.db.update_settings(delta=LONG[name][0], polish_refine_iter=LONG[name][1])
        g2 = check(f"{name} delta {LONG[name][0]:g}, {LONG[name][1]} steps")
        assert (g2["astat"] == 1).all()


# ---------------------------------------------------------------- 5: eliminated plan --
def test_eliminated_plan_replans_and_stays_finite(torch):
    b = mpc.make_batch(3, 4)
    args = (b["P"], b["A"], b["Px"], b["Ax"], b["q"], b["l"], b["u"])
    bt = _Batch(torch, *args, **b["settings"])
    assert bt.db.plan_info()["n_eliminated"] > 0
    x, y, st, _ = bt.solve()
    assert (st == 1).all()
    gx = np.zeros((bt.B, bt.n))
    gx[:, b["u_slice"].start] = 1.0
    g = _np(bt.adjoint(gx, None))
    info = bt.db.plan_info()
    assert info["n_eliminated"] == 0 and info["plan_choice"] == 0
    for k in FIELDS + ("ares",):
        assert np.isfinite(g[k]).all(), k
    assert np.isin(g["astat"], (1, -1)).all()
    print(f"cfg3 (slack layout): astat {g['astat']}, ares {g['ares']}")
    # the classes are the helper's; ares is the helper's residual of what came back
    hres = []
    for i in range(bt.B):
        P, A = bt.instance(i)
        act = ref.row_classes(A, bt.l[i], bt.u[i], x[i], y[i])
        hres.append(ref.residual(P, A, g["act"][i], g["rx"][i], g["ry"][i], gx[i], None,
                                 scaling=ref.ruiz_scaling(P, bt.q[i], A)))
        print(f"cfg3[{i}]: classes differing from the helper's at eps 1e-3: {int((act != g['act'][i]).sum())}")
    _check_ares("cfg3", g["ares"], np.array(hres))
    # a following warm-started solve: as on a handle that is on the plain plan from its setup
    # (set up with polish=True, polish turned off before its first solve)
    other = _Batch(torch, *args, **dict(b["settings"], polish=True))
    other.db.update_settings(polish=False)
    assert other.db.plan_info()["n_eliminated"] == 0
    xo, _, sto, ito = other.solve()
    lb, ub = b["l"].copy(), b["u"].copy()
    lb[:, :5] = ub[:, :5] = b["l"][:, :5] * 0.95
    for t in (bt, other):
        tl, tu = _dev(torch, lb), _dev(torch, ub)
        torch.cuda.synchronize()
        t.db.update(l=tl, u=tu)
        t.db.synchronize()
    xa, _, sta, ita = bt.solve()
    xb, _, stb, itb = other.solve()
    print(f"cfg3 re-solve: iterations {ita} / {itb}, max |dx| {np.abs(xa - xb).max():.2e}")
    assert np.array_equal(sta, stb) and (sta == 1).all()
    same = ita == itb
    assert same.sum() >= bt.B - 1
    # both stopped on eps 1e-3 from warm starts that differ by rounding: equal to far below it
    assert np.abs(xa - xb)[same].max() < 1e-6 * max(1.0, np.abs(xb).max())


# --------------------------------------------------------------------- 6: one-shot --
def test_one_shot_state_is_gone(torch, cfg2):
    b = cfg2["b"]
    bt = _Batch(torch, b["P"], b["A"], b["Px"], b["Ax"], b["q"], b["l"], b["u"], warm_start=True, **TIGHT)
    assert bt.db.one_shot(True) > 0
    torch.cuda.synchronize()
    bt.db.setup_solve(*bt.t)
    bt.db.synchronize()
    with pytest.raises(ValueError, match="one-shot"):
        bt.adjoint(cfg2["gx"], None)


# ---------------------------------------------------------------------- 7: QPLayer --
def test_qp_layer_backward_is_the_adjoint(torch, cfg2):
    from osqp_amd.torch_qp import QPLayer
    b, bt, u0 = cfg2["b"], cfg2["bt"], cfg2["u0"]
    layer = QPLayer(bt.P, bt.A, bt.B, warm_start=True, **TIGHT)
    ins = [_dev(torch, v).requires_grad_(True) for v in (bt.Px, bt.Ax, bt.q, bt.l, bt.u)]
    x, y = layer(*ins)
    assert x.dtype == torch.float64 and np.array_equal(x.detach().cpu().numpy(), cfg2["x"])
    grads = torch.autograd.grad(x[:, u0].sum(), ins)
    assert (layer.astat == 1).all()
    tg = _dev(torch, cfg2["gx"][:, 0])
    torch.cuda.synchronize()
    g = layer.batch.adjoint(tg, None)       # (the layer's own batch: the state backward saw)
    layer.batch.synchronize()
    g = _np(g)
    for t, k in zip(grads, ("gPx", "gAx", "gq", "gl", "gu")):
        assert np.array_equal(t.cpu().numpy(), g[k]), k
    # gradients only for the inputs that require them
    q_only = [v.detach() for v in ins]
    q_only[2].requires_grad_(True)
    x2, _ = layer(*q_only)
    (gq,) = torch.autograd.grad(x2[:, u0].sum(), [q_only[2]])
    assert np.array_equal(gq.cpu().numpy(), g["gq"])
    # a second forward before backward: the first graph's backward raises
    xa, _ = layer(*ins)
    xb, _ = layer(*ins)
    with pytest.raises(RuntimeError, match="another forward"):
        xa[:, u0].sum().backward()
    xb[:, u0].sum().backward()
    assert np.array_equal(ins[2].grad.cpu().numpy(), g["gq"])


def test_qp_layer_refuses_unreliable_gradients(torch, cfg2):
    """Instances that are not solved (max_iter = 5: astat 0) make backward raise; with
    strict=False they get zero gradients."""
    from osqp_amd.torch_qp import QPLayer
    bt, u0 = cfg2["bt"], cfg2["u0"]
    vals = (bt.Px, bt.Ax, bt.q, bt.l, bt.u)
    for strict in (True, False):
        layer = QPLayer(bt.P, bt.A, bt.B, strict=strict, warm_start=True, **dict(TIGHT, max_iter=5))
        ins = [_dev(torch, v).requires_grad_(True) for v in vals]
        x, _ = layer(*ins)
        assert (layer.status != 1).all()
        if strict:
            with pytest.raises(RuntimeError, match="no reliable gradient"):
                x[:, u0].sum().backward()
        else:
            x[:, u0].sum().backward()
            assert (layer.astat == 0).all() and all(not t.grad.any() for t in ins)


# ------------------------------------------------------------------ 8: the MPC gain --
def test_mpc_gain_matches_finite_differences(torch):
    """d du_0 / d theta of the vanilla lateral layout: the adjoint's gq, gl, gu chained through
    the assembler's affine map (q | l | u)(theta), against central differences (h = 1e-3) of
    device solves at eps 1e-9 with polish.  Tolerance 1e-8 / h * 10 = 1e-4 relative to the
    instance's largest derivative (the solves are within 1e-8 of the optimum)."""
    from osqp_amd.mpc_device import LateralAssembler
    b = mpc.make_batch(2, 4)
    asm = LateralAssembler("vanilla", N=b["N"])
    theta = b["theta"]
    B, npar, u0, h = 4, asm.nparam, b["u_slice"].start, 1e-3
    # the map's linear part, exactly: differences of its own evaluation
    E = np.concatenate([np.zeros((1, npar)), np.eye(npar)])
    ev = np.concatenate(asm.map.evaluate(E), axis=1)
    J = (ev[1:] - ev[:1]).T                                   # (n + 2m, nparam)
    # directions: the four states of x0 (the feedback gain) and two dense ones
    rng = np.random.default_rng(3)
    dirs = np.concatenate([np.eye(npar)[:4], rng.standard_normal((2, npar))])
    K = len(dirs)
    th = np.concatenate([theta] + [theta + s * h * d for d in dirs for s in (1.0, -1.0)])   # (B (1 + 2K), npar)
    Bt = th.shape[0]
    Px, Ax = asm.matrices()
    P, A = canonical_data(asm.P, asm.A)
    db = DeviceBatch(P, A, Bt, warm_start=True, polish=True, **TIGHT)
    tth = _dev(torch, th)
    q, l, u = asm.assemble(tth)
    x = torch.empty((Bt, asm.n), dtype=torch.float64, device="cuda:0")
    st = torch.empty(Bt, dtype=torch.int32, device="cuda:0")
    gx = torch.zeros((Bt, asm.n), dtype=torch.float64, device="cuda:0")
    gx[:, u0] = 1.0
    tPx, tAx = _dev(torch, Px), _dev(torch, Ax)
    torch.cuda.synchronize()
    db.setup(tPx, tAx, q, l, u)
    db.solve(x, None, st, None)
    g = db.adjoint(gx, None)
    db.synchronize()
    assert (st.cpu().numpy() == 1).all() and (g.astat[:B].cpu().numpy() == 1).all()
    act = g.act.cpu().numpy().reshape(1 + 2 * K, B, -1)
    du0 = x[:, u0].cpu().numpy().reshape(1 + 2 * K, B)
    grad = np.concatenate([g.gq.cpu().numpy()[:B], g.gl.cpu().numpy()[:B], g.gu.cpu().numpy()[:B]], axis=1) @ J
    used = 0
    for i in range(B):
        if not (act[:, i] == act[0, i]).all():
            print(f"gain[{i}]: the active set changes within the steps, skipped")
            continue
        used += 1
        fd = np.array([(du0[1 + 2 * k, i] - du0[2 + 2 * k, i]) / (2 * h) for k in range(K)])
        an = dirs @ grad[i]
        scale = np.abs(fd).max()
        print(f"gain[{i}]: fd {fd}, adjoint {an}, deviation {np.abs(fd - an).max() / max(scale, 1e-300):.2e}")
        if act[0, i, asm.m - (asm.n - u0)] in (1, 2):   # the input sits at its bound: no gain at all
            assert scale < 1e-9 and np.abs(an).max() < 1e-9  # (rounding of solves that agree to ~1e-13, over h)
            continue
        assert np.abs(fd - an).max() < 1e-4 * scale
    assert used >= B - 1
