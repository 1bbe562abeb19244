"""The MPC-step VJPs on the device (include/mpcqp.h): each entry point against its
numpy restatement, the assembly with weights per call, the torch functions of osqp_amd.torch_mpc
against the VJP methods they wrap, and MPCLayer end to end against the CPU chain of
tests/test_mpc_vjp_ref.py and central differences of device solves.

Copies and negations (gAd, gBd, ggd, gx0, gxlo, gxhi) are held bit for bit -- the incremental
layout's gBd is one addition, the same one in numpy.  The summed outputs are held to ten times the
deviation measured on the MI355X, max |a - b| / max |b| per output array (DESIGN.md §15 has the
table): BAR_SUM for gXr, gQ, gQN, gR and gtheta, BAR_LIN for the linearisation's VJP, BAR_CHAIN for
MPCLayer's gradients against the CPU chain at the device's own solution.
"""
import numpy as np
import pytest

import test_mpc_vjp_ref as cpu
from osqp_amd import mpc

pytestmark = pytest.mark.gpu

BAR_SUM = 2.4e-15          # measured: gXr 2.0e-16, gQ 2.34e-16, gQN 0, gR 0, gtheta 1.72e-16
BAR_LIN = 3.7e-15          # measured: 3.69e-16
BAR_CHAIN = 5.4e-14        # measured: x0 <= 5.4e-15 (ltv N=5), diag Q <= 9.7e-16
# measured 0 (the same products in the same order); ten times the spacing of doubles, which is the
# rounding of the host's own matrix product that stands as the reference here
BAR_AFFINE_GAIN = 10 * 2.2e-16
# the adjoint's linear solve on the incremental layout at N = 3: at the default
# delta 1e-6 and 3 refinement steps ares is 9e-11 .. 8.8e-9 on the interior case and 1.85e-8 on
# three of the five active-set instances (astat -1); §14's setting for kin_incr_n40 is taken
INCR_ADJOINT = dict(delta=1e-4, polish_refine_iter=30)
SENTINEL = 1234.5
GUARD = 64
TIGHT = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=100000, verbose=False, polish=True)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def _dev(torch, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).to("cuda:0").contiguous()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


class Arena:
    """Output buffers with a guard of sentinels on either side of each."""

    def __init__(self, torch, shapes):
        self.torch, self.full, self.view = torch, {}, {}
        for k, shape in shapes.items():
            n = int(np.prod(shape))
            self.full[k] = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda:0")
            self.view[k] = self.full[k][GUARD:GUARD + n].view(shape)

    def guards_intact(self):
        return all(bool((f[:GUARD] == SENTINEL).all()) and bool((f[-GUARD:] == SENTINEL).all())
                   for f in self.full.values())

    def untouched(self, k):
        return bool((self.full[k] == SENTINEL).all())


def make_layout(kind, name, N, rng):
    from osqp_amd.mpc_device import IncrementalLayout, LTVLayout
    nx, nu, mA, mB = cpu.LAYOUTS[name]
    Q, QN, R = cpu.sym_weights(rng, nx, nu)
    if kind == "ltv":
        lay = LTVLayout(N, Q, QN, R, -np.ones(nx), np.ones(nx), -np.ones(nu), np.ones(nu), mA, mB)
    else:
        lay = IncrementalLayout(N, Q, QN, R, -np.ones(nx + nu), np.ones(nx + nu), -np.ones(nu), np.ones(nu),
                                maskA=mA, maskB=mB)
    return lay, (Q, QN, R), (nx, nu, mA, mB)


def random_inputs(rng, lay, B, mA, mB):
    N, nx, nu, nxa = lay.N, lay.nx, lay.nu, lay.nxa
    d = dict(Ad=rng.standard_normal((B, N, nx, nx)) * mA, Bd=rng.standard_normal((B, N, nx, nu)) * mB,
             gd=rng.standard_normal((B, N, nx)), x0=rng.standard_normal((B, nxa)),
             Xr=rng.standard_normal((B, nx, N + 1)))
    if lay._kind == "ltv":
        xlo, xhi = -1 - rng.uniform(0, 1, (B, N + 1, nx)), 1 + rng.uniform(0, 1, (B, N + 1, nx))
        xlo[:, 0, 0], xhi[:, 1, 0], xhi[-1, N, nx - 1] = -np.inf, np.inf, 2e30
        d.update(xlo=xlo, xhi=xhi)
    return d


MEASURED = {}


def _measure(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), value)
    print(f"measured {key}: {value:.3e} (largest so far {MEASURED[key]:.3e})")


# ----------------------------------------------------------------------- kernels alone --
@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", list(cpu.LAYOUTS))
@pytest.mark.parametrize("kind", ["ltv", "incr"])
def test_assembly_vjp_matches_the_host_statement(torch, kind, name, N, B):
    rng = np.random.default_rng(11 + N + B)
    lay, (Q, QN, R), (nx, nu, mA, mB) = make_layout(kind, name, N, rng)
    P, A, _, _ = lay.pattern()
    d = random_inputs(rng, lay, B, mA, mB)
    cot = dict(gPx=rng.standard_normal((B, lay.nnzP)), gAx=rng.standard_normal((B, lay.nnzA)),
               gq=rng.standard_normal((B, lay.n)), gl=rng.standard_normal((B, lay.m)),
               gu=rng.standard_normal((B, lay.m)))
    fwd = dict(Xr=d["Xr"]) if kind == "incr" else dict(Xr=d["Xr"], xlo=d["xlo"], xhi=d["xhi"])
    fn = mpc.ltv_qp_vjp if kind == "ltv" else mpc.incremental_qp_vjp
    want = fn(P, A, N, nx, nu, Q, QN, **fwd, **cot)
    names = [k for k in lay.VJP_OUTPUTS if kind == "ltv" or k not in ("gxlo", "gxhi")]
    shapes = {k: getattr(want, k).shape for k in names}
    tc = {k: _dev(torch, v) for k, v in cot.items()}
    tf = {k: _dev(torch, v) for k, v in fwd.items()}
    arena = Arena(torch, shapes)
    g = lay.assemble_vjp(**tc, **tf, want=names, out=arena.view)
    torch.cuda.synchronize()
    got = {k: getattr(g, k).cpu().numpy() for k in names}
    assert arena.guards_intact()
    for k in names:
        w = getattr(want, k)
        if k in ("gXr", "gQ", "gQN", "gR"):
            dev = _rel(got[k], w)
            _measure(f"assembly {k}", dev)
            assert dev < BAR_SUM, (k, dev)
        else:
            assert _bits(got[k], w), k
    assert not got["gAd"][:, :, mA == 0].any() and not got["gBd"][:, :, mB == 0].any()
    # two identical calls return identical bits
    arena2 = Arena(torch, shapes)
    lay.assemble_vjp(**tc, **tf, want=names, out=arena2.view)
    torch.cuda.synchronize()
    for k in names:
        assert _bits(arena2.view[k].cpu().numpy(), got[k]), k
    # an output that is not wanted is NULL and is not written; the others do not change
    some = ["gBd", "gXr", "gQN"]
    arena3 = Arena(torch, shapes)
    lay.assemble_vjp(**tc, **tf, want=some, out={k: arena3.view[k] for k in some})
    torch.cuda.synchronize()
    assert arena3.guards_intact()
    for k in names:
        if k in some:
            assert _bits(arena3.view[k].cpu().numpy(), got[k]), k
        else:
            assert arena3.untouched(k), k
    # NULL cotangents are zeros
    g0 = lay.assemble_vjp(gq=tc["gq"], Xr=tf["Xr"], want=["gAd", "ggd", "gXr", "gR"])
    torch.cuda.synchronize()
    assert not g0.gAd.any() and not g0.ggd.any() and not g0.gR.any()
    assert _bits(g0.gXr.cpu().numpy(), got["gXr"])


def test_incremental_gbd_takes_each_slot(torch):
    """A cotangent on one of Bd_k's two slots alone arrives alone."""
    rng = np.random.default_rng(3)
    lay, (Q, QN, R), (nx, nu, mA, mB) = make_layout("incr", "kin", 2, rng)
    P, A, _, _ = lay.pattern()
    gAx = np.zeros((2, lay.nnzA))
    i, j = np.argwhere(mB != 0)[0]
    nxa, ns = nx + nu, 3 * (nx + nu)
    s_aug = mpc._slots(A, [nxa + i], [nx + j])[0]
    s_b = mpc._slots(A, [nxa + i], [ns + j])[0]
    gAx[0, s_aug], gAx[1, s_b] = 2.0, 3.0
    g = lay.assemble_vjp(gAx=_dev(torch, gAx), want=["gBd"])
    torch.cuda.synchronize()
    want = np.zeros((2, 2, nx, nu))
    want[0, 0, i, j], want[1, 0, i, j] = 2.0, 3.0
    assert np.array_equal(g.gBd.cpu().numpy(), want)


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("layout,N", [("vanilla", 3), ("slack", 4)])
def test_affine_vjp_matches_the_host_statement(torch, layout, N, B):
    from osqp_amd.mpc_device import LateralAssembler
    asm = LateralAssembler(layout, N=N)
    rng = np.random.default_rng(B)
    g = [rng.standard_normal((B, w)) for w in (asm.n, asm.m, asm.m)]
    want = asm.map.vjp(*g)
    tg = [_dev(torch, v) for v in g]
    wide = torch.full((B, asm.nparam + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    got = asm.assemble_vjp(*tg, out=wide)
    again = asm.assemble_vjp(*tg)
    only_q = asm.assemble_vjp(tg[0], None, None)
    torch.cuda.synchronize()
    assert bool((wide[:, asm.nparam:] == SENTINEL).all())
    dev = _rel(got[:, :asm.nparam].cpu().numpy(), want)
    _measure("affine gtheta", dev)
    assert dev < BAR_SUM
    assert _bits(again.cpu().numpy(), got[:, :asm.nparam].cpu().numpy())
    assert _rel(only_q.cpu().numpy(), asm.map.vjp(g[0], None, None)) < BAR_SUM


@pytest.mark.parametrize("B", [1, 130])
def test_kin_linearise_vjp_matches_the_host_statement(torch, B):
    from osqp_amd.mpc_device import KinVehicle, linearise_kinematics_vjp
    veh, N = KinVehicle(), 3
    rng = np.random.default_rng(20 + B)
    x = np.stack([rng.standard_normal((B, N)), rng.standard_normal((B, N)), rng.uniform(2, 12, (B, N)),
                  rng.uniform(-1, 1, (B, N))], -1)
    u = np.stack([rng.uniform(-0.25, 0.25, (B, N)), rng.uniform(-1, 1, (B, N))], -1)
    cots = [rng.standard_normal((B, N, 4, 4)), rng.standard_normal((B, N, 4, 2)), rng.standard_normal((B, N, 4))]
    wx, wu = mpc.linearise_kinematics_vjp(veh.l_f, veh.l_r, veh.dt, x, u, *cots)
    tx, tu, tc = _dev(torch, x), _dev(torch, u), [_dev(torch, c) for c in cots]
    gx, gu = linearise_kinematics_vjp(veh, tx, tu, *tc)
    gx2, gu2 = linearise_kinematics_vjp(veh, tx, tu, *tc)
    torch.cuda.synchronize()
    gx, gu = gx.cpu().numpy(), gu.cpu().numpy()
    assert not gx[..., :2].any() and not gu[..., 1].any()
    dev = max(_rel(gx, wx), _rel(gu, wu))
    _measure("linearise vjp", dev)
    assert dev < BAR_LIN
    assert _bits(gx2.cpu().numpy(), gx) and _bits(gu2.cpu().numpy(), gu)
    # one (x, u) for every stage (stage stride 0): the outputs stay dense, per stage
    xs, us = tx[:, :1].expand(B, N, 4), tu[:, :1].expand(B, N, 2)
    sx, su = linearise_kinematics_vjp(veh, xs, us, *tc)
    torch.cuda.synchronize()
    ex, eu = mpc.linearise_kinematics_vjp(veh.l_f, veh.l_r, veh.dt, np.repeat(x[:, :1], N, 1),
                                          np.repeat(u[:, :1], N, 1), *cots)
    assert sx.shape == (B, N, 4) and max(_rel(sx.cpu().numpy(), ex), _rel(su.cpu().numpy(), eu)) < BAR_LIN


# ---------------------------------------------------------------- weights per call --
@pytest.mark.parametrize("kind", ["ltv", "incr"])
def test_assemble_with_weights(torch, kind):
    from osqp_amd.mpc_device import IncrementalLayout, LTVLayout
    rng = np.random.default_rng(31)
    N, B = 3, 130
    lay, (Q, QN, R), (nx, nu, mA, mB) = make_layout(kind, "kin", N, rng)
    d = random_inputs(rng, lay, B, mA, mB)
    ins = [_dev(torch, d[k]) for k in ("Ad", "Bd", "gd", "x0", "Xr")]
    kw = dict(xlo=_dev(torch, d["xlo"]), xhi=_dev(torch, d["xhi"])) if kind == "ltv" else {}
    plain = lay.assemble(*ins, **kw)
    null = lay.assemble(*ins, **kw, weights=(None, None, None))
    own = lay.assemble(*ins, **kw, weights=tuple(_dev(torch, W) for W in (Q, QN, R)))
    torch.cuda.synchronize()
    P, A, _, _ = lay.pattern()
    for out in (null, own):
        for a, b in zip(out[:4], plain):
            assert _bits(a.cpu().numpy(), b.cpu().numpy())
        assert _bits(out[4].cpu().numpy(), P.data)
    # other weights of the same pattern, one stored entry now zero: it stays as an explicit zero
    Q2, QN2, R2 = cpu.sym_weights(rng, nx, nu)
    Q2[0, 1] = Q2[1, 0] = 0.0
    other = lay.assemble(*ins, **kw, weights=tuple(_dev(torch, W) for W in (Q2, QN2, R2)))
    # against a layout created with those weights (its q, bit for bit; its P drops the zero) ...
    Q2c = Q2.copy()
    if kind == "ltv":
        lay2 = LTVLayout(N, Q2c, QN2, R2, -np.ones(nx), np.ones(nx), -np.ones(nu), np.ones(nu), mA, mB)
    else:
        lay2 = IncrementalLayout(N, Q2c, QN2, R2, -np.ones(nx + nu), np.ones(nx + nu), -np.ones(nu), np.ones(nu),
                                 maskA=mA, maskB=mB)
    plain2 = lay2.assemble(*ins, **kw)
    torch.cuda.synchronize()
    for a, b in zip(other[:4], plain2):
        assert _bits(a.cpu().numpy(), b.cpu().numpy())
    # ... and against the host builder on the stored pattern
    nxa = lay.nxa
    Wfull = [np.zeros((nxa, nxa)) for _ in range(2)]
    Wfull[0][:nx, :nx], Wfull[1][:nx, :nx] = Q2, QN2
    import scipy.sparse as sp
    Pd = sp.block_diag([sp.kron(sp.eye(N), Wfull[0]), Wfull[1], sp.kron(sp.eye(N), R2)]).toarray()
    rows, cols = P.indices, np.repeat(np.arange(lay.n), np.diff(P.indptr))
    Px = other[4].cpu().numpy()
    assert _bits(Px, Pd[rows, cols]) and (Px == 0).sum() == N
    b = 7
    if kind == "ltv":
        _, qh, _, _, _ = mpc.ltv_qp(list(d["Ad"][b]), list(d["Bd"][b]), list(d["gd"][b]), d["x0"][b], d["Xr"][b], Q2,
                                    QN2, R2, N, -np.ones(nx), np.ones(nx), -np.ones(nu), np.ones(nu))
    else:
        _, qh, _, _, _ = mpc.incremental_qp(list(d["Ad"][b]), list(d["Bd"][b]), list(d["gd"][b]), d["x0"][b],
                                            d["Xr"][b], Q2, QN2, R2, N, -np.ones(nxa), np.ones(nxa), -np.ones(nu),
                                            np.ones(nu))
    assert np.allclose(other[1][b].cpu().numpy(), qh, rtol=0, atol=1e-13 * np.abs(qh).max())


# ----------------------------------------------------------------------------- torch --
def test_torch_functions_are_wired_to_the_vjps(torch):
    """One contraction per function of torch_mpc: backward returns what the VJP method returns."""
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import KinVehicle, LateralAssembler, linearise_kinematics_vjp
    rng = np.random.default_rng(41)
    B, N = 5, 3

    def leaf(a):
        return _dev(torch, a).requires_grad_(True)

    # linearise_kinematics, and a stride-0 expand over the stages: the stage sum
    veh = KinVehicle()
    x = np.concatenate([rng.standard_normal((B, 2)), rng.uniform(2, 12, (B, 1)), rng.uniform(-1, 1, (B, 1))], 1)
    u = np.stack([rng.uniform(-0.25, 0.25, B), rng.uniform(-1, 1, B)], 1)
    tx, tu = leaf(x), leaf(u)
    outs = tm.linearise_kinematics(veh, tx[:, None, :].expand(B, N, 4), tu[:, None, :].expand(B, N, 2))
    cots = [_dev(torch, rng.standard_normal(tuple(o.shape))) for o in outs]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    gx, gu = linearise_kinematics_vjp(veh, tx.detach()[:, None, :].expand(B, N, 4),
                                      tu.detach()[:, None, :].expand(B, N, 2), *cots)
    assert torch.allclose(tx.grad, gx.sum(1), rtol=1e-14, atol=0) and torch.allclose(tu.grad, gu.sum(1), rtol=1e-14,
                                                                                      atol=0)
    # the assembly of both layouts, weights included
    for kind in ("ltv", "incr"):
        lay, (Q, QN, R), (nx, nu, mA, mB) = make_layout(kind, "kin", N, rng)
        d = random_inputs(rng, lay, B, mA, mB)
        ins = [leaf(d[k]) for k in ("Ad", "Bd", "gd", "x0", "Xr")]
        w = [leaf(W) for W in (Q, QN, R)]
        if kind == "ltv":
            bounds = [leaf(np.clip(d["xlo"], -1e30, 1e30)), leaf(np.clip(d["xhi"], -1e30, 1e30))]
            outs = tm.ltv_assemble(lay, *ins, *bounds, weights=tuple(w))
        else:
            bounds = []
            outs = tm.incr_assemble(lay, *ins, weights=tuple(w))
        assert len(outs) == 5 and tuple(outs[4].shape) == (lay.nnzP,)
        cots = [_dev(torch, rng.standard_normal(tuple(o.shape))) for o in outs]
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        gP = torch.zeros((B, lay.nnzP), dtype=torch.float64, device="cuda:0")
        gP[0] = cots[4]
        kw = dict(xlo=bounds[0].detach(), xhi=bounds[1].detach()) if bounds else {}
        g = lay.assemble_vjp(cots[0], cots[1], cots[2], cots[3], gPx=gP, Xr=ins[4].detach(),
                             weights=(w[0].detach(), w[1].detach(), None), **kw)
        pairs = list(zip(ins, (g.gAd, g.gBd, g.ggd, g.gx0, g.gXr))) + list(zip(bounds, (g.gxlo, g.gxhi)))
        for t, want in pairs:
            assert torch.equal(t.grad, want)
        for t, want in zip(w, (g.gQ, g.gQN, g.gR)):
            assert torch.equal(t.grad, want.sum(0))
        # gradients only for the inputs that require them; the plain call has four outputs
        only = [v.detach() for v in ins]
        only[3].requires_grad_(True)
        outs = (tm.ltv_assemble if kind == "ltv" else tm.incr_assemble)(lay, *only)
        assert len(outs) == 4
        (gx0,) = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), [only[3]])
        assert torch.equal(gx0, g.gx0)
    # the affine assembler
    asm = LateralAssembler("vanilla", N=N)
    theta = leaf(rng.standard_normal((B, asm.nparam)))
    outs = tm.affine_assemble(asm, theta)
    cots = [_dev(torch, rng.standard_normal(tuple(o.shape))) for o in outs]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    assert torch.equal(theta.grad, asm.assemble_vjp(*cots))


# ----------------------------------------------------------------------- end to end --
PERT = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, -0.5, 0.7, 0.3], [-0.6, 1.0, -1.0, 0.5], [0.4, 0.8, 0.9, -1.0],
                 [-1.0, -0.9, 0.2, -0.7]])
E2E = {
    # kind, N, x0, u0, the entry of U_0 that is the loss, the scale of PERT, solver settings
    "ltv N=2": ("ltv", 2, cpu.X0_LTV, cpu.U0_LTV, 0, 1e-2, {}),
    "ltv N=3": ("ltv", 3, cpu.X0_LTV, cpu.U0_LTV, 0, 1e-2, {}),
    "ltv N=5": ("ltv", 5, cpu.X0_LTV, cpu.U0_LTV, 0, 1e-2, {}),
    "incr interior": ("incr", 3, cpu.INCR_CASES["interior steer"][0], cpu.INCR_CASES["interior steer"][1], 0, 1e-4,
                      INCR_ADJOINT),
    "incr active": ("incr", 3, cpu.INCR_CASES["active accel"][0], cpu.INCR_CASES["active accel"][1], 1, 1e-3,
                    INCR_ADJOINT),
}


def _mpc_layout(kind, N):
    from osqp_amd.mpc_device import IncrementalLayout, LTVLayout
    if kind == "ltv":
        return LTVLayout(N, mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R, mpc.KINLTV_XMIN, mpc.KINLTV_XMAX,
                         mpc.KINLTV_UMIN, mpc.KINLTV_UMAX, mpc.KIN_MASK_A, mpc.KIN_MASK_B), mpc.KINLTV_Q
    return IncrementalLayout(N, mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, mpc.KIN_XMIN_T, mpc.KIN_XMAX_T, mpc.KIN_DUMIN,
                             -mpc.KIN_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B), mpc.KIN_Q


@pytest.mark.parametrize("case", list(E2E))
def test_mpc_layer_end_to_end(torch, case):
    """MPCLayer on B = 5 states (the base point and four deterministic perturbations): the loss
    U[:, 0, j].sum() backward to x0 -- through linearise_kinematics expanded to every stage -- and to
    the diagonal of Q, against the CPU chain at the device's own solution (BAR_CHAIN) and, for x0,
    loosely against central differences of device solves by the rule of
    test_mpc_gain_matches_finite_differences: h = 1e-3, 1e-8 / h * 10 = 1e-4 of the instance's
    largest derivative.  (The weights' derivatives are ~1e-6, below what that rule resolves: they
    are held to the CPU chain alone, which tests/test_mpc_vjp_ref.py differences on the oracle.)"""
    from osqp_amd import torch_mpc as tm
    from osqp_amd.mpc_device import KinVehicle
    kind, N, x0b, u0, j, scale, extra = E2E[case]
    B, h = len(PERT), 1e-3
    veh = KinVehicle()
    assert (veh.l_f, veh.l_r, veh.dt) == (cpu.LF, cpu.LR, cpu.DT)
    lay, Qw = _mpc_layout(kind, N)
    x0s = x0b + scale * PERT
    Xr = np.tile(cpu.ltv_reference(N), (B, 1, 1))
    settings = dict(TIGHT, warm_start=True, **extra)

    def forward(layer, x0_np, qdiag=None, grad=False):
        Bn = x0_np.shape[0]
        tx = _dev(torch, x0_np).requires_grad_(grad)
        tu = _dev(torch, np.tile(u0, (Bn, 1)))
        Ad, Bd, gd = tm.linearise_kinematics(veh, tx[:, None, :].expand(Bn, N, 4), tu[:, None, :].expand(Bn, N, 2))
        start = tx if kind == "ltv" else torch.cat([tx, tu], dim=1)
        weights = None
        if qdiag is not None:
            weights = (torch.diag(qdiag), None, None)
        X, U, y = layer(Ad, Bd, gd, start, _dev(torch, Xr[:1].repeat(Bn, 0)), weights=weights)
        return tx, X, U, y

    layer = tm.MPCLayer(lay, B, strict=False, **settings)   # (astat is asserted below, after it is printed)
    qdiag = _dev(torch, np.diag(Qw)).requires_grad_(True)
    tx, X, U, y = forward(layer, x0s, qdiag, grad=True)
    U[:, 0, j].sum().backward()
    torch.cuda.synchronize()
    print(f"{case}: status {layer.status.tolist()} iters {layer.iters.tolist()} astat {layer.astat.tolist()} "
          f"ares {layer.ares.flatten().tolist()}")
    assert (layer.status == 1).all() and (layer.astat == 1).all()
    gx0, gq = tx.grad.cpu().numpy(), qdiag.grad.cpu().numpy()
    xs = torch.cat([X.reshape(B, -1), U.reshape(B, -1)], dim=1).detach().cpu().numpy()
    ys = y.detach().cpu().numpy()
    seed_index = (N + 1) * lay.nxa + j
    seed = np.zeros(lay.n)
    seed[seed_index] = 1.0
    totals, gQs, acts = [], [], []
    for b in range(B):
        P, q, A, l, u, _ = cpu.chain_problem(kind, N, x0s[b], u0)
        a, frozen, total, gQ = cpu.chain_gradients(kind, N, x0s[b], u0, P, A, l, u, xs[b], ys[b], seed, Qw)
        totals.append(total); gQs.append(np.diag(gQ)); acts.append(a.act)
    totals, gQsum = np.array(totals), np.sum(gQs, axis=0)
    dev_x = max(_rel(gx0[b], totals[b]) for b in range(B))
    dev_q = _rel(gq, gQsum)
    print(f"{case}: d U0[{j}] / d x0 [0] device {gx0[0]} chain {totals[0]}\n{case}: d loss / d diag Q device {gq} "
          f"chain {gQsum}")
    _measure(f"e2e {case} x0", dev_x)
    _measure(f"e2e {case} Q", dev_q)
    assert dev_x < BAR_CHAIN and dev_q < BAR_CHAIN
    if kind == "incr":
        rows = 2 * (N + 1) * 6 + 2 * np.arange(N)
        on = np.isin(acts[0][rows], (1, 2)).any()
        assert on == (case == "incr active")
    # central differences of device solves in x0, every instance, classes equal at every point
    pts = np.concatenate([x0s[b] + s * h * e for b in range(B) for e in np.eye(4) for s in (1.0, -1.0)]
                         ).reshape(-1, 4)
    fdl = tm.MPCLayer(lay, len(pts), **settings)
    _, Xf, Uf, _ = forward(fdl, pts)
    gxf = torch.zeros((len(pts), lay.n), dtype=torch.float64, device="cuda:0")
    gxf[:, seed_index] = 1.0
    torch.cuda.synchronize()
    gf = fdl.qp.batch.adjoint(gxf, None)
    fdl.qp.batch.synchronize()
    assert (fdl.status == 1).all()
    actf = gf.act.cpu().numpy().reshape(B, 8, -1)
    base = layer.qp.batch.adjoint(gxf[:B].contiguous(), None)
    layer.qp.batch.synchronize()
    act0 = base.act.cpu().numpy()
    val = Uf[:, 0, j].detach().cpu().numpy().reshape(B, 4, 2)
    for b in range(B):
        assert (actf[b] == act0[b]).all(), f"{case}[{b}]: the active set changes within the steps"
        fd = (val[b, :, 0] - val[b, :, 1]) / (2 * h)
        sc = np.abs(fd).max()
        print(f"{case}[{b}]: fd {fd} backward {gx0[b]} deviation {np.abs(fd - gx0[b]).max() / sc:.2e}")
        assert np.abs(fd - gx0[b]).max() < 1e-4 * sc


def test_affine_gain_through_assemble_vjp(torch):
    """The vanilla-lateral gain of test_mpc_gain_matches_finite_differences with
    LateralAssembler.assemble_vjp in place of the host Jacobian: the same product, to rounding."""
    from osqp_amd import DeviceBatch, canonical_data
    from osqp_amd.mpc_device import LateralAssembler
    b = mpc.make_batch(2, 4)
    asm = LateralAssembler("vanilla", N=b["N"])
    B, npar, u0 = 4, asm.nparam, b["u_slice"].start
    E = np.concatenate([np.zeros((1, npar)), np.eye(npar)])
    ev = np.concatenate(asm.map.evaluate(E), axis=1)
    J = (ev[1:] - ev[:1]).T
    Px, Ax = asm.matrices()
    P, A = canonical_data(asm.P, asm.A)
    db = DeviceBatch(P, A, B, warm_start=True, **TIGHT)
    q, l, u = asm.assemble(_dev(torch, b["theta"]))
    x = torch.empty((B, asm.n), dtype=torch.float64, device="cuda:0")
    st = torch.empty(B, dtype=torch.int32, device="cuda:0")
    gx = torch.zeros((B, asm.n), dtype=torch.float64, device="cuda:0")
    gx[:, u0] = 1.0
    tPx, tAx = _dev(torch, Px), _dev(torch, Ax)
    torch.cuda.synchronize()
    db.setup(tPx, tAx, q, l, u)
    db.solve(x, None, st, None)
    g = db.adjoint(gx, None)
    db.synchronize()
    assert (st == 1).all() and (g.astat == 1).all()
    got = asm.assemble_vjp(g.gq, g.gl, g.gu).cpu().numpy()
    host = np.concatenate([g.gq.cpu().numpy(), g.gl.cpu().numpy(), g.gu.cpu().numpy()], axis=1) @ J
    dev = _rel(got, host)
    _measure("affine gain", dev)
    assert dev < BAR_AFFINE_GAIN
