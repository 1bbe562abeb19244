"""torch_mpc -- the MPC step as differentiable torch functions.

Between the quantities an MPC user holds (the state x0, the reference Xr, the weights Q, QN, R, the
linearised model Ad, Bd, gd and the point (x, u) it was linearised at) and the solution of the QP
sit the device kernels of mpc_device (linearisation, assembly) and the batched solve.  Each piece
here is a ``torch.autograd.Function`` over one forward entry point and its VJP (include/mpcqp.h,
DESIGN.md §15):

  linearise_kinematics(veh, x, u)                       -> Ad, Bd, gd
  linearise_dynamics(veh, x, u)                         -> Ad, Bd, gd
  ltv_assemble(layout, Ad, Bd, gd, x0, Xr, ...)         -> Ax, q, l, u [, Px]
  incr_assemble(layout, Ad, Bd, gd, xt0, Xr, ...)       -> Ax, q, l, u [, Px]
  affine_assemble(assembler, theta, regime)             -> q, l, u

and ``MPCLayer`` composes the assembly with one ``QPLayer``: (Ad, Bd, gd, x0, Xr[, weights]) ->
(X, U, y), so that d u_0 / d x0 and d loss / d Q are one backward call on the device.  Every call
runs on torch's current stream (the QP solve on the layer's own, ordered with it, as QPLayer does).
Gradients are formed only for the inputs that require them.

With ``linearise_dynamics`` the closed loop of mpc_dynamics.main is differentiable end to end: its
plant step is Ad_0 x + Bd_0 u + gd_0 and its shift copies stages of the solution, both plain torch
operations between one MPCLayer per control step.
"""
from __future__ import annotations

from . import mpc_device as md
from .torch_qp import QPLayer

__all__ = ["linearise_kinematics", "linearise_dynamics", "ltv_assemble", "incr_assemble", "affine_assemble", "MPCLayer"]

_FN = None


def _c(t):
    return None if t is None else t.detach().contiguous()


def _functions():
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from types import SimpleNamespace

    class Linearise(torch.autograd.Function):
        """inputs (model, veh, x, u); model = (forward, vjp) of mpc_device"""

        @staticmethod
        def forward(ctx, model, veh, x, u):
            ctx.vjp, ctx.veh = model[1], veh
            ctx.save_for_backward(x, u)
            ctx.set_materialize_grads(False)
            return model[0](veh, x.detach(), u.detach())

        @staticmethod
        def backward(ctx, gAd, gBd, ggd):
            x, u = ctx.saved_tensors
            if gAd is None and gBd is None and ggd is None:
                return None, None, None, None
            gx, gu = ctx.vjp(ctx.veh, x.detach(), u.detach(), _c(gAd), _c(gBd), _c(ggd))
            need = ctx.needs_input_grad
            return None, None, gx if need[2] else None, gu if need[3] else None

    class Assemble(torch.autograd.Function):
        """inputs (layout, Ad, Bd, gd, x0, Xr, xlo, xhi, Q, QN, R, use_w)"""
        NAMES = ("gAd", "gBd", "ggd", "gx0", "gXr", "gxlo", "gxhi", "gQ", "gQN", "gR")

        @staticmethod
        def forward(ctx, layout, Ad, Bd, gd, x0, Xr, xlo, xhi, Q, QN, R, use_w):
            ins = [_c(t) for t in (Ad, Bd, gd, x0, Xr)]
            xlo, xhi, Q, QN, R = (_c(t) for t in (xlo, xhi, Q, QN, R))
            kw = dict(xlo=xlo, xhi=xhi) if layout._kind == "ltv" else {}
            if use_w:
                kw["weights"] = (Q, QN, R)
            ctx.layout, ctx.use_w = layout, use_w
            ctx.save_for_backward(ins[4], *(t if t is not None else ins[4].new_empty(0) for t in (xlo, xhi, Q, QN)))
            ctx.set_materialize_grads(False)
            return layout.assemble(*ins, **kw)

        @staticmethod
        def backward(ctx, gAx, gq, gl, gu, gPx=None):
            layout = ctx.layout
            Xr, xlo, xhi, Q, QN = (t if t.numel() else None for t in ctx.saved_tensors)
            need = ctx.needs_input_grad[1:11]
            want = [k for k, n in zip(Assemble.NAMES, need) if n]
            cots = [_c(t) for t in (gAx, gq, gl, gu)]
            if not want or (all(t is None for t in cots) and gPx is None):
                return (None,) * 12
            B = Xr.shape[0]
            gP = None
            if gPx is not None:  # one Px for the batch: its cotangent rides on instance 0, gQ is summed below
                gP = gPx.new_zeros((B, layout.nnzP))
                gP[0] = gPx
            g = layout.assemble_vjp(cots[0], cots[1], cots[2], cots[3], gPx=gP, Xr=Xr, xlo=xlo, xhi=xhi,
                                    weights=(Q, QN, None) if ctx.use_w else None, want=want)
            out = [getattr(g, k) for k in Assemble.NAMES]
            for i in (7, 8, 9):  # the weights are shared by the batch
                if out[i] is not None:
                    out[i] = out[i].sum(0)
            return (None, *out, None)

    class Affine(torch.autograd.Function):
        @staticmethod
        def forward(ctx, assembler, theta, regime):
            ctx.assembler, ctx.regime = assembler, regime
            ctx.shape = theta.shape
            ctx.set_materialize_grads(False)
            return tuple(assembler.assemble(theta.detach(), regime))

        @staticmethod
        def backward(ctx, gq, gl, gu):
            if not ctx.needs_input_grad[1] or (gq is None and gl is None and gu is None):
                return None, None, None
            a = ctx.assembler
            gt = a.assemble_vjp(_c(gq), _c(gl), _c(gu), ctx.regime)
            if ctx.shape[1] > a.nparam:  # columns of theta the map does not read
                gt = torch.cat([gt, gt.new_zeros((ctx.shape[0], ctx.shape[1] - a.nparam))], dim=1)
            return None, gt, None

    _FN = SimpleNamespace(Linearise=Linearise, Assemble=Assemble, Affine=Affine)
    return _FN


def linearise_kinematics(veh, x, u):
    """mpc_device.linearise_kinematics, differentiable in x and u (3-D (B, N, 4) / (B, N, 2), any
    strides with a contiguous last axis: an ``expand`` over the stages gets the stage sum)."""
    return _functions().Linearise.apply((md.linearise_kinematics, md.linearise_kinematics_vjp), veh, x, u)


def linearise_dynamics(veh, x, u):
    """mpc_device.linearise (the dynamic bicycle: Pacejka tyres, the low-speed guard), differentiable
    in x and u (3-D (B, N, 6) / (B, N, 2) or 2-D, any strides with a contiguous last axis: an
    ``expand`` over the stages gets the stage sum).  The gradient is that of the forward as it
    computes (mpc_device.linearise_vjp): zero in X, Y and in what the guard replaced."""
    return _functions().Linearise.apply((md.linearise, md.linearise_vjp), veh, x, u)


def _split_weights(weights):
    if weights is None:
        return None, None, None, False
    Q, QN, R = weights
    return Q, QN, R, True


def ltv_assemble(layout, Ad, Bd, gd, x0, Xr, xlo=None, xhi=None, weights=None):
    """LTVLayout.assemble, differentiable in Ad, Bd, gd, x0, Xr, xlo, xhi and the weights
    (Q, QN, R) of the call (each may be None: the layout's own): (Ax, q, l, u), and Px (nnzP,) as
    well when weights are given."""
    if layout._kind != "ltv":
        raise ValueError("ltv_assemble needs an LTVLayout")
    return _functions().Assemble.apply(layout, Ad, Bd, gd, x0, Xr, xlo, xhi, *_split_weights(weights))


def incr_assemble(layout, Ad, Bd, gd, xt0, Xr, weights=None):
    """IncrementalLayout.assemble, differentiable in Ad, Bd, gd, xt0, Xr and the weights of the call."""
    if layout._kind != "incr":
        raise ValueError("incr_assemble needs an IncrementalLayout")
    return _functions().Assemble.apply(layout, Ad, Bd, gd, xt0, Xr, None, None, *_split_weights(weights))


def affine_assemble(assembler, theta, regime=None):
    """LateralAssembler.assemble, differentiable in theta: (q, l, u)."""
    return _functions().Affine.apply(assembler, theta, regime)


class MPCLayer:
    """One MPC step of either layout as a differentiable map
    ``layer(Ad, Bd, gd, x0, Xr, weights=None, xlo=None, xhi=None) -> (X, U, y)``:
    X (B, N+1, nxa) the predicted (augmented) states, U (B, N, nu) the inputs (increments under the
    incremental layout), y (B, m) the duals.  It composes ltv_assemble / incr_assemble with one
    QPLayer on the layout's pattern; P's values come from the layout or from ``weights``
    = (Q, QN, R) device tensors (each None: the layout's own), expanded to the batch.  x0 is xt0
    (B, nx+nu) under the incremental layout; xlo / xhi are the LTV layout's per-stage bounds.
    ``status``, ``iters``, ``astat``, ``ares``, ``strict`` and the rule of one differentiated solve
    per layer are QPLayer's; ``settings`` are DeviceBatch's."""

    def __init__(self, layout, B, device=0, strict=True, **settings):
        import torch
        self.torch = torch
        self.layout = layout
        P, A, _, _ = layout.pattern()
        self.qp = QPLayer(P, A, B, device=device, strict=strict, **settings)
        self.B = int(B)
        self.Px = torch.from_numpy(P.data.copy()).to(self.qp.dev)

    status = property(lambda self: self.qp.status)
    iters = property(lambda self: self.qp.iters)
    astat = property(lambda self: self.qp.astat)
    ares = property(lambda self: self.qp.ares)

    def __call__(self, Ad, Bd, gd, x0, Xr, weights=None, xlo=None, xhi=None):
        L = self.layout
        if L._kind == "ltv":
            out = ltv_assemble(L, Ad, Bd, gd, x0, Xr, xlo, xhi, weights)
        else:
            if xlo is not None or xhi is not None:
                raise ValueError("MPCLayer: only the LTV layout takes per-stage bounds")
            out = incr_assemble(L, Ad, Bd, gd, x0, Xr, weights)
        Ax, q, l, u = out[:4]
        Px = (out[4] if weights is not None else self.Px).expand(self.B, L.nnzP)
        x, y = self.qp(Px, Ax, q, l, u)
        ns = (L.N + 1) * L.nxa
        return x[:, :ns].reshape(self.B, L.N + 1, L.nxa), x[:, ns:].reshape(self.B, L.N, L.nu), y
