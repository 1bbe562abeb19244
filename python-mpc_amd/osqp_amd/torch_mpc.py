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
  incr_shift(layout, veh, sol, Ad, Bd, gd, xt)          -> xt', pred', pdu'

and ``MPCLayer`` composes the assembly with one ``QPLayer``: (Ad, Bd, gd, x0, Xr[, weights]) ->
(X, U, y), so that d u_0 / d x0 and d loss / d Q are one backward call on the device.  Every call
runs on torch's current stream (the QP solve on the layer's own, ordered with it, as QPLayer does).
Gradients are formed only for the inputs that require them.

With ``linearise_dynamics`` the closed loop of mpc_dynamics.main is differentiable end to end: its
plant step is Ad_0 x + Bd_0 u + gd_0 and its shift copies stages of the solution, both plain torch
operations between one MPCLayer per control step.  ``DynamicRollout`` differentiates
T steps of that loop -- terminal Euler step included -- on ONE solver handle: the forward keeps a
tape of small solution records, the backward sets each step up again, loads its record and runs the
adjoint.
"""
from __future__ import annotations

from . import mpc_device as md
from .torch_qp import QPLayer

__all__ = ["linearise_kinematics", "linearise_dynamics", "ltv_assemble", "incr_assemble", "affine_assemble",
           "incr_shift", "MPCLayer", "DynamicRollout"]

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

    class IncrShift(torch.autograd.Function):
        """inputs (layout, veh, sol, Ad, Bd, gd, xt)"""

        @staticmethod
        def forward(ctx, layout, veh, sol, Ad, Bd, gd, xt):
            sol, Ad, Bd, gd, xt = (_c(t) for t in (sol, Ad, Bd, gd, xt))
            ctx.layout, ctx.veh = layout, veh
            ctx.save_for_backward(sol, Ad, Bd, xt)
            ctx.set_materialize_grads(False)
            return md.incr_shift(layout, veh, sol, Ad, Bd, gd, xt)

        @staticmethod
        def backward(ctx, gxt, gpred, gpdu):
            if gxt is None and gpred is None and gpdu is None:
                return (None,) * 7
            sol, Ad, Bd, xt = ctx.saved_tensors
            need = ctx.needs_input_grad[2:]  # (sol, Ad, Bd, gd, xt)
            want = [k for k, n in zip(md.SHIFT_VJP_OUTPUTS, need) if n]
            g = md.incr_shift_vjp(ctx.layout, ctx.veh, sol, Ad, Bd, xt, _c(gxt), _c(gpred), _c(gpdu), want=want)

            def stage0(t, like_tail):  # the model outputs are stage 0's
                if t is None:
                    return None
                full = t.new_zeros((t.shape[0], ctx.layout.N) + like_tail)
                full[:, 0] = t
                return full

            return (None, None, g.gsol, stage0(g.gAd0, (6, 6)), stage0(g.gBd0, (6, 2)), stage0(g.ggd0, (6,)), g.gxt)

    class Rollout(torch.autograd.Function):
        """inputs (roll, T, path, xt0, pred0, Xr, Q, QN, R, use_w)"""

        @staticmethod
        def forward(ctx, roll, T, path, xt0, pred0, Xr, Q, QN, R, use_w):
            xt0, pred0, Xr, Q, QN, R = (_c(t) for t in (xt0, pred0, Xr, Q, QN, R))
            weights = (Q, QN, R) if use_w else None
            ctx.roll, ctx.path, ctx.weights, ctx.Xr = roll, path, weights, Xr
            ctx.set_materialize_grads(False)
            XT, DU0, pred, ctx.tape = roll._on_stream(lambda: roll._forward(xt0, pred0, T, Xr, path, weights))
            return XT, DU0, pred

        @staticmethod
        def backward(ctx, gXT, gDU0, gpred):
            if gXT is None and gDU0 is None and gpred is None:
                return (None,) * 10
            roll = ctx.roll
            need = dict(zip(("xt0", "pred0", "Xr", "Q", "QN", "R"), ctx.needs_input_grad[3:9]))
            g = roll._on_stream(lambda: roll._backward(ctx.tape, ctx.Xr, ctx.path, ctx.weights, _c(gXT), _c(gDU0),
                                                       _c(gpred), need))
            return (None, None, None, g["xt0"], g["pred0"], g["Xr"], g["Q"], g["QN"], g["R"], None)

    _FN = SimpleNamespace(Linearise=Linearise, Assemble=Assemble, Affine=Affine, IncrShift=IncrShift, Rollout=Rollout)
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


def incr_shift(layout, veh, sol, Ad, Bd, gd, xt):
    """mpc_device.incr_shift -- the plant step, the horizon shift and the terminal Euler step of
    mpc_dynamics.main's loop -- differentiable in sol, Ad, Bd, gd and xt (mpc_device.incr_shift_vjp):
    (xt', pred', pdu').  Only stage 0 of Ad, Bd, gd is read, and only it gets a gradient."""
    if layout._kind != "incr":
        raise ValueError("incr_shift needs an IncrementalLayout")
    return _functions().IncrShift.apply(layout, veh, sol, Ad, Bd, gd, xt)


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


class DynamicRollout:
    """T steps of the dynamic closed loop (mpc_device.DynamicMPC's step) as ONE differentiable map on
    ONE solver handle:

        roll = DynamicRollout(layout, B, veh, device=0, strict=True, warm_start=False, **settings)
        XT, DU0, pred_T = roll(xt0, pred0, T, Xr=None, path=None, weights=None)

    xt0 (B, 8) the augmented state, pred0 (B, N+1, 8) the predicted horizon the first step
    linearises at; XT (B, T+1, 8) the states with XT[:, 0] = xt0, DU0 (B, T, 2) each step's du_0,
    pred_T (B, N+1, 8) the horizon after the last step.  Each step: the reference -- searched on
    ``path`` = (path_x, path_y) device tensors (reference_search) or the given ``Xr`` (T, B, 6, N+1)
    --, the linearisation of stages 0..N-1 of pred, the assembly (``weights`` = (Q, QN, R) of the
    call, each None: the layout's own), setup, with ``warm_start`` the previous solution shifted one
    stage, the solve, and incr_shift.  With weights None and a path, XT equals DynamicMPC's xt step
    for step, bit for bit.

    The forward keeps, per step, xt and pred from before the step, the solution and its record
    (DeviceBatch.save_solution): (N+2) 8 + 2n + 2m + 1 doubles per instance, owned by the autograd
    context, so several rollouts of one object can be alive at once.  The backward walks the steps
    in reverse: it rebuilds the step's QP from the tape, runs setup + load_solution, the shift's VJP,
    ONE adjoint call (seed: the shift's gsol plus the step's own du_0 cotangent), the assembly's
    and the linearisation's VJPs, and accumulates into the cotangents of (xt, pred).  The searched
    reference is piecewise constant and carries no gradient; a given Xr gets its own.  Gradients go
    to xt0, pred0, Q, QN, R (summed over the batch) and Xr, each formed only when required.

    ``status``, ``iters`` (T, B) hold the last forward's solves; after a backward they are that
    rollout's, with ``astat`` (T, B), ``ares`` (T, B) and ``act`` (T, B, m) of its adjoint calls.
    ``strict`` is QPLayer's rule: backward raises when an instance's astat is not 1 at some step;
    with strict=False such an instance gets zero gradients in every input and the weight sums
    leave it out.  ``settings`` are DeviceBatch's."""

    def __init__(self, layout, B, veh, device=0, strict=True, warm_start=False, **settings):
        import torch
        from . import DeviceBatch
        if layout._kind != "incr" or (layout.nx, layout.nu) != (6, 2):
            raise ValueError("DynamicRollout needs an IncrementalLayout of the dynamic bicycle (nx 6, nu 2)")
        self.torch, self.layout, self.veh = torch, layout, veh
        self.B, self.N = int(B), layout.N
        self.dev = torch.device("cuda", int(device))
        self.strict, self.shift_warm = bool(strict), bool(warm_start)
        P, A, _, _ = layout.pattern()
        settings.pop("verbose", None)
        self.batch = DeviceBatch(P, A, self.B, device=int(device), **settings)
        self.Px = torch.from_numpy(P.data.copy()).to(self.dev)[None, :].repeat(self.B, 1).contiguous()
        self.stream = torch.cuda.Stream(self.dev)
        self.status = self.iters = self.astat = self.ares = self.act = None
        self._fn = _functions().Rollout

    def tape_doubles_per_instance(self):
        """Doubles the tape holds per step and instance: xt, pred, sol and the record."""
        L = self.layout
        return 8 + (L.N + 1) * 8 + L.n + self.batch.record_width

    def __call__(self, xt0, pred0, T, Xr=None, path=None, weights=None):
        torch, B, N = self.torch, self.B, self.N
        T = int(T)
        if T < 1:
            raise ValueError("DynamicRollout: T must be at least 1")
        if (Xr is None) == (path is None):
            raise ValueError("DynamicRollout: give either Xr (T, B, 6, N+1) or path = (path_x, path_y)")
        for t, shape, k in ((xt0, (B, 8), "xt0"), (pred0, (B, N + 1, 8), "pred0"), (Xr, (T, B, 6, N + 1), "Xr")):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != self.dev):
                raise ValueError(f"DynamicRollout: {k} must be a float64 tensor of shape {shape} on {self.dev}")
        if path is not None:
            path = tuple(_c(p) for p in path)
        Q, QN, R, use_w = _split_weights(weights)
        return self._fn.apply(self, T, path, xt0, pred0, Xr, Q, QN, R, use_w)

    def _on_stream(self, fn):
        """fn() on the rollout's stream, ordered after the caller's current stream; the caller's
        stream is ordered after it (mpc_device._ClosedLoop's rule)."""
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            out = fn()
        caller.wait_stream(self.stream)
        return out

    def _problem(self, xt, pred, Xr_t, path, weights):
        """One step's reference, linearisation and QP values from (xt, pred), as DynamicMPC._step."""
        N, L = self.N, self.layout
        Xr = md.reference_search(path[0], path[1], pred, self.veh.dt) if Xr_t is None else Xr_t
        Ad, Bd, gd = md.linearise(self.veh, pred[:, :N, :6], pred[:, :N, 6:])
        out = L.assemble(Ad, Bd, gd, xt, Xr, weights=weights)
        Px = self.Px if weights is None else out[4][None, :].repeat(self.B, 1)
        return Xr, Ad, Bd, gd, Px, out[:4]

    def _forward(self, xt, pred, T, Xr, path, weights):
        torch, B, N, L, b = self.torch, self.B, self.N, self.layout, self.batch
        st = md._stream(torch, self.dev)  # self.stream
        kw = dict(dtype=torch.float64, device=self.dev)
        XT, DU0 = torch.empty((B, T + 1, 8), **kw), torch.empty((B, T, 2), **kw)
        status = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        iters = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        XT[:, 0] = xt
        tape, y, nd = [], None, (N + 1) * 8
        for t in range(T):
            _, Ad, Bd, gd, Px, (Ax, q, l, u) = self._problem(xt, pred, None if Xr is None else Xr[t], path, weights)
            b.setup(Px, Ax, q, l, u, stream=st)
            if self.shift_warm and t > 0:
                b.warm_start(*md.warm_shift(N, 8, 2, tape[-1][2], y), stream=st)
            sol, y = torch.empty((B, L.n), **kw), torch.empty((B, L.m), **kw)
            b.solve(sol, y, status[t], iters[t], stream=st)
            rec = b.save_solution(torch.empty((B, b.record_width), **kw), stream=st)
            tape.append((xt, pred, sol, rec))
            xt, pred, _ = md.incr_shift(L, self.veh, sol, Ad, Bd, gd, xt)
            XT[:, t + 1] = xt
            DU0[:, t] = sol[:, nd:nd + 2]
        self.status, self.iters = status, iters
        return XT, DU0, pred, dict(steps=tape, status=status, iters=iters)

    def _backward(self, tape, Xr, path, weights, gXT, gDU0, gpred, need):
        torch, B, N, L, b = self.torch, self.B, self.N, self.layout, self.batch
        st = md._stream(torch, self.dev)
        steps = tape["steps"]
        T, nd = len(steps), (N + 1) * 8
        kw = dict(dtype=torch.float64, device=self.dev)
        astat = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        ares = torch.empty((T, B), **kw)
        act = torch.empty((T, B, L.m), dtype=torch.int8, device=self.dev)
        wnames = [k for k in ("Q", "QN", "R") if weights is not None and need[k]]
        gw = {k: torch.zeros((B,) + ((2, 2) if k == "R" else (6, 6)), **kw) for k in wnames}
        gXr = torch.zeros((T, B, 6, N + 1), **kw) if Xr is not None and need["Xr"] else None
        want = ["gAd", "gBd", "ggd", "gx0"] + ["gXr"] * (gXr is not None) + ["g" + k for k in wnames]
        g_xt = gXT[:, T].clone() if gXT is not None else torch.zeros((B, 8), **kw)
        g_pred = gpred
        for t in reversed(range(T)):
            xt, pred, sol, rec = steps[t]
            Xr_t, Ad, Bd, gd, Px, (Ax, q, l, u) = self._problem(xt, pred, None if Xr is None else Xr[t], path, weights)
            b.setup(Px, Ax, q, l, u, stream=st)
            b.load_solution(rec, stream=st)
            sh = md.incr_shift_vjp(L, self.veh, sol, Ad, Bd, xt, g_xt, g_pred, None)
            if gDU0 is not None:
                sh.gsol[:, nd:nd + 2] += gDU0[:, t]
            a = b.adjoint(sh.gsol, None, act=act[t], ares=ares[t], astat=astat[t], stream=st)
            v = L.assemble_vjp(a.gAx, a.gq, a.gl, a.gu, gPx=a.gPx if wnames else None, Xr=Xr_t,
                               weights=None if weights is None else (weights[0], weights[1], None), want=want)
            v.gAd[:, 0] += sh.gAd0
            v.gBd[:, 0] += sh.gBd0
            v.ggd[:, 0] += sh.ggd0
            gx, gu = md.linearise_vjp(self.veh, pred[:, :N, :6], pred[:, :N, 6:], v.gAd, v.gBd, v.ggd)
            g_pred = torch.zeros((B, N + 1, 8), **kw)
            g_pred[:, :N, :6] = gx
            g_pred[:, :N, 6:] = gu
            g_xt = sh.gxt + v.gx0
            if gXT is not None:
                g_xt += gXT[:, t]
            for k in wnames:
                gw[k] += getattr(v, "g" + k)
            if gXr is not None:
                gXr[t] = v.gXr
        self.status, self.iters = tape["status"], tape["iters"]
        self.astat, self.ares, self.act = astat, ares, act
        bad = (astat != 1).any(0)
        if bool(bad.any()):
            if self.strict:
                idx = bad.nonzero().flatten().tolist()
                raise RuntimeError(f"DynamicRollout: no reliable gradient for instance(s) {idx[:8]} (astat per step "
                                   f"{astat[:, bad].T.tolist()[:8]}; strict=False gives them zero gradients)")
            zero = lambda g: None if g is None else torch.where(bad.view((-1,) + (1,) * (g.dim() - 1)), 0.0, g)
            g_xt, g_pred = zero(g_xt), zero(g_pred)
            gw = {k: zero(g) for k, g in gw.items()}
            if gXr is not None:
                gXr = torch.where(bad.view(1, -1, 1, 1), 0.0, gXr)
        out = dict(xt0=g_xt if need["xt0"] else None, pred0=g_pred if need["pred0"] else None, Xr=gXr,
                   Q=None, QN=None, R=None)
        for k in wnames:
            out[k] = gw[k].sum(0)
        return out
