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
  kin_shift(layout, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt, done)
                                                        -> xt', pred', pdu', finish_cnt', done', mode
  kin_ltv_shift(layout, veh, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u)
                                                        -> x', u', pred_x', pred_u', mode

and ``MPCLayer`` composes the assembly with one ``QPLayer``: (Ad, Bd, gd, x0, Xr[, weights]) ->
(X, U, y), so that d u_0 / d x0 and d loss / d Q are one backward call on the device.  Every call
runs on torch's current stream (the QP solve on the layer's own, ordered with it, as QPLayer does).
Gradients are formed only for the inputs that require them.

With ``linearise_dynamics`` the closed loop of mpc_dynamics.main is differentiable end to end: its
plant step is Ad_0 x + Bd_0 u + gd_0 and its shift copies stages of the solution, both plain torch
operations between one MPCLayer per control step.  ``DynamicRollout`` differentiates
T steps of that loop -- terminal Euler step included -- on ONE solver handle: the forward keeps a
tape of small solution records, the backward sets each step up again, loads its record and runs the
adjoint.  ``KinematicRollout`` and ``KinematicLTVRollout`` are the same body over the
two kinematic loops (KinematicMPC, KinematicLTVMPC), whose tails carry the stop rule's and the skip
rule's masks.

``fleet(params)`` makes the vehicle itself an input: a (B, 9) or (B, 3) tensor of constructor
arguments, one row per vehicle, accepted wherever ``veh`` is; when it requires grad, the backward of
the linearisations, the three tails and the three rollouts also returns d loss / d params
(DESIGN.md §25).
"""
from __future__ import annotations

from . import mpc_device as md
from .torch_qp import QPLayer

__all__ = ["linearise_kinematics", "linearise_dynamics", "ltv_assemble", "incr_assemble", "affine_assemble",
           "incr_shift", "kin_shift", "kin_ltv_shift", "MPCLayer", "DynamicRollout", "KinematicRollout",
           "KinematicLTVRollout", "fleet", "ParamFleet"]

_FN = None


def _c(t):
    return None if t is None else t.detach().contiguous()


class ParamFleet:
    """``fleet(params)``: a fleet whose constructor arguments are a tensor.  ``params`` (B, 9) in
    mpc_device.Vehicle's field order (m, l_f, l_r, width, length, C_d, A_f, C_roll, dt) or (B, 3) in
    KinVehicle's (l_f, l_r, dt); ``table`` the mpc_device.Fleet / KinFleet made of its values at
    creation (a snapshot: after changing params, call ``fleet`` again)."""

    def __init__(self, params, device=None):
        import torch
        if not isinstance(params, torch.Tensor) or params.dim() != 2 or params.shape[1] not in (9, 3) or \
                params.dtype != torch.float64:
            raise ValueError("fleet: params must be a float64 tensor of shape (B, 9) or (B, 3)")
        if device is None:
            device = params.device.index or 0 if params.is_cuda else 0
        kind, struct = (md.Fleet, md.Vehicle) if params.shape[1] == 9 else (md.KinFleet, md.KinVehicle)
        self.params = params
        self.table = kind([struct(*row) for row in params.detach().cpu().tolist()], device=int(device))

    def __len__(self):
        return len(self.table)

    @property
    def dt(self):
        return self.table.dt


def fleet(params, device=None):
    """A fleet of B vehicles from a (B, 9) or (B, 3) float64 tensor of constructor arguments, accepted
    wherever this module takes ``veh``.  When ``params.requires_grad``, the backward of
    linearise_dynamics / linearise_kinematics, incr_shift / kin_shift / kin_ltv_shift and the three
    rollouts also returns d loss / d params: the linearisations' part from
    mpc_device.linearise_pvjp / kin_linearise_pvjp, the tails' from the terminal-step kernels on views
    of the solution, both chained through ``constants_vjp``.  ``device``: the table's (default: the
    tensor's, or 0 for a host tensor; the gradient arrives on params' own device)."""
    return ParamFleet(params, device)


def _veh(veh):
    """(what mpc_device takes, the params tensor or None) of a ``veh`` argument."""
    return (veh.table, veh.params) if isinstance(veh, ParamFleet) else (veh, None)


def _chain(device, table, gK):
    """d loss / d params, on params' device, from the cotangent of the table's constants (the chain
    runs on the host: B x 13 doubles)."""
    import torch
    return torch.from_numpy(table.constants_vjp(gK)).to(device)


def _terminal_pvjp(tail, table, N, sol, gpred, mode):
    """The terminal step of a tail with respect to the table's constants: the point is a pair of
    views into the solution (mpc_device.hip's DynamicIncrTail / KinIncrTail / KinLtvTail), the
    cotangent the state part of gpred[N]."""
    if tail == "incr":  # euler_step_guarded(x_N, u_{N-1}) of x~ = (x, u), nxa 8
        x, u, w = sol[:, N * 8:N * 8 + 6], sol[:, (N - 1) * 8 + 6:N * 8], None if gpred is None else gpred[:, N, :6]
        return md.euler_step_pvjp(table, x, u, None if w is None else w.contiguous(), mode)
    if tail == "kin":   # kin_update(x_N, u_N) of x~ = (x, u), nxa 6
        x, u, w = sol[:, N * 6:N * 6 + 4], sol[:, N * 6 + 4:N * 6 + 6], None if gpred is None else gpred[:, N, :4]
    else:               # kin_update(S_N, U_{N-1}) of sol = (S_0..S_N, U_0..U_{N-1})
        o = (N + 1) * 4 + (N - 1) * 2
        x, u, w = sol[:, N * 4:N * 4 + 4], sol[:, o:o + 2], None if gpred is None else gpred[:, N]
    return md.kin_update_pvjp(table, x, u, None if w is None else w.contiguous(), mode)


def _functions():
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from types import SimpleNamespace

    class Linearise(torch.autograd.Function):
        """inputs (model, veh, x, u, params); model = (forward, vjp, pvjp) of mpc_device; params: a
        ParamFleet's tensor (veh is then its table) or None"""

        @staticmethod
        def forward(ctx, model, veh, x, u, params):
            ctx.vjp, ctx.pvjp, ctx.veh, ctx.pdev = model[1], model[2], veh, getattr(params, "device", None)
            ctx.save_for_backward(x, u)
            ctx.set_materialize_grads(False)
            return model[0](veh, x.detach(), u.detach())

        @staticmethod
        def backward(ctx, gAd, gBd, ggd):
            x, u = ctx.saved_tensors
            if gAd is None and gBd is None and ggd is None:
                return None, None, None, None, None
            need = ctx.needs_input_grad
            gx = gu = gp = None
            if need[2] or need[3]:
                gx, gu = ctx.vjp(ctx.veh, x.detach(), u.detach(), _c(gAd), _c(gBd), _c(ggd))
            if need[4]:
                gp = _chain(ctx.pdev, ctx.veh,ctx.pvjp(ctx.veh, x.detach(), u.detach(), _c(gAd), _c(gBd), _c(ggd)))
            return None, None, gx if need[2] else None, gu if need[3] else None, gp

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

    def stage0(t, N):  # the tails read the model of stage 0 only: its cotangent, zero in the others
        if t is None:
            return None
        full = t.new_zeros((t.shape[0], N) + tuple(t.shape[1:]))
        full[:, 0] = t
        return full

    class IncrShift(torch.autograd.Function):
        """inputs (layout, veh, sol, Ad, Bd, gd, xt, params)"""

        @staticmethod
        def forward(ctx, layout, veh, sol, Ad, Bd, gd, xt, params):
            sol, Ad, Bd, gd, xt = (_c(t) for t in (sol, Ad, Bd, gd, xt))
            ctx.layout, ctx.veh, ctx.pdev = layout, veh, getattr(params, "device", None)
            ctx.save_for_backward(sol, Ad, Bd, xt)
            ctx.set_materialize_grads(False)
            return md.incr_shift(layout, veh, sol, Ad, Bd, gd, xt)

        @staticmethod
        def backward(ctx, gxt, gpred, gpdu):
            if gxt is None and gpred is None and gpdu is None:
                return (None,) * 8
            sol, Ad, Bd, xt = ctx.saved_tensors
            need = ctx.needs_input_grad[2:7]  # (sol, Ad, Bd, gd, xt)
            want = [k for k, n in zip(md.SHIFT_VJP_OUTPUTS, need) if n]
            g = md.incr_shift_vjp(ctx.layout, ctx.veh, sol, Ad, Bd, xt, _c(gxt), _c(gpred), _c(gpdu), want=want)
            N = ctx.layout.N
            gp = _chain(ctx.pdev, ctx.veh,_terminal_pvjp("incr", ctx.veh, N, sol, _c(gpred), None)) \
                if ctx.needs_input_grad[7] else None
            return (None, None, g.gsol, stage0(g.gAd0, N), stage0(g.gBd0, N), stage0(g.ggd0, N), g.gxt, gp)

    class KinShift(torch.autograd.Function):
        """inputs (layout, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt, done, params)"""

        @staticmethod
        def forward(ctx, layout, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt, done, params):
            sol, Ad, Bd, gd, Xr, xt, pred, pdu = (_c(t) for t in (sol, Ad, Bd, gd, Xr, xt, pred, pdu))
            xt1, pred1, pdu1, cnt1, done1, mode = md.kin_shift(layout, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu,
                                                               finish_cnt, done)
            ctx.layout, ctx.veh, ctx.pdev = layout, veh, getattr(params, "device", None)
            ctx.save_for_backward(sol, Ad, Bd, xt, mode)
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(cnt1, done1, mode)
            return xt1, pred1, pdu1, cnt1, done1, mode

        @staticmethod
        def backward(ctx, gxt, gpred, gpdu, *_):
            if gxt is None and gpred is None and gpdu is None:
                return (None,) * 13
            sol, Ad, Bd, xt, mode = ctx.saved_tensors
            need = ctx.needs_input_grad
            want = [k for k, n in zip(md.SHIFT_VJP_OUTPUTS, (need[2], need[3], need[4], need[5], need[7])) if n]
            g = md.kin_shift_vjp(ctx.layout, ctx.veh, sol, Ad, Bd, xt, mode, _c(gxt), _c(gpred), _c(gpdu), want=want)
            N = ctx.layout.N
            gp = _chain(ctx.pdev, ctx.veh,_terminal_pvjp("kin", ctx.veh, N, sol, _c(gpred), mode)) if need[12] else None
            return (None, None, g.gsol, stage0(g.gAd0, N), stage0(g.gBd0, N), stage0(g.ggd0, N), None, g.gxt,
                    g.gpred_prev if need[8] else None, g.gpdu_prev if need[9] else None, None, None, gp)

    class KinLTVShift(torch.autograd.Function):
        """inputs (layout, veh, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u, params)"""

        @staticmethod
        def forward(ctx, layout, veh, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u, params):
            sol, Ad, Bd, gd, x, u, pred_x, pred_u = (_c(t) for t in (sol, Ad, Bd, gd, x, u, pred_x, pred_u))
            x1, u1, px1, pu1, mode = md.kin_ltv_shift(layout, veh, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u)
            ctx.layout, ctx.veh, ctx.pdev = layout, veh, getattr(params, "device", None)
            ctx.save_for_backward(sol, Ad, Bd, x, mode)
            ctx.set_materialize_grads(False)
            ctx.mark_non_differentiable(mode)
            return x1, u1, px1, pu1, mode

        @staticmethod
        def backward(ctx, gx, gu, gpx, gpu, *_):
            if gx is None and gu is None and gpx is None and gpu is None:
                return (None,) * 12
            sol, Ad, Bd, x, mode = ctx.saved_tensors
            need = ctx.needs_input_grad
            want = [k for k, n in zip(md.KIN_LTV_SHIFT_VJP_OUTPUTS, (need[2], need[4], need[5], need[6], need[7])) if n]
            g = md.kin_ltv_shift_vjp(ctx.layout, ctx.veh, sol, Ad, Bd, x, mode, _c(gx), _c(gu), _c(gpx), _c(gpu),
                                     want=want)
            N = ctx.layout.N
            gp = _chain(ctx.pdev, ctx.veh,_terminal_pvjp("ltv", ctx.veh, N, sol, _c(gpx), mode)) if need[11] else None
            return (None, None, g.gsol, None, stage0(g.gAd0, N), stage0(g.gBd0, N), stage0(g.ggd0, N), g.gx,
                    g.gu_prev if need[8] else None, g.gpred_x_prev if need[9] else None,
                    g.gpred_u_prev if need[10] else None, gp)

    class Rollout(torch.autograd.Function):
        """inputs (roll, T, path, use_w, *state, *hor, Xr, Q, QN, R, params), the state and the horizon
        as many tensors as roll._STATE and roll._HOR say, params a ParamFleet's tensor or None; outputs
        (*trajectories, [DU0,] *horizon)"""

        @staticmethod
        def forward(ctx, roll, T, path, use_w, *tensors):
            tensors = tuple(_c(t) for t in tensors)
            ns, nh = len(roll._STATE), len(roll._HOR)
            Xr, Q, QN, R = tensors[ns + nh:ns + nh + 4]
            weights = (Q, QN, R) if use_w else None
            ctx.roll, ctx.path, ctx.weights, ctx.Xr = roll, path, weights, Xr
            ctx.set_materialize_grads(False)
            trajs, DU0, hor, ctx.tape = roll._on_stream(lambda: roll._forward(tensors[:ns], tensors[ns:ns + nh], T, Xr,
                                                                              path, weights))
            return (*trajs, *((DU0,) if roll._DU0 else ()), *hor)

        @staticmethod
        def backward(ctx, *cots):
            roll = ctx.roll
            ns, nh = len(roll._STATE), len(roll._HOR)
            if all(g is None for g in cots):
                return (None,) * (9 + ns + nh)
            cots = tuple(_c(g) for g in cots)
            n = ctx.needs_input_grad[4:]
            need = dict(state=n[:ns], hor=n[ns:ns + nh], Xr=n[-5], Q=n[-4], QN=n[-3], R=n[-2], params=n[-1])
            gDU0 = cots[ns] if roll._DU0 else None
            g = roll._on_stream(lambda: roll._backward(ctx.tape, ctx.Xr, ctx.path, ctx.weights, cots[:ns], gDU0,
                                                       cots[len(cots) - nh:], need))
            return (None, None, None, None, *g["state"], *g["hor"], g["Xr"], g["Q"], g["QN"], g["R"], g["params"])

    _FN = SimpleNamespace(Linearise=Linearise, Assemble=Assemble, Affine=Affine, IncrShift=IncrShift,
                          KinShift=KinShift, KinLTVShift=KinLTVShift, Rollout=Rollout)
    return _FN


def linearise_kinematics(veh, x, u):
    """mpc_device.linearise_kinematics, differentiable in x and u (3-D (B, N, 4) / (B, N, 2), any
    strides with a contiguous last axis: an ``expand`` over the stages gets the stage sum)."""
    table, params = _veh(veh)
    return _functions().Linearise.apply((md.linearise_kinematics, md.linearise_kinematics_vjp, md.kin_linearise_pvjp),
                                        table, x, u, params)


def linearise_dynamics(veh, x, u):
    """mpc_device.linearise (the dynamic bicycle: Pacejka tyres, the low-speed guard), differentiable
    in x and u (3-D (B, N, 6) / (B, N, 2) or 2-D, any strides with a contiguous last axis: an
    ``expand`` over the stages gets the stage sum).  The gradient is that of the forward as it
    computes (mpc_device.linearise_vjp): zero in X, Y and in what the guard replaced."""
    table, params = _veh(veh)
    return _functions().Linearise.apply((md.linearise, md.linearise_vjp, md.linearise_pvjp), table, x, u, params)


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
    table, params = _veh(veh)
    return _functions().IncrShift.apply(layout, table, sol, Ad, Bd, gd, xt, params)


def kin_shift(layout, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt=None, done=None):
    """mpc_device.kin_shift -- the tail of simulate's loop on the kinematic bicycle: stop rule, plant
    step, horizon shift, terminal update_kinematics_model step -- differentiable in sol, Ad, Bd, gd,
    xt, pred and pdu (mpc_device.kin_shift_vjp): (xt', pred', pdu', finish_cnt', done', mode).  Only
    stage 0 of Ad, Bd, gd is read.  pred and pdu get a gradient only where the vehicle was already
    done (mode 1: they pass through); Xr only steers the stop rule and gets none."""
    if layout._kind != "incr":
        raise ValueError("kin_shift needs an IncrementalLayout")
    table, params = _veh(veh)
    return _functions().KinShift.apply(layout, table, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt, done, params)


def kin_ltv_shift(layout, veh, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u):
    """mpc_device.kin_ltv_shift -- the tail of mpc_kinematics_pred_matrix.main's loop: skip rule,
    plant step, horizon shift, terminal update_kinematics_model step -- differentiable in sol, Ad,
    Bd, gd, x, u, pred_x and pred_u (mpc_device.kin_ltv_shift_vjp): (x', u', pred_x', pred_u', mode).
    u, pred_x and pred_u get a gradient only where the vehicle was skipped (status != 1: they pass
    through)."""
    if layout._kind != "ltv":
        raise ValueError("kin_ltv_shift needs an LTVLayout")
    table, params = _veh(veh)
    return _functions().KinLTVShift.apply(layout, table, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u, params)


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


class _Rollout:
    """What the rollouts share: T control steps on ONE DeviceBatch with a tape of solution records,
    and the backward that walks it in reverse.  The loop's state and its
    predicted horizon are tuples of tensors of widths ``_STATE`` and ``_HOR`` (per stage).  A subclass
    states its ``_NAME``, ``_LAYOUT`` = (kind, nx, nu, words) and the model-specific parts:

      _problem(state, hor, Xr_t, path, weights)  -> Xr, Ad, Bd, gd, Px, (Ax, q, l, u)
      _shift(sol, status, Ad, Bd, gd, Xr, state, hor, aux) -> state', hor', mode, aux'
      _shift_vjp(sol, Ad, Bd, state, mode, g_state, g_hor) -> (namespace with gsol, gAd0, gBd0, ggd0),
                                                   [cotangents of the state before], [of the previous
                                                   horizon through the tail's masks] or None
      _linearise_vjp(hor, gAd, gBd, ggd)         -> [cotangents of the horizon]
      _exempt(mode)                              -> (B,) bool of the vehicles whose solution the step
                                                   did not use, or None

    ``_DU0``: the outputs include each step's first input rows of the solution, whose cotangent is
    added to the adjoint's seed.  ``aux`` is what the tail carries besides state and horizon.

    ``veh`` may be ``fleet(params)``: its table runs the loop and, when params requires grad, the
    backward also returns d loss / d params -- per step ``_TAIL``'s terminal step and
    ``_linearise_pvjp(hor, gAd, gBd, ggd)``, summed in the table's coordinates (``gK`` of the last
    backward stays on the object) and chained once to the constructor arguments."""

    _DU0 = True

    def __init__(self, layout, B, veh, device=0, strict=True, warm_start=False, **settings):
        import torch
        from . import DeviceBatch
        kind, nx, nu, words = self._LAYOUT
        if layout._kind != kind or (layout.nx, layout.nu) != (nx, nu):
            raise ValueError(f"{self._NAME} needs {words} (nx {nx}, nu {nu})")
        veh, self.params = _veh(veh)  # fleet(params): its table runs the loop, its tensor gets the gradient
        self.torch, self.layout, self.veh = torch, layout, veh
        self.B, self.N = int(B), layout.N
        if isinstance(veh, (md.Fleet, md.KinFleet)) and len(veh) != self.B:  # one table entry per vehicle
            raise ValueError(f"{self._NAME}: a fleet of {len(veh)} vehicles was given a batch of {self.B}")
        self.dev = torch.device("cuda", int(device))
        self.strict, self.shift_warm = bool(strict), bool(warm_start)
        P, A, _, _ = layout.pattern()
        settings.pop("verbose", None)
        self.batch = DeviceBatch(P, A, self.B, device=int(device), **settings)
        self.Px = torch.from_numpy(P.data.copy()).to(self.dev)[None, :].repeat(self.B, 1).contiguous()
        self.stream = torch.cuda.Stream(self.dev)
        self.status = self.iters = self.astat = self.ares = self.act = self.mode = self.gK = None

    def tape_doubles_per_instance(self):
        """Doubles the tape holds per step and instance: the state, the horizon, sol and the record
        (a loop with masks keeps one int32 mode per step and instance besides)."""
        L = self.layout
        return sum(self._STATE) + (L.N + 1) * sum(self._HOR) + L.n + self.batch.record_width

    def _check_call(self, T, Xr, path, tensors, path_words):
        torch, B, N = self.torch, self.B, self.N
        if T < 1:
            raise ValueError(f"{self._NAME}: T must be at least 1")
        nx = self.layout.nx
        if (Xr is None) == (path is None):
            raise ValueError(f"{self._NAME}: give either Xr (T, B, {nx}, N+1) or path = {path_words}")
        for t, shape, k in tensors + ((Xr, (T, B, nx, N + 1), "Xr"),):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != self.dev):
                raise ValueError(f"{self._NAME}: {k} must be a float64 tensor of shape {shape} on {self.dev}")

    def _apply(self, T, path, weights, *tensors):
        """The rollout as one autograd node; tensors = (*state, *hor, Xr)."""
        Q, QN, R, use_w = _split_weights(weights)
        return _functions().Rollout.apply(self, T, path, use_w, *tensors, Q, QN, R, self.params)

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

    def _aux0(self):
        return None

    def _exempt(self, mode):
        return None

    def _forward(self, state, hor, T, Xr, path, weights):
        torch, B, N, L, b = self.torch, self.B, self.N, self.layout, self.batch
        st = md._stream(torch, self.dev)  # self.stream
        kw = dict(dtype=torch.float64, device=self.dev)
        trajs = [torch.empty((B, T + 1, w), **kw) for w in self._STATE]
        DU0 = torch.empty((B, T, L.nu), **kw) if self._DU0 else None
        status = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        iters = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        for X, s in zip(trajs, state):
            X[:, 0] = s
        tape, y, nd, aux = [], None, (N + 1) * L.nxa, self._aux0()
        for t in range(T):
            Xr_t, Ad, Bd, gd, Px, (Ax, q, l, u) = self._problem(state, hor, None if Xr is None else Xr[t], path,
                                                                weights)
            b.setup(Px, Ax, q, l, u, stream=st)
            if self.shift_warm and t > 0:
                b.warm_start(*md.warm_shift(N, L.nxa, L.nu, tape[-1][2], y), stream=st)
            sol, y = torch.empty((B, L.n), **kw), torch.empty((B, L.m), **kw)
            b.solve(sol, y, status[t], iters[t], stream=st)
            rec = b.save_solution(torch.empty((B, b.record_width), **kw), stream=st)
            state1, hor1, mode, aux = self._shift(sol, status[t], Ad, Bd, gd, Xr_t, state, hor, aux)
            tape.append((state, hor, sol, rec, mode))
            state, hor = state1, hor1
            for X, s in zip(trajs, state):
                X[:, t + 1] = s
            if DU0 is not None:
                DU0[:, t] = sol[:, nd:nd + L.nu]
        self.status, self.iters = status, iters
        if tape[0][4] is not None:
            self.mode = torch.stack([s[4] for s in tape])
        return trajs, DU0, hor, dict(steps=tape, status=status, iters=iters)

    def _backward(self, tape, Xr, path, weights, gtraj, gDU0, ghor, need):
        torch, B, N, L, b = self.torch, self.B, self.N, self.layout, self.batch
        st = md._stream(torch, self.dev)
        steps = tape["steps"]
        T, nd, nx, nu = len(steps), (N + 1) * L.nxa, L.nx, L.nu
        kw = dict(dtype=torch.float64, device=self.dev)
        astat = torch.empty((T, B), dtype=torch.int32, device=self.dev)
        ares = torch.empty((T, B), **kw)
        act = torch.empty((T, B, L.m), dtype=torch.int8, device=self.dev)
        exempt = torch.zeros((T, B), dtype=torch.bool, device=self.dev)
        wnames = [k for k in ("Q", "QN", "R") if weights is not None and need[k]]
        gw = {k: torch.zeros((B,) + ((nu, nu) if k == "R" else (nx, nx)), **kw) for k in wnames}
        gXr = torch.zeros((T, B, nx, N + 1), **kw) if Xr is not None and need["Xr"] else None
        want = ["gAd", "gBd", "ggd", "gx0"] + ["gXr"] * (gXr is not None) + ["g" + k for k in wnames]
        g_state = [g[:, T].clone() if g is not None else torch.zeros((B, w), **kw) for g, w in zip(gtraj, self._STATE)]
        g_hor = list(ghor)
        # d loss / d the table's constants: each step's terminal step and its linearisation (§25)
        gK = torch.zeros((B, 13 if nx == 6 else 3), **kw) if need["params"] else None
        for t in reversed(range(T)):
            state, hor, sol, rec, mode = steps[t]
            Xr_t, Ad, Bd, gd, Px, (Ax, q, l, u) = self._problem(state, hor, None if Xr is None else Xr[t], path,
                                                                weights)
            b.setup(Px, Ax, q, l, u, stream=st)
            b.load_solution(rec, stream=st)
            sh, g_before, g_hor_prev = self._shift_vjp(sol, Ad, Bd, state, mode, g_state, g_hor)
            if gK is not None:
                gK += _terminal_pvjp(self._TAIL, self.veh, N, sol, g_hor[0], mode)
            if gDU0 is not None:
                sh.gsol[:, nd:nd + nu] += gDU0[:, t]
            a = b.adjoint(sh.gsol, None, act=act[t], ares=ares[t], astat=astat[t], stream=st)
            v = L.assemble_vjp(a.gAx, a.gq, a.gl, a.gu, gPx=a.gPx if wnames else None, Xr=Xr_t,
                               weights=None if weights is None else (weights[0], weights[1], None), want=want)
            v.gAd[:, 0] += sh.gAd0
            v.gBd[:, 0] += sh.gBd0
            v.ggd[:, 0] += sh.ggd0
            skip = self._exempt(mode)
            if skip is not None:  # the step did not use these solutions: nothing flows through their solves
                exempt[t] = skip
                for k in want:
                    g = getattr(v, k)
                    g.masked_fill_(skip.view((-1,) + (1,) * (g.dim() - 1)), 0.0)
            if gK is not None:
                gK += self._linearise_pvjp(hor, v.gAd, v.gBd, v.ggd)
            g_hor = self._linearise_vjp(hor, v.gAd, v.gBd, v.ggd)
            if g_hor_prev is not None:
                g_hor = [g if p is None else g + p for g, p in zip(g_hor, g_hor_prev)]
            g_state = list(g_before)
            g_state[0] = g_state[0] + v.gx0
            for i, g in enumerate(gtraj):
                if g is not None:
                    g_state[i] += g[:, t]
            for k in wnames:
                gw[k] += getattr(v, "g" + k)
            if gXr is not None:
                gXr[t] = v.gXr
        self.status, self.iters = tape["status"], tape["iters"]
        self.astat, self.ares, self.act = astat, ares, act
        bad = ((astat != 1) & ~exempt).any(0)
        if bool(bad.any()):
            if self.strict:
                idx = bad.nonzero().flatten().tolist()
                raise RuntimeError(f"{self._NAME}: no reliable gradient for instance(s) {idx[:8]} (astat per step "
                                   f"{astat[:, bad].T.tolist()[:8]}; strict=False gives them zero gradients)")
            zero = lambda g: None if g is None else torch.where(bad.view((-1,) + (1,) * (g.dim() - 1)), 0.0, g)
            g_state, g_hor = [zero(g) for g in g_state], [zero(g) for g in g_hor]
            gw = {k: zero(g) for k, g in gw.items()}
            if gXr is not None:
                gXr = torch.where(bad.view(1, -1, 1, 1), 0.0, gXr)
            gK = zero(gK)
        self.gK = gK  # the cotangent of the table's constants, before the chain to params
        out = dict(state=[g if n else None for g, n in zip(g_state, need["state"])],
                   hor=[g if n else None for g, n in zip(g_hor, need["hor"])], Xr=gXr, Q=None, QN=None, R=None,
                   params=None if gK is None else _chain(self.params.device, self.veh, gK))
        for k in wnames:
            out[k] = gw[k].sum(0)
        return out


class DynamicRollout(_Rollout):
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

    _NAME = "DynamicRollout"
    _LAYOUT = ("incr", 6, 2, "an IncrementalLayout of the dynamic bicycle")
    _STATE, _HOR = (8,), (8,)

    def __call__(self, xt0, pred0, T, Xr=None, path=None, weights=None):
        B, N, T = self.B, self.N, int(T)
        self._check_call(T, Xr, path, ((xt0, (B, 8), "xt0"), (pred0, (B, N + 1, 8), "pred0")), "(path_x, path_y)")
        if path is not None:
            path = tuple(_c(p) for p in path)
        return self._apply(T, path, weights, xt0, pred0, Xr)

    def _problem(self, state, hor, Xr_t, path, weights):
        """One step's reference, linearisation and QP values from (xt, pred), as DynamicMPC._step."""
        N, L, (xt,), (pred,) = self.N, self.layout, state, hor
        Xr = md.reference_search(path[0], path[1], pred, self.veh.dt) if Xr_t is None else Xr_t
        Ad, Bd, gd = md.linearise(self.veh, pred[:, :N, :6], pred[:, :N, 6:])
        out = L.assemble(Ad, Bd, gd, xt, Xr, weights=weights)
        Px = self.Px if weights is None else out[4][None, :].repeat(self.B, 1)
        return Xr, Ad, Bd, gd, Px, out[:4]

    def _shift(self, sol, status, Ad, Bd, gd, Xr, state, hor, aux):
        xt, pred, _ = md.incr_shift(self.layout, self.veh, sol, Ad, Bd, gd, state[0])
        return (xt,), (pred,), None, aux

    def _shift_vjp(self, sol, Ad, Bd, state, mode, g_state, g_hor):
        sh = md.incr_shift_vjp(self.layout, self.veh, sol, Ad, Bd, state[0], g_state[0], g_hor[0], None)
        return sh, [sh.gxt], None

    def _linearise_vjp(self, hor, gAd, gBd, ggd):
        N, (pred,) = self.N, hor
        gx, gu = md.linearise_vjp(self.veh, pred[:, :N, :6], pred[:, :N, 6:], gAd, gBd, ggd)
        g = pred.new_zeros((self.B, N + 1, 8))
        g[:, :N, :6] = gx
        g[:, :N, 6:] = gu
        return [g]

    _TAIL = "incr"

    def _linearise_pvjp(self, hor, gAd, gBd, ggd):
        N, (pred,) = self.N, hor
        return md.linearise_pvjp(self.veh, pred[:, :N, :6], pred[:, :N, 6:], gAd, gBd, ggd)


def _incr_kin_problem(self, state, hor, Xr_t, path, weights):
    """KinematicMPC._step's reference, linearisation and QP values; with the (x, pred_x, pred_u) of
    the LTV loop, KinematicLTVMPC._step's."""
    N, L = self.N, self.layout
    if L._kind == "incr":
        x0, xs, us = state[0], hor[0][:, :, :4], hor[0][:, :, 4:]
    else:
        x0, xs, us = state[0], hor[0], hor[1]
    Xr = md.reference_search_kin(path[0], path[1], path[2], path[3], hor[0], self.veh.dt) if Xr_t is None else Xr_t
    Ad, Bd, gd = md.linearise_kinematics(self.veh, xs[:, :N], us[:, :N])
    out = L.assemble(Ad, Bd, gd, x0, Xr, weights=weights)
    Px = self.Px if weights is None else out[4][None, :].repeat(self.B, 1)
    return Xr, Ad, Bd, gd, Px, out[:4]


class KinematicRollout(_Rollout):
    """T steps of the kinematic closed loop (mpc_device.KinematicMPC's step; its tail is also
    LaneChangeMPC's) as ONE differentiable map on ONE solver handle, as DynamicRollout:

        roll = KinematicRollout(layout, B, veh, device=0, strict=True, warm_start=False, **settings)
        XT, DU0, pred_T = roll(xt0, pred0, T, Xr=None, path=None, set_speed=None, weights=None)

    xt0 (B, 6) = (X, Y, v, yaw, steer, accel), pred0 (B, N+1, 6); XT (B, T+1, 6), DU0 (B, T, 2),
    pred_T (B, N+1, 6).  The reference is searched on ``path`` = (path_x, path_y, path_yaw) with
    ``set_speed`` (B,) (default: xt0's v, as KinematicMPC) or given as ``Xr`` (T, B, 4, N+1).  The
    forward runs the loop's own tail (mpc_device.kin_shift), stop rule included, with finish_cnt and
    done starting at zero; ``done`` (T, B) and ``mode`` (T, B) of the last forward stay on the object.
    A vehicle that no longer moves is still solved: DU0[:, t] is that solve's du_0, and its cotangent
    goes through that step's adjoint like any other.  The backward is DynamicRollout's with
    mpc_device.kin_shift_vjp and linearise_kinematics_vjp."""

    _NAME = "KinematicRollout"
    _LAYOUT = ("incr", 4, 2, "an IncrementalLayout of the kinematic bicycle")
    _STATE, _HOR = (6,), (6,)
    _problem = _incr_kin_problem

    def __call__(self, xt0, pred0, T, Xr=None, path=None, set_speed=None, weights=None):
        B, N, T = self.B, self.N, int(T)
        self._check_call(T, Xr, path, ((xt0, (B, 6), "xt0"), (pred0, (B, N + 1, 6), "pred0"),
                                       (set_speed, (B,), "set_speed")), "(path_x, path_y, path_yaw)")
        if path is not None:
            speed = xt0[:, 2] if set_speed is None else set_speed
            path = tuple(_c(p) for p in path) + (_c(speed),)
        return self._apply(T, path, weights, xt0, pred0, Xr)

    def _aux0(self):
        torch, B = self.torch, self.B
        ikw = dict(dtype=torch.int32, device=self.dev)
        return (torch.zeros((B, self.N + 1, 2), dtype=torch.float64, device=self.dev), torch.zeros(B, **ikw),
                torch.zeros(B, **ikw))

    def _shift(self, sol, status, Ad, Bd, gd, Xr, state, hor, aux):
        xt, pred, pdu, cnt, done, mode = md.kin_shift(self.layout, self.veh, sol, Ad, Bd, gd, Xr, state[0], hor[0],
                                                      *aux)
        return (xt,), (pred,), mode, (pdu, cnt, done)

    def _forward(self, state, hor, T, Xr, path, weights):
        out = super()._forward(state, hor, T, Xr, path, weights)
        self.done = (self.mode != 0).to(self.torch.int32)
        return out

    def _shift_vjp(self, sol, Ad, Bd, state, mode, g_state, g_hor):
        sh = md.kin_shift_vjp(self.layout, self.veh, sol, Ad, Bd, state[0], mode, g_state[0], g_hor[0], None)
        return sh, [sh.gxt], [sh.gpred_prev]

    def _linearise_vjp(self, hor, gAd, gBd, ggd):
        N, (pred,) = self.N, hor
        gx, gu = md.linearise_kinematics_vjp(self.veh, pred[:, :N, :4], pred[:, :N, 4:], gAd, gBd, ggd)
        g = pred.new_zeros((self.B, N + 1, 6))
        g[:, :N, :4] = gx
        g[:, :N, 4:] = gu
        return [g]

    _TAIL = "kin"

    def _linearise_pvjp(self, hor, gAd, gBd, ggd):
        N, (pred,) = self.N, hor
        return md.kin_linearise_pvjp(self.veh, pred[:, :N, :4], pred[:, :N, 4:], gAd, gBd, ggd)


class KinematicLTVRollout(_Rollout):
    """T steps of the direct-input kinematic closed loop (mpc_device.KinematicLTVMPC's step) as ONE
    differentiable map on ONE solver handle:

        roll = KinematicLTVRollout(layout, B, veh, device=0, strict=True, warm_start=False, **settings)
        X, U, pred_x_T, pred_u_T = roll(x0, u0, pred_x0, pred_u0, T, Xr=None, path=None, weights=None)

    x0 (B, 4), u0 (B, 2), pred_x0 (B, N+1, 4), pred_u0 (B, N+1, 2); X (B, T+1, 4), U (B, T+1, 2) with
    U[:, 0] = u0 and U[:, t+1] the control held after step t.  The reference is searched on ``path``
    = (path_x, path_y) (set speed 10, path yaw 0, as KinematicLTVMPC) or given as ``Xr``
    (T, B, 4, N+1).  The tail is mpc_device.kin_ltv_shift with its skip rule: a vehicle whose solve
    did not end `solved` keeps x, u, pred_x, pred_u bit for bit (``mode`` (T, B) of the last forward
    stays on the object).  In the backward such a (step, vehicle) pair seeds its adjoint with zero,
    passes its cotangents through unchanged and is exempt from the ``strict`` rule -- its solution was
    not used; ``strict`` otherwise follows DynamicRollout's rule."""

    _NAME, _DU0 = "KinematicLTVRollout", False
    _LAYOUT = ("ltv", 4, 2, "an LTVLayout of the kinematic bicycle")
    _STATE, _HOR = (4, 2), (4, 2)
    _problem = _incr_kin_problem
    SET_SPEED = md.KinematicLTVMPC.SET_SPEED

    def __call__(self, x0, u0, pred_x0, pred_u0, T, Xr=None, path=None, weights=None):
        torch, B, N, T = self.torch, self.B, self.N, int(T)
        self._check_call(T, Xr, path, ((x0, (B, 4), "x0"), (u0, (B, 2), "u0"), (pred_x0, (B, N + 1, 4), "pred_x0"),
                                       (pred_u0, (B, N + 1, 2), "pred_u0")), "(path_x, path_y)")
        if path is not None:
            px, py = (_c(p) for p in path)
            path = (px, py, torch.zeros_like(px), torch.full((B,), self.SET_SPEED, dtype=torch.float64, device=self.dev))
        return self._apply(T, path, weights, x0, u0, pred_x0, pred_u0, Xr)

    def _shift(self, sol, status, Ad, Bd, gd, Xr, state, hor, aux):
        x, u, px, pu, mode = md.kin_ltv_shift(self.layout, self.veh, sol, status, Ad, Bd, gd, *state, *hor)
        return (x, u), (px, pu), mode, aux

    def _exempt(self, mode):
        return mode != 0

    def _shift_vjp(self, sol, Ad, Bd, state, mode, g_state, g_hor):
        sh = md.kin_ltv_shift_vjp(self.layout, self.veh, sol, Ad, Bd, state[0], mode, g_state[0], g_state[1],
                                  g_hor[0], g_hor[1])
        return sh, [sh.gx, sh.gu_prev], [sh.gpred_x_prev, sh.gpred_u_prev]

    def _linearise_vjp(self, hor, gAd, gBd, ggd):
        N, (px, pu) = self.N, hor
        gx, gu = md.linearise_kinematics_vjp(self.veh, px[:, :N], pu[:, :N], gAd, gBd, ggd)
        gpx, gpu = px.new_zeros(px.shape), pu.new_zeros(pu.shape)
        gpx[:, :N] = gx
        gpu[:, :N] = gu
        return [gpx, gpu]

    _TAIL = "ltv"

    def _linearise_pvjp(self, hor, gAd, gBd, ggd):
        N, (px, pu) = self.N, hor
        return md.kin_linearise_pvjp(self.veh, px[:, :N], pu[:, :N], gAd, gBd, ggd)
