"""torch_qp -- the batched QP as a differentiable torch layer.

``QPLayer(P, A, B)`` holds one ``DeviceBatch``; ``layer(Px, Ax, q, l, u)`` sets the batch up,
solves it on the device and returns ``(x, y)``.  The backward pass is one
``DeviceBatch.adjoint`` call (mpcqp_adjoint_device, one seed per instance): the adjoint of the
solution map on the active set the solve ended on -- see include/mpcqp.h for the definition and
DESIGN.md ("Gradients of the solution") for its limits.  Two uses: the local feedback gain of an
MPC step (d du_0 / d x_0 through q, l, u) and tuning weights by gradient (through Px).
"""
from __future__ import annotations

from . import DeviceBatch, OSQP_INFTY

__all__ = ["QPLayer"]


def _function():
    import torch

    class _QPFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, layer, Px, Ax, q, l, u):
            x, y = layer._solve(Px, Ax, q, l, u)
            ctx.layer = layer
            ctx.generation = layer.generation
            # record=True: the context owns what a later backward rebuilds the solve from
            ctx.tape = layer._tape() if layer.record else None
            ctx.set_materialize_grads(False)
            return x, y

        @staticmethod
        def backward(ctx, gx, gy):
            layer = ctx.layer
            if ctx.tape is None and ctx.generation != layer.generation:
                raise RuntimeError("QPLayer: backward after another forward of the same layer (its batch holds "
                                   "the later solve); use one layer per solve that is differentiated")
            if gx is None and gy is None:
                return (None,) * 6
            g = layer._adjoint(gx, gy, ctx.tape)
            need = ctx.needs_input_grad  # (layer, Px, Ax, q, l, u)
            out = (g.gPx, g.gAx, g.gq, g.gl, g.gu)
            return (None,) + tuple(t if need[k + 1] else None for k, t in enumerate(out))

    return _QPFunction


class QPLayer:
    """B QPs of one sparsity pattern as a differentiable map (Px, Ax, q, l, u) -> (x, y).

    P_pattern, A_pattern: scipy sparse matrices giving the pattern (canonicalised as osqp-python
    does: triu(P) and A in sorted CSC order -- the order of Px's and Ax's columns).  Inputs are
    float64 tensors on ``device``: Px (B, nnz(triu(P))), Ax (B, nnz(A)), q (B, n), l, u (B, m).
    Outputs x (B, n), y (B, m); ``status`` and ``iters`` (int32, (B,)) hold the solve's.
    ``strict``: backward raises RuntimeError when an instance's gradients are not reliable
    (``astat`` != 1: not solved, or the adjoint solve's residual above 1e-8 -- a singular active
    set); with strict=False those instances get zero gradients instead.
    A layer holds one solve at a time: backward raises RuntimeError once the layer has run
    another forward.  With ``record=True`` every forward keeps the solve's solution record
    (DeviceBatch.save_solution, n + 2m + 1 doubles per instance) and its five inputs in the autograd
    context, and the backward runs setup + load_solution + adjoint: a backward after later forwards
    of the same layer is then valid and returns the same bits.  Gradients are formed only for the
    inputs that require them.
    """

    def __init__(self, P_pattern, A_pattern, B, device=0, strict=True, record=False, **settings):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", int(device))
        self.batch = DeviceBatch(P_pattern, A_pattern, B, device=int(device), **settings)
        self.B, self.n, self.m = self.batch.B, self.batch.n, self.batch.m
        self.strict = bool(strict)
        self.record = bool(record)
        self.generation = 0
        self._last = None
        self.stream = torch.cuda.Stream(self.dev)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.iters = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.astat = None
        self.ares = None
        self._fn = _function()

    def __call__(self, Px, Ax, q, l, u):
        return self._fn.apply(self, Px, Ax, q, l, u)

    def _on_stream(self, fn):
        """fn() enqueues the batch's calls on the layer's stream: ordered after the caller's
        current stream and before whatever the caller enqueues next.  (torch's current stream
        stays the caller's, so the tensors fn allocates belong to it.)"""
        caller = self.torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        out = fn()
        caller.wait_stream(self.stream)
        return out

    def _arg(self, t, shape, name):
        torch = self.torch
        if tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != self.dev:
            raise ValueError(f"QPLayer: {name} must be a float64 tensor of shape {shape} on {self.dev}")
        return t.detach().contiguous()

    def _solve(self, Px, Ax, q, l, u):
        torch, b = self.torch, self.batch
        B, n, m = self.B, self.n, self.m
        Px = self._arg(Px, (B, b.nnzP), "Px")
        Ax = self._arg(Ax, (B, b.nnzA), "Ax")
        q = self._arg(q, (B, n), "q")
        l = self._arg(l, (B, m), "l").clamp(min=-OSQP_INFTY)
        u = self._arg(u, (B, m), "u").clamp(max=OSQP_INFTY)
        self.generation += 1
        x = torch.empty((B, n), dtype=torch.float64, device=self.dev)
        y = torch.empty((B, m), dtype=torch.float64, device=self.dev)
        s = self.stream.cuda_stream
        rec = torch.empty((B, b.record_width), dtype=torch.float64, device=self.dev) if self.record else None

        def run():
            b.setup(Px, Ax, q, l, u, stream=s)
            b.solve(x, y, self.status, self.iters, stream=s)
            if rec is not None:
                b.save_solution(rec, stream=s)

        self._on_stream(run)
        self._last = (Px, Ax, q, l, u, rec) if self.record else None
        return x, y

    def _tape(self):
        """The last forward's inputs as the setup took them, and its solution record."""
        return self._last

    def _adjoint(self, gx, gy, tape=None):
        gx = None if gx is None else gx.contiguous()
        gy = None if gy is None else gy.contiguous()
        s = self.stream.cuda_stream

        def run():
            if tape is not None:
                self.batch.setup(*tape[:5], stream=s)
                self.batch.load_solution(tape[5], stream=s)
            return self.batch.adjoint(gx, gy, stream=s)

        g = self._on_stream(run)
        self.astat, self.ares = g.astat, g.ares
        bad = g.astat != 1
        if bool(bad.any()):
            if self.strict:
                idx = bad.nonzero().flatten().tolist()
                raise RuntimeError(f"QPLayer: no reliable gradient for instance(s) {idx[:8]} "
                                   f"(astat {g.astat[bad].tolist()[:8]}; strict=False gives them zero gradients)")
            keep = (~bad).to(g.gq.dtype)[:, None]
            for k in ("gPx", "gAx", "gq", "gl", "gu"):
                setattr(g, k, getattr(g, k) * keep)
        return g
