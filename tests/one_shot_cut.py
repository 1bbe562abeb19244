"""Shared by the one-shot tests (tests/test_one_shot.py, tests/test_one_shot_ladder.py) and
tools/one_shot_diff.py: batches with a moved second call, bit comparison, the handle factory for
every rung of the one-shot kernel ladder and the run that holds the rungs to one
another.  Not collected.

The cut: 32 instances of mpc.make_batch(2, B=1024, seed=2000) -- the 8 with the highest oracle
iteration counts (run here, on the host, once per process) and the first 24 of the others -- chosen
to go through every accessor of the swizzled S_k^{-1} tiles several times; its second call moves
the equality bounds, which leaves some instances infeasible.
"""
import functools
import os

import numpy as np

from osqp_amd import mpc

# solve_wave.hip::one_shot_gl on the headline's shape: the best rung the plan allows (5 with
# amax = bmax = 5, else 4), capped by MPCQP_ONE_SHOT_LOOP
CAP = {"lds": 1, "wave": 3, "roles": 4, None: 5}
LOOPS = ("lds", "wave", "roles", None)


def moved_bounds(l, u, seed):
    """A second call's bounds: the first call's equality rows moved (a new measured state per
    instance)."""
    rng = np.random.default_rng(seed)
    l2, u2 = l.copy(), u.copy()
    fin = np.isfinite(l2) & np.isfinite(u2) & (l2 == u2)
    shift = rng.normal(scale=0.05, size=l2.shape)
    l2[fin] += shift[fin]
    u2[fin] += shift[fin]
    return l2, u2


def _inputs(cfg, B, seed, dev):
    import torch
    from osqp_amd import _drop_common_zeros
    b = mpc.make_batch(cfg, B=B, seed=seed)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    l2, u2 = moved_bounds(b["l"], b["u"], seed + 1)
    return P, A, s, (t(Px), t(Ax), t(b["q"])), [(t(b["l"]), t(b["u"])), (t(l2), t(u2))], b


def out(B, n, m, dev):
    import torch
    return (torch.empty((B, n), dtype=torch.float64, device=dev), torch.empty((B, m), dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


def same_bits(a, c):
    """Bit-identical (NaN outputs of unsolved instances included); on a mismatch, which
    instances differ and by how much."""
    import torch
    ab, cb = (t.view(torch.int64) if t.dtype == torch.float64 else t for t in (a, c))
    if torch.equal(ab, cb):
        return True
    rows = (ab != cb).reshape(ab.shape[0], -1).any(1).nonzero().flatten().tolist()
    raise AssertionError(f"{len(rows)} instances differ, first {rows[:8]}; max |diff| "
                         f"{(a - c).abs().nan_to_num(0).max().item() if a.dtype == torch.float64 else None}")


@functools.lru_cache(maxsize=None)
def cut():
    """(batch, settings, second-call bounds, indices into the full batch, the full batch's oracle
    result); read-only."""
    import pyoracle
    from osqp_amd import _drop_common_zeros
    b = mpc.make_batch(2, B=1024, seed=2000)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    full = pyoracle.solve_batch(P, A, Px, b["q"], Ax, b["l"], b["u"], nthreads=8, **s)
    top = np.argsort(-full.iter, kind="stable")[:8]
    rest = np.setdiff1d(np.arange(1024), top)[:24]
    idx = np.concatenate([top, rest])
    pick = lambda v: np.ascontiguousarray(v[idx]) if np.ndim(v) == 2 else v  # noqa: E731
    bs = dict(b, P=P, A=A, Px=pick(Px), Ax=pick(Ax), q=pick(b["q"]), l=pick(b["l"]), u=pick(b["u"]))
    print("oracle iteration counts of the cut:", full.iter[idx].tolist())
    return bs, s, moved_bounds(bs["l"], bs["u"], 2001), idx, full


def handle(P, A, B, s, loop=None, one_shot=True, best=5):
    """A handle created under MPCQP_ONE_SHOT_LOOP=loop (read at creation only; None: unset, the
    default); one_shot False: the persisting kernel.  The handle must report the instantiation
    one_shot_gl gives its plan: -1 when persisting; by form 0 / 2 for forms 1 / 3; for form 2 GL 1
    off the headline's shape, else min(CAP[loop], best) -- best is 5 where the plan has amax =
    bmax = 5 (plan_info does not show bmax: the caller says which it expects)."""
    from osqp_amd import DeviceBatch
    old = os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
    try:
        if loop:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = loop
        h = DeviceBatch(P, A, B, device=0, **s)
    finally:
        os.environ.pop("MPCQP_ONE_SHOT_LOOP", None)
        if old is not None:
            os.environ["MPCQP_ONE_SHOT_LOOP"] = old
    assert h.one_shot_kernel() == -1
    if one_shot:
        form, pi = h.one_shot(True), h.plan_info()
        headline = pi["n_eliminated"] == 0 and pi["amax"] <= 5
        want = {0: -1, 1: 0, 3: 2, 2: min(CAP[loop], best) if headline else 1}[form]
        assert h.one_shot_kernel() == want, (loop, form, pi, h.one_shot_kernel(), want)
    return h


def ladder(P, A, B, s, best=5):
    """The five handles of the ladder: persisting, lds, wave, roles, default."""
    hs = {"persisting": handle(P, A, B, s, one_shot=False)}
    hs.update({loop or "default": handle(P, A, B, s, loop, best=best) for loop in LOOPS})
    return hs


def run_ladder(handles, inputs, bounds, label=""):
    """Every handle's setup_solve of inputs = (Px, Ax, q) under every (l, u) of bounds (device
    tensors); x, y, status and iterations of each handle are held bit-identical to those of
    handles["default"] in every call.  Returns the default's first-call outputs (numpy)."""
    import torch
    d = handles["default"]
    pi = d.plan_info()
    B, n, m, dev = d.B, pi["n"], pi["m"], inputs[0].device
    first, bad = None, []
    for call, (l, u) in enumerate(bounds):
        outs = {k: out(B, n, m, dev) for k in handles}
        for k, h in handles.items():
            h.setup_solve(*inputs, l, u, *outs[k])
        torch.cuda.synchronize()
        o = outs["default"]
        st = o[2].cpu().numpy()
        print(f"{label}, call {call}: status counts {dict(zip(*np.unique(st, return_counts=True)))}, "
              f"iterations {o[3].cpu().tolist()}")
        for k in handles:
            for what, a, c in zip(("x", "y", "status", "iterations"), outs[k], o):
                try:
                    same_bits(a, c)
                except AssertionError as e:
                    bad.append(f"{label}, call {call}, {k} against default, {what}: {e}")
        if call == 0:
            first = [v.cpu().numpy() for v in o]
    assert not bad, "\n".join(bad)
    return first
