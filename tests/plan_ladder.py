"""Which shape takes which solve kernel: the rungs the default selection (solve.hip::
solve_variant) is held to the oracle at -- TEST INFRASTRUCTURE (test_plan_ladder.py; DESIGN.md,
"Which shape takes which kernel").

A rung is a builder, a horizon N and a seed, with what mpcqp_plan_preview gave for its pattern
(variant, nb, amax, n_eliminated) recorded next to it.  B = 3 on every rung.  The vanilla and
slack builders give every instance the same Px and Ax, which would hide a wrong per-instance
matrix offset: instance b's Px is scaled by (1, 0.5, 2)[b] here (still convex, same pattern);
the dynamic and dense builders vary Ax themselves.

Seeds: the first of 1..20 at which the two CPU solvers (pyoracle, osqp_dense_ref.solve) agree
in status, iteration count and -- on the fixed-count run -- rho updates on all three instances
of both runs, and at which the oracle solves every instance of the run to convergence with
counts that do not move at eps 0.95e-3 and 1.05e-3 (no instance on the edge of its deciding
check).  tools/ladder_seeds.py repeats the search; test_ladder_premises holds the taken seed
to the same conditions.  `converge` False: no seed in 1..20 met the margin, the rung keeps the
fixed-count run only."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sparse

import osqp_dense_ref
import pyoracle
from osqp_amd import mpc

B = 3
PX_SCALE = np.array([1.0, 0.5, 2.0])

Rung = namedtuple("Rung", "builder N n m variant nb amax ne seed converge")

RUNGS = [
    #    builder       N    n     m   var nb amax ne seed converge
    Rung("vanilla",    1,    9,   17,  4,  1,  0,  0, 1, True),   # one block, no coupling
    Rung("vanilla",    6,   34,   62,  4,  2,  3,  0, 1, True),   # two blocks
    Rung("vanilla",   12,   64,  116,  4,  3,  5,  0, 1, True),   # three blocks
    Rung("vanilla",   18,   94,  170, 17,  4,  5,  0, 1, True),   # smallest four-wave plan
    Rung("vanilla",   23,  119,  215, 10,  4,  5,  0, 1, True),   # two-wave kernel by default
    Rung("vanilla",   24,  124,  224, 11,  5,  5,  0, 3, True),   # smallest long-horizon plan
    Rung("vanilla",   45,  229,  413,  3,  8,  5,  0, 1, True),   # RS = 2
    Rung("vanilla",   70,  354,  638, 11, 12,  5,  0, 2, True),   # last nb of big12
    Rung("vanilla",   80,  404,  728, 12, 14,  5,  0, 2, True),   # first vanilla horizon on big18
    Rung("vanilla",  120,  604, 1088, 13, 21,  5,  0, 1, True),   # big24, three rows per thread
    Rung("vanilla",  150,  754, 1358,  6, 26,  5,  0, 1, True),   # past every register / LDS form
    Rung("vanilla_eq", 42, 214,  214,  1,  8,  5,  0, 1, True),   # variant 1
    Rung("slack",      9,  109,  109,  4,  4, 11,  0, 1, True),   # four blocks, amax > 8
    Rung("slack",     10,  120,  120, 11,  5, 11,  0, 3, True),
    Rung("slack",     16,  186,  186, 17,  4,  6, 85, 2, True),   # smallest eliminated plan
    Rung("slack",     21,  241,  241, 11,  9, 11,  0, 1, True),   # elimination rejected
    Rung("slack",     35,  395,  395, 12, 14, 11,  0, 1, True),
    Rung("slack",     50,  560,  560, 13, 19, 11,  0, 1, False),   # no seed with the margin
    Rung("slack",     60,  670,  670,  5, 23, 11,  0, 1, False),   # variant 5; no seed with the margin
    Rung("slack",     90, 1000, 1000,  6, 34, 11,  0, 1, False),   # no seed with the margin
    Rung("dynamic",    1,   18,   34,  4,  1,  0,  0, 2, True),   # gather lists of 8
    Rung("dynamic",   11,  118,  214,  4,  4, 10,  0, 1, True),
    Rung("dynamic",   12,  128,  232, 11,  5, 10,  0, 1, True),
    Rung("dynamic",   21,  218,  394,  3,  8, 10,  0, 1, True),   # RS = 2 with A = 16
    Rung("dynamic",   55,  558, 1006,  5, 19, 10,  0, 2, True),   # LDS bound of big24 exceeded
    Rung("dense",      7,   92,  156,  6,  4, 19,  0, 1, True),   # amax > 16, gather lists of 13
]

# the fixed-count run: test_solve_shell.py's no_check setting plus rho steps at 25 and 50
FIXED = dict(max_iter=60, check_termination=0, adaptive_rho_interval=25, polish=False, warm_start=False)
RUNS = ("fixed", "converge")
MARGIN_EPS = (0.95e-3, 1.05e-3)

STATUS_VAL = {"solved": 1, "solved inaccurate": 2, "max_iter": -2}


def rung_id(r):
    return f"{r.builder}-N{r.N}"


def _scaled(b):
    b["Px"] = np.ascontiguousarray(b["Px"] * PX_SCALE[:, None])
    return b


def _vanilla_eq(N, seed):
    """The vanilla batch without its state-bound rows: the (N+1) nx equality rows and the N
    input-bound rows stay (m = n, eight blocks: solve variant 1)."""
    b = _scaled(mpc.make_batch(2, B=B, seed=seed, N=N))
    neq = (N + 1) * 4
    rows = np.r_[0:neq, 2 * neq:b["m"]]
    A = b["A"].tocsr()[rows].tocsc()
    A.sort_indices()
    # (one nonzero value per entry of the shared pattern: take them by position through a CSC of indices)
    pos = sparse.csc_matrix((np.arange(1, b["A"].nnz + 1, dtype=np.float64), b["A"].indices, b["A"].indptr),
                            shape=b["A"].shape).tocsr()[rows].tocsc()
    pos.sort_indices()
    idx = pos.data.astype(np.int64) - 1
    b.update(A=A, Ax=np.ascontiguousarray(b["Ax"][:, idx]), l=np.ascontiguousarray(b["l"][:, rows]),
             u=np.ascontiguousarray(b["u"][:, rows]), m=rows.size)
    return b


def _dense(N, seed):
    """mpc.vanilla_qp with dense random dynamics, nx = 8, nu = 4 (Ad = I + 0.1 randn, Bd = randn,
    drawn per instance; identity weights, unit boxes): rows and columns of A with 13 nonzeros,
    amax = 19."""
    nx, nu = 8, 4
    rng = np.random.default_rng(seed)
    Ps, As, qs, ls, us = [], [], [], [], []
    for _ in range(B):
        Ad = np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
        Bd = rng.standard_normal((nx, nu))
        x0 = rng.uniform(-0.3, 0.3, nx)
        P, q, A, l, u = mpc.vanilla_qp(Ad, Bd, np.zeros(nx), x0, np.zeros((nx, N + 1)), np.eye(nx), np.eye(nx),
                                       np.eye(nu), N, -np.ones(nx), np.ones(nx), -np.ones(nu), np.ones(nu))
        Ps.append(P); As.append(A); qs.append(q); ls.append(l); us.append(u)
    P, A = Ps[0], As[0]
    for Pk, Ak in zip(Ps, As):
        assert np.array_equal(Pk.indices, P.indices) and np.array_equal(Pk.indptr, P.indptr)
        assert np.array_equal(Ak.indices, A.indices) and np.array_equal(Ak.indptr, A.indptr)
    ucol = (N + 1) * nx
    b = dict(P=P, A=A, Px=np.stack([M.data for M in Ps]), Ax=np.stack([M.data for M in As]), q=np.stack(qs),
             l=np.stack(ls), u=np.stack(us), n=P.shape[0], m=A.shape[0], N=N, B=B, nu=nu,
             u_block=slice(ucol, ucol + N * nu), settings=dict(verbose=False, warm_start=True), cfg="dense")
    return _scaled(b)


BUILDERS = {
    "vanilla": lambda N, seed: _scaled(mpc.make_batch(2, B=B, seed=seed, N=N)),
    "vanilla_eq": _vanilla_eq,
    "slack": lambda N, seed: _scaled(mpc.make_batch(3, B=B, seed=seed, N=N)),
    "dynamic": lambda N, seed: mpc.make_batch(5, B=B, seed=seed, N=N),
    "dense": _dense,
}


@functools.lru_cache(maxsize=None)
def build(builder, N, seed):
    return BUILDERS[builder](N, seed)


def batch(r):
    return build(r.builder, r.N, r.seed)


def pattern(b):
    """(P, A) as the handles plan them: the entries zero in every instance dropped."""
    from osqp_amd import _drop_common_zeros
    P, _ = _drop_common_zeros(b["P"], b["Px"])
    A, _ = _drop_common_zeros(b["A"], b["Ax"])
    return P, A


def settings(b, run, **kw):
    if run == "fixed":
        return dict(FIXED, **kw)
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    return {**s, "polish": False, **kw}


def preview(b):
    """(variant, nb, amax, n_eliminated) of mpcqp_plan_preview for the batch's pattern."""
    import osqp_amd
    P, A = pattern(b)
    info = osqp_amd.plan_preview(P, A, **settings(b, "converge"))
    return info["variant"], info["nb"], info["amax"], info["n_eliminated"]


def solve_oracle(b, run, **kw):
    return pyoracle.solve_batch(b["P"], b["A"], b["Px"], b["q"], b["Ax"], b["l"], b["u"], nthreads=B,
                                **settings(b, run, **kw))


@functools.lru_cache(maxsize=None)
def oracle(r, run):
    """The oracle's result of the rung's batch -- computed once, shared, not to be changed."""
    bo = solve_oracle(batch(r), run)
    for v in (bo.x, bo.y, bo.status_val, bo.iter):
        v.setflags(write=False)
    return bo


def oracle_rho_updates(b, run):
    """info.rho_updates per instance (solve_batch does not return them)."""
    out = []
    for k in range(B):
        P, A = b["P"].copy(), b["A"].copy()
        P.data, A.data = b["Px"][k].copy(), b["Ax"][k].copy()
        o = pyoracle.OSQP()
        o.setup(P, b["q"][k], A, b["l"][k], b["u"][k], **settings(b, run))
        out.append(o.solve().info.rho_updates)
    return np.array(out)


def solve_dense(b, run):
    """osqp_dense_ref.solve (the reduced matrix inverted: the device's formulation) over the batch:
    x, y, status_val, iter, rho_updates."""
    s = settings(b, run)
    check = s.get("check_termination", 25)
    kw = dict(max_iter=s.get("max_iter", 4000), check=check,
              interval=s.get("adaptive_rho_interval", 0) or (4 * check if check else 100))
    xs, ys, st, it, nr = [], [], [], [], []
    for k in range(B):
        P, A = b["P"].copy(), b["A"].copy()
        P.data, A.data = b["Px"][k].copy(), b["Ax"][k].copy()
        x, y, status, iters, nref = osqp_dense_ref.solve(P.toarray(), b["q"][k], A.toarray(), b["l"][k], b["u"][k],
                                                         **kw)
        xs.append(x); ys.append(y); st.append(STATUS_VAL[status]); it.append(iters); nr.append(nref)
    return SimpleNamespace(x=np.stack(xs), y=np.stack(ys), status_val=np.array(st), iter=np.array(it),
                           rho_updates=np.array(nr))


def deviation(x, y, ref):
    """(max |x - x_ref| / max(1, |x_ref|_inf), the same of y) over the batch, per instance scales."""
    sx = np.maximum(1.0, np.abs(ref.x).max(axis=1))
    sy = np.maximum(1.0, np.abs(ref.y).max(axis=1))
    return float((np.abs(x - ref.x).max(axis=1) / sx).max()), float((np.abs(y - ref.y).max(axis=1) / sy).max())


def premises(b, runs=RUNS, margin=True):
    """The conditions of the module docstring for batch b: (ok, what failed or "", details)."""
    det = {}
    for run in runs:
        bo, bd = solve_oracle(b, run), solve_dense(b, run)
        det[run] = (bo, bd)
        if not np.array_equal(bo.status_val, bd.status_val):
            return False, f"{run}: status {bo.status_val} / {bd.status_val}", det
        if not np.array_equal(bo.iter, bd.iter):
            return False, f"{run}: iterations {bo.iter} / {bd.iter}", det
        if run == "fixed":
            ru = oracle_rho_updates(b, run)
            if not np.array_equal(ru, bd.rho_updates):
                return False, f"fixed: rho updates {ru} / {bd.rho_updates}", det
            if not (bo.iter == FIXED["max_iter"]).all():
                return False, f"fixed: iterations {bo.iter}", det
        else:
            if not (bo.status_val == 1).all():  # (infeasible instances are not this ladder's subject)
                return False, f"converge: status {bo.status_val}", det
            if margin:
                for eps in MARGIN_EPS:
                    be = solve_oracle(b, run, eps_abs=eps, eps_rel=eps)
                    if not (np.array_equal(be.iter, bo.iter) and np.array_equal(be.status_val, bo.status_val)):
                        return False, f"converge: at eps {eps} iterations {be.iter} / {bo.iter}", det
    return True, "", det


def handle(r, run):
    """DeviceBatch over the rung's batch, its inputs on the device (solve_families.handle's steps)."""
    import torch
    from osqp_amd import DeviceBatch, _drop_common_zeros
    b = batch(r)
    dev = torch.device("cuda", 0)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    X = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (Px, Ax, b["q"], b["l"], b["u"])]
    torch.cuda.synchronize()  # (the handle's stream is not ordered with torch's)
    return DeviceBatch(P, A, B, device=0, **settings(b, run)), X
