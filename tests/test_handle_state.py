"""What a handle carries from one call to the next -- x, z, y, rho, the row classes, factor
freshness -- through every production kernel family at B = 3 (solve_families.py), each call
sequence against one CPU oracle object per instance making the same calls; and setup_warm()
against setup() + warm_start() on the register-list setup plans (cfg 2, cfg 3), bit for bit.

Every solve here ends at an iteration cap chosen with the oracle alone (each oracle-side run
asserts iter == cap and status != solved), so status and count agree by construction and
parity.check_agreement (min_match 1.0, U_TOL) compares the iterates the cap leaves.

Warm-start parts: 5 iterations, warm_start of 0.5 x and / or 0.5 y of the oracle's result, 5
more.  OSQP 0.6: x sets z = A x, y alone keeps x and z (after a solve z != A x).  Premises
(oracle alone, per instance): the controls move by at least 100 U_TOL against the run without
the warm-start call, and for y alone against warm_start(x of the first solve, y0) -- the form
that sets z = A x.  The oracle's smallest such distances over the three instances:
  cfg 2: x 1.001e-2, y 8.2e-2, xy 8.0e-2, y against the both-form 1.19e-2
  cfg 3: x 1.9e-2,   y 2.1e-2, xy 3.3e-2, y against the both-form 2.3e-2
  cfg 5: x 1.2e2,    y 3.9,    xy 1.2e2,  y against the both-form 1.4e2
Both sides are given the oracle's first result halved, so the warm start's inputs are the same.

Call sequence (adaptive_rho_interval 50, warm starting): a solve to test_solve_shell.py's
rho_steps cap K1; update(q 1.01, l, u with the initial-state rows moved by up to 0.02);
max_iter K2 and a solve; warm_start(x, y) of that result, both perturbed by up to 1 %, update(q)
with the same q, max_iter K3 and a solve.  Premises (oracle alone): every instance takes a rho
step in the first solve and every solve ends at its cap unsolved.

The repeated update(q) changes no data.  OSQP 0.6's osqp_solve keeps info.status_val of the
previous solve unless an osqp_update_* call reset it, and then skips the approximate check at
the cap; the device starts every solve unsolved (mpcqp.h, mpcqp_solve_batch).  Without that
call the oracle's third status on cfg 3's instance 1 is the second solve's 2 ("solved
inaccurate") with a dual residual 3.1 times the approximate tolerance, the device's -2; with
it both report -2.  (In the warm-start parts the oracle's second status is the first solve's
as well; there the two are equal.)

At the settings' rho 0.1 the oracle takes no rho step within K1 on cfg 2 and cfg 5 at these
seeds (its estimates at the rho checks stay within the tolerance 5 of 0.1), so there the first
solve starts from a rho it does move: 1e-3 on cfg 2, 1.0 on cfg 5.  K2 and K3: the largest of
5, 10, ... at which all three instances are still unsolved (cfg 2, cfg 3); cfg 5 is unsolved to
120 and beyond: 60, a rho check at 50 and the cap after it.  The oracle's counts (the rho steps
are all in the first solve; status 2 is the conclusion's looser check at the cap):
  cfg 2: rho 1e-3, K1 90,  K2 25, K3 15   rho steps 1, 1, 1   status -2 -2 -2 / 2 2 2 / 2 2 2
  cfg 3: rho 0.1,  K1 120, K2 40, K3 20   rho steps 1, 2, 1   status 2 -2 2 / 2 2 2 / 2 -2 2
  cfg 5: rho 1.0,  K1 120, K2 60, K3 60   rho steps 1, 1, 1   status 2 2 2 / 2 2 2 / 2 2 2
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
from osqp_amd import mpc
from parity import U_TOL, check_agreement
from solve_families import B, FAMILIES, batch, env, handle, out_of, settings

K1 = {2: 90, 3: 120, 5: 120}
K2 = {2: 25, 3: 40, 5: 60}
K3 = {2: 15, 3: 20, 5: 60}
RHO0 = {2: 1e-3, 3: 0.1, 5: 1.0}  # (see the module docstring)
X0_ROWS = {2: 4, 3: 5, 5: 8}  # the initial-state equality rows of mpc.make_batch's layouts
FIRST_CAP = 5
HALF = 0.5


class _Oracles:
    """One pyoracle.OSQP per instance of batch(cfg); solve() in pyoracle.solve_batch's form."""

    def __init__(self, cfg, **kw):
        b = batch(cfg)
        self.o = []
        for k in range(B):
            P, A = b["P"].copy(), b["A"].copy()
            P.data, A.data = b["Px"][k].copy(), b["Ax"][k].copy()
            o = pyoracle.OSQP()
            o.setup(P, b["q"][k], A, b["l"][k], b["u"][k], **settings(cfg, **kw))
            self.o.append(o)

    def each(self, name, **rows):
        for k, o in enumerate(self.o):
            getattr(o, name)(**{key: v[k] if isinstance(v, np.ndarray) else v for key, v in rows.items()})

    def solve(self, cap):
        r = [o.solve() for o in self.o]
        bo = SimpleNamespace(x=np.stack([v.x for v in r]), y=np.stack([v.y for v in r]),
                             status_val=np.array([v.info.status_val for v in r], np.int32),
                             iter=np.array([v.info.iter for v in r], np.int32),
                             rho_updates=np.array([v.info.rho_updates for v in r]))
        assert (bo.iter == cap).all() and (bo.status_val != 1).all(), (bo.iter, bo.status_val)  # (the caps' premise)
        return bo


def _du(cfg, a, c):
    ub = batch(cfg)["u_block"]
    return np.abs(a.x[:, ub] - c.x[:, ub]).max(axis=1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _solve(h):
    o = out_of(h)
    h.solve(*o)
    h.synchronize()
    return [t.cpu().numpy() for t in o]


# ---- a. warm-start parts ----
def _start(first, part):
    return {k: HALF * getattr(first, k) for k in part}


@functools.lru_cache(maxsize=None)
def _oracle_parts(cfg, part):
    """(the first solve, the solve after warm_start(part)), the premises asserted."""
    def run(start):
        orc = _Oracles(cfg, max_iter=FIRST_CAP, warm_start=True)
        first = orc.solve(FIRST_CAP)
        if start is not None:
            orc.each("warm_start", **start(first))
        return first, orc.solve(FIRST_CAP)

    first, second = run(lambda f: _start(f, part))
    d = _du(cfg, second, run(None)[1])
    print("premise", cfg, part, "against no warm start", d)
    assert (d >= 100 * U_TOL).all(), d
    if part == "y":
        d = _du(cfg, second, run(lambda f: dict(x=f.x, y=HALF * f.y))[1])
        print("premise", cfg, part, "against the both-form", d)
        assert (d >= 100 * U_TOL).all(), d
    return first, second


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["x", "y", "xy"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_warm_start_parts_match_oracle(family, part, monkeypatch):
    cfg, variant, elim, vid = FAMILIES[family]
    first, second = _oracle_parts(cfg, part)
    env(monkeypatch, variant, elim)
    h, X = handle(cfg, max_iter=FIRST_CAP, warm_start=True)
    assert h.plan_info()["variant"] == vid
    h.setup(*X)
    check_agreement(f"state {family} first", batch(cfg), *_solve(h), first, min_match=1.0)
    start = {k: _dev(v) for k, v in _start(first, part).items()}
    import torch
    torch.cuda.synchronize()  # (the handle's stream is not ordered with torch's)
    h.warm_start(**start)
    x, y, st, it = _solve(h)
    print(family, part, "status", st, "iter", it, "du", _du(cfg, SimpleNamespace(x=x), second))
    check_agreement(f"state {family} warm {part}", batch(cfg), x, y, st, it, second, min_match=1.0)


# ---- b. a call sequence with carried rho ----
def _sequence_data(cfg):
    """(q, l, u) of the update and the warm start's relative perturbations of x and y."""
    b = batch(cfg)
    rng = np.random.default_rng(7)
    r = X0_ROWS[cfg]
    l, u = b["l"].copy(), b["u"].copy()
    x0 = -l[:, :r] + rng.uniform(-0.02, 0.02, (B, r))
    l[:, :r] = -x0
    u[:, :r] = -x0
    return 1.01 * b["q"], l, u, 1 + rng.uniform(-0.01, 0.01, (B, b["n"])), 1 + rng.uniform(-0.01, 0.01, (B, b["m"]))


@functools.lru_cache(maxsize=None)
def _oracle_sequence(cfg):
    k2, k3 = K2[cfg], K3[cfg]
    q, l, u, px, py = _sequence_data(cfg)
    orc = _Oracles(cfg, max_iter=K1[cfg], rho=RHO0[cfg], adaptive_rho_interval=50, warm_start=True)
    r1 = orc.solve(K1[cfg])
    assert (r1.rho_updates >= 1).all(), r1.rho_updates
    orc.each("update", q=q, l=l, u=u)
    orc.each("update_settings", max_iter=k2)
    r2 = orc.solve(k2)
    orc.each("warm_start", x=r2.x * px, y=r2.y * py)
    orc.each("update", q=q)  # (the same q: see the module docstring)
    orc.each("update_settings", max_iter=k3)
    r3 = orc.solve(k3)
    return r1, r2, r3


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_call_sequence_matches_oracle(family, monkeypatch):
    cfg, variant, elim, vid = FAMILIES[family]
    r1, r2, r3 = _oracle_sequence(cfg)
    q, l, u, px, py = _sequence_data(cfg)
    b = batch(cfg)
    moved = dict(b, q=q, l=l, u=u)
    env(monkeypatch, variant, elim)
    h, X = handle(cfg, max_iter=K1[cfg], rho=RHO0[cfg], adaptive_rho_interval=50, warm_start=True)
    assert h.plan_info()["variant"] == vid
    h.setup(*X)
    check_agreement(f"state {family} sequence 1", b, *_solve(h), r1, min_match=1.0)
    import torch
    dq, dl, du, dx, dy = (_dev(a) for a in (q, l, u, r2.x * px, r2.y * py))
    torch.cuda.synchronize()  # (the handle's stream is not ordered with torch's)
    h.update(q=dq, l=dl, u=du)
    h.update_settings(max_iter=K2[cfg])
    check_agreement(f"state {family} sequence 2", moved, *_solve(h), r2, min_match=1.0)
    h.warm_start(x=dx, y=dy)
    h.update(q=dq)
    h.update_settings(max_iter=K3[cfg])
    check_agreement(f"state {family} sequence 3", moved, *_solve(h), r3, min_match=1.0)


# ---- c. setup_warm on the register-list setup plans ----
def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


@functools.lru_cache(maxsize=None)
def _setup_warm_case(cfg, nb):
    """The batch on the device, its pattern and settings, and the default solve's x and y (on
    the handle that solved it: its rho adapted)."""
    import torch
    from osqp_amd import DeviceBatch, _drop_common_zeros
    b = batch(cfg) if nb == B else mpc.make_batch(cfg, B=nb, seed=41)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    s = {k: v for k, v in b["settings"].items() if k != "verbose"}
    X = [_dev(v) for v in (Px, Ax, b["q"], b["l"], b["u"])]
    torch.cuda.synchronize()
    make = lambda: DeviceBatch(P, A, nb, device=0, **s)  # noqa: E731
    outs = lambda: (torch.empty((nb, b["n"]), dtype=torch.float64, device=X[0].device),  # noqa: E731
                    torch.empty((nb, b["m"]), dtype=torch.float64, device=X[0].device),
                    torch.empty(nb, dtype=torch.int32, device=X[0].device),
                    torch.empty(nb, dtype=torch.int32, device=X[0].device))
    used = make()
    o = outs()
    used.setup(*X)
    used.solve(*o)
    used.synchronize()
    assert (o[2].cpu().numpy() == 1).mean() > 0.99
    return X, make, outs, used, o[0], o[1]


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["xy", "x", "y"])
@pytest.mark.parametrize("nb", [3, 512])
@pytest.mark.parametrize("cfg", [2, 3])
def test_setup_warm_equals_setup_then_warm_start(cfg, nb, part):
    """cfg 2 and cfg 3 set up through the register-list kernel (k_setup_r), which has no fused
    warm form: setup_warm() must run it and the warm-start kernel, not the wide setup's one-kernel
    form (another summation order of the cost scale) -- setup_warm_fused() says 0, and the solve
    equals setup() + warm_start()'s bit for bit, on a fresh handle and on one that has solved
    (its rho adapted, its iterates and row classes set).  B = 512: the batch size from which the
    wide setup would take its 512-thread form."""
    X, make, outs, used, x0, y0 = _setup_warm_case(cfg, nb)
    start = dict(x=x0 if "x" in part else None, y=y0 if "y" in part else None)
    runs = []
    for h, fused in ((make(), False), (make(), True), (used, True)):
        assert h.setup_warm_fused() == 0
        o = outs()
        if fused:
            h.setup_warm(*X, **start)
        else:
            h.setup(*X)
            h.warm_start(**start)
        h.solve(*o)
        h.synchronize()
        runs.append([v.cpu().numpy() for v in o])
    print(cfg, nb, part, "iter", np.bincount(runs[0][3]).nonzero()[0], "solved", (runs[0][2] == 1).mean())
    for r in runs[1:]:
        for a, c in zip(runs[0], r):
            assert np.array_equal(_bits(a), _bits(c)), np.flatnonzero((_bits(a) != _bits(c)).reshape(nb, -1).any(axis=1))
    assert (runs[0][2] == 1).mean() > 0.99
