"""Every solve kernel the default selection can take (solve.hip::solve_variant), at the smallest
shape and at the shape edges of each, against the CPU oracle: the rungs of plan_ladder.RUNGS
("Which shape takes which kernel").

CPU: the rung table is what mpcqp_plan_preview gives, and the two CPU solvers agree on every
rung (the premises of the GPU tests).  GPU, per rung, both after asserting the plan_info of the
handle against the table: (a) a fixed count of 60 iterations with rho steps at 25 and 50 --
equal counts by construction, x and y compared directly; (b) the run to convergence at the
builder's call-site settings, through parity.check_agreement.  Nothing here sets
MPCQP_VARIANT or MPCQP_ELIM: the tests delete them."""
import numpy as np
import pytest

import plan_ladder as L
import pyoracle
from osqp_amd import mpc
from parity import check_agreement
from solve_families import env as _env, run as _run

IDS = [L.rung_id(r) for r in L.RUNGS]
CONVERGE = [r for r in L.RUNGS if r.converge]
X_TOL, Y_TOL = 1e-6, 1e-5  # test_gpu_parity.py::_cmp_single's bars, relative to max(1, |ref|_inf)


def test_ladder_plans(monkeypatch):
    """Every rung's plan_preview (variant, nb, amax, n_eliminated; n and m) equals the table, and
    the rungs' variants are exactly the ones the default selection can reach from the builders:
    {1, 3, 4, 5, 6, 10, 11, 12, 13, 17}.  Variants 0, 2 and 7 are the default on no rung (17 and
    10 precede 0 in the preference order, 7 is not in it): they stay where they are run today, by
    override -- test_gpu_parity.py::test_alternative_kernel_variants (0, 7) and the families of
    solve_families.py (0, 2)."""
    _env(monkeypatch, None, None)
    for r in L.RUNGS:
        b = L.batch(r)
        assert (b["n"], b["m"]) == (r.n, r.m), L.rung_id(r)
        assert L.preview(b) == (r.variant, r.nb, r.amax, r.ne), (L.rung_id(r), L.preview(b))
        assert b["Px"].shape[0] == L.B
    assert {r.variant for r in L.RUNGS} == {1, 3, 4, 5, 6, 10, 11, 12, 13, 17}
    # run (b) may be absent on at most four rungs, and on none of variants 1 and 3; variant 5 keeps it on one
    assert len(L.RUNGS) - len(CONVERGE) <= 4
    assert {1, 3, 5} <= {r.variant for r in CONVERGE}
    assert all(r.converge for r in L.RUNGS if r.variant in (1, 3))


def test_ladder_elimination_rejected_rung(monkeypatch):
    """The slack plan at N = 21: an eliminated plan exists and is rejected (plan_choice 2)."""
    import osqp_amd
    _env(monkeypatch, None, None)
    b = L.batch(next(r for r in L.RUNGS if (r.builder, r.N) == ("slack", 21)))
    P, A = L.pattern(b)
    info = osqp_amd.plan_preview(P, A, **L.settings(b, "converge"))
    assert info["plan_choice"] == 2 and info["n_eliminated"] == 0 and info["note"], info


@pytest.mark.parametrize("r", L.RUNGS, ids=IDS)
def test_ladder_premises(r):
    """What the GPU tests rest on, with the two CPU solvers alone: pyoracle.solve_batch and
    osqp_dense_ref.solve (which inverts the reduced matrix, the device's own formulation) give the
    same status and iteration count on all three instances of both runs, the same number of rho
    updates on the fixed-count run; and on the run to convergence the oracle solves every
    instance with counts unchanged at eps 0.95e-3 and 1.05e-3."""
    b = L.batch(r)
    ok, what, det = L.premises(b, runs=L.RUNS if r.converge else ("fixed",))
    assert ok, (L.rung_id(r), r.seed, what)
    bo, bd = det["fixed"]
    dx, dy = L.deviation(bd.x, bd.y, bo)
    print(f"{L.rung_id(r)} seed {r.seed} fixed: dense restatement vs oracle x {dx:.1e} y {dy:.1e}, status "
          f"{bo.status_val.tolist()}" + (f"; converge: iterations {det['converge'][0].iter.tolist()}" if r.converge else ""))
    assert dx < X_TOL and dy < Y_TOL  # (the restatement itself meets the device's bars, by orders of magnitude)
    assert np.array_equal(L.oracle(r, "fixed").x, bo.x)  # the cached result the GPU tests compare with


def test_ladder_refusals(monkeypatch):
    """Shapes no instantiation takes: the dynamic layout at N = 120 previews as variant -1
    (m = 2176 > 8 * 256 rows); dense dynamics with nx = 12, nu = 4 are refused by the plan."""
    import osqp_amd
    _env(monkeypatch, None, None)
    b = mpc.make_batch(5, B=L.B, seed=1, N=120)
    assert b["m"] == 2176
    P, A = L.pattern(b)
    assert osqp_amd.plan_preview(P, A, **L.settings(b, "converge"))["variant"] == -1
    rng = np.random.default_rng(1)
    nx, nu, N = 12, 4, 7
    P, _, A, _, _ = mpc.vanilla_qp(np.eye(nx) + 0.1 * rng.standard_normal((nx, nx)), rng.standard_normal((nx, nu)),
                                   np.zeros(nx), np.zeros(nx), np.zeros((nx, N + 1)), np.eye(nx), np.eye(nx),
                                   np.eye(nu), N, -np.ones(nx), np.ones(nx), -np.ones(nu), np.ones(nu))
    with pytest.raises(Exception, match="unsupported sparsity"):
        osqp_amd.plan_preview(P, A)


def _assert_plan(h, r):
    info = h.plan_info()
    assert (info["variant"], info["nb"], info["n_eliminated"]) == (r.variant, r.nb, r.ne), (L.rung_id(r), info)


def _fixed_run(r):
    """Run (a) of rung r on the device against the oracle; the deviations (x, y)."""
    h, X = L.handle(r, "fixed")
    _assert_plan(h, r)
    x, y, st, it = _run(h, X, False)
    bo = L.oracle(r, "fixed")
    dx, dy = L.deviation(x, y, bo)
    print(f"ladder fixed {L.rung_id(r)} variant {r.variant}: x {dx:.2e} y {dy:.2e} status {st.tolist()} "
          f"iter {it.tolist()} (oracle {bo.status_val.tolist()} {bo.iter.tolist()})")
    assert np.array_equal(st, bo.status_val) and np.array_equal(it, bo.iter)
    assert (it == L.FIXED["max_iter"]).all()
    assert np.isfinite(x).all() and np.isfinite(y).all()
    assert dx < X_TOL, (L.rung_id(r), dx)
    assert dy < Y_TOL, (L.rung_id(r), dy)
    return dx, dy


@pytest.mark.gpu
@pytest.mark.parametrize("r", L.RUNGS, ids=IDS)
def test_ladder_fixed_count(r, monkeypatch):
    """(a) 60 iterations, no termination check, rho steps at 25 and 50: status and count equal on
    all three instances, x within 1e-6 max(1, |x_ref|_inf) and y within 1e-5 max(1, |y_ref|_inf)
    of the oracle.  DESIGN.md §20's table has the measured deviations (1e-15 to 7e-11).  The rho
    steps fall on iterations without a termination check: the regression test of the two- and
    four-wave kernels' rho step (solve_wave.hip: the barrier before the restore of L.res), which
    gave NaN iterates on the vanilla N = 18 and N = 23 rungs without it."""
    _env(monkeypatch, None, None)
    _fixed_run(r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", CONVERGE, ids=[L.rung_id(r) for r in CONVERGE])
def test_ladder_converged(r, monkeypatch):
    """(b) the run to convergence at the builder's call-site settings, polish off, through the
    host batch API: status and iteration count equal on all three instances (min_match 1.0: the
    seeds keep every instance off the edge of its deciding check, test_ladder_premises)."""
    from osqp_amd import OSQPBatch
    _env(monkeypatch, None, None)
    b = L.batch(r)
    s = L.settings(b, "converge")
    bg = OSQPBatch()
    bg.setup(b["P"], b["q"], b["A"], b["l"], b["u"], Px=b["Px"], Ax=b["Ax"], **s)
    _assert_plan(bg, r)
    rg = bg.solve()
    bo = L.oracle(r, "converge")

    def tight(d):
        return pyoracle.solve_batch(b["P"], b["A"], b["Px"][d], b["q"][d], b["Ax"][d], b["l"][d], b["u"][d],
                                    **dict(s, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000)).x
    print(f"ladder converge {L.rung_id(r)} variant {r.variant}: status {rg.status_val.tolist()} iter "
          f"{rg.iter.tolist()} (oracle {bo.status_val.tolist()} {bo.iter.tolist()})")
    check_agreement(f"ladder {L.rung_id(r)} variant {r.variant}", b, rg.x, rg.y, rg.status_val, rg.iter, bo,
                    min_match=1.0, tight=tight)
    assert (rg.status_val == 1).all()


@pytest.mark.gpu
def test_ladder_refused_shape_leaves_nothing_behind(monkeypatch):
    """(c) setup of the dynamic layout at N = 120 is refused; a fresh handle then sets up and
    solves a valid rung as if nothing had happened."""
    from osqp_amd import OSQPBatch
    _env(monkeypatch, None, None)
    b = mpc.make_batch(5, B=L.B, seed=1, N=120)
    with pytest.raises(Exception, match="outside the solve kernel's instantiations"):
        OSQPBatch().setup(b["P"], b["q"], b["A"], b["l"], b["u"], Px=b["Px"], Ax=b["Ax"], **L.settings(b, "converge"))
    _fixed_run(next(r for r in L.RUNGS if (r.builder, r.N) == ("dynamic", 11)))
