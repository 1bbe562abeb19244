"""The ADMM shell the solve kernels share (solve_phases.h: reject_instance, run_stop, adapt_rho,
check_and_adapt, conclude), run through every production kernel family at B = 3: solves that
end at the iteration cap (the conclusion's own checks, with and without rho steps before it)
against the CPU oracle, and an instance with invalid data next to two valid ones.

Seeds (mpc.make_batch(cfg, B=3, seed), chosen with the oracle alone): under every capped
setting below all three instances are still unsolved at the cap, so both sides stop at the
same count by construction.  The oracle's iteration counts at the default settings:
  cfg 2, seed 337: 225, 100, 225     cfg 3, seed 6: 150, 375, 250     cfg 5, seed 75: 625, 650, 325
cfg 2 has no seed below 600 whose three instances are all unsolved after 120 iterations with a
rho step every 50 (most of its instances solve in 25 to 150): its third setting's cap is 90 --
still a rho step (at 50) with the cap after it.

tools/isa_diff.py (CPU): the production library against itself."""
import functools
import os
import sys

import numpy as np
import pytest

import isa_shape
import pyoracle
from parity import check_agreement
from solve_families import FAMILIES, batch as _batch, env as _env, handle as _handle, run as _run, \
    out_of as _out_of, settings as _settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "python-mpc_amd", "osqp_amd", "libmpcqp.so")


def _capped(cfg):
    return {
        "cap_between_checks": dict(max_iter=30),  # the conclusion's first and approximate checks
        "no_check": dict(max_iter=60, check_termination=0),  # no check before the conclusion
        # rho steps and refactorisations, the cap after a rho step (cfg 2: see the module docstring)
        "rho_steps": dict(max_iter=90 if cfg == 2 else 120, adaptive_rho_interval=50),
    }


@functools.lru_cache(maxsize=None)
def _oracle(cfg, setting):
    b = _batch(cfg)
    bo = pyoracle.solve_batch(b["P"], b["A"], b["Px"], b["q"], b["Ax"], b["l"], b["u"],
                              **_settings(cfg, **_capped(cfg)[setting]))
    cap = _capped(cfg)[setting]["max_iter"]
    assert (bo.iter == cap).all() and (bo.status_val != 1).all(), (bo.iter, bo.status_val)  # (the seeds' premise)
    return bo


def _check_capped(label, cfg, setting, x, y, st, it):
    bo = _oracle(cfg, setting)
    print(label, "status", st, "iter", it, "oracle", bo.status_val, bo.iter)
    check_agreement(label, _batch(cfg), x, y, st, it, bo, min_match=1.0)


def _bad_lower(X):
    """The lower bounds with l > u in one row of instance 1."""
    bad = X[3].clone()
    bad[1, 10] = X[4][1, 10] + 1.0
    return bad


def _check_invalid(first, second):
    (x1, y1, st1, it1), (x2, y2, st2, it2) = first, second
    print("first", st1, it1, "second", st2, it2)
    assert (st1 == 1).all() and (it1 > 0).all()
    assert st2[1] == -7 and it2[1] == 0
    assert np.isnan(x2[1]).all() and np.isnan(y2[1]).all()
    for i in (0, 2):
        assert st2[i] == 1 and it2[i] > 0 and it2[i] == it1[i]
        assert np.array_equal(x2[i], x1[i]) and np.array_equal(y2[i], y1[i])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["cap_between_checks", "no_check", "rho_steps"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_capped_runs_match_oracle(family, setting, monkeypatch):
    cfg, variant, elim, vid = FAMILIES[family]
    _env(monkeypatch, variant, elim)
    h, X = _handle(cfg, **_capped(cfg)[setting])
    assert h.plan_info()["variant"] == vid
    _check_capped(f"shell {family} {setting}", cfg, setting, *_run(h, X, False))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_invalid_instance_exits(family, monkeypatch):
    """update(l) with l > u in one row of instance 1: that instance exits before any iteration
    (status 'non convex', iter 0, NaN x and y); the cold solves of the other two repeat bit for bit.
    A solve leaves its adapted rho behind for the next one (as OSQP does: without more, the second
    solve of cfg 2 takes 50 iterations where the first took 225), so a cold second solve needs the
    setup repeated before the update: then both start from the settings' rho."""
    cfg, variant, elim, vid = FAMILIES[family]
    _env(monkeypatch, variant, elim)
    h, X = _handle(cfg)
    assert h.plan_info()["variant"] == vid
    first = _run(h, X, False)
    h.setup(*X)
    h.update(l=_bad_lower(X))
    o = _out_of(h)
    h.solve(*o)
    h.synchronize()
    _check_invalid(first, [t.cpu().numpy() for t in o])


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["w4", "w4_elim"])
def test_one_shot_capped_run_matches_oracle(family, monkeypatch):
    cfg, variant, elim, vid = FAMILIES[family]
    _env(monkeypatch, variant, elim)
    h, X = _handle(cfg, one_shot=True, **_capped(cfg)["cap_between_checks"])
    assert h.plan_info()["variant"] == vid
    _check_capped(f"shell one-shot {family}", cfg, "cap_between_checks", *_run(h, X, True))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["w4", "w4_elim"])
def test_one_shot_invalid_instance_exits(family, monkeypatch):
    cfg, variant, elim, vid = FAMILIES[family]
    _env(monkeypatch, variant, elim)
    h, X = _handle(cfg, one_shot=True)
    assert h.plan_info()["variant"] == vid
    first = _run(h, X, True)
    _check_invalid(first, _run(h, X[:3] + [_bad_lower(X), X[4]], True))


@pytest.mark.skipif(not isa_shape.tools_present() or not os.path.exists(LIB), reason="no llvm tools or library")
def test_isa_diff_of_the_library_against_itself():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_diff
    rows, only = isa_diff.diff(LIB, LIB)
    assert not only and len(rows) > 0
    for name, meta_equal, n_old, n_new, _, exact, norm in rows:
        assert meta_equal and n_old == n_new and exact and norm, name
    names = [r[0] for r in rows]
    for key, (symbol, _) in isa_shape.HOT.items():
        hit = [r for r in rows if symbol in r[0]]
        assert len(hit) == 1 and hit[0][4] > 0, (key, names)  # (present, with an ADMM loop selected)
