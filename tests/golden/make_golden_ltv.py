"""Generate the direct-input LTV loop fixtures from the reference's OWN code.

Run where the reference checkout exists (see make_golden.py, whose stub machinery is
imported here: the osqp capture stub, _OracleOSQP behind it, _csc, _save):
    MPLBACKEND=Agg python tests/golden/make_golden_ltv.py [kinltv_sim_n40 kinltv_sim_n100 kinltv_sim_small kinltv_run]

Only DATA is committed.  Control/MPC/mpc_kinematics_pred_matrix.py:main is run from its own
source text (inspect.getsource) with N / sim_time replaced, capture calls inserted and its
plotting replaced by no-ops; nothing of that text is kept.  The solutions come from this
repository's CPU oracle behind the osqp stub, so the fixtures pin the reference's data path
around the solve, not the solve.

Fixtures:
  kinltv_sim_n40.npz   main (:355-563) with N = 40 for 3 steps: each step's inputs (x, the
                       predicted horizon pred_x / pred_u, Xr, Ad/Bd/gd lists), its QP (one CSC
                       of A per step: the structural zeros follow the values), the oracle's
                       solution and iteration count, and x, pred_x, pred_u after the shift
  kinltv_sim_n100.npz  the same for 2 steps at main's own N = 100
  kinltv_sim_n2.npz, kinltv_sim_n3.npz  the same for 3 steps at the shortest horizons (N = 2: the
                       shift's copy loops of main run zero times)
  kinltv_run_n20.npz   40 steps at N = 20: the rows of plt_states / plt_actions, and traj_sens:
                       per column, the largest difference between this run and the same run
                       with the oracle at eps_abs = eps_rel = 1e-6; every solve is `solved`
"""
import contextlib
import inspect
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
from make_golden_kin import _Quiet  # noqa: E402


def _main_path():
    """mpc_kinematics_pred_matrix.main's path (:377-379)."""
    px = np.linspace(-10, 100, int(100 / 0.5))
    return px, px * 0.0 - 5.0


def _sub(src, old, new):
    assert src.count(old) == 1, (old, src.count(old))
    return src.replace(old, new)


def _run_main(N, steps, oracle=None):
    """main() (its own start (0, 0, 20, 0) and path y = -5) from its source text with N and
    sim_time replaced and capture calls inserted; returns (the capture record, the osqp
    stub's captured setups / solves)."""
    import mpc_kinematics_pred_matrix as mk
    src = inspect.getsource(mk.main)
    src = _sub(src, "    N = 100 # Prediction horizon\n", f"    N = {N}\n")
    src = _sub(src, "    sim_time = 1000\n", f"    sim_time = {steps}\n")
    src = _sub(src, "        # Solve MPC\n",
               "        _cap_in(i, x, pred_x, pred_u, Xr, Ad_list, Bd_list, gd_list)\n        # Solve MPC\n")
    src = _sub(src, "        pred_u[:,-1] = pred_u[:,N-1]\n",
               "        pred_u[:,-1] = pred_u[:,N-1]\n"
               "        _cap_out(i, x, pred_x, pred_u, plt_states[:,i], plt_actions[:,i])\n")
    rec = {"in": [], "out": []}
    ns = dict(vars(mk))
    ns["_cap_in"] = lambda i, x, px_, pu_, Xr, A_, B_, g_: rec["in"].append(
        dict(i=i, x=x[:, 0].copy(), pred_x=px_.copy(), pred_u=pu_.copy(), Xr=Xr.copy(), Ad=np.stack(A_),
             Bd=np.stack(B_), gd=np.stack(g_)[..., 0]))
    ns["_cap_out"] = lambda i, x, px_, pu_, ps, pa: rec["out"].append(
        dict(i=i, x=x[:, 0].copy(), pred_x=px_.copy(), pred_u=pu_.copy(), row=np.concatenate([ps, pa])))
    ns["plt"] = _Quiet()                       # plt.pause and the per-step drawing neutralised
    ns["plot_car"] = lambda *a, **k: None
    exec(compile(src, "mpc_kinematics_pred_matrix.py", "exec"), ns)
    sys.modules["osqp"].OSQP = oracle or mg._OracleOSQP
    mg.captured.clear()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ns["main"]()
    finally:
        sys.modules["osqp"].OSQP = mg._CaptureOSQP
    return rec, list(mg.captured)


def _sim(name, N, steps):
    rec, cap = _run_main(N, steps)
    setups = [c for c in cap if c["kind"] == "setup"]
    sols = [c for c in cap if c["kind"] == "solve"]
    assert len(setups) == len(sols) == len(rec["in"]) == len(rec["out"]) == steps
    assert all(s_["status"] == "solved" for s_ in sols)
    d = {}
    mg._csc("P", setups[0]["P"], d)
    d["settings"] = np.array(json.dumps(setups[0]["kw"]))
    for k in ("x", "pred_x", "pred_u", "Xr", "Ad", "Bd", "gd"):
        d["in_" + k] = np.stack([r[k] for r in rec["in"]])
    for k in ("x", "pred_x", "pred_u", "row"):
        d["out_" + k] = np.stack([r[k] for r in rec["out"]])
    for t, s_ in enumerate(setups):  # A's structural zeros follow the step's Ad / Bd: one CSC per step
        mg._csc(f"A{t}", s_["A"], d)
    d.update(q=np.stack([s_["q"] for s_ in setups]), l=np.stack([s_["l"] for s_ in setups]),
             u=np.stack([s_["u"] for s_ in setups]), sol=np.stack([s_["x"] for s_ in sols]),
             sol_iter=np.array([s_["iter"] for s_ in sols]))
    px, py = _main_path()
    d.update(path_x=px, path_y=py, x0=rec["in"][0]["x"], u0=rec["in"][0]["pred_u"][:, 0])
    mg._save(name, d)


def kinltv_sim_n40():
    _sim("kinltv_sim_n40.npz", 40, 3)


def kinltv_sim_n100():
    _sim("kinltv_sim_n100.npz", 100, 2)


def kinltv_sim_small():
    _sim("kinltv_sim_n2.npz", 2, 3)
    _sim("kinltv_sim_n3.npz", 3, 3)


class _TightOracleOSQP(mg._OracleOSQP):
    def setup(self, P, q, A, l, u, **kw):
        super().setup(P, q, A, l, u, **dict(kw, eps_abs=1e-6, eps_rel=1e-6))


def kinltv_run(N=20, steps=40):
    rec, cap = _run_main(N, steps)
    rec_t, cap_t = _run_main(N, steps, oracle=_TightOracleOSQP)
    # every solve is `solved`, so the reference skipped no step
    for c in cap + cap_t:
        assert c["kind"] != "solve" or c["status"] == "solved", c
    assert [r["i"] for r in rec["out"]] == list(range(steps)) == [r["i"] for r in rec_t["out"]]
    traj = np.stack([r["row"] for r in rec["out"]])          # (steps, 6): x, y, v, yaw, steer, accel
    tight = np.stack([r["row"] for r in rec_t["out"]])
    sens = np.abs(traj - tight).max(0)
    assert (sens > 0).all(), sens
    iters = np.array([c["iter"] for c in cap if c["kind"] == "solve"])
    print("kinltv_run: traj_sens", sens, "iters", iters.min(), iters.max())
    px, py = _main_path()
    mg._save("kinltv_run_n20.npz", dict(traj=traj, traj_sens=sens, x0=rec["in"][0]["x"],
                                        u0=rec["in"][0]["pred_u"][:, 0], N=np.array(N), steps=np.array(steps),
                                        iters=iters, path_x=px, path_y=py))


if __name__ == "__main__":
    mg._install_stub()
    which = set(sys.argv[1:])
    for f in (kinltv_sim_n40, kinltv_sim_n100, kinltv_sim_small, kinltv_run):
        if not which or f.__name__ in which:
            f()
