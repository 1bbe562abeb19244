"""Generate the kinematic-loop fixtures from the reference's OWN code.

Run where the reference checkout exists (see make_golden.py, whose stub machinery is
imported here: the osqp capture stub, _OracleOSQP behind it, _csc, _save):
    MPLBACKEND=Agg python tests/golden/make_golden_kin.py [kin_linearise kin_refsearch kin_sim kin_stop]

Only DATA is committed.  Control/MPC/mpc_incre_kine_func.py:simulate is run from its own
source text (inspect.getsource) with capture calls inserted and its plotting replaced by
no-ops; nothing of that text is kept.  The solutions come from this repository's CPU
oracle behind the osqp stub, so the fixtures pin the reference's data path around the
solve, not the solve.

Fixtures:
  kin_linearise.npz  Vehicle_Kinematics.get_kinematics_model (vehicle_models.py:835-863) at 48
                     seeded (x, u), incl. yaw = 0, steer = 0 and negative v
  kin_refsearch.npz  mpc_incre_kine_func.py:28-81 reference_search (with nearest_point) on
                     main()'s path (:440-442) with a non-zero path_yaw, 64 seeded predicted
                     horizons, a quarter reversing
  kin_sim_n40.npz    simulate (:223-436) from (0, -3.7, 10, 0.02) for 3 steps: each step's
                     inputs (x~, predicted horizon, pred_du, Xr, Ad/Bd/gd lists), its QP
                     (one CSC of A per step), the oracle's solution and iteration count,
                     and the state after the plant step and horizon shift
  kin_stop_n40.npz   the same start run until simulate breaks by itself: the four trajectory
                     lists, the number of loop passes, each pass's stop-rule distance, and
                     traj_sens: per trajectory, the largest difference between this run and
                     the same run with the oracle at eps_abs = eps_rel = 1e-6
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

START = (0.0, -3.7, 10.0, 0.02)


def _main_path():
    """mpc_incre_kine_func.main's path (:440-442)."""
    px = np.linspace(-10, 100, int(100 / 0.5))
    return px, px * 0.0 - 4.0, px * 0.0


def kin_linearise():
    import vehicle_models
    veh = vehicle_models.Vehicle_Kinematics(l_f=1.25, l_r=1.40, dt=0.02)
    rng = np.random.default_rng(17)
    X, U, Ad, Bd, gd = [], [], [], [], []
    for t in range(48):
        x = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(2, 25), rng.uniform(-np.pi, np.pi)])
        u = np.array([np.deg2rad(rng.uniform(-15, 15)), rng.uniform(-3, 1)])
        if t >= 40:  # special points: yaw 0, steer 0, both, reversing, standstill
            x[3] = [0.0, x[3], 0.0, x[3], x[3], 0.0, x[3], x[3]][t - 40]
            u[0] = [u[0], 0.0, 0.0, u[0], u[0], 0.0, u[0], 0.0][t - 40]
            x[2] = [x[2], x[2], x[2], -4.0, -0.3, -12.0, 0.0, x[2]][t - 40]
        A_, B_, C_ = veh.get_kinematics_model(x.copy(), u.copy())
        X.append(x); U.append(u); Ad.append(A_); Bd.append(B_); gd.append(C_[:, 0])
    mg._save("kin_linearise.npz", dict(x=np.stack(X), u=np.stack(U), Ad=np.stack(Ad), Bd=np.stack(Bd),
                                       gd=np.stack(gd), l_f=np.array(1.25), l_r=np.array(1.40), dt=np.array(0.02)))


def kin_refsearch():
    import mpc_incre_kine_func as mf
    px, py, _ = _main_path()
    pyaw = 0.05 * np.sin(px / 7.0) + 0.01
    rng = np.random.default_rng(23)
    B, N, dt = 64, 40, 0.02
    preds, xrs, speeds = [], [], []
    for b in range(B):
        s0 = rng.uniform(-5, 60)
        pred = np.zeros((4, N + 1))
        pred[0] = s0 + rng.normal(0, 1)
        pred[1] = -4.0 + rng.normal(0, 3)
        pred[2] = rng.uniform(0, 30, N + 1) * (-1 if b < B // 4 else 1)  # reversing: |v| is used
        pred[3] = rng.uniform(-0.3, 0.3, N + 1)
        speed = rng.uniform(5, 25)
        Xr, _ = mf.reference_search(px, py, pyaw, speed, pred, dt, N)
        preds.append(pred); xrs.append(Xr); speeds.append(speed)
    mg._save("kin_refsearch.npz", dict(path_x=px, path_y=py, path_yaw=pyaw, set_speed=np.array(speeds),
                                       pred=np.stack(preds), Xr=np.stack(xrs), dt=np.array(dt)))


class _Quiet:
    """Stands in for matplotlib.pyplot inside simulate: every call (cla, plot, pause, ...) is a no-op."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def _run_simulate(sim_time=None, oracle=None):
    """simulate(START, main()'s path) from its source text with capture calls inserted;
    returns (the four lists, the capture record, the osqp stub's captured setups / solves)."""
    import mpc_incre_kine_func as mf
    src = inspect.getsource(mf.simulate)
    if sim_time is not None:
        src = src.replace("sim_time = 5000", f"sim_time = {sim_time}")
        assert f"sim_time = {sim_time}" in src
    src = src.replace("        # Solve MPC\n",
                      "        _cap_in(i, x_tilda_vec, pred_x_tilda, pred_del_u, Xr, Ad_list, Bd_list, gd_list)\n"
                      "        # Solve MPC\n")
    src = src.replace('        print("dist :", dist)\n', '        print("dist :", dist)\n        _cap_dist(dist)\n')
    src = src.replace("        toc = time.time()\n", "        _cap_out(i, x_tilda, pred_x_tilda, pred_del_u)\n"
                                                     "        toc = time.time()\n")
    assert "_cap_in" in src and "_cap_out" in src and "_cap_dist" in src
    rec = {"in": [], "out": [], "dist": []}
    ns = dict(vars(mf))
    ns["_cap_in"] = lambda i, xt, pred, pdu, Xr, A_, B_, g_: rec["in"].append(
        dict(xt=xt.copy(), pred=pred.copy(), pdu=pdu.copy(), Xr=Xr.copy(), Ad=np.stack(A_), Bd=np.stack(B_),
             gd=np.stack(g_)[..., 0]))
    ns["_cap_out"] = lambda i, xt, pred, pdu: rec["out"].append(dict(xt=xt[:, 0].copy(), pred=pred.copy(),
                                                                   pdu=pdu.copy()))
    ns["_cap_dist"] = lambda d: rec["dist"].append(float(d))
    ns["plt"] = _Quiet()                       # plt.pause and the per-step drawing neutralised
    ns["plot_car"] = lambda *a, **k: None
    exec(compile(src, "mpc_incre_kine_func.py", "exec"), ns)
    px, py, pyaw = _main_path()
    sys.modules["osqp"].OSQP = oracle or mg._OracleOSQP
    mg.captured.clear()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            lists = ns["simulate"](np.array(START).reshape(4, 1), px, py, pyaw)
    finally:
        sys.modules["osqp"].OSQP = mg._CaptureOSQP
    return [np.array(v, float) for v in lists], rec, list(mg.captured)


def kin_sim(steps=3):
    _, rec, cap = _run_simulate(sim_time=steps)
    setups = [c for c in cap if c["kind"] == "setup"]
    sols = [c for c in cap if c["kind"] == "solve"]
    assert len(setups) == len(sols) == len(rec["in"]) == len(rec["out"]) == steps
    d = {}
    mg._csc("P", setups[0]["P"], d)
    d["settings"] = np.array(json.dumps(setups[0]["kw"]))
    for k in ("xt", "pred", "pdu", "Xr", "Ad", "Bd", "gd"):
        d["in_" + k] = np.stack([r[k] for r in rec["in"]])
    for k in ("xt", "pred", "pdu"):
        d["out_" + k] = np.stack([r[k] for r in rec["out"]])
    for t, s_ in enumerate(setups):  # A's structural zeros follow the step's Ad / Bd: one CSC per step
        mg._csc(f"A{t}", s_["A"], d)
    d.update(q=np.stack([s_["q"] for s_ in setups]), l=np.stack([s_["l"] for s_ in setups]),
             u=np.stack([s_["u"] for s_ in setups]), sol=np.stack([s_["x"] for s_ in sols]),
             sol_iter=np.array([s_["iter"] for s_ in sols]))
    px, py, pyaw = _main_path()
    d.update(path_x=px, path_y=py, path_yaw=pyaw, x0=np.array(START))
    mg._save("kin_sim_n40.npz", d)


class _TightOracleOSQP(mg._OracleOSQP):
    def setup(self, P, q, A, l, u, **kw):
        super().setup(P, q, A, l, u, **dict(kw, eps_abs=1e-6, eps_rel=1e-6))


def kin_stop():
    lists, rec, cap = _run_simulate()
    tight, rec_t, cap_t = _run_simulate(oracle=_TightOracleOSQP)
    steps = len(rec["dist"])
    # both runs stop at the same step
    assert steps == len(rec_t["dist"]), (steps, len(rec_t["dist"]))
    assert all(len(v) == steps + 1 for v in lists + tight)
    # every solve is `solved`
    for c in cap + cap_t:
        assert c["kind"] != "solve" or c["status"] == "solved", c
    sens = np.array([np.abs(a - b).max() for a, b in zip(lists, tight)])
    dist = np.array(rec["dist"])
    # no distance is within 2 traj_sens[x] of the stop rule's 0.5
    assert np.abs(dist - 0.5).min() > 2 * sens[0], (np.abs(dist - 0.5).min(), sens)
    iters = np.array([c["iter"] for c in cap if c["kind"] == "solve"])
    print("kin_stop: steps", steps, "min |dist - 0.5|", np.abs(dist - 0.5).min(), "traj_sens", sens, "iters",
          iters.min(), iters.max())
    px, py, pyaw = _main_path()
    mg._save("kin_stop_n40.npz", dict(traj_x=lists[0], traj_y=lists[1], traj_yaw=lists[2], traj_steer=lists[3],
                                      steps=np.array(steps), dist=dist, traj_sens=sens, x0=np.array(START),
                                      path_x=px, path_y=py, path_yaw=pyaw))


if __name__ == "__main__":
    mg._install_stub()
    which = set(sys.argv[1:])
    for f in (kin_linearise, kin_refsearch, kin_sim, kin_stop):
        if not which or f.__name__ in which:
            f()
