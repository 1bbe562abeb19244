"""Generate the fixtures of the last two Control/MPC closed loops from the reference's OWN code.

Run where the reference checkout exists (see make_golden.py, whose stub machinery is
imported here: the osqp capture stub, _OracleOSQP behind it, _csc, _save):
    MPLBACKEND=Agg python tests/golden/make_golden_loops.py [lane_sim lane_run kinfrozen_sim kinfrozen_run]

Only DATA is committed.  Control/MPC/mpc_increment_kinematics_pred_matrix.py:main and
Control/MPC/mpc_kinematics.py:main are run from their own source text (inspect.getsource) with
N, sim_time and the step count replaced, capture calls inserted and the plotting replaced by
no-ops; nothing of that text is kept.  The solutions come from this repository's CPU oracle
behind the osqp stub, so the fixtures pin the reference's data path around the solve, not the
solve.  Every captured solve must end `solved`.

mpc_kinematics.main as written passes a float count to np.linspace (:290-292), which present
numpy rejects: that expression is replaced by its int(...).  Its initial pred_u is random
(:318-323): numpy is seeded before the call and the initial pred_u / pred_x are stored.

Fixtures (lane = mpc_increment_kinematics_pred_matrix.main, kinfrozen = mpc_kinematics.main):
  lane_sim_n2.npz, lane_sim_n3.npz, lane_sim_n10.npz
                       three steps with sim_time = 10, so the path switches (i > 0.5, i > 1.5)
                       fall between them: step 0 on path 0, step 1 on path 1, step 2 on path 0.
                       Each step's inputs (x~, pred_x~, pred_du, the path it searched, Xr,
                       Ad/Bd/gd lists), its QP (one CSC of A per step), the oracle's solution
                       and iteration count, and x~, pred_x~, pred_du, the recorded row after
                       the tail
  lane_sim_n40.npz     the same for two steps at main's own N = 40
  lane_run_n10.npz     60 steps at N = 10 with sim_time = 200 (switches after steps 10 and 30):
                       the rows of plt_states / plt_actions, and traj_sens: per column, the
                       largest difference between this run and the same run with the oracle at
                       eps_abs = eps_rel = 1e-6
  kinfrozen_sim_n2.npz, kinfrozen_sim_n3.npz, kinfrozen_sim_n20.npz
                       three steps, seed 0: the initial pred_u / pred_x, each step's inputs (x,
                       u, pred_x, Xr, the one model), its QP, the solution, and x, u, pred_x,
                       the recorded row after the tail
  kinfrozen_sim_n100.npz  the same for two steps at main's own N = 100
  kinfrozen_run_n20.npz   30 steps at N = 20, seed 0: traj and traj_sens as above
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
from make_golden_ltv import _TightOracleOSQP, _sub  # noqa: E402

SEED = 0


def _path_x():
    return np.linspace(-10, 100, int(100 / 0.5))


def _run(mod, src, ns_extra, oracle, seed=None):
    ns = dict(vars(mod))
    ns.update(ns_extra)
    ns["plt"] = _Quiet()                       # plt.pause and the per-step drawing neutralised
    ns["plot_car"] = lambda *a, **k: None
    exec(compile(src, mod.__name__ + ".py", "exec"), ns)
    sys.modules["osqp"].OSQP = oracle or mg._OracleOSQP
    mg.captured.clear()
    if seed is not None:
        np.random.seed(seed)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ns["main"]()
    finally:
        sys.modules["osqp"].OSQP = mg._CaptureOSQP
    cap = list(mg.captured)
    for c in cap:
        assert c["kind"] != "solve" or c["status"] == "solved", c
    return cap


def _qp_record(d, cap, steps):
    setups = [c for c in cap if c["kind"] == "setup"]
    sols = [c for c in cap if c["kind"] == "solve"]
    assert len(setups) == len(sols) == steps
    mg._csc("P", setups[0]["P"], d)
    d["settings"] = np.array(json.dumps(setups[0]["kw"]))
    for t, s_ in enumerate(setups):  # A's structural zeros follow the step's Ad / Bd: one CSC per step
        mg._csc(f"A{t}", s_["A"], d)
    d.update(q=np.stack([s_["q"] for s_ in setups]), l=np.stack([s_["l"] for s_ in setups]),
             u=np.stack([s_["u"] for s_ in setups]), sol=np.stack([s_["x"] for s_ in sols]),
             sol_iter=np.array([s_["iter"] for s_ in sols]))


def _stack(d, rec, side, keys):
    for k in keys:
        d[f"{side}_{k}"] = np.stack([r[k] for r in rec[side]])


# ------------------------------------------------------------------ the lane-change loop --
def _run_lane(N, sim_time, steps, oracle=None):
    """main() of mpc_increment_kinematics_pred_matrix with N, sim_time and the number of loop
    passes replaced; returns (the capture record, the osqp stub's captured setups / solves)."""
    import mpc_increment_kinematics_pred_matrix as mk
    src = inspect.getsource(mk.main)
    src = _sub(src, "    N = 40 # Prediction horizon\n", f"    N = {N}\n")
    src = _sub(src, "    sim_time = 1000\n", f"    sim_time = {sim_time}\n")
    src = _sub(src, "    for i in range(sim_time):\n", f"    for i in range({steps}):\n")
    src = _sub(src, "        # Solve MPC\n",
               "        _cap_in(i, x_tilda_vec, pred_x_tilda, pred_del_u, Xr, Ad_list, Bd_list, gd_list, path_y)\n"
               "        # Solve MPC\n")
    src = _sub(src, "        pred_del_u[:,-1] = pred_del_u[:,-2]\n",
               "        pred_del_u[:,-1] = pred_del_u[:,-2]\n"
               "        _cap_out(i, x_tilda, pred_x_tilda, pred_del_u, plt_states[:,i], plt_actions[:,i])\n")
    rec = {"in": [], "out": []}
    cap_in = lambda i, xt, pred, pdu, Xr, A_, B_, g_, py: rec["in"].append(
        dict(i=i, xt=xt.copy(), pred=pred.copy(), pdu=pdu.copy(), Xr=Xr.copy(), Ad=np.stack(A_), Bd=np.stack(B_),
             gd=np.stack(g_)[..., 0], path_y=py.copy()))
    cap_out = lambda i, xt, pred, pdu, ps, pa: rec["out"].append(
        dict(i=i, xt=xt[:, 0].copy(), pred=pred.copy(), pdu=pdu.copy(), row=np.concatenate([ps, pa])))
    cap = _run(mk, src, dict(_cap_in=cap_in, _cap_out=cap_out), oracle)
    assert [r["i"] for r in rec["in"]] == list(range(steps)) == [r["i"] for r in rec["out"]]
    return rec, cap


def _lane_scenario(sim_time):
    """The script's two lanes (:317-319, :382-391) and its switches as integer thresholds:
    i > 0.05 sim_time  <=>  i > floor(0.05 sim_time) for integer i."""
    px = _path_x()
    return px, np.stack([px * 0.0 + 0.0, px * 0.0 + 4]), np.array(
        [int(np.floor(0.05 * sim_time)), int(np.floor(0.15 * sim_time))], np.int32)


def _lane_path_ids(rec, paths_y):
    ids = []
    for r in rec["in"]:
        hit = [p for p in range(len(paths_y)) if np.array_equal(r["path_y"], paths_y[p])]
        assert len(hit) == 1
        ids.append(hit[0])
    return np.array(ids, np.int32)


def _lane_sim(name, N, steps, sim_time=10):
    rec, cap = _run_lane(N, sim_time, steps)
    d = {}
    _qp_record(d, cap, steps)
    _stack(d, rec, "in", ("xt", "pred", "pdu", "Xr", "Ad", "Bd", "gd"))
    _stack(d, rec, "out", ("xt", "pred", "pdu", "row"))
    px, paths_y, sw = _lane_scenario(sim_time)
    d["in_path_id"] = _lane_path_ids(rec, paths_y)
    if steps >= 3:  # one captured step on each side of each switch
        assert d["in_path_id"].tolist()[:3] == [0, 1, 0], d["in_path_id"]
    d.update(path_x=px, paths_y=paths_y, switch_steps=sw, paths_of=np.array([0, 1, 0], np.int32),
             sim_time=np.array(sim_time), N=np.array(N))
    mg._save(name, d)


def lane_sim():
    for N in (2, 3, 10):
        _lane_sim(f"lane_sim_n{N}.npz", N, 3)
    _lane_sim("lane_sim_n40.npz", 40, 2)


def _sens(rec, rec_t, what):
    traj = np.stack([r["row"] for r in rec["out"]])
    tight = np.stack([r["row"] for r in rec_t["out"]])
    sens = np.abs(traj - tight).max(0)
    assert (sens > 0).all(), (what, sens)
    return traj, sens


def lane_run(N=10, steps=60, sim_time=200):
    rec, cap = _run_lane(N, sim_time, steps)
    rec_t, _ = _run_lane(N, sim_time, steps, oracle=_TightOracleOSQP)
    traj, sens = _sens(rec, rec_t, "lane_run")      # (steps, 6): x, y, v, yaw, steer, accel
    iters = np.array([c["iter"] for c in cap if c["kind"] == "solve"])
    print("lane_run: traj_sens", sens, "iters", iters.min(), iters.max())
    px, paths_y, sw = _lane_scenario(sim_time)
    ids = _lane_path_ids(rec, paths_y)
    assert ids[10] == 0 and ids[11] == 1 and ids[30] == 1 and ids[31] == 0 and sw.tolist() == [10, 30]
    mg._save("lane_run_n10.npz", dict(traj=traj, traj_sens=sens, x0=rec["in"][0]["xt"][:4], u0=rec["in"][0]["xt"][4:],
                                      N=np.array(N), steps=np.array(steps), iters=iters, path_x=px, paths_y=paths_y,
                                      switch_steps=sw, paths_of=np.array([0, 1, 0], np.int32), path_id=ids))


# ------------------------------------------------------------------ the frozen-model loop --
def _run_frozen(N, steps, oracle=None):
    """main() of mpc_kinematics with N and sim_time replaced, the float linspace count made an
    int, numpy seeded; returns (the capture record, the stub's captured setups / solves)."""
    import mpc_kinematics as mk
    src = inspect.getsource(mk.main)
    src = _sub(src, "    N = 100 # Prediction horizon\n", f"    N = {N}\n")
    assert src.count(", 100/0.5)") == 2
    src = src.replace(", 100/0.5)", ", int(100/0.5))")
    src = _sub(src, "    sim_time = 1000\n", f"    sim_time = {steps}\n")
    src = _sub(src, "    # ========== Reference state ==========\n",
               "    _cap_init(x0, u0, x, u, pred_x, pred_u)\n    # ========== Reference state ==========\n")
    src = _sub(src, "        # Solve MPC\n",
               "        _cap_in(i, x_vec, u, pred_x, Xr, Ad_mat, Bd_mat, gd_mat)\n        # Solve MPC\n")
    src = _sub(src, "        x = x_next\n",
               "        x = x_next\n        _cap_out(i, x, u, pred_x, plt_states[:,i], plt_actions[:,i])\n")
    rec = {"init": [], "in": [], "out": []}
    cap_init = lambda x0, u0, x, u, px_, pu_: rec["init"].append(
        dict(x0_after=x0[:, 0].copy(), u0=u0[:, 0].copy(), x=x[:, 0].copy(), u=u[:, 0].copy(), pred_x=px_.copy(),
             pred_u=pu_.copy()))
    cap_in = lambda i, xv, u, px_, Xr, A_, B_, g_: rec["in"].append(
        dict(i=i, x=xv.copy(), u=u[:, 0].copy(), pred_x=px_.copy(), Xr=Xr.copy(), Ad=A_.copy(), Bd=B_.copy(),
             gd=g_[:, 0].copy()))
    cap_out = lambda i, x, u, px_, ps, pa: rec["out"].append(
        dict(i=i, x=x[:, 0].copy(), u=u[:, 0].copy(), pred_x=px_.copy(), row=np.concatenate([ps, pa])))
    cap = _run(mk, src, dict(_cap_init=cap_init, _cap_in=cap_in, _cap_out=cap_out), oracle, seed=SEED)
    assert [r["i"] for r in rec["in"]] == list(range(steps)) == [r["i"] for r in rec["out"]]
    return rec, cap


def _frozen_common(rec):
    px = _path_x()
    init = rec["init"][0]
    # main's own start (:297-302); the rollout (:327-329) advances it in place through x0 = x
    return dict(path_x=px, path_y=px * 0.0 - 5.0, x0=init["pred_x"][:, 0].copy(), u0=init["u0"],
                x_start=init["x"], init_pred_x=init["pred_x"], init_pred_u=init["pred_u"], seed=np.array(SEED))


def _frozen_sim(name, N, steps):
    rec, cap = _run_frozen(N, steps)
    d = {}
    _qp_record(d, cap, steps)
    _stack(d, rec, "in", ("x", "u", "pred_x", "Xr", "Ad", "Bd", "gd"))
    _stack(d, rec, "out", ("x", "u", "pred_x", "row"))
    d.update(_frozen_common(rec), N=np.array(N))
    mg._save(name, d)


def kinfrozen_sim():
    for N in (2, 3, 20):
        _frozen_sim(f"kinfrozen_sim_n{N}.npz", N, 3)
    _frozen_sim("kinfrozen_sim_n100.npz", 100, 2)


def kinfrozen_run(N=20, steps=30):
    rec, cap = _run_frozen(N, steps)
    rec_t, _ = _run_frozen(N, steps, oracle=_TightOracleOSQP)
    traj, sens = _sens(rec, rec_t, "kinfrozen_run")  # (steps, 6): x, y, v, yaw, steer, accel
    iters = np.array([c["iter"] for c in cap if c["kind"] == "solve"])
    print("kinfrozen_run: traj_sens", sens, "iters", iters.min(), iters.max())
    mg._save("kinfrozen_run_n20.npz", dict(traj=traj, traj_sens=sens, N=np.array(N), steps=np.array(steps),
                                           iters=iters, **_frozen_common(rec)))


if __name__ == "__main__":
    mg._install_stub()
    which = set(sys.argv[1:])
    for f in (lane_sim, lane_run, kinfrozen_sim, kinfrozen_run):
        if not which or f.__name__ in which:
            f()
