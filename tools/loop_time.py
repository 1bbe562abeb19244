#!/usr/bin/env python3
"""First timings of the closed loops on the device (osqp_amd.mpc_device).  No target; numbers to
compare later work against.

  dyn        DynamicMPC          mpc_dynamics.main
  kin        KinematicMPC        mpc_incre_kine_func.simulate
  ltv        KinematicLTVMPC     mpc_kinematics_pred_matrix.main
  lat        LateralMPC          vehicle_lateral_mpc_slack_increment.py
  lane       LaneChangeMPC       mpc_increment_kinematics_pred_matrix.main (step0 in [0, 200): both
                                 lanes are in the batch and vehicles change lane inside the window)
  kinfrozen  KinematicFrozenMPC  mpc_kinematics.main

B vehicles step N-stage horizons.  The same `--steps` steps after the warm-up steps are timed
twice, each time by a fresh controller from the same seeded starts:

  1. event timing off: host clock around the window (ends in a device synchronise) and a
     device-event pair around it -> ms_per_step, vehicle-steps/s;
  2. mpcqp_timing on: the solver's own event pairs give its setup and solve kernel time; the
     window's device-event total minus that is the data path (the loop's other kernels plus launch
     gaps), so solver + data_path = the second pass's device time ("window").

lat keeps its problem alive, so its setup is not in the step and its update launch is not
event-timed; its split is its own: a window that enqueues only the data path
(LateralAssembler.assemble + mpcqp_lti_step_device, on the loop's stream, over the solutions the
first window left) -> data_path; solver (update + solve) = the full window's device time minus
that; the pass with mpcqp_timing on gives the solve kernel's own event time.  --shim-steps K also
runs the script's loop through the `import osqp` drop-in on ONE vehicle for K steps
(tests/test_gpu_parity.py::_slack_script_loop's calls) -> shim_ms_per_step_one_vehicle.

--fleet (every loop but lat, whose model is fixed at setup) runs the same loop with a fleet of B
distinct vehicles -- masses, axle distances and, for the dynamic bicycle, drag and rolling
coefficients drawn within +-20 % of the default car's -- in place of B copies of that car.

One JSON line per horizon in --N, every horizon measured by a fresh child process under its own
time limit; a horizon that fails prints an {"error": ...} line and later ones are not started.

  python tools/loop_time.py dyn       [--N 30]     [--batch 4096] [--steps 20] [--warmup 3] [--warm-start] [--fleet]
  python tools/loop_time.py kin       [--N 40]     [--batch 4096] [--steps 50] [--warmup 5] [--warm-start]
  python tools/loop_time.py ltv       [--N 40 100] [--batch 4096] [--steps 20] [--warmup 3] [--shift-warm]
  python tools/loop_time.py lat       [--N 20 100] [--batch 4096] [--steps 50] [--warmup 5] [--step0-max 1200]
                                      [--shim-steps 200]
  python tools/loop_time.py lane      [--N 40]     [--batch 4096] [--steps 20] [--warmup 3] [--shift-warm]
  python tools/loop_time.py kinfrozen [--N 100]    [--batch 4096] [--steps 20] [--warmup 3]
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd")]

import numpy as np  # noqa: E402

CHILD_LIMIT_S = 240
PX = np.linspace(-10, 100, 200)  # the scripts' path: 200 points on a line of constant y


# ------------------------------------------------------------------- seeded starts --
def _starts(rng, B, y, v_lo=8, yaw_deg=3):
    """x0 (B, 4): X in [0, 20), then y(B), v in [v_lo, 20), yaw within +-yaw_deg; u0 = (0, 0.01)."""
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(0, 20, B)
    x0[:, 1] = y(B)
    x0[:, 2] = rng.uniform(v_lo, 20, B)
    x0[:, 3] = np.deg2rad(rng.uniform(-yaw_deg, yaw_deg, B))
    return x0, np.tile([0.0, 0.01], (B, 1))


def _beside(rng, y0, far):
    """1 to `far` m on either side of the path y = y0."""
    return lambda B: y0 + rng.uniform(1.0, far, B) * rng.choice([-1.0, 1.0], B)


def dyn_states(B, seed=5):
    """Starts around mpc_dynamics.main's own: up to 2 m beside the path's start, yaw within 8 deg, vx in [10, 20)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 6))
    x0[:, 1] = 5.0 + rng.uniform(-2, 2, B)
    x0[:, 2] = np.deg2rad(26.57 + rng.uniform(-8, 8, B))
    x0[:, 3] = rng.uniform(10, 20, B)
    return x0, np.zeros((B, 2))


def fleet_of(a, dynamic, seed=11):
    """None without --fleet (the loop's default car for everyone); with it a.batch distinct cars within
    +-20 % of the default's constants."""
    if not a.fleet:
        return None
    from osqp_amd import mpc_device as md
    rng = np.random.default_rng(seed)
    base = md.Vehicle() if dynamic else md.KinVehicle()
    names = ("m", "l_f", "l_r", "C_d", "A_f", "C_roll") if dynamic else ("l_f", "l_r")
    cls = md.Fleet if dynamic else md.KinFleet
    return cls.from_arrays(dt=base.dt, **{k: getattr(base, k) * rng.uniform(0.8, 1.2, a.batch) for k in names})


def kin_states(B, seed=5):
    """Lane-change starts around simulate's own: 1 to 4 m beside main()'s path (y = -4)."""
    rng = np.random.default_rng(seed)
    return _starts(rng, B, _beside(rng, -4.0, 4.0))


def ltv_states(B, seed=5):
    """Starts around main's own (0, 0, 20, 0): 1 to 5 m beside its path (y = -5)."""
    rng = np.random.default_rng(seed)
    return _starts(rng, B, _beside(rng, -5.0, 5.0))


def lat_states(B, step0_max, seed=5):
    """Starts around the script's own (0, 0, 5 deg, 3, 0), entering the bound schedule at a
    step drawn from [0, step0_max): 1200 spreads them over both regimes, 1 starts everyone at
    the schedule's beginning as the script does."""
    from osqp_amd import mpc
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-.02, .02, B), rng.uniform(-.05, .05, B), rng.uniform(-6, 6, B) * mpc.DEG,
                   rng.uniform(-3, 3, B), rng.uniform(-2, 2, B) * mpc.DEG], axis=1)
    return x0, rng.integers(0, step0_max, B).astype(np.int32)


def lane_states(B, seed=5):
    """Starts around main's own (0, 0, 20, 0), up to 1 m beside the lane their step0 puts them on."""
    rng = np.random.default_rng(seed)
    step0 = rng.integers(0, 200, B).astype(np.int32)
    x0, u0 = _starts(rng, B, lambda B: 4.0 * ((step0 > 50) & (step0 <= 150)) + rng.uniform(-1.0, 1.0, B))
    return x0, u0, step0


def kinfrozen_states(B, N, seed=5):
    """Starts around main's own (0, 0, 5, 30 deg), 1 to 5 m beside its path (y = -5), and the
    script's noise on the initial pred_u (:313-323: sigma 1 deg steer, 0.1 accel)."""
    rng = np.random.default_rng(seed)
    x0, u0 = _starts(rng, B, _beside(rng, -5.0, 5.0), v_lo=5, yaw_deg=30)
    pred_u0 = u0[:, None] + rng.normal(0.0, [np.deg2rad(1), 0.1], (B, N + 1, 2))
    pred_u0[:, N] = pred_u0[:, N - 1]
    return x0, u0, pred_u0


# --------------------------------------------------- controllers from those starts --
def _dyn(a, N):
    from osqp_amd.mpc_device import DynamicMPC
    x0, u0 = dyn_states(a.batch)                        # mpc_dynamics.main's path (:468-469)
    veh = fleet_of(a, True)
    return lambda: DynamicMPC(x0, u0, PX, PX * 0.5 + 5, N=N, warm_start=a.warm_start, veh=veh)


def _kin(a, N):
    from osqp_amd.mpc_device import KinematicMPC
    x0, u0 = kin_states(a.batch)                        # mpc_incre_kine_func.main's path (:440-442)
    veh = fleet_of(a, False)
    return lambda: KinematicMPC(x0, u0, PX, PX * 0.0 - 4.0, PX * 0.0, N=N, warm_start=a.warm_start, veh=veh)


def _ltv(a, N):
    from osqp_amd.mpc_device import KinematicLTVMPC
    x0, u0 = ltv_states(a.batch)                        # mpc_kinematics_pred_matrix.main's path (:377-379)
    veh = fleet_of(a, False)
    return lambda: KinematicLTVMPC(x0, u0, PX, PX * 0.0 - 5.0, N=N, shift_warm=a.shift_warm, veh=veh)


def _lat(a, N):
    from osqp_amd.mpc_device import LateralMPC
    x0, step0 = lat_states(a.batch, a.step0_max)
    return lambda: LateralMPC(x0, N=N, step0=step0)


def _lane(a, N):
    from osqp_amd.mpc_device import LaneChangeMPC
    x0, u0, step0 = lane_states(a.batch)                # main's path and its second lane (:317-319, :382-383)
    paths_y = np.stack([PX * 0.0, PX * 0.0 + 4])
    veh = fleet_of(a, False)
    return lambda: LaneChangeMPC(x0, u0, PX, paths_y, N=N, step0=step0, shift_warm=a.shift_warm, veh=veh)


def _kinfrozen(a, N):
    from osqp_amd.mpc_device import KinematicFrozenMPC
    x0, u0, pred_u0 = kinfrozen_states(a.batch, N)      # mpc_kinematics.main's path (:290-292)
    veh = fleet_of(a, False)
    return lambda: KinematicFrozenMPC(x0, u0, PX, PX * 0.0 - 5.0, N=N, pred_u0=pred_u0, veh=veh)


# --------------------------------------------------------------------- measurement --
def window(torch, steps, fn):
    """(host seconds, device-event ms, iteration counts (steps, B)) of `steps` calls of fn(); the
    counts are those of the calls that return (status, iters), None when none does."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        out = fn()
        if out is not None:
            iters.append(out[1].clone())
    e1.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, e0.elapsed_time(e1), torch.stack(iters).cpu().numpy() if iters else None


def _warmed(fresh, warmup):
    ctl = fresh()
    for _ in range(warmup):
        ctl.step()
    return ctl


def _frac(t):
    return float(t.cpu().numpy().mean())


def _line(loop, a, N, ctl, wall, dev_ms, split, config):
    info = ctl.solver.plan_info()
    plan = {k: info[k] for k in ("variant", "threads_per_qp") + (("lds_bytes_solve",) if loop["lds"] else ())
            + ("plan_choice",)}
    return {"metric": loop["metric"], "value": a.batch * a.steps / wall, "unit": "vehicle-steps/s",
            "ms_per_step": wall / a.steps * 1e3, "device_ms_per_step": dev_ms / a.steps, "split_ms_per_step": split,
            "config": {"vehicles": a.batch, "N": N, **config, **plan}}


def _iters(loop, it):
    if loop["lds"]:
        return {"iters_mean": float(it.mean()), "iters_max": int(it.max())}
    return {"iters_mean": float(it.mean()), "iters_max_per_step_mean": float(it.max(axis=1).mean())}


def measure(loop, a, N):
    """The two passes of a loop that sets its problem up every step."""
    import torch
    fresh = loop["build"](a, N)
    ctl = _warmed(fresh, a.warmup)
    wall, dev_ms, it = window(torch, a.steps, ctl.step)
    end_key, end_attr = loop["end"]
    end = _frac(getattr(ctl, end_attr))
    ctl = _warmed(fresh, a.warmup)                      # the same steps again, with the solver's events on
    ctl.solver.timing(True, setup=True)
    _, dev2_ms, it2 = window(torch, a.steps, ctl.step)
    t = ctl.solver.timing_read()
    ctl.solver.timing(False)
    solver_ms = t["setup_ms"] + t["solve_ms"]
    split = {"solver_setup": t["setup_ms"] / a.steps, "solver_solve": t["solve_ms"] / a.steps,
             "data_path": (dev2_ms - solver_ms) / a.steps, "window": dev2_ms / a.steps,
             "launches": [t["n_setup"], t["n_solve"]]}
    flag = {k: getattr(a, k) for k in loop["flags"]}
    flag["fleet"] = a.fleet
    return _line(loop, a, N, ctl, wall, dev_ms, split,
                 {"n": ctl.layout.n, "m": ctl.layout.m, **flag, "steps": a.steps, "warmup": a.warmup,
                  **_iters(loop, it), "iters_mean_split_window": float(it2.mean()),
                  "solved_frac_last": _frac(ctl.status == 1), end_key: end})


def _lat_data_path_only(ctl):
    """One step's data path alone: the assembly and the step kernel, no update and no solve."""
    from osqp_amd.mpc_device import _stream

    def fn():
        st = _stream(ctl.torch, ctl.dev)
        ctl.asm.assemble(ctl.theta, ctl.regime, out=(ctl.q, ctl.l, ctl.u), stream=st)
        ctl._tail(st)
    return lambda: ctl._on_stream(fn)


def _lat_shim_ms_per_step(steps, N):
    """The script's loop on one vehicle through the drop-in osqp module, ms per step."""
    from osqp_amd import mpc
    spec = importlib.util.spec_from_file_location("osqp", os.path.join(ROOT, "python-mpc_amd", "shim", "osqp.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    x0 = np.array([0.0, 0.0, 5 * mpc.DEG, 3.0, 0.0])
    P, q, A, l, u = mpc.slack_qp(N, x0)
    prob = shim.OSQP()
    prob.setup(P, q, A, l, u, warm_start=True)
    At, Bt = mpc.augment(mpc.LATERAL_AD, mpc.LATERAL_BD)
    t0 = None
    for i in range(steps + 5):
        if i == 5:
            t0 = time.perf_counter()
        _, q, _, l, u = mpc.slack_qp(N, x0, regime=int(mpc.slack_regime(i)))
        prob.update(q=q, l=l, u=u)
        res = prob.solve()
        x0 = At @ x0 + Bt @ res.x[(N + 1) * 5:(N + 1) * 5 + 1]
        l[:5] = -x0
        u[:5] = -x0
        prob.update(l=l, u=u)
    return (time.perf_counter() - t0) / steps * 1e3


def measure_lat(loop, a, N):
    """lat's own passes: the full window, the data path alone, the solve kernel's events."""
    import torch
    fresh = loop["build"](a, N)
    ctl = _warmed(fresh, a.warmup)
    wall, dev_ms, it = window(torch, a.steps, ctl.step)
    solved, failed = _frac(ctl.status == 1), _frac(ctl.failed)
    _, data_ms, _ = window(torch, a.steps, _lat_data_path_only(ctl))
    ctl = _warmed(fresh, a.warmup)                      # the same steps again, with the solver's events on
    ctl.solver.timing(True, setup=False)
    window(torch, a.steps, ctl.step)
    t = ctl.solver.timing_read()
    ctl.solver.timing(False)
    split = {"data_path": data_ms / a.steps, "solver": (dev_ms - data_ms) / a.steps,
             "solve_kernel": t["solve_ms"] / a.steps}
    line = _line(loop, a, N, ctl, wall, dev_ms, split,
                 {"n": ctl.asm.n, "m": ctl.asm.m, "steps": a.steps, "warmup": a.warmup, "step0_max": a.step0_max,
                  **_iters(loop, it), "solved_frac_last": solved, "failed_frac_end": failed})
    if a.shim_steps:
        line["shim_ms_per_step_one_vehicle"] = _lat_shim_ms_per_step(a.shim_steps, N)
    return line


# ----------------------------------------------------------------------- the loops --
# build(a, N) -> a callable making a fresh controller; N / steps / warmup: the defaults; options:
# the loop's own command-line options; flags: those of them that go into "config" under their name;
# end: ("config" key, controller tensor whose mean it is); lds: report iters_max and lds_bytes_solve
# (the three newer loops) rather than iters_max_per_step_mean.
LOOPS = {
    "dyn": dict(build=_dyn, initial_states=dyn_states, measure=measure, N=[30], steps=20, warmup=3, lds=False,
                metric="dynamic closed-loop step (DynamicMPC.step, mpc_dynamics.main)",
                options={"--warm-start": dict(action="store_true")}, flags=("warm_start",),
                end=("status_mean_end", "status")),
    "kin": dict(build=_kin, initial_states=kin_states, measure=measure, N=[40], steps=50, warmup=5, lds=False,
                metric="kinematic closed-loop step (KinematicMPC.step, mpc_incre_kine_func.simulate)",
                options={"--warm-start": dict(action="store_true")}, flags=("warm_start",),
                end=("done_frac_end", "done")),
    "ltv": dict(build=_ltv, initial_states=ltv_states, measure=measure, N=[40, 100], steps=20, warmup=3, lds=True,
                metric="direct-input LTV closed-loop step (KinematicLTVMPC.step, mpc_kinematics_pred_matrix.main)",
                options={"--shift-warm": dict(action="store_true")}, flags=("shift_warm",),
                end=("skipped_per_vehicle", "skipped")),
    "lat": dict(build=_lat, initial_states=lat_states, measure=measure_lat, N=[20, 100], steps=50, warmup=5, lds=False,
                metric="slack lateral closed-loop step (LateralMPC.step, vehicle_lateral_mpc_slack_increment.py)",
                options={"--step0-max": dict(type=int, default=1200), "--shim-steps": dict(type=int, default=0)}),
    "lane": dict(build=_lane, initial_states=lane_states, measure=measure, N=[40], steps=20, warmup=3, lds=True,
                 metric="lane-change closed-loop step (LaneChangeMPC.step, "
                        "mpc_increment_kinematics_pred_matrix.main)",
                 options={"--shift-warm": dict(action="store_true")}, flags=("shift_warm",),
                 end=("on_lane_1_at_end", "path_id")),
    "kinfrozen": dict(build=_kinfrozen, initial_states=kinfrozen_states, measure=measure, N=[100], steps=20, warmup=3,
                      lds=True, metric="frozen-model closed-loop step (KinematicFrozenMPC.step, mpc_kinematics.main)",
                      options={}, flags=(), end=("skipped_per_vehicle", "skipped")),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="loop", required=True)
    for name, loop in LOOPS.items():
        p = sub.add_parser(name, help=loop["metric"])
        p.add_argument("--batch", type=int, default=4096)
        p.add_argument("--N", type=int, nargs="+", default=loop["N"])
        p.add_argument("--steps", type=int, default=loop["steps"])
        p.add_argument("--warmup", type=int, default=loop["warmup"])
        for opt, kw in loop["options"].items():
            p.add_argument(opt, **kw)
        if name != "lat":
            p.add_argument("--fleet", action="store_true", help="B distinct vehicles in place of B copies of one")
        p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    loop = LOOPS[a.loop]
    if a.child:
        print(json.dumps(loop["measure"](loop, a, a.N[0])), flush=True)
        return 0
    for k, N in enumerate(a.N):  # a fresh child per horizon, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child", "--N", str(N)]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            later = "; later horizons not started" if k + 1 < len(a.N) else ""
            print(json.dumps({"error": f"{a.loop}: N = {N}, B = {a.batch} ended with status {rc}{later}"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
