#!/usr/bin/env python3
"""First timing of the lane-change closed loop on the device (osqp_amd.mpc_device.LaneChangeMPC:
mpc_increment_kinematics_pred_matrix.main, batched).  No target; a number to compare later work
against.

B vehicles step N-stage horizons: reference search on each vehicle's path -> linearisation -> QP
assembly -> setup + solve -> record / plant step / shift / path schedule.  The vehicles start
spread over the schedule (step0 in [0, 200)), so both lanes are in the batch and vehicles change
lane inside the window.  The `--steps` steps after the warm-up steps are timed as
tools/ltv_loop_time.py times them (its `window`): host clock and device events with the solver's
event timing off, then the same steps by a fresh controller with it on for the solver / data-path
split.

One JSON line for the stated --batch and --N, measured by a child process under a time limit.

  python tools/lane_loop_time.py [--N 40] [--batch 4096] [--steps 20] [--warmup 3] [--shift-warm]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

from ltv_loop_time import window  # noqa: E402

CHILD_LIMIT_S = 240


def initial_states(B, seed=5):
    """Starts around main's own (0, 0, 20, 0), up to 1 m beside the lane their step0 puts them on."""
    rng = np.random.default_rng(seed)
    step0 = rng.integers(0, 200, B).astype(np.int32)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(0, 20, B)
    x0[:, 1] = 4.0 * ((step0 > 50) & (step0 <= 150)) + rng.uniform(-1.0, 1.0, B)
    x0[:, 2] = rng.uniform(8, 20, B)
    x0[:, 3] = np.deg2rad(rng.uniform(-3, 3, B))
    return x0, np.tile([0.0, 0.01], (B, 1)), step0


def measure(a):
    import torch
    from osqp_amd.mpc_device import LaneChangeMPC
    px = np.linspace(-10, 100, 200)                     # main's path and its second lane (:317-319, :382-383)
    paths_y = np.stack([px * 0.0, px * 0.0 + 4])
    x0, u0, step0 = initial_states(a.batch)

    def warmed():
        c = LaneChangeMPC(x0, u0, px, paths_y, N=a.N, step0=step0, shift_warm=a.shift_warm)
        for _ in range(a.warmup):
            c.step()
        return c

    ctl = warmed()
    wall, dev_ms, it = window(torch, ctl, a.steps)
    lane1 = float(ctl.path_id.cpu().numpy().mean())
    ctl = warmed()                                      # the same steps again, with the solver's events on
    ctl.solver.timing(True, setup=True)
    _, dev2_ms, it2 = window(torch, ctl, a.steps)
    t = ctl.solver.timing_read()
    ctl.solver.timing(False)
    solver_ms = t["setup_ms"] + t["solve_ms"]
    info = ctl.solver.plan_info()
    line = {"metric": "lane-change closed-loop step (LaneChangeMPC.step, mpc_increment_kinematics_pred_matrix.main)",
            "value": a.batch * a.steps / wall, "unit": "vehicle-steps/s",
            "ms_per_step": wall / a.steps * 1e3, "device_ms_per_step": dev_ms / a.steps,
            "split_ms_per_step": {"solver_setup": t["setup_ms"] / a.steps, "solver_solve": t["solve_ms"] / a.steps,
                                  "data_path": (dev2_ms - solver_ms) / a.steps, "window": dev2_ms / a.steps,
                                  "launches": [t["n_setup"], t["n_solve"]]},
            "config": {"vehicles": a.batch, "N": a.N, "n": ctl.layout.n, "m": ctl.layout.m,
                       "shift_warm": a.shift_warm, "steps": a.steps, "warmup": a.warmup,
                       "iters_mean": float(it.mean()), "iters_max": int(it.max()),
                       "iters_mean_split_window": float(it2.mean()),
                       "solved_frac_last": float((ctl.status.cpu().numpy() == 1).mean()),
                       "on_lane_1_at_end": lane1,
                       "variant": info["variant"], "threads_per_qp": info["threads_per_qp"],
                       "lds_bytes_solve": info["lds_bytes_solve"], "plan_choice": info["plan_choice"]}}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift-warm", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    try:  # a fresh child under its own limit
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:],
                            timeout=CHILD_LIMIT_S).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        print(json.dumps({"error": f"N = {a.N}, B = {a.batch} ended with status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
