#!/usr/bin/env python3
"""First timing of the frozen-model closed loop on the device
(osqp_amd.mpc_device.KinematicFrozenMPC: mpc_kinematics.main, batched).  No target; a number to
compare later work against.

B vehicles step N-stage horizons: reference search -> ONE linearisation per vehicle (expanded over
the stages) -> QP assembly -> setup + solve -> skip rule / unpack / record / plant step.  The
`--steps` steps after the warm-up steps are timed as tools/ltv_loop_time.py times them (its
`window`): host clock and device events with the solver's event timing off, then the same steps by
a fresh controller with it on for the solver / data-path split.

One JSON line for the stated --batch and --N, measured by a child process under a time limit.

  python tools/kinfrozen_loop_time.py [--N 100] [--batch 4096] [--steps 20] [--warmup 3]
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


def initial_states(B, N, seed=5):
    """Starts around main's own (0, 0, 5, 30 deg), 1 to 5 m beside its path (y = -5), and the
    script's noise on the initial pred_u (:313-323: sigma 1 deg steer, 0.1 accel)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(0, 20, B)
    x0[:, 1] = -5.0 + rng.uniform(1.0, 5.0, B) * rng.choice([-1.0, 1.0], B)
    x0[:, 2] = rng.uniform(5, 20, B)
    x0[:, 3] = np.deg2rad(rng.uniform(-30, 30, B))
    u0 = np.tile([0.0, 0.01], (B, 1))
    pred_u0 = u0[:, None] + rng.normal(0.0, [np.deg2rad(1), 0.1], (B, N + 1, 2))
    pred_u0[:, N] = pred_u0[:, N - 1]
    return x0, u0, pred_u0


def measure(a):
    import torch
    from osqp_amd.mpc_device import KinematicFrozenMPC
    px = np.linspace(-10, 100, 200)                     # mpc_kinematics.main's path (:290-292)
    x0, u0, pred_u0 = initial_states(a.batch, a.N)

    def warmed():
        c = KinematicFrozenMPC(x0, u0, px, px * 0.0 - 5.0, N=a.N, pred_u0=pred_u0)
        for _ in range(a.warmup):
            c.step()
        return c

    ctl = warmed()
    wall, dev_ms, it = window(torch, ctl, a.steps)
    skipped = float(ctl.skipped.cpu().numpy().mean())
    ctl = warmed()                                      # the same steps again, with the solver's events on
    ctl.solver.timing(True, setup=True)
    _, dev2_ms, it2 = window(torch, ctl, a.steps)
    t = ctl.solver.timing_read()
    ctl.solver.timing(False)
    solver_ms = t["setup_ms"] + t["solve_ms"]
    info = ctl.solver.plan_info()
    line = {"metric": "frozen-model closed-loop step (KinematicFrozenMPC.step, mpc_kinematics.main)",
            "value": a.batch * a.steps / wall, "unit": "vehicle-steps/s",
            "ms_per_step": wall / a.steps * 1e3, "device_ms_per_step": dev_ms / a.steps,
            "split_ms_per_step": {"solver_setup": t["setup_ms"] / a.steps, "solver_solve": t["solve_ms"] / a.steps,
                                  "data_path": (dev2_ms - solver_ms) / a.steps, "window": dev2_ms / a.steps,
                                  "launches": [t["n_setup"], t["n_solve"]]},
            "config": {"vehicles": a.batch, "N": a.N, "n": ctl.layout.n, "m": ctl.layout.m,
                       "steps": a.steps, "warmup": a.warmup,
                       "iters_mean": float(it.mean()), "iters_max": int(it.max()),
                       "iters_mean_split_window": float(it2.mean()),
                       "solved_frac_last": float((ctl.status.cpu().numpy() == 1).mean()),
                       "skipped_per_vehicle": skipped,
                       "variant": info["variant"], "threads_per_qp": info["threads_per_qp"],
                       "lds_bytes_solve": info["lds_bytes_solve"], "plan_choice": info["plan_choice"]}}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
