#!/usr/bin/env python3
"""First timing of the direct-input LTV closed loop on the device
(osqp_amd.mpc_device.KinematicLTVMPC: mpc_kinematics_pred_matrix.main, batched).  No target;
a number to compare later work against.

B vehicles step N-stage horizons: reference search -> linearisation -> QP assembly ->
setup + solve -> skip rule / record / plant step / shift.  The same `--steps` steps after
the warm-up steps are timed twice, each time by a fresh controller from the same starts:

  1. event timing off: host clock around the window (ends in a device synchronise) and a
     device-event pair around it -> ms_per_step, vehicle-steps/s;
  2. mpcqp_timing on: the solver's own event pairs give its setup and solve kernel time;
     the window's device-event total minus that is the data path (the four kernels above
     plus launch gaps), so solver + data_path = the second pass's device time ("window").

Without --N, one JSON line each for N = 40 and N = 100 (main's own horizon), every horizon
measured by a fresh child process under its own time limit; the second is not started when
the first fails.  With --N, that horizon in this process.

  python tools/ltv_loop_time.py [--N 40] [--batch 4096] [--steps 20] [--warmup 3] [--shift-warm]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd")]

import numpy as np  # noqa: E402

HORIZONS = (40, 100)
CHILD_LIMIT_S = 240


def initial_states(B, seed=5):
    """Starts around main's own (0, 0, 20, 0): 1 to 5 m beside its path (y = -5)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(0, 20, B)
    x0[:, 1] = -5.0 + rng.uniform(1.0, 5.0, B) * rng.choice([-1.0, 1.0], B)
    x0[:, 2] = rng.uniform(8, 20, B)
    x0[:, 3] = np.deg2rad(rng.uniform(-3, 3, B))
    return x0, np.tile([0.0, 0.01], (B, 1))


def window(torch, ctl, steps):
    """(host seconds, device-event ms, iteration counts (steps, B)) of `steps` steps."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        _, it = ctl.step()
        iters.append(it.clone())
    e1.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, e0.elapsed_time(e1), torch.stack(iters).cpu().numpy()


def measure(a):
    import torch
    from osqp_amd.mpc_device import KinematicLTVMPC
    px = np.linspace(-10, 100, 200)                     # mpc_kinematics_pred_matrix.main's path (:377-379)
    x0, u0 = initial_states(a.batch)

    def warmed():
        c = KinematicLTVMPC(x0, u0, px, px * 0.0 - 5.0, N=a.N, shift_warm=a.shift_warm)
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
    line = {"metric": "direct-input LTV closed-loop step (KinematicLTVMPC.step, mpc_kinematics_pred_matrix.main)",
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
                       "skipped_per_vehicle": skipped,
                       "variant": info["variant"], "threads_per_qp": info["threads_per_qp"],
                       "lds_bytes_solve": info["lds_bytes_solve"], "plan_choice": info["plan_choice"]}}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift-warm", action="store_true")
    a = ap.parse_args()
    if a.N is not None:
        return measure(a)
    for N in HORIZONS:  # a fresh child per horizon, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--N", str(N), "--batch", str(a.batch), "--steps",
               str(a.steps), "--warmup", str(a.warmup)] + (["--shift-warm"] if a.shift_warm else [])
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"error": f"N = {N} ended with status {rc}; later horizons not started"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
