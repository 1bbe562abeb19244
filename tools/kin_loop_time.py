#!/usr/bin/env python3
"""First timing of the kinematic closed loop on the device (osqp_amd.mpc_device.KinematicMPC:
mpc_incre_kine_func.simulate, batched).  No target; a number to compare later work against.

B vehicles step N = 40 horizons: reference search -> linearisation -> QP assembly ->
setup + solve -> record / stop rule / plant step / shift.  The same `--steps` steps after
the warm-up steps are timed twice, each time by a fresh controller from the same starts:

  1. event timing off: host clock around the window (ends in a device synchronise) and a
     device-event pair around it -> ms_per_step, vehicle-steps/s;
  2. mpcqp_timing on: the solver's own event pairs give its setup and solve kernel time;
     the window's device-event total minus that is the data path (the four kernels above
     plus launch gaps), so solver + data_path = the second pass's device time ("window").

Prints one JSON line.

  python tools/kin_loop_time.py [--batch 4096] [--steps 50] [--warmup 5] [--warm-start]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd")]

import numpy as np  # noqa: E402


def initial_states(B, seed=5):
    """Lane-change starts around simulate's own: 1 to 4 m beside main()'s path (y = -4)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(0, 20, B)
    x0[:, 1] = -4.0 + rng.uniform(1.0, 4.0, B) * rng.choice([-1.0, 1.0], B)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=40)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--warm-start", action="store_true")
    a = ap.parse_args()
    import torch
    from osqp_amd.mpc_device import KinematicMPC
    px = np.linspace(-10, 100, 200)                     # mpc_incre_kine_func.main's path (:440-442)
    x0, u0 = initial_states(a.batch)

    def warmed():
        c = KinematicMPC(x0, u0, px, px * 0.0 - 4.0, px * 0.0, N=a.N, warm_start=a.warm_start)
        for _ in range(a.warmup):
            c.step()
        return c

    ctl = warmed()
    wall, dev_ms, it = window(torch, ctl, a.steps)
    done_frac = float(ctl.done.cpu().numpy().mean())
    ctl = warmed()                                      # the same steps again, with the solver's events on
    ctl.solver.timing(True, setup=True)
    _, dev2_ms, it2 = window(torch, ctl, a.steps)
    t = ctl.solver.timing_read()
    ctl.solver.timing(False)
    solver_ms = t["setup_ms"] + t["solve_ms"]
    info = ctl.solver.plan_info()
    line = {"metric": "kinematic closed-loop step (KinematicMPC.step, mpc_incre_kine_func.simulate)",
            "value": a.batch * a.steps / wall, "unit": "vehicle-steps/s",
            "ms_per_step": wall / a.steps * 1e3, "device_ms_per_step": dev_ms / a.steps,
            "split_ms_per_step": {"solver_setup": t["setup_ms"] / a.steps, "solver_solve": t["solve_ms"] / a.steps,
                                  "data_path": (dev2_ms - solver_ms) / a.steps, "window": dev2_ms / a.steps,
                                  "launches": [t["n_setup"], t["n_solve"]]},
            "config": {"vehicles": a.batch, "N": a.N, "n": ctl.layout.n, "m": ctl.layout.m,
                       "warm_start": a.warm_start, "steps": a.steps, "warmup": a.warmup,
                       "iters_mean": float(it.mean()), "iters_max_per_step_mean": float(it.max(axis=1).mean()),
                       "iters_mean_split_window": float(it2.mean()),
                       "solved_frac_last": float((ctl.status.cpu().numpy() == 1).mean()),
                       "done_frac_end": done_frac,
                       "variant": info["variant"], "threads_per_qp": info["threads_per_qp"],
                       "plan_choice": info["plan_choice"]}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
