#!/usr/bin/env python3
"""First timing of the slack lateral closed loop on the device (osqp_amd.mpc_device.LateralMPC:
vehicle_lateral_mpc_slack_increment.py's loop, batched).  No target; numbers to compare later
work against.

B vehicles, for each horizon in --N (default 20 and 100): assemble q, l, u -> update ->
warm-started solve -> raise rule / record / plant step / schedule.  After the warm-up steps
the same `--steps` steps are timed by a host clock around the window (it ends in a device
synchronise) and by a device-event pair around it.  The split: a second window enqueues only
the data path (LateralAssembler.assemble + mpcqp_lti_step_device, on the loop's stream, over
the solutions the first window left) -> data_path; solver (update + solve) = the full window's
device time minus that.  A third window with mpcqp_timing on gives the solve kernel's own
event time (the update launch is not event-timed).

--shim-steps K also runs the script's loop through the `import osqp` drop-in on ONE vehicle
for K steps (tests/test_gpu_parity.py::_slack_script_loop's calls) -> shim_ms_per_step.

Prints one JSON line per horizon.

  python tools/lat_loop_time.py [--batch 4096] [--N 20 100] [--steps 50] [--warmup 5] [--step0-max 1200]
                                [--shim-steps 200]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-mpc_amd")]

import numpy as np  # noqa: E402


def initial_states(B, step0_max, seed=5):
    """Starts around the script's own (0, 0, 5 deg, 3, 0), entering the bound schedule at a
    step drawn from [0, step0_max): 1200 spreads them over both regimes, 1 starts everyone at
    the schedule's beginning as the script does."""
    from osqp_amd import mpc
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-.02, .02, B), rng.uniform(-.05, .05, B), rng.uniform(-6, 6, B) * mpc.DEG,
                   rng.uniform(-3, 3, B), rng.uniform(-2, 2, B) * mpc.DEG], axis=1)
    return x0, rng.integers(0, step0_max, B).astype(np.int32)


def window(torch, steps, fn):
    """(host seconds, device-event ms) of `steps` calls of fn()."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, e0.elapsed_time(e1)


def data_path_only(ctl):
    """One step's data path alone: the assembly and the step kernel, no update and no solve."""
    from osqp_amd.mpc_device import _stream

    def fn():
        st = _stream(ctl.torch, ctl.dev)
        ctl.asm.assemble(ctl.theta, ctl.regime, out=(ctl.q, ctl.l, ctl.u), stream=st)
        ctl._tail(st)
    return lambda: ctl._on_stream(fn)


def shim_ms_per_step(steps, N):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shim-steps", type=int, default=0)
    ap.add_argument("--step0-max", type=int, default=1200)
    a = ap.parse_args()
    import torch
    from osqp_amd.mpc_device import LateralMPC
    x0, step0 = initial_states(a.batch, a.step0_max)
    for N in a.N:
        def warmed():
            c = LateralMPC(x0, N=N, step0=step0)
            c.run(a.warmup)
            return c

        ctl = warmed()
        its = []
        wall, dev_ms = window(torch, a.steps, lambda: its.append(ctl.step()[1].clone()))
        it = torch.stack(its).cpu().numpy()
        solved = float((ctl.status.cpu().numpy() == 1).mean())
        failed = float(ctl.failed.cpu().numpy().mean())
        _, data_ms = window(torch, a.steps, data_path_only(ctl))
        ctl = warmed()                                  # the same steps again, with the solver's events on
        ctl.solver.timing(True, setup=False)
        window(torch, a.steps, ctl.step)
        t = ctl.solver.timing_read()
        ctl.solver.timing(False)
        info = ctl.solver.plan_info()
        line = {"metric": "slack lateral closed-loop step (LateralMPC.step, vehicle_lateral_mpc_slack_increment.py)",
                "value": a.batch * a.steps / wall, "unit": "vehicle-steps/s",
                "ms_per_step": wall / a.steps * 1e3, "device_ms_per_step": dev_ms / a.steps,
                "split_ms_per_step": {"data_path": data_ms / a.steps, "solver": (dev_ms - data_ms) / a.steps,
                                      "solve_kernel": t["solve_ms"] / a.steps},
                "config": {"vehicles": a.batch, "N": N, "n": ctl.asm.n, "m": ctl.asm.m, "steps": a.steps,
                           "warmup": a.warmup, "step0_max": a.step0_max, "iters_mean": float(it.mean()),
                           "iters_max_per_step_mean": float(it.max(axis=1).mean()), "solved_frac_last": solved,
                           "failed_frac_end": failed, "variant": info["variant"],
                           "threads_per_qp": info["threads_per_qp"], "plan_choice": info["plan_choice"]}}
        if a.shim_steps:
            line["shim_ms_per_step_one_vehicle"] = shim_ms_per_step(a.shim_steps, N)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
