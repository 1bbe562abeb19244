#!/usr/bin/env python3
"""Event-timed cost of the parameter-gradient linearisation, beside the VJP in
the point it is modelled on.

    python tools/pvjp_time.py [--batch 8192] [--stages 50] [--reps 50]

mpc_device.linearise_pvjp (two launches: the groups of 7 and 6 constants) and
mpc_device.linearise_vjp on the same fleet, points and cotangents; HIP events around `reps`
back-to-back calls after a warm-up, the mean per call in microseconds, three rounds.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-mpc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--stages", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import numpy as np
    import torch
    from osqp_amd import mpc_device as md
    B, N = a.batch, a.stages
    rng = np.random.default_rng(0)
    dev = lambda v: torch.as_tensor(v, dtype=torch.float64).to("cuda:0").contiguous()
    x = rng.standard_normal((B, N, 6)) * [3.0, 3.0, 0.3, 1.0, 0.3, 0.1] + [0.0, 0.0, 0.0, 12.0, 0.0, 0.0]
    u = rng.standard_normal((B, N, 2)) * [0.05, 0.5]
    tx, tu = dev(x), dev(u)
    cots = [dev(rng.standard_normal(s)) for s in ((B, N, 6, 6), (B, N, 6, 2), (B, N, 6))]
    b = np.arange(B)
    fleet = md.Fleet.from_arrays(m=1000.0 + 0.1 * b, l_f=1.0 + 0.00004 * b, dt=0.05)
    gK = torch.empty((B, 13), dtype=torch.float64, device="cuda:0")
    gx, gu = torch.empty((B, N, 6), dtype=torch.float64, device="cuda:0"), torch.empty((B, N, 2), dtype=torch.float64,
                                                                                        device="cuda:0")
    calls = dict(linearise_pvjp=lambda: md.linearise_pvjp(fleet, tx, tu, *cots, out=gK),
                 linearise_vjp=lambda: md.linearise_vjp(fleet, tx, tu, *cots, out=(gx, gu)))
    for name, call in calls.items():
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        print(f"{name} B={B} N={N}: {min(us):.1f} - {max(us):.1f} us per call (mean of {a.reps}, three rounds)")


if __name__ == "__main__":
    main()
