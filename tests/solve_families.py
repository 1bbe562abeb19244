"""The production solve-kernel families at B = 3 and the handles the tests run them through
(test_solve_shell.py, test_handle_state.py) -- TEST INFRASTRUCTURE.

Seeds (mpc.make_batch(cfg, B=3, seed), chosen with the oracle alone; test_solve_shell.py's
docstring has the oracle's iteration counts at them)."""
import functools

import numpy as np

from osqp_amd import mpc

B = 3
SEED = {2: 337, 3: 6, 5: 75}

FAMILIES = {  # name: (config, MPCQP_VARIANT, MPCQP_ELIM, plan_info()["variant"])
    "w4": (2, None, None, 17),
    "w4_elim": (3, None, None, 17),
    "w2": (2, "10", None, 10),
    "tri256": (2, "0", None, 0),
    "sweep256": (3, "2", "0", 2),
    "big": (5, "12", None, 12),
}


def env(monkeypatch, variant, elim):
    for k, v in (("MPCQP_VARIANT", variant), ("MPCQP_ELIM", elim)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def batch(cfg):
    return mpc.make_batch(cfg, B=B, seed=SEED[cfg])


def settings(cfg, **kw):
    s = {k: v for k, v in batch(cfg)["settings"].items() if k != "verbose"}
    return {**s, "polish": False, "warm_start": False, **kw}


def handle(cfg, one_shot=False, **kw):
    """DeviceBatch over batch(cfg), its inputs on the device, and fresh outputs."""
    import torch
    from osqp_amd import DeviceBatch, _drop_common_zeros
    b = batch(cfg)
    dev = torch.device("cuda", 0)
    P, Px = _drop_common_zeros(b["P"], b["Px"])
    A, Ax = _drop_common_zeros(b["A"], b["Ax"])
    X = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (Px, Ax, b["q"], b["l"], b["u"])]
    torch.cuda.synchronize()  # (the handle's stream is not ordered with torch's)
    h = DeviceBatch(P, A, B, device=0, **settings(cfg, **kw))
    if one_shot:
        assert h.one_shot(True) == {2: 2, 3: 3}[cfg]
    return h, X


def run(h, X, fused):
    """One cold solve of the inputs X: (x, y, status, iter) as numpy arrays."""
    o = out_of(h)
    if fused:
        h.setup_solve(*X, *o)
    else:
        h.setup(*X)
        h.solve(*o)
    h.synchronize()
    return [t.cpu().numpy() for t in o]


def out_of(h):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.empty((B, h.n), dtype=torch.float64, device=dev), torch.empty((B, h.m), dtype=torch.float64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
