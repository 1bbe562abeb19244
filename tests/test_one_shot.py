"""One-shot fused setup + solve (mpcqp_set_one_shot).

The reference's Control/MPC call pattern builds a fresh osqp.OSQP(), calls setup() and solve()
and drops the object (mpc_kinematics.py:194-198), so nothing reads the workspace afterwards.
The one-shot form of the fused four-wave kernel keeps the scaled problem and the G blocks on chip
and stores no warm-start iterates or certificates (solve_wave.hip, setup_r.h ONE).  These
tests hold it to the persisting kernel bit for bit -- x, y, status, iteration count -- on the
cfg-2 headline batch and a cfg-3 sample, over two calls (the second one runs in the LPT dispatch
order the first call's iteration counts set), and check that the calls which read the workspace
refuse to run after a one-shot call until a setup.
"""
import numpy as np
import pytest

from one_shot_cut import _inputs, out, same_bits


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,B", [(2, 1024), (3, 4096)])
def test_one_shot_is_bit_identical(cfg, B):
    import torch
    from osqp_amd import DeviceBatch
    dev = torch.device("cuda", 0)
    P, A, s, (Px, Ax, q), bounds, b = _inputs(cfg, B, 31, dev)
    torch.cuda.synchronize()  # (the handles' streams are not ordered with torch's)
    keep, one = DeviceBatch(P, A, B, device=0, **s), DeviceBatch(P, A, B, device=0, **s)
    # cfg 2: the G blocks in an LDS region of their own; cfg 3 (two workgroups per CU leave no
    # room for one): straight into the solve's copy (factorize_w4_gl)
    assert one.one_shot(True) == {2: 2, 3: 3}[cfg]
    for call, (l, u) in enumerate(bounds):
        o1, o2 = out(B, b["n"], b["m"], dev), out(B, b["n"], b["m"], dev)
        keep.setup_solve(Px, Ax, q, l, u, *o1)
        one.setup_solve(Px, Ax, q, l, u, *o2)
        torch.cuda.synchronize()
        st = o1[2].cpu().numpy()
        for a, c in zip(o1, o2):
            assert same_bits(a, c), np.unique(st, return_counts=True)
        if call == 0:  # (the moved bounds of the second call leave some instances infeasible)
            assert (o1[2] == 1).float().mean().item() > 0.99
    # the workspace is gone: the calls that read it refuse, until a setup
    o = out(B, b["n"], b["m"], dev)
    with pytest.raises(ValueError, match="one-shot"):
        one.solve(*o)
    with pytest.raises(ValueError, match="one-shot"):
        one.update(q=q)
    with pytest.raises(ValueError, match="one-shot"):
        one.warm_start(x=o[0])
    one.setup(Px, Ax, q, *bounds[1])
    one.solve(*o)
    keep.setup(Px, Ax, q, *bounds[1])
    o1 = out(B, b["n"], b["m"], dev)
    keep.solve(*o1)
    torch.cuda.synchronize()
    for a, c in zip(o1, o):
        assert same_bits(a, c)


@pytest.mark.gpu
def test_one_shot_elsewhere_runs_as_usual():
    """cfg 5 (the long-horizon kernel): the one-shot switch does not apply; setup_solve runs the
    persisting path and the workspace stays usable (a warm start + solve after it)."""
    import torch
    from osqp_amd import DeviceBatch
    dev = torch.device("cuda", 0)
    B = 256
    P, A, s, (Px, Ax, q), bounds, b = _inputs(5, B, 7, dev)
    torch.cuda.synchronize()
    h = DeviceBatch(P, A, B, device=0, **s)
    assert h.one_shot(True) == 0
    o = out(B, b["n"], b["m"], dev)
    h.setup_solve(Px, Ax, q, *bounds[0], *o)
    h.warm_start(o[0], o[1])
    o2 = out(B, b["n"], b["m"], dev)
    h.solve(*o2)
    torch.cuda.synchronize()
    assert (o2[2] == 1).all()
