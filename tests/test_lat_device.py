"""The slack lateral MPC closed loop on the device (csrc/mpc_device.hip: k_lti_step /
mpcqp_lti_step_device; osqp_amd.mpc.lti_step, slack_regime; osqp_amd.mpc_device.LateralMPC):
vehicle_lateral_mpc_slack_increment.py's loop (:123-269) -- one setup, then per step
update(q=, l=, u=) and a warm-started solve -- for B vehicles.

  * mpc.lti_step, the host restatement of the kernel, against a scalar loop and against
    At @ x + Bt @ du (CPU);
  * the kernel against mpc.lti_step on random inputs, bit for bit;
  * LateralMPC against a HOST-DRIVEN loop on a second DeviceBatch of the same shape (q, l, u
    built by mpc.slack_qp on the host, the tail by mpc.lti_step), bit for bit after every step;
  * LateralMPC against one free-running oracle loop per vehicle making the script's calls;
  * the failure rule (the script's raise) with max_iter = 25.

S is the script's own x0 = (0, 0, 5 deg, 3, 0) (:27).
"""
import ctypes as C

import numpy as np
import pytest

from loop_checks import EINVAL, EUNSUPPORTED
from osqp_amd import canonical_data, mpc

DEG = mpc.DEG
S = (0.0, 0.0, 5 * DEG, 3.0, 0.0)
AT, BT = mpc.augment(mpc.LATERAL_AD, mpc.LATERAL_BD)
U_TOL = 1e-4  # the project's bar on the first control (tests/test_gpu_parity.py)


def _script_regime(i):
    """:158-172, as written."""
    if i <= 400:
        return 0
    elif i <= 900:
        return 1
    else:
        return 0


def _offsets(N, nxa=5, nu=1):
    """(n, du_off, slack_off) of the slack layout (x~_0..x~_N, du_0..du_{N-1}, s_0..s_N): du_0
    (:256) and the slack of e_y in s_0 (:259)."""
    du_off = (N + 1) * nxa
    return du_off + N * nu + (N + 1) * nxa, du_off, du_off + N * nu + 3


# ------------------------------------------------------------------------------ T0 --
def _scalar_plant(At, Bt, x, du):
    """The kernel's stated order with Python floats: every product and sum rounded on its own."""
    nxa, nu = Bt.shape
    out = []
    for i in range(nxa):
        acc = float(At[i, 0]) * float(x[0])
        for j in range(1, nxa):
            acc = acc + float(At[i, j]) * float(x[j])
        bu = float(Bt[i, 0]) * float(du[0])
        for j in range(1, nu):
            bu = bu + float(Bt[i, j]) * float(du[j])
        out.append(acc + bu)
    return np.array(out)


def _random_call(rng, B, At, Bt, n, du_off, traj_cap):
    """Inputs of one lti_step call: statuses 1 / 2 / -2, some vehicles already failed, step
    counters around both switches, some records already full."""
    nxa, nu = Bt.shape
    return dict(
        sol=rng.normal(size=(B, n)), status=rng.choice([1, 1, 1, 2, -2], B).astype(np.int32),
        xt=rng.normal(size=(B, nxa)) * 3, step=rng.choice([399, 400, 401, 899, 900, 901], B).astype(np.int32),
        regime=rng.integers(0, 2, B).astype(np.int32), failed=(rng.uniform(size=B) < 0.2).astype(np.int32),
        fail_step=rng.integers(0, 50, B).astype(np.int32),
        traj=rng.normal(size=(B, traj_cap, nxa + nu + 1)), traj_len=rng.integers(0, traj_cap + 1, B).astype(np.int32))


def test_lti_step_host_restatement():
    """mpc.lti_step's plant row equals the scalar loop bit for bit, and At @ x + Bt @ du to
    rtol 1e-15 (states of one sign, as the script's own, so that the sum is well conditioned:
    the two differ only in summation order, a few ulp of sum |terms|); slack_regime equals the
    script's if / elif; a failed or non-solved vehicle is returned unchanged."""
    rng = np.random.default_rng(11)
    B, N = 64, 3
    n, du_off, slack_off = _offsets(N)
    c = _random_call(rng, B, AT, BT, n, du_off, 2)
    c["xt"] = np.concatenate([[S], rng.uniform(0.5, 1.5, (B - 1, 5))])
    c["sol"][:, du_off] = rng.uniform(0.001, 0.01, B)
    out = mpc.lti_step(AT, BT, c["sol"], c["status"], c["xt"], c["step"], c["regime"], c["failed"], c["fail_step"],
                       du_off, slack_off, traj=c["traj"], traj_len=c["traj_len"])
    xt, step, regime, failed, fail_step, traj, traj_len = out
    go = (c["failed"] == 0) & (c["status"] == 1)
    bad = (c["failed"] == 0) & (c["status"] != 1)
    assert go.sum() > 10 and bad.sum() > 3 and (c["failed"] != 0).sum() > 3
    for b in np.flatnonzero(go):
        du = c["sol"][b, du_off:du_off + 1]
        assert np.array_equal(xt[b], _scalar_plant(AT, BT, c["xt"][b], du))
        np.testing.assert_allclose(xt[b], AT @ c["xt"][b] + BT @ du, rtol=1e-15, atol=0)
        assert step[b] == c["step"][b] + 1 and regime[b] == _script_regime(step[b])
        if c["traj_len"][b] < 2:
            row = np.concatenate([c["xt"][b, :4], xt[b, 4:], du, [c["sol"][b, slack_off]]])
            assert np.array_equal(traj[b, c["traj_len"][b]], row) and traj_len[b] == c["traj_len"][b] + 1
        else:
            assert np.array_equal(traj[b], c["traj"][b]) and traj_len[b] == 2
    assert np.array_equal(failed[bad], np.ones(bad.sum(), np.int32)) and np.array_equal(fail_step[bad], c["step"][bad])
    for k, v in (("xt", xt), ("step", step), ("regime", regime), ("traj", traj), ("traj_len", traj_len)):
        assert np.array_equal(v[~go], c[k][~go]), k   # the raise, or failed before: nothing else changes
    was = c["failed"] != 0
    assert np.array_equal(failed[was], c["failed"][was]) and np.array_equal(fail_step[was], c["fail_step"][was])
    # a general model (nxa 8, nu 2): the scalar loop again
    At8, Bt8 = rng.normal(size=(8, 8)), rng.normal(size=(8, 2))
    c8 = _random_call(rng, 16, At8, Bt8, 30, 20, 2)
    c8["status"][:] = 1; c8["failed"][:] = 0
    x8 = mpc.lti_step(At8, Bt8, c8["sol"], c8["status"], c8["xt"], c8["step"], c8["regime"], c8["failed"],
                      c8["fail_step"], 20)[0]
    for b in range(16):
        assert np.array_equal(x8[b], _scalar_plant(At8, Bt8, c8["xt"][b], c8["sol"][b, 20:22]))
    for k in (0, 400, 401, 900, 901):
        assert mpc.slack_regime(k) == _script_regime(k), k
    ks = np.arange(0, 1500)
    assert np.array_equal(mpc.slack_regime(ks), [_script_regime(k) for k in ks])


def _call_kernel(L, At, Bt, n, du_off, slack_off, ptrs, B, xt_stride, sw, reg, traj_cap, device=0, stream=None):
    At, Bt = np.ascontiguousarray(At, np.float64), np.ascontiguousarray(Bt, np.float64)
    sw, reg = np.ascontiguousarray(sw, np.int32), np.ascontiguousarray(reg, np.int32)
    nxa, nu = Bt.shape
    return L.mpcqp_lti_step_device(B, nxa, nu, At.ctypes.data, Bt.ctypes.data, n, du_off, slack_off, ptrs["sol"],
                                   ptrs["status"], ptrs["xt"], xt_stride, len(sw), sw.ctypes.data, reg.ctypes.data,
                                   ptrs["step"], ptrs["regime"], ptrs["failed"], ptrs["fail_step"], ptrs["traj"],
                                   traj_cap, ptrs["traj_len"], device, stream)


def test_lti_step_rejects_other_models():
    """nxa > 8, nu > 2 and more than 8 switches are MPCQP_EUNSUPPORTED, bad offsets MPCQP_EINVAL
    -- decided on the host, before anything is launched."""
    from osqp_amd.mpc_device import _bind
    L = _bind()
    buf = np.zeros(64)
    p = {k: buf.ctypes.data for k in ("sol", "status", "xt", "step", "regime", "failed", "fail_step", "traj",
                                      "traj_len")}
    sw, reg = mpc.SLACK_SWITCH_STEPS, mpc.SLACK_REGIMES
    assert _call_kernel(L, np.eye(9), np.ones((9, 1)), 43, 20, 26, p, 1, 9, sw, reg, 0) == EUNSUPPORTED
    assert _call_kernel(L, np.eye(5), np.ones((5, 3)), 43, 20, 26, p, 1, 5, sw, reg, 0) == EUNSUPPORTED
    assert _call_kernel(L, AT, BT, 43, 20, 26, p, 1, 5, np.arange(9), np.zeros(10), 0) == EUNSUPPORTED
    assert _call_kernel(L, AT, BT, 43, 43, 26, p, 1, 5, sw, reg, 0) == EINVAL     # du_0 past the solution
    assert _call_kernel(L, AT, BT, 43, 20, 43, p, 1, 5, sw, reg, 0) == EINVAL     # so is the slack
    assert _call_kernel(L, AT, BT, 43, 20, 26, p, 1, 4, sw, reg, 0) == EINVAL     # xt rows overlap
    assert _call_kernel(L, AT, BT, 43, 20, 26, p, 0, 5, sw, reg, 0) == 0          # B = 0: nothing to do


# ------------------------------------------------------------------------------ T1 --
@pytest.mark.gpu
@pytest.mark.parametrize("model", ["script", "nxa8_nu2"])
def test_lti_step_kernel_equals_host(model):
    """One kernel call on random inputs, B = 37: statuses 1 / 2 / -2, some vehicles already
    failed, step counters 399..401 and 899..901, traj_cap = 2 with some records already full.
    Every output equals mpc.lti_step.  `script`: the slack script's model and layout offsets,
    x~ at stride 9 inside theta; `nxa8_nu2`: a random 8-state, 2-input model without a slack."""
    import torch
    from osqp_amd.mpc_device import _bind
    L = _bind()
    rng = np.random.default_rng(37)
    B, cap = 37, 2
    if model == "script":
        At, Bt, stride = AT, BT, 9
        n, du_off, slack_off = _offsets(3)
    else:
        At, Bt, stride = rng.normal(size=(8, 8)), rng.normal(size=(8, 2)), 8
        n, du_off, slack_off = 30, 20, -1
    nxa = At.shape[0]
    c = _random_call(rng, B, At, Bt, n, du_off, cap)
    assert {1, 2, -2} <= set(c["status"]) and (c["failed"] != 0).any() and (c["traj_len"] == cap).any()
    assert set(c["step"]) == {399, 400, 401, 899, 900, 901}
    exp = mpc.lti_step(At, Bt, c["sol"], c["status"], c["xt"], c["step"], c["regime"], c["failed"], c["fail_step"],
                       du_off, slack_off, traj=c["traj"], traj_len=c["traj_len"])
    dev = torch.device("cuda", 0)
    theta = rng.normal(size=(B, stride))
    theta[:, :nxa] = c["xt"]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    d["xt"] = torch.from_numpy(theta).to(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    code = _call_kernel(L, At, Bt, n, du_off, slack_off, {k: v.data_ptr() for k, v in d.items()}, B, stride,
                        mpc.SLACK_SWITCH_STEPS, mpc.SLACK_REGIMES, cap, stream=stream.cuda_stream)
    assert code == 0, L.mpcqp_last_error()
    torch.cuda.synchronize()
    got_theta = d["xt"].cpu().numpy()
    assert np.array_equal(got_theta[:, nxa:], theta[:, nxa:])    # the rest of a theta row is not touched
    got = (got_theta[:, :nxa],) + tuple(d[k].cpu().numpy() for k in ("step", "regime", "failed", "fail_step", "traj",
                                                                   "traj_len"))
    for name, g, e in zip(("xt", "step", "regime", "failed", "fail_step", "traj", "traj_len"), got, exp):
        assert g.dtype == e.dtype and np.array_equal(g, e), name


# ------------------------------------------------------------------------- T2, T3 --
def _against_host_driven_loop(N, x0, xr, step0, steps, **settings):
    """LateralMPC against a host-driven loop on a second DeviceBatch of the same shape: q, l, u
    built per step from mpc.slack_qp (once per (vehicle, regime), rows 0..4 set to -x~0), the
    tail by mpc.lti_step.  After EVERY step xt, sol, status, iters, steps, regime are bit-identical,
    at the end traj and traj_len too."""
    import torch
    from osqp_amd import DeviceBatch
    from osqp_amd.mpc_device import LateralMPC
    x0, xr, step0 = np.array(x0, float), np.array(xr, float), np.array(step0, np.int32)
    B = len(x0)
    n, du_off, slack_off = _offsets(N)
    dev = torch.device("cuda", 0)
    ctl = LateralMPC(x0, xr=xr, N=N, step0=step0, traj_cap=steps, **settings)
    assert (ctl.du_off, ctl.slack_off, ctl.asm.n) == (du_off, slack_off, n)

    cache = {}

    def qp_vectors(xt, regime):
        out = []
        for b in range(B):
            key = (b, int(regime[b]))
            if key not in cache:
                cache[key] = mpc.slack_qp(N, np.zeros(5), xr=xr[b], regime=key[1])
            _, q, _, l, u = cache[key]
            l, u = l.copy(), u.copy()
            l[:5] = u[:5] = -xt[b]
            out.append((q, l, u))
        return [torch.from_numpy(np.stack(v)).to(dev) for v in zip(*out)]

    P, A = canonical_data(*mpc.slack_qp(N, np.zeros(5))[0:3:2])
    Px, Ax = torch.from_numpy(P.data.copy()).to(dev), torch.from_numpy(A.data.copy()).to(dev)
    h = DeviceBatch(P, A, B, device=0, **{"warm_start": True, **settings})
    m = A.shape[0]
    kw = dict(dtype=torch.float64, device=dev)
    sol, y = torch.empty((B, n), **kw), torch.empty((B, m), **kw)
    status, iters = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    xt, step, regime = x0.copy(), step0.copy(), mpc.slack_regime(step0)
    failed, fail_step = np.zeros(B, np.int32), np.zeros(B, np.int32)
    traj, traj_len = np.zeros((B, steps, 7)), np.zeros(B, np.int32)
    q, l, u = qp_vectors(xt, np.zeros(B, int))       # the set-up before the loop (:87-121): regime 0
    torch.cuda.synchronize()
    h.setup(Px, Ax, q, l, u)
    h.synchronize()
    regimes_seen = set()
    for k in range(steps):
        regimes_seen |= set(regime.tolist())
        q, l, u = qp_vectors(xt, regime)
        torch.cuda.synchronize()
        h.update(q, l, u)
        h.solve(sol, y, status, iters)
        h.synchronize()
        hsol, hstatus, hiters = sol.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()
        xt, step, regime, failed, fail_step, traj, traj_len = mpc.lti_step(
            AT, BT, hsol, hstatus, xt, step, regime, failed, fail_step, du_off, slack_off, traj=traj,
            traj_len=traj_len)
        ctl.step()
        torch.cuda.synchronize()
        for name, g, e in (("xt", ctl.xt, xt), ("sol", ctl.sol, hsol), ("status", ctl.status, hstatus),
                           ("iters", ctl.iters, hiters), ("steps", ctl.steps, step), ("regime", ctl.regime, regime)):
            assert np.array_equal(g.cpu().numpy(), e), (name, k)
    assert (hstatus == 1).all() and not failed.any() and not ctl.failed.any().item()
    dtraj, dlen = ctl.trajectories()
    assert np.array_equal(dlen, traj_len) and np.array_equal(dtraj, traj) and (dlen == steps).all()
    return regimes_seen, step


@pytest.mark.gpu
def test_loop_equals_host_driven_loop():
    """B = 6, 300 steps: vehicles in both bound regimes and across both switches (step0 = 350 ->
    401 at step 51, step0 = 850 -> 901 at step 51), one with a nonzero reference."""
    x0 = [S, (0, 0, -4 * DEG, -2, 0), (0, 0, 8 * DEG, 6, -3 * DEG), S, (0, 0, 2 * DEG, 1, 0), (0, 0, 0, 0, 0)]
    xr = np.zeros((6, 4)); xr[4] = (0, 0, 0, 0.5)
    seen, step = _against_host_driven_loop(20, x0, xr, [0, 0, 0, 350, 850, 380], 300)
    assert seen == {0, 1} and step.tolist() == [300, 300, 300, 650, 1150, 680]


@pytest.mark.gpu
def test_loop_equals_host_driven_loop_long_horizon():
    """B = 2, N = 100 (the script's own horizon, :14), 30 steps: the long-horizon plan."""
    _against_host_driven_loop(100, [S, (0, 0, 2 * DEG, 1, 0)], np.zeros((2, 4)), [0, 395], 30)


# ------------------------------------------------------------------------------ T4 --
def _oracle_loop(N, x0, xr, step0, steps):
    """One free-running pyoracle.OSQP loop making the script's calls (setup :121, update :237,
    solve :248, raise :252-253, plant :257, update :267-269), the schedule entered at step0.
    Returns per step (du_0, iterations, slack, max |x~0| the step started from)."""
    import pyoracle
    x0 = np.array(x0, float)
    P, q, A, l, u = mpc.slack_qp(N, x0, xr=xr)
    prob = pyoracle.OSQP()
    prob.setup(P, q, A, l, u, warm_start=True)
    out = []
    built = {r: mpc.slack_qp(N, np.zeros(5), xr=xr, regime=r) for r in (0, 1)}   # :201-229 but for -x0
    for i in range(steps):
        _, q_new, _, l_new, u_new = built[_script_regime(step0 + i)]
        l_new, u_new = l_new.copy(), u_new.copy()
        l_new[:5] = u_new[:5] = -x0
        prob.update(q=q_new, l=l_new, u=u_new)
        res = prob.solve()
        if res.info.status != "solved":
            raise ValueError("OSQP did not solve the problem!")
        du = res.x[(N + 1) * 5:(N + 1) * 5 + 1]
        out.append((du[0], res.info.iter, res.x[-(N + 1) * 5:][3], np.abs(x0).max()))
        x0 = AT @ x0 + BT @ du
        l_new[:5] = -x0
        u_new[:5] = -x0
        prob.update(l=l_new, u=u_new)
    return np.array(out)


@pytest.mark.gpu
def test_loop_against_oracle():
    """B = 6, 300 steps, against one free-running oracle loop per vehicle.  Every step is solved;
    iteration counts are equal at every step; |du_0 - oracle| < 1e-4; the slack is within a tenth
    of eps_abs + eps_rel max |x~0| at that step (the bar of
    test_gpu_parity.py::test_slack_script_configs0_1500_steps).  The vehicles are ones whose
    oracle loop keeps every iteration count when du_0 is perturbed at solver-rounding level; both
    regime switches fall inside the window.  Measured on an MI355X: no iteration mismatch,
    |du_0 - oracle| at most 1.1e-7, the slack at most 1.9e-3 of its bar."""
    import torch
    from osqp_amd.mpc_device import LateralMPC
    steps = 300
    x0 = [S, (0.01, 0.02, 1 * DEG, 0.5, 2 * DEG), S, (0, 0, 2 * DEG, 1, 0), (0, 0, 0, 0, 0), (0, 0, 2 * DEG, 1, 0)]
    step0 = [0, 0, 350, 850, 380, 0]
    xr = np.zeros((6, 4)); xr[5] = (0, 0, 0, 0.5)
    ctl = LateralMPC(x0, xr=xr, step0=step0, traj_cap=steps)
    its, sts = [], []
    for _ in range(steps):
        st, it = ctl.step()
        its.append(it.clone()); sts.append(st.clone())
    torch.cuda.synchronize()
    its, sts = torch.stack(its).cpu().numpy(), torch.stack(sts).cpu().numpy()
    traj, tlen = ctl.trajectories()
    assert (sts == 1).all() and not ctl.failed.any().item() and (tlen == steps).all()
    for b in range(6):
        o = _oracle_loop(20, x0[b], xr[b], step0[b], steps)
        d_du, d_s = np.abs(traj[b, :, 5] - o[:, 0]).max(), np.abs(traj[b, :, 6] - o[:, 2])
        tol = 0.1 * (1e-3 + 1e-3 * o[:, 3])
        print(f"vehicle {b}: max |du_0 - oracle| {d_du:.3e}, max slack diff / bar {np.max(d_s / tol):.3e}, "
              f"iteration mismatches {np.count_nonzero(its[:, b] != o[:, 1])}")
        assert np.array_equal(its[:, b], o[:, 1].astype(its.dtype)), np.flatnonzero(its[:, b] != o[:, 1])[:10]
        assert d_du < U_TOL, d_du
        assert np.all(d_s <= tol), np.max(d_s / tol)


# ------------------------------------------------------------------------------ T5 --
@pytest.mark.gpu
def test_failure_rule():
    """max_iter = 25: S does not solve at step 0 (`maximum iterations reached`) and is frozen
    where the script raises; the zero-state vehicle solves in 25 iterations every step."""
    from osqp_amd.mpc_device import LateralMPC
    ctl = LateralMPC([S, (0, 0, 0, 0, 0)], traj_cap=8, max_iter=25)
    for _ in range(5):
        st, it = ctl.step()
        assert st.cpu().tolist() == [-2, 1] and it.cpu().tolist() == [25, 25]
    assert ctl.failed.cpu().tolist() == [1, 0] and ctl.fail_step.cpu().tolist() == [0, 0]
    assert np.array_equal(ctl.xt.cpu().numpy()[0], S)
    assert ctl.steps.cpu().tolist() == [0, 5] and ctl.regime.cpu().tolist() == [0, 0]
    traj, tlen = ctl.trajectories()
    assert tlen.tolist() == [0, 5] and not traj[0].any()
    with pytest.raises(ValueError, match="OSQP did not solve the problem!"):
        ctl.run(5, strict=True)
