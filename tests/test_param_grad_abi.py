"""Host-side checks of the parameter-gradient ABI of DESIGN.md §25 (no GPU needed; nothing here
reaches the device): the header declares and the library exports the five symbols; the four device
entry points refuse bad arguments, a NULL fleet, a batch that is not the fleet's size and another
device with the messages mpcqp.h states, B = 0 is a no-op, and N > 256 is MPCQP_EUNSUPPORTED -- the
decision mpcqp.h documents for the stage sum; mpcqp_vehicle_constants_vjp against
mpc.vehicle_constants_vjp and against differences of mpcqp_fleet_constants; the Python wrappers'
refusals.  What needs a device is in tests/test_param_grad_device.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fleet_cases as fc
import osqp_amd
from osqp_amd import mpc, mpc_device as md

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcqp.h")
LINEARISE = ("linearise_pvjp", "kin_linearise_pvjp")
STEP = ("euler_step_pvjp", "kin_update_pvjp")
SYMBOLS = [f"mpcqp_{n}_fleet_device" for n in LINEARISE + STEP] + ["mpcqp_vehicle_constants_vjp"]
FIELDS = ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")


def _code(name):
    return int(re.search(rf"#define\s+{name}\s+(-?\d+)", open(HEADER).read()).group(1))


EINVAL, EUNSUPPORTED = _code("MPCQP_EINVAL"), _code("MPCQP_EUNSUPPORTED")


@pytest.mark.parametrize("name", SYMBOLS)
def test_header_declares_and_library_exports(name):
    assert f"int {name}(" in open(HEADER).read()
    assert hasattr(C.CDLL(osqp_amd.LIB_PATH), name)


def _fleet(name):
    return md.Fleet(fc.vehicles(md, "cars")) if not name.startswith("kin") else md.KinFleet(fc.kin_vehicles(md, "cars"))


def _args(name, fleet, B, buf, N=2, device=0, null=()):
    """Arguments that pass the entry point's own checks, every pointer on one scratch buffer;
    `null`: names among x, u, gAd, gBd, ggd, w, mode, gK passed as NULL."""
    p = lambda k: None if k in null else C.cast(buf, C.c_void_p)
    if name in LINEARISE:
        return [fleet, B, N, p("x"), 1, 1, p("u"), 1, 1, p("gAd"), p("gBd"), p("ggd"), p("gK"), device, None]
    return [fleet, B, p("x"), 1, p("u"), 1, p("w"), p("mode"), p("gK"), device, None]


def _call(name, *a, **kw):
    L = md._bind()
    rc = getattr(L, f"mpcqp_{name}_fleet_device")(*_args(name, *a, **kw))
    return rc, L.mpcqp_last_error()


@pytest.mark.parametrize("name", LINEARISE + STEP)
def test_refusals_come_before_any_device_call(name):
    buf = (C.c_double * 512)()
    f = _fleet(name)
    bad = f"{name}_fleet: bad arguments".encode()
    assert _call(name, None, 3, buf) == (EINVAL, bad)
    for k in ("x", "u", "gK"):
        assert _call(name, f._h, 3, buf, null=(k,)) == (EINVAL, bad), k
    assert _call(name, f._h, -1, buf) == (EINVAL, bad)
    if name in LINEARISE:
        assert _call(name, f._h, 3, buf, N=0) == (EINVAL, bad)
    for B in (2, 4, 0):
        rc, msg = _call(name, f._h, B, buf)
        assert rc == EINVAL and msg.startswith(f"{name}_fleet:".encode()) and b"fleet's size 3" in msg, (B, msg)
    rc, msg = _call(name, f._h, 3, buf, device=1)
    assert rc == EINVAL and b"created for device 0, the call is on device 1" in msg, msg
    assert not np.frombuffer(buf, dtype=np.float64).any()


@pytest.mark.parametrize("name", LINEARISE)
def test_more_stages_than_a_block_holds_is_unsupported(name):
    """The stage sum keeps whole vehicles in one 256-thread block (mpcqp.h): N = 256 passes the
    check -- and then meets the fleet's size check, still before any device call -- N = 257 is
    MPCQP_EUNSUPPORTED, and so for a fleet of the right size."""
    buf = (C.c_double * 512)()
    f = _fleet(name)
    rc, msg = _call(name, f._h, 3, buf, N=257)
    assert rc == EUNSUPPORTED and msg.startswith(f"{name}_fleet: need N <= 256".encode()), (rc, msg)
    rc, msg = _call(name, f._h, 2, buf, N=257)
    assert rc == EUNSUPPORTED, (rc, msg)
    rc, msg = _call(name, f._h, 2, buf, N=256)
    assert rc == EINVAL and b"fleet's size 3" in msg, (rc, msg)
    assert not np.frombuffer(buf, dtype=np.float64).any()


@pytest.mark.parametrize("name", LINEARISE + STEP)
def test_an_empty_batch_never_reaches_the_device(name):
    """B = 0 is a no-op in the entry points that take a struct; a fleet has at least one vehicle
    (mpcqp_fleet_create), so here B = 0 is the size refusal, as in the twelve twins."""
    buf = (C.c_double * 512)()
    rc, msg = _call(name, _fleet(name)._h, 0, buf)
    assert rc == EINVAL and b"B = 0 is not the fleet's size 3" in msg
    assert not np.frombuffer(buf, dtype=np.float64).any()


def _params(car):
    return np.array([fc.CARS[car][k] for k in FIELDS] + [fc.DT_DYN])


def _constants(p):
    return md.Fleet([md.Vehicle(*p)]).constants()[0]


@pytest.mark.parametrize("car", list(fc.CARS))
def test_vehicle_constants_vjp_is_the_host_statement_and_the_differences(car):
    """Against mpc.vehicle_constants_vjp (the same dual arithmetic, the same order: 4 ulp of the
    row's largest entry) and against central differences of mpcqp_fleet_constants (h = 1e-6
    relative; the scaled measure of tests/test_param_grad_ref.py, bar 1e-8 as there)."""
    L = md._bind()
    p = _params(car)
    rng = np.random.default_rng(3)
    gk, out = rng.standard_normal(13), np.empty(9)
    veh = md.Vehicle(*p)
    assert L.mpcqp_vehicle_constants_vjp(C.byref(veh), md._np_ptr(gk), md._np_ptr(out)) == 0
    want = mpc.vehicle_constants_vjp(p, gk)
    print(f"{car}: vs host statement {np.abs(out - want).max() / np.abs(want).max():.2e}")
    assert np.abs(out - want).max() <= 4 * np.finfo(float).eps * np.abs(want).max()
    fd = np.empty(9)
    for a in range(9):
        up, dn = p.copy(), p.copy()
        up[a] *= 1 + 1e-6
        dn[a] *= 1 - 1e-6
        fd[a] = (np.dot(gk, _constants(up)) - np.dot(gk, _constants(dn))) / 2e-6
    dev = np.abs(out * p - fd).max() / np.abs(out * p).max()
    print(f"{car}: vs differences of mpcqp_fleet_constants {dev:.2e}")
    assert dev <= 1e-8
    # the Jacobian's structure: width and length reach Iz only, C_d and A_f cda only, dt itself
    e = np.zeros(13)
    e[3] = 1.0
    assert L.mpcqp_vehicle_constants_vjp(C.byref(veh), md._np_ptr(e), md._np_ptr(out)) == 0
    assert np.isclose(out[0], (p[3] ** 2 + p[4] ** 2) / 12, rtol=4e-16, atol=0) and not out[[1, 2, 5, 6, 7, 8]].any()
    e[:] = 0.0
    e[4] = 1.0
    assert L.mpcqp_vehicle_constants_vjp(C.byref(veh), md._np_ptr(e), md._np_ptr(out)) == 0
    assert list(out) == [0.0] * 8 + [1.0]


def test_vehicle_constants_vjp_refuses_null():
    L = md._bind()
    a = np.zeros(13)
    veh = md.Vehicle()
    for args in ((None, md._np_ptr(a), md._np_ptr(a)), (C.byref(veh), None, md._np_ptr(a)),
                 (C.byref(veh), md._np_ptr(a), None)):
        assert L.mpcqp_vehicle_constants_vjp(*args) == EINVAL
        assert L.mpcqp_last_error().startswith(b"vehicle_constants_vjp:")


def test_fleet_constants_vjp_of_the_classes():
    f = md.Fleet(fc.vehicles(md, "cars"))
    gK = np.random.default_rng(1).standard_normal((3, 13))
    g = f.constants_vjp(gK)
    assert g.shape == (3, 9)
    for b, car in enumerate(fc.ORDER):
        assert np.allclose(g[b], mpc.vehicle_constants_vjp(_params(car), gK[b]), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match=r"\(3, 13\)"):
        f.constants_vjp(gK[:2])
    k = md.KinFleet(fc.kin_vehicles(md, "cars"))
    assert np.array_equal(k.constants_vjp(gK[:, :3]), gK[:, :3])
    with pytest.raises(ValueError):
        k.constants_vjp(gK)
