"""Host-side checks of the fleet ABI of DESIGN.md §24 (no GPU needed): the header declares and the
library exports every new symbol, creation refuses what mpcqp.h says it refuses -- before any device
call: these tests run where there is no device -- and a valid call after a refusal succeeds; every
`_fleet` twin refuses a NULL fleet and a batch that is not the fleet's size; mpcqp_fleet_constants
against osqp_amd.mpc.VehicleParams; the Python classes.  What needs a device is in
tests/test_fleet_device.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import fleet_cases as fc
import osqp_amd
from osqp_amd import mpc, mpc_device as md

EINVAL = 1  # include/mpcqp.h (tests/test_rollout_abi.py holds it to the header)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcqp.h")
TWINS = ("linearise", "linearise_vjp", "incr_shift", "incr_shift_vjp", "kin_linearise", "kin_linearise_vjp",
         "kin_shift", "kin_shift_vjp", "kin_rollout", "kin_ltv_shift", "kin_ltv_shift_vjp", "lane_tail")
DYNAMIC = ("linearise", "linearise_vjp", "incr_shift", "incr_shift_vjp")
SYMBOLS = [("int", "mpcqp_fleet_create"), ("int", "mpcqp_kin_fleet_create"), ("int", "mpcqp_fleet_constants"),
           ("void", "mpcqp_fleet_free"), ("void", "mpcqp_kin_fleet_free")] + \
          [("int", f"mpcqp_{t}_fleet_device") for t in TWINS]


@pytest.mark.parametrize("ret,name", SYMBOLS)
def test_header_declares_and_library_exports(ret, name):
    assert f"{ret} {name}(" in open(HEADER).read()
    assert hasattr(C.CDLL(osqp_amd.LIB_PATH), name)


def _create(kind, structs, B=None, null_veh=False, null_out=False):
    L = md._bind()
    arr = (kind * max(len(structs), 1))(*structs)
    h = md.vp()
    fn = L.mpcqp_fleet_create if kind is md.Vehicle else L.mpcqp_kin_fleet_create
    rc = fn(len(structs) if B is None else B, None if null_veh else arr, 0, None if null_out else C.byref(h))
    return rc, h, L.mpcqp_last_error()


def _free(kind, h):
    L = md._bind()
    (L.mpcqp_fleet_free if kind is md.Vehicle else L.mpcqp_kin_fleet_free)(h)


def _with(kind, **kw):
    return [kind(), kind(**kw)]


REFUSALS = [(f"{kind.__name__} {what}", kind, make) for kind in (md.Vehicle, md.KinVehicle) for what, make in (
    ("NULL veh", lambda k: dict(structs=[k()], null_veh=True)),
    ("NULL out", lambda k: dict(structs=[k()], null_out=True)),
    ("B = 0", lambda k: dict(structs=[k()], B=0)),
    ("B < 0", lambda k: dict(structs=[k()], B=-3)),
    ("nan field", lambda k: dict(structs=_with(k, l_r=math.nan))),
    ("inf field", lambda k: dict(structs=_with(k, dt=math.inf))),
    ("l_f = 0", lambda k: dict(structs=_with(k, l_f=0.0))),
    ("l_r < 0", lambda k: dict(structs=_with(k, l_r=-1.4))),
    ("dt = 0", lambda k: dict(structs=_with(k, dt=0.0))),
    ("another dt", lambda k: dict(structs=_with(k, dt=np.nextafter(k().dt, 1.0)))),
)] + [(f"Vehicle {what}", md.Vehicle, make) for what, make in (
    ("m = 0", lambda k: dict(structs=_with(k, m=0.0))),
    ("nan C_d", lambda k: dict(structs=_with(k, C_d=math.nan))),
    ("no extent", lambda k: dict(structs=_with(k, width=0.0, length=0.0))),
)]


@pytest.mark.parametrize("label,kind,make", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_create_refuses_and_a_valid_call_follows(label, kind, make):
    rc, h, msg = _create(kind, **make(kind))
    assert rc == EINVAL and msg.startswith(b"fleet_create:"), (rc, msg)
    assert not h.value
    rc, h, _ = _create(kind, [kind(), kind(l_f=1.1)])
    assert rc == 0 and h.value
    _free(kind, h)


def test_constants_refuses_what_is_not_there():
    L = md._bind()
    f = md.Fleet([md.Vehicle()])
    out = np.zeros(13)
    for args in ((None, 0, md._np_ptr(out)), (f._h, 0, None), (f._h, 1, md._np_ptr(out)), (f._h, -1, md._np_ptr(out))):
        assert L.mpcqp_fleet_constants(*args) == EINVAL and L.mpcqp_last_error().startswith(b"fleet_constants:")
    assert L.mpcqp_fleet_constants(f._h, 0, md._np_ptr(out)) == 0 and out[0] == 1300.0


def _ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


@pytest.mark.parametrize("car", list(fc.CARS))
def test_constants_are_vehicle_params(car):
    """(m, l_f, l_r, Iz, dt, cda, roll, B_f, C_f, D_f, B_r, C_r, D_r) against mpc.VehicleParams.  Equal
    where both sides are one expression in one order: m, l_f, l_r, dt, C, roh C_d A_f, C_roll m 9.81.
    Two ulp for Iz (width ** 2 is pow there, width * width here), for D (a0 Fz ** 2 there, (a0 Fz) Fz
    here) and for B = BCD / (C D) 180 / pi, which divides by that D."""
    p = fc.params(car)
    k = md.Fleet([md.Vehicle(dt=fc.DT_DYN, **fc.CARS[car])]).constants()[0]
    (Bf, Cf, Df), (Br, Cr, Dr) = p.pacejka()
    want = [p.m, p.l_f, p.l_r, p.Iz, p.dt, p.roh * p.C_d * p.A_f, p.C_roll * p.m * 9.81, Bf, Cf, Df, Br, Cr, Dr]
    names = ["m", "l_f", "l_r", "Iz", "dt", "cda", "roll", "B_f", "C_f", "D_f", "B_r", "C_r", "D_r"]
    loose = {"Iz", "B_f", "D_f", "B_r", "D_r"}
    for n, got, w in zip(names, k, want):
        print(f"{car} {n}: {got!r} vs {w!r}, {_ulps(got, w):.1f} ulp")
    for n, got, w in zip(names, k, want):
        assert got == w if n not in loose else _ulps(got, w) <= 2.0, (car, n, got, w)


def _layouts():
    dyn = md.IncrementalLayout(3, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                               -mpc.DYN_DUMIN)
    kin = md.IncrementalLayout(3, mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, mpc.KIN_XMIN_T, mpc.KIN_XMAX_T, mpc.KIN_DUMIN,
                               -mpc.KIN_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B)
    ltv = md.LTVLayout(3, mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R, mpc.KINLTV_XMIN, mpc.KINLTV_XMAX, mpc.KINLTV_UMIN,
                       mpc.KINLTV_UMAX, mpc.KIN_MASK_A, mpc.KIN_MASK_B)
    return {"incr_shift": dyn, "incr_shift_vjp": dyn, "kin_shift": kin, "kin_shift_vjp": kin, "lane_tail": kin,
            "kin_ltv_shift": ltv, "kin_ltv_shift_vjp": ltv}


def _twin_args(twin, fleet, B, buf):
    """Arguments of mpcqp_<twin>_fleet_device that pass the twin's own checks: every pointer on one
    scratch buffer, N = 2 where the call takes one (the int32 after B), strides 1, device 0, no
    trajectory record, an empty schedule."""
    fn = getattr(md._bind(), f"mpcqp_{twin}_fleet_device")
    lay = _layouts().get(twin)
    lead = [] if lay is None else [lay._h]
    rest = []
    for i, t in enumerate(fn.argtypes[len(lead) + 2:]):
        rest.append(C.cast(buf, C.c_void_p) if t is md.vp else 1 if t is C.c_int64 else (2 if i == 0 else 0))
    return fn, lead + [fleet, B] + rest, lay


@pytest.mark.parametrize("twin", TWINS)
def test_twin_refuses_null_and_wrong_size_before_any_device_call(twin):
    L = md._bind()
    buf = (C.c_double * 512)()
    fleet = md.Fleet(fc.vehicles(md, "cars")) if twin in DYNAMIC else md.KinFleet(fc.kin_vehicles(md, "cars"))
    fn, args, _lay = _twin_args(twin, None, 3, buf)
    assert fn(*args) == EINVAL, L.mpcqp_last_error()
    for B in (2, 4, 0):
        fn, args, _lay = _twin_args(twin, fleet._h, B, buf)
        assert fn(*args) == EINVAL, (B, L.mpcqp_last_error())
        assert b"fleet's size 3" in L.mpcqp_last_error(), L.mpcqp_last_error()
    assert not np.frombuffer(buf, dtype=np.float64).any()


def test_fleet_classes():
    cars = fc.vehicles(md, "cars")
    f = md.Fleet(cars)
    assert len(f) == 3 and f.dt == fc.DT_DYN and f.constants().shape == (3, 13)
    for b, car in enumerate(fc.ORDER):
        assert isinstance(f[b], md.Vehicle) and f[b].m == fc.CARS[car]["m"] and f[b].C_roll == fc.CARS[car]["C_roll"]
    assert f[-1].m == f[2].m
    with pytest.raises(IndexError):
        f[3]
    k = md.KinFleet(fc.kin_vehicles(md, "cars"))
    assert len(k) == 3 and k.dt == fc.DT_KIN and k[0].l_f == fc.CARS["van"]["l_f"]
    with pytest.raises(TypeError):
        md.Fleet(fc.kin_vehicles(md, "cars"))
    with pytest.raises(Exception, match="fleet_create"):
        md.Fleet([])
    with pytest.raises(Exception, match="fleet_create"):
        md.KinFleet([md.KinVehicle(), md.KinVehicle(dt=0.05)])


def test_from_arrays_broadcasts():
    b = np.arange(fc.B_SWEEP)
    f = md.Fleet.from_arrays(m=1000 + 5 * b, l_f=1.0 + 0.004 * b, dt=fc.DT_DYN)
    ref = md.Fleet(fc.vehicles(md, "sweep"))
    assert len(f) == fc.B_SWEEP and np.array_equal(f.constants(), ref.constants())
    assert f[7].m == 1035.0 and f[7].l_r == md.Vehicle().l_r
    k = md.KinFleet.from_arrays(l_f=[1.0, 1.1], l_r=1.3)
    assert len(k) == 2 and (k[1].l_f, k[1].l_r, k[1].dt) == (1.1, 1.3, md.KinVehicle().dt)
    assert len(md.Fleet.from_arrays()) == 1
    with pytest.raises(TypeError):
        md.KinFleet.from_arrays(m=[1.0])


def test_a_fleet_of_another_size_is_a_value_error():
    f = md.KinFleet(fc.kin_vehicles(md, "cars"))
    with pytest.raises(ValueError, match="fleet of 3"):
        md._entry("kin_shift", f, 2)
    fn, arg = md._entry("kin_shift", f, 3)
    assert fn is md._bind().mpcqp_kin_shift_fleet_device and arg is f._h
