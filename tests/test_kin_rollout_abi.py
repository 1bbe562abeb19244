"""Host-side checks of the two entry points of DESIGN.md §19 (no GPU needed): the header declares
them, the library exports them, and both refuse bad arguments before any device call.  What needs a
device is in tests/test_kin_rollout_device.py."""
import ctypes as C
import os

import numpy as np
import pytest

import osqp_amd
from osqp_amd import mpc, mpc_device

EINVAL, EUNSUPPORTED = 1, 2  # include/mpcqp.h (tests/test_rollout_abi.py holds them to the header)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcqp.h")
# name -> (error prefix, argument names after (L, veh, B), the state-before argument, the outputs)
ENTRY = {
    "mpcqp_kin_shift_vjp_device": (b"kin_shift_vjp", ("sol", "Ad", "Bd", "gd", "xt", "mode", "gxt", "gpred", "gpdu",
                                                       "gsol", "gAd0", "gBd0", "ggd0", "gxt_o"), "xt",
                                   ("gsol", "gAd0", "gBd0", "ggd0", "gxt_o")),
    "mpcqp_kin_ltv_shift_vjp_device": (b"kin_ltv_shift_vjp", ("sol", "Ad", "Bd", "x", "mode", "gx", "gu", "gpred_x",
                                                               "gpred_u", "gsol", "gAd0", "gBd0", "ggd0", "gx_o"),
                                       "x", ("gsol", "gAd0", "gBd0", "ggd0", "gx_o")),
}


@pytest.mark.parametrize("name", list(ENTRY))
def test_header_declares_and_library_exports(name):
    assert f"int {name}(" in open(HEADER).read()
    assert hasattr(C.CDLL(osqp_amd.LIB_PATH), name)


def _kin_incr(N=3):
    return mpc_device.IncrementalLayout(N, mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, mpc.KIN_XMIN_T, mpc.KIN_XMAX_T,
                                        mpc.KIN_DUMIN, -mpc.KIN_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B)


def _kin_ltv(N=3):
    return mpc_device.LTVLayout(N, mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R, mpc.KINLTV_XMIN, mpc.KINLTV_XMAX,
                                mpc.KINLTV_UMIN, mpc.KINLTV_UMAX, mpc.KIN_MASK_A, mpc.KIN_MASK_B)


def _layout(name):
    return _kin_incr() if name == "mpcqp_kin_shift_vjp_device" else _kin_ltv()


def _args(name, layout, B=1, null=()):
    buf = (C.c_double * 256)()
    ptr = C.cast(buf, C.c_void_p)
    veh = mpc_device.KinVehicle()
    return [None if "L" in null else layout._h, None if "veh" in null else C.byref(veh), B] + \
        [None if k in null else ptr for k in ENTRY[name][1]] + [None], buf, veh


@pytest.mark.parametrize("null,B", [("L", 1), ("veh", 1), ("sol", 1), ("Ad", 1), ("Bd", 1), ("state", 1), (None, -1)])
@pytest.mark.parametrize("name", list(ENTRY))
def test_bad_arguments_are_einval(name, null, B):
    L = mpc_device._bind()
    null = ENTRY[name][2] if null == "state" else null
    args, _, _veh = _args(name, _layout(name), B, () if null is None else (null,))
    assert getattr(L, name)(*args) == EINVAL
    assert ENTRY[name][0] + b": bad arguments" in L.mpcqp_last_error()


def test_kin_shift_vjp_needs_the_kinematic_bicycle():
    L = mpc_device._bind()
    dyn = mpc_device.IncrementalLayout(3, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T,
                                       mpc.DYN_DUMIN, -mpc.DYN_DUMIN)
    assert (dyn.nx, dyn.nu) == (6, 2)
    args, _, _veh = _args("mpcqp_kin_shift_vjp_device", dyn)
    assert L.mpcqp_kin_shift_vjp_device(*args) == EUNSUPPORTED
    assert b"kin_shift_vjp" in L.mpcqp_last_error() and b"nx 4, nu 2" in L.mpcqp_last_error()


def test_kin_ltv_shift_vjp_needs_the_kinematic_bicycle():
    L = mpc_device._bind()
    six = mpc_device.LTVLayout(3, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T[:6], mpc.DYN_XMAX_T[:6],
                               mpc.DYN_XMIN_T[6:], mpc.DYN_XMAX_T[6:], mpc.DYN_MASK_A, mpc.DYN_MASK_B)
    assert (six.nx, six.nu) == (6, 2)
    args, _, _veh = _args("mpcqp_kin_ltv_shift_vjp_device", six)
    assert L.mpcqp_kin_ltv_shift_vjp_device(*args) == EUNSUPPORTED
    assert b"kin_ltv_shift_vjp" in L.mpcqp_last_error() and b"nx 4, nu 2" in L.mpcqp_last_error()


@pytest.mark.parametrize("name", list(ENTRY))
def test_nothing_to_do_touches_nothing(name):
    """B = 0, or no output asked for: success without a device call (these tests run where there is no device)."""
    L = mpc_device._bind()
    lay = _layout(name)
    args, buf, _veh = _args(name, lay, 0)
    assert getattr(L, name)(*args) == 0
    cots = tuple(k for k in ENTRY[name][1] if k.startswith("g") and k not in ENTRY[name][3])
    args, buf, _veh = _args(name, lay, 1, ENTRY[name][3] + cots + ("mode",))
    assert getattr(L, name)(*args) == 0
    assert not np.frombuffer(buf, dtype=np.float64).any()
