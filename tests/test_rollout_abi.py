"""Host-side checks of the three entry points of DESIGN.md §18 (no GPU needed): the header declares
them, the library exports them, and mpcqp_incr_shift_vjp_device refuses bad arguments before any
device call.  What needs a device is in tests/test_rollout_device.py."""
import ctypes as C
import os

import numpy as np
import pytest

import osqp_amd
from osqp_amd import mpc, mpc_device

EINVAL, EUNSUPPORTED = 1, 2  # include/mpcqp.h
NEW = ("mpcqp_save_solution_device", "mpcqp_load_solution_device", "mpcqp_incr_shift_vjp_device")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcqp.h")


def test_error_codes_are_the_headers():
    text = open(HEADER).read()
    assert f"#define MPCQP_EINVAL {EINVAL} " in text and f"#define MPCQP_EUNSUPPORTED {EUNSUPPORTED} " in text


@pytest.mark.parametrize("name", NEW)
def test_header_declares_and_library_exports(name):
    assert f"int {name}(" in open(HEADER).read()
    assert hasattr(C.CDLL(osqp_amd.LIB_PATH), name)


def _dyn_layout(N=3):
    return mpc_device.IncrementalLayout(N, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T,
                                        mpc.DYN_DUMIN, -mpc.DYN_DUMIN)


def _args(layout, veh, B=1, null=()):
    buf = (C.c_double * 256)()
    ptr = C.cast(buf, C.c_void_p)
    names = ("sol", "Ad", "Bd", "gd", "xt", "gxt", "gpred", "gpdu", "gsol", "gAd0", "gBd0", "ggd0", "gxt_o")
    return [None if "L" in null else layout._h, None if "veh" in null else C.byref(veh), B] + \
        [None if k in null else ptr for k in names] + [None], buf


@pytest.mark.parametrize("null,B", [("L", 1), ("veh", 1), ("sol", 1), ("Ad", 1), ("Bd", 1), ("xt", 1), (None, -1)])
def test_shift_vjp_bad_arguments_are_einval(null, B):
    L = mpc_device._bind()
    lay, veh = _dyn_layout(), mpc_device.Vehicle()
    args, _ = _args(lay, veh, B, () if null is None else (null,))
    assert L.mpcqp_incr_shift_vjp_device(*args) == EINVAL
    assert b"incr_shift_vjp: bad arguments" in L.mpcqp_last_error()


def test_shift_vjp_needs_the_dynamic_bicycle():
    L = mpc_device._bind()
    kin = mpc_device.IncrementalLayout(3, mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, mpc.KIN_XMIN_T, mpc.KIN_XMAX_T,
                                       mpc.KIN_DUMIN, -mpc.KIN_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B)
    assert (kin.nx, kin.nu) == (4, 2)
    args, _ = _args(kin, mpc_device.Vehicle())
    assert L.mpcqp_incr_shift_vjp_device(*args) == EUNSUPPORTED
    assert b"incr_shift_vjp" in L.mpcqp_last_error() and b"nx 6, nu 2" in L.mpcqp_last_error()


def test_shift_vjp_with_nothing_to_do_touches_nothing():
    """B = 0, or no output asked for: success without a device call (this machine has no device)."""
    L = mpc_device._bind()
    lay, veh = _dyn_layout(), mpc_device.Vehicle()
    args, buf = _args(lay, veh, 0)
    assert L.mpcqp_incr_shift_vjp_device(*args) == 0
    args, buf = _args(lay, veh, 1, ("gsol", "gAd0", "gBd0", "ggd0", "gxt_o", "gd", "gxt", "gpred", "gpdu"))
    assert L.mpcqp_incr_shift_vjp_device(*args) == 0
    assert not np.frombuffer(buf, dtype=np.float64).any()


@pytest.mark.parametrize("name", ["mpcqp_save_solution_device", "mpcqp_load_solution_device"])
def test_record_entry_points_refuse_null(name):
    L = osqp_amd.lib()
    buf = (C.c_double * 8)()
    assert getattr(L, name)(None, C.cast(buf, C.c_void_p), None) == EINVAL
    assert name.encode() in L.mpcqp_last_error()
