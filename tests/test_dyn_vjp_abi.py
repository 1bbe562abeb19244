"""Host-side checks of mpcqp_linearise_vjp_device (no GPU needed): the symbol is exported and bad
arguments are refused with MPCQP_EINVAL and a message before any device call.  What needs a device
is in tests/test_dyn_vjp_device.py."""
import ctypes as C

import pytest

import osqp_amd
from osqp_amd import mpc_device

EINVAL = 1  # include/mpcqp.h


def test_symbol_is_exported():
    assert hasattr(C.CDLL(osqp_amd.LIB_PATH), "mpcqp_linearise_vjp_device")


@pytest.mark.parametrize("null,B,N", [("veh", 1, 1), ("x", 1, 1), ("u", 1, 1), (None, -1, 1), (None, 1, 0)])
def test_bad_arguments_are_einval(null, B, N):
    L = mpc_device._bind()
    buf = (C.c_double * 36)()
    ptr = C.cast(buf, C.c_void_p)
    veh = mpc_device.Vehicle()
    args = [None if null == "veh" else C.byref(veh), B, N, None if null == "x" else ptr, 6, 6,
            None if null == "u" else ptr, 2, 2, ptr, ptr, ptr, ptr, ptr, 0, None]
    assert L.mpcqp_linearise_vjp_device(*args) == EINVAL
    assert b"linearise_vjp: bad arguments" in L.mpcqp_last_error()
    assert b"kin_" not in L.mpcqp_last_error()
