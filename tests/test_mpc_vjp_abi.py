"""Host-side checks of the MPC-step VJP entry points (no GPU needed): every new symbol is exported
and a NULL layout / NULL affine map is refused with MPCQP_EINVAL and a message before any device
call.  What needs a device is in tests/test_mpc_vjp_device.py."""
import ctypes as C

import pytest

import osqp_amd
from osqp_amd import mpc_device

EINVAL = 1  # include/mpcqp.h
SYMBOLS = ("mpcqp_ltv_assemble_vjp_device", "mpcqp_incr_assemble_vjp_device", "mpcqp_ltv_assemble_w_device",
           "mpcqp_incr_assemble_w_device", "mpcqp_affine_vjp_device", "mpcqp_kin_linearise_vjp_device")


def test_vjp_symbols_are_exported():
    lib = C.CDLL(osqp_amd.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


@pytest.mark.parametrize("symbol,nargs,msg", [
    ("mpcqp_ltv_assemble_vjp_device", 21, b"ltv_assemble_vjp: NULL layout"),
    ("mpcqp_incr_assemble_vjp_device", 17, b"incr_assemble_vjp: NULL layout"),
    ("mpcqp_ltv_assemble_w_device", 16, b"ltv_assemble_w: bad arguments"),
    ("mpcqp_incr_assemble_w_device", 14, b"incr_assemble_w: bad arguments"),
])
def test_null_layout_is_einval(symbol, nargs, msg):
    L = mpc_device._bind()
    buf = (C.c_double * 4)()
    ptr = C.cast(buf, C.c_void_p)
    # a non-NULL pointer everywhere but the layout: the refusal is the layout's
    assert getattr(L, symbol)(None, 1, *([ptr] * (nargs - 1)), None) == EINVAL
    assert msg in L.mpcqp_last_error()


def test_null_affine_is_einval():
    L = mpc_device._bind()
    buf = (C.c_double * 4)()
    ptr = C.cast(buf, C.c_void_p)
    assert L.mpcqp_affine_vjp_device(None, 1, ptr, ptr, ptr, None, ptr, 4, None) == EINVAL
    assert b"affine_vjp: NULL affine map" in L.mpcqp_last_error()


def test_null_vehicle_is_einval():
    L = mpc_device._bind()
    buf = (C.c_double * 4)()
    ptr = C.cast(buf, C.c_void_p)
    assert L.mpcqp_kin_linearise_vjp_device(None, 1, 1, ptr, 4, 4, ptr, 2, 2, ptr, ptr, ptr, ptr, ptr, 0,
                                            None) == EINVAL
    assert b"kin_linearise_vjp: bad arguments" in L.mpcqp_last_error()
