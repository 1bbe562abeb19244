"""Host-side checks of the adjoint entry points (no GPU needed): both symbols are exported and a
NULL handle is refused with MPCQP_EINVAL before any device call.  The argument checks that need
a handle (nrhs < 1, both seeds NULL, no solve yet) are in tests/test_adjoint_device.py."""
import ctypes as C

import osqp_amd

EINVAL = 1  # include/mpcqp.h


def test_adjoint_symbols_are_exported():
    lib = C.CDLL(osqp_amd.LIB_PATH)
    assert hasattr(lib, "mpcqp_adjoint_device") and hasattr(lib, "mpcqp_adjoint_batch")


def test_adjoint_null_handle_is_einval():
    L = osqp_amd.lib()
    null = C.c_void_p()
    gx = (C.c_double * 2)(1.0, 0.0)
    assert L.mpcqp_adjoint_batch(null, 1, gx, None, None, None, None, None, None, None, None, None, None,
                                 None) == EINVAL
    assert b"NULL handle" in L.mpcqp_last_error()
    assert L.mpcqp_adjoint_device(null, 1, C.cast(gx, C.c_void_p), None, None, None, None, None, None, None, None,
                                  None, None, None, None) == EINVAL


def test_adjoint_needs_a_set_up_object():
    import numpy as np
    import pytest
    with pytest.raises(ValueError, match="not initialized"):
        osqp_amd.OSQP().adjoint(gx=np.ones(2))
    with pytest.raises(ValueError, match="not initialized"):
        osqp_amd.OSQPBatch().adjoint(gx=np.ones((1, 2)))
