"""The yaw-lock entry points without a device (tests/test_abi.py proves that they are exported and bound): a NULL context is
PB_ERR_ARG everywhere.  pb_yawlock_init's own argument checks (modes 0 and 2 on a 15-state context) need a context, and a
context cannot be created without a device (pb_create: PB_ERR_NO_DEVICE, no CPU fallback): they are checked on the GPU,
tests/test_yawlock.py::test_argument_checks."""
import ctypes as C

import pytest

from pronto_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_null_context_is_an_argument_error(lib):
    one = (C.c_uint8 * 1)(1)
    g = (C.c_double * 1)(0.0)
    jp = (C.c_float * 16)()
    poses, info = (C.c_double * 14)(), (C.c_int64 * 4)()
    assert lib.pb_yawlock_init(None, 1, 1, 0, 1.0, 1.0, 1.0, 1.0) == _lib.PB_ERR_ARG
    assert lib.pb_yawlock_set_standing(None, one, _lib.PB_HOST_BROADCAST) == _lib.PB_ERR_ARG
    assert lib.pb_yawlock_set_gyro(None, g, _lib.PB_HOST_BROADCAST) == _lib.PB_ERR_ARG
    assert lib.pb_yawlock_update_joints(None, 0, None, None, 16, jp, _lib.PB_HOST_BROADCAST, None, None, None) == _lib.PB_ERR_ARG
    assert lib.pb_step_yawlock_joints(None, 0, None, None, 16, jp, _lib.PB_HOST_BROADCAST, None, None, None) == _lib.PB_ERR_ARG
    assert lib.pb_yawlock_get(None, 0, poses, info) == _lib.PB_ERR_ARG
