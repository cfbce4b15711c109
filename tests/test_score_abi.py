"""pb_score_*: the paths that need no device -- a NULL context, and the binding's shape checks, which precede every ABI call."""
import ctypes as C

import numpy as np
import pytest

from pronto_amd import _lib
from pronto_amd import batch as pa


def test_null_context_is_an_argument_error():
    _lib.build()
    lib = _lib.load()
    pose = np.zeros(7)
    ut, out10 = C.c_int64(), (C.c_double * 10)()
    f, v = C.c_int(), C.c_double()
    assert lib.pb_score_init(None, 10.0, 0.0) == _lib.PB_ERR_ARG
    assert lib.pb_score_ground_truth(None, 0, None, pose.ctypes.data, None, _lib.PB_SLOT_HEAD, _lib.PB_SCORE_DRIFT, _lib.PB_HOST_BROADCAST) == _lib.PB_ERR_ARG
    assert lib.pb_score_get(None, 0, 0, None, None, _lib.PB_HOST) == _lib.PB_ERR_ARG
    assert lib.pb_score_last(None, 0, C.byref(ut), out10) == _lib.PB_ERR_ARG
    assert lib.pb_score_best(None, _lib.PB_SCORE_MEAN_PDDT, C.byref(f), C.byref(v)) == _lib.PB_ERR_ARG


def test_python_constants_match_the_header():
    import score_common as sc
    for name in ("DRIFT", "ABS", "ROWS", "COUNTS", "MEAN_PDDT", "RMS_DRIFT", "ATE_RMSE"):
        assert getattr(_lib, "PB_SCORE_" + name) == sc.R(name)


def test_binding_refuses_misshaped_arrays_before_calling_the_abi():
    class Shapes(pa.BatchEstimator):
        def __init__(self):
            self.B, self.n = 8, 15

        def close(self):
            pass
        __del__ = close

    f = Shapes()
    ok = np.zeros((7, 8))
    bad = [(f.score_ground_truth, (0, np.zeros((7, 7)))),
           (f.score_ground_truth, (0, np.zeros((6, 8)))),
           (f.score_ground_truth, (0, np.zeros(6))),
           (f.score_ground_truth, (0, None)),
           (f.score_ground_truth, (0, ok, np.ones(7, dtype=np.uint8))),
           (f.score_ground_truth, (0, ok, None, np.zeros(9, dtype=np.int64))),
           (f.score_ground_truth, (0, ok, None, None, -1, False, False)),
           (f.score_init, (-1.0, 0.0)),
           (f.score_init, (10.0, -0.25)),
           (f.score_init, (float("nan"), 0.0)),
           (f.score_get, (4, 5)),
           (f.score_get, (-1, 2)),
           (f.score_last, (8,)),
           (f.score_best, ("likelihood",)),
           (f.score_best, (3,))]
    for fn, args in bad:
        with pytest.raises(ValueError):
            fn(*args)
