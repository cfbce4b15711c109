"""pb_set_imu_valid in front of pb_step_legodo_split with the IMU block and the leg-odometry block in the SAME space: the call is
handed on to pb_step_legodo, which must still see the one-shot mask (first item: it used to be taken by the
split entry and lost).  Against pb_set_imu_valid + pb_step_legodo on the same inputs, bit for bit; the masked half of the filters
(no IMU message, no measurement) keeps its prior."""
import numpy as np
import pytest

from pronto_amd import _lib
from pronto_amd.synth import Workload

pytestmark = pytest.mark.gpu


def _run(n, B, split, mem):
    import torch
    from pronto_amd.batch import BatchEstimator
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    q4 = w.process_noise()
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    est.predict(w.imu_block(0), q4)          # (omega / accel entries that are not the initial ones)
    est.sync()
    prior = est.get_head()
    imu = np.ascontiguousarray(w.imu_block(1))
    lo, mask = w.legodo_block(1)
    valid = (np.arange(B) % 2).astype(np.uint8)
    lo_mask = (mask.astype(bool) & valid.astype(bool)).astype(np.uint8)
    d_valid = torch.from_numpy(valid).to("cuda:0")
    if mem == _lib.PB_DEVICE:
        imu_a, lo_a, m_a = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (imu, lo, lo_mask))
    else:
        imu_a, lo_a, m_a = imu, np.ascontiguousarray(lo), lo_mask
    torch.cuda.synchronize()
    import ctypes as C
    ptr = lambda a: C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    q = (C.c_double * 4)(*q4)
    assert est._L.pb_set_imu_valid(est._h, C.c_void_p(d_valid.data_ptr())) == _lib.PB_OK
    if split:
        rc = est._L.pb_step_legodo_split(est._h, ptr(imu_a), mem, ptr(lo_a), ptr(m_a), mem, q)
    else:
        rc = est._L.pb_step_legodo(est._h, ptr(imu_a), ptr(lo_a), ptr(m_a), q, mem)
    assert rc == _lib.PB_OK, est._L.pb_last_error(est._h)
    est.sync()
    post = est.get_head()
    est.close()
    return prior, post, valid


@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("mem", [_lib.PB_DEVICE, _lib.PB_HOST])
def test_split_step_keeps_the_imu_mask(n, mem):
    B = 130
    prior, post_split, valid = _run(n, B, True, mem)
    _, post_ref, _ = _run(n, B, False, mem)
    for a, b in zip(post_split, post_ref):
        assert a.tobytes() == b.tobytes()
    idle = valid == 0
    v0, q0, P0, ll0 = prior
    v1, q1, P1, ll1 = post_split
    # the filters without a message: pose, velocity, biases, covariance and log-likelihood stay; for 15 states exactly everything,
    # for 21 the angular-velocity / acceleration entries are re-derived through the biases (omega + bg - bg: to the last bit)
    rows = np.arange(n)
    exact = rows if n == 15 else rows[(rows >= 3) & (rows < 12) | (rows >= 15)]
    assert v1[exact][:, idle].tobytes() == v0[exact][:, idle].tobytes()
    assert np.max(np.abs(v1[:, idle] - v0[:, idle])) <= 1e-15 * max(1.0, np.max(np.abs(v0[:, idle])))
    assert q1[:, idle].tobytes() == q0[:, idle].tobytes()
    assert P1[:, :, idle].tobytes() == P0[:, :, idle].tobytes()
    assert ll1[idle].tobytes() == ll0[idle].tobytes()
    # ... and the others did take the step
    assert np.all(np.any(P1[:, :, ~idle] != P0[:, :, ~idle], axis=(0, 1)))
