"""pb_set_pred_slot: the fused step (pb_step_legodo / pb_step_legodo_split) also writes its INS posterior -- the prediction, before
the leg-odometry update behind it -- into a checkpoint slot (what EKFSmoothBackwardsPass reads at every INS update,
mav_state_est.cpp:98-189).  The slot must hold what pb_predict alone leaves from the same head, the filtered head must be what the
same call leaves without a predicted slot (bit for bit), and the setting is one-shot.  Runs on the MI355X."""
import numpy as np
import pytest

from smoother_ref import start_of
from util import embed21, rel

from pronto_amd.synth import Workload

TOL = 1e-9        # against the oracle (block-relative, as tests/test_gpu_parity.py)
TOL_PRED = 1e-13  # against pb_predict from the same head (observed: bit for bit for 15 states, 1.1e-16 for 21)

pytestmark = pytest.mark.gpu


def _inputs(w, mem, masked, dev, k=0):
    import torch
    imu = w.imu_block(k)
    lo, mask = w.legodo_block(k)
    if not masked:
        mask = None
    if mem == "broadcast":
        return np.ascontiguousarray(imu[:, 0]), np.ascontiguousarray(lo[:, 0]), None
    if mem == "device":
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t(imu), t(lo), t(mask)
    return imu, lo, mask


def _fresh(oracle, w, n, B, slots=4):
    from pronto_amd.batch import BatchEstimator
    est = BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    vec, quat, P0, q4 = start_of(w)
    est.reset(vec, quat, P0)
    est.history_reserve(slots)
    return est, q4


def _split(est, imu, lo, mask, q4, imu_mem_differs):
    """pb_step_legodo_split: with imu_mem != lo_mem (a broadcast IMU message, the measurement where it is), or with both in the same
    space (the call delegates to pb_step_legodo)."""
    import ctypes as C
    from pronto_amd.batch import _ptr, _ptr_block, _same_mem, PB_HOST_BROADCAST
    if imu_mem_differs:   # one IMU message for every filter (PB_HOST_BROADCAST): the first filter's
        imu = np.ascontiguousarray((imu if isinstance(imu, np.ndarray) else imu.cpu().numpy())[:, 0])
    pi, m1 = _ptr_block(imu, 7, est.B)
    pl, m2 = _ptr_block(lo, 6, est.B)
    pm, m3 = _ptr(mask, np.uint8, shape=(est.B,))
    mlo = _same_mem(m2, m3)
    assert (m1 != mlo) == imu_mem_differs or m1 == PB_HOST_BROADCAST
    q = (C.c_double * 4)(*q4)
    est._chk(est._L.pb_step_legodo_split(est._h, pi, m1, pl, pm, mlo, q))
    return imu


CASES = [(n, B, mem, masked) for n in (15, 21) for B in (64, 1000, 65536) for mem in ("host", "device", "broadcast")
         for masked in (False, True) if not (mem == "broadcast" and masked)]


@pytest.mark.parametrize("n,B,mem,masked", CASES)
def test_pred_slot_is_the_prediction_and_the_head_is_unchanged(oracle, n, B, mem, masked):
    import torch
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = _inputs(w, mem, masked, dev)
    # the fused step with a predicted slot
    est, q4 = _fresh(oracle, w, n, B)
    est.set_pred_slot(1)
    est.step_legodo(imu, lo, mask, q4)
    pred = est.get_slot(1)
    head_sum = est.state_checksum()
    slot_sum = est.state_checksum(1)
    # one-shot: the next step writes no slot
    imu1, lo1, mask1 = _inputs(w, mem, masked, dev, k=1)
    est.step_legodo(imu1, lo1, mask1, q4)
    assert est.state_checksum(1) == slot_sum
    est.close()
    # the same call without a predicted slot: the same filtered head, bit for bit
    ref, _ = _fresh(oracle, w, n, B)
    ref.step_legodo(imu, lo, mask, q4)
    assert ref.state_checksum() == head_sum
    ref.close()
    # pb_predict alone from the same head
    ref, _ = _fresh(oracle, w, n, B)
    ref.predict(imu, q4)
    want = ref.get_head()
    ref.close()
    worst = max(rel(a, b) for a, b in zip(pred, want))
    bits = all(np.array_equal(a, b) for a, b in zip(pred, want))
    print("n=%d B=%d %s mask=%s: predicted slot vs pb_predict %.1e (%s)" % (n, B, mem, masked, worst, "bit for bit" if bits else "not bit for bit"))
    assert worst <= TOL_PRED, worst
    # ... and the oracle's predict
    if B <= 1000:
        vec, quat, P0, _ = start_of(w)
        v21, P21 = embed21(vec, P0)
        ob = oracle.OracleBatch(v21, quat, P21)
        imu0 = w.imu_block(0)
        ob.predict(np.repeat(imu0[:, :1], B, axis=1) if mem == "broadcast" else imu0, q4)
        v, q, P, _ = pred
        err = max(rel(v, ob.vec[:n]), rel(q, ob.quat), rel(P, ob.cov[:n, :n]))
        assert err < TOL, err


@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("B", [64, 1000, 65536])
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("differs", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_pred_slot_through_the_split_entry_point(oracle, n, B, mem, differs, masked):
    """pb_step_legodo_split with imu_mem != lo_mem, and with imu_mem == lo_mem (delegated to pb_step_legodo: the setting must survive
    the delegation and be consumed once)."""
    import torch
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = _inputs(w, mem, masked, dev)
    est, q4 = _fresh(oracle, w, n, B)
    est.set_pred_slot(2)
    imu_used = _split(est, imu, lo, mask, q4, differs)
    pred = est.get_slot(2)
    head_sum, slot_sum = est.state_checksum(), est.state_checksum(2)
    est.step_legodo(*_inputs(w, mem, masked, dev, k=1), q4)   # consumed: slot 2 stays
    assert est.state_checksum(2) == slot_sum
    est.close()
    ref, _ = _fresh(oracle, w, n, B)
    _split(ref, imu, lo, mask, q4, differs)
    assert ref.state_checksum() == head_sum
    ref.close()
    ref, _ = _fresh(oracle, w, n, B)
    ref.predict(imu_used, q4)
    want = ref.get_head()
    ref.close()
    assert max(rel(a, b) for a, b in zip(pred, want)) <= TOL_PRED


@pytest.mark.parametrize("n", [15, 21])
def test_pred_slot_and_output_slot_in_one_call(oracle, n):
    import torch
    B = 1000
    w = Workload(B, n_states=n)
    imu, lo, mask = _inputs(w, "host", True, torch.device("cuda:0"))
    est, q4 = _fresh(oracle, w, n, B)
    est.set_output_slot(3)
    est.set_pred_slot(0)
    est.step_legodo(imu, lo, mask, q4)
    assert est._L.pb_head_slot(est._h) == 3
    pred, filt = est.get_slot(0), est.get_slot(3)
    # a second pair from a head that lives in a slot: the prediction must not land on it
    est.set_pred_slot(1)
    est.set_output_slot(2)
    est.step_legodo(*_inputs(w, "host", True, torch.device("cuda:0"), k=1), q4)
    pred1, filt1 = est.get_slot(1), est.get_slot(2)
    assert all(np.array_equal(a, b) for a, b in zip(est.get_slot(3), filt))   # the checkpoint it read is untouched
    est.close()
    ref, _ = _fresh(oracle, w, n, B)
    ref.predict(imu, q4)
    assert max(rel(a, b) for a, b in zip(pred, ref.get_head())) <= TOL_PRED
    ref.close()
    ref, _ = _fresh(oracle, w, n, B)
    ref.step_legodo(imu, lo, mask, q4)
    assert all(np.array_equal(a, b) for a, b in zip(ref.get_head(), filt))
    i1, l1, m1 = _inputs(w, "host", True, torch.device("cuda:0"), k=1)
    ref.state_save(0)
    ref.predict(i1, q4)
    assert max(rel(a, b) for a, b in zip(pred1, ref.get_head())) <= TOL_PRED
    ref.state_restore(0)
    ref.step_legodo(i1, l1, m1, q4)
    assert all(np.array_equal(a, b) for a, b in zip(ref.get_head(), filt1))
    ref.close()


def test_pred_slot_errors(oracle):
    import torch
    from pronto_amd.batch import PbError
    from pronto_amd._lib import PB_CORR_POS_ORIENT
    PB_ERR_ARG, PB_ERR_STATE = 1, 4
    n, B = 15, 64
    w = Workload(B, n_states=n)
    imu, lo, mask = _inputs(w, "host", False, torch.device("cuda:0"))
    est, q4 = _fresh(oracle, w, n, B)
    L, h = est._L, est._h
    assert L.pb_set_pred_slot(h, 4) == PB_ERR_ARG          # out of range
    assert L.pb_set_pred_slot(h, -2) == PB_ERR_ARG
    assert L.pb_set_output_slot(h, 1) == 0
    assert L.pb_set_pred_slot(h, 1) == PB_ERR_ARG          # the pending output slot
    est.step_legodo(imu, lo, mask, q4)                    # (head now in slot 1)
    assert L.pb_set_pred_slot(h, 1) == PB_ERR_ARG          # the head's slot
    assert L.pb_set_pred_slot(h, 0) == 0 and L.pb_set_pred_slot(h, -1) == 0   # -1 cancels
    before = est.state_checksum(0)
    est.step_legodo(imu, lo, mask, q4)
    assert est.state_checksum(0) == before
    # entry points that do not write a predicted slot refuse and forget it
    for call in (lambda: est.predict(imu, q4),
                 lambda: est.update_indexed([3, 4, 5], np.ascontiguousarray(lo[0:3]), np.ascontiguousarray(lo[3:6])),
                 lambda: est.update_indexed([9, 10, 11, 6, 7, 8], np.zeros((6, B)), [1.0] * 6, quat_meas=np.tile([[1.0], [0], [0], [0]], (1, B)))):
        assert L.pb_set_pred_slot(h, 2) == 0
        with pytest.raises(PbError) as e:
            call()
        assert e.value.code == PB_ERR_STATE
        call()                                           # cleared: the same call now goes through
    # the leg pair entry points refuse before anything else (also before their own pb_legodo_init check)
    import ctypes as C
    q = (C.c_double * 4)(*q4)
    assert L.pb_set_pred_slot(h, 2) == 0
    assert L.pb_step_legodo_joints(h, C.c_void_p(imu.ctypes.data), 0, q, 0, 0, None, None, None, 0, 1.0, 1.0, None, None) == PB_ERR_STATE
    assert "no predicted slot" in L.pb_last_error(h).decode()
    assert L.pb_set_pred_slot(h, 2) == 0
    assert L.pb_step_legodo_feet(h, C.c_void_p(imu.ctypes.data), 0, q, 0, None, None, 0, 1.0, 1.0, None, None) == PB_ERR_STATE
    assert "no predicted slot" in L.pb_last_error(h).decode()
    # cleared: the same call now fails on its own account (no pb_legodo_init here)
    assert L.pb_step_legodo_feet(h, C.c_void_p(imu.ctypes.data), 0, q, 0, None, None, 0, 1.0, 1.0, None, None) == PB_ERR_STATE
    assert "pb_legodo_init" in L.pb_last_error(h).decode()
    assert L.pb_set_pred_slot(h, 2) == 0
    with pytest.raises(PbError) as e:
        est.step_legodo_correct(imu, lo, mask, q4, PB_CORR_POS_ORIENT, np.zeros((6, B)), [1.0] * 6, np.tile([[1.0], [0], [0], [0]], (1, B)))
    assert e.value.code == PB_ERR_STATE
    # pb_set_output_slot after pb_set_pred_slot naming the same slot: the step refuses, and consumes the setting
    assert L.pb_set_pred_slot(h, 3) == 0 and L.pb_set_output_slot(h, 3) == 0
    with pytest.raises(PbError) as e:
        est.step_legodo(imu, lo, mask, q4)
    assert e.value.code == PB_ERR_ARG
    L.pb_set_output_slot(h, -1)
    before = est.state_checksum(3)
    est.step_legodo(imu, lo, mask, q4)
    assert est.state_checksum(3) == before
    est.close()


@pytest.mark.parametrize("n", [15, 21])
def test_pred_slot_is_forgotten_by_the_whole_log_smoother(oracle, n):
    """pb_smooth_log (the process step and the update as two launches) runs a whole log of steps of its own: a predicted slot that is
    pending at its entry is forgotten there, as pb_smooth_log_fused forgets it, and the next pb_step_legodo writes no slot."""
    import torch
    dev = torch.device("cuda:0")
    B, T, K = 64, 6, 3
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    est, q4 = _fresh(oracle, w, n, B, slots=0)
    need = est.smooth_log_slots(T, K)
    est.history_reserve(need + 1)
    s = need                                             # a slot the smoother does not use
    before = est.state_checksum(s)
    est.set_pred_slot(s)
    est.smooth_log(*(torch.from_numpy(a).to(dev) for a in (imu, lo, mask)), q4, 1e-3, K, first_slot=0)
    assert est.state_checksum(s) == before
    est.step_legodo(imu[0], lo[0], mask[0], q4)
    assert est.state_checksum(s) == before
    est.close()


def test_pred_slot_beyond_the_two_wave_batch_limit(oracle):
    """Above 393 216 15-state filters the step runs one lane per filter (k_step<15>), which has no predicted-slot variant: the predict
    into the slot and the fused step as two launches -- the same contract."""
    n, B = 15, 393216 + 64 * 3
    w = Workload(B, n_states=n)
    imu, lo, mask = _inputs(w, "host", True, None)
    est, q4 = _fresh(oracle, w, n, B, slots=2)
    est.set_pred_slot(0)
    est.step_legodo(imu, lo, mask, q4)
    pred, head_sum = est.get_slot(0, count=4096), est.state_checksum()
    est.close()
    ref, _ = _fresh(oracle, w, n, B, slots=1)
    ref.step_legodo(imu, lo, mask, q4)
    assert ref.state_checksum() == head_sum
    ref.close()
    ref, _ = _fresh(oracle, w, n, B, slots=1)
    ref.predict(imu, q4)
    assert all(np.array_equal(a, b) for a, b in zip(pred, ref.get_head(count=4096)))
    ref.close()
