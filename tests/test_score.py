"""GPU tier of the ground-truth scorer (pb_score_*, k_score_gt / k_score_best) against the numpy restatement of
drift_per_distance.py (tests/score_ref.py) and against the g++ build of the same per-lane functions (tests/score_host.cpp),
under the CPU tier's conditions (score_common.compare): discrete outcomes identical, lengths and angles to 1e-12, percent_ddt
to 1e-9 relative over windows with dist >= 0.1 m."""
import ctypes as C

import numpy as np
import pytest

import score_common as sc
from pronto_amd._lib import PB_DEVICE, PB_ERR_ARG, PB_ERR_STATE, PB_HOST, PB_HOST_BROADCAST, PB_SLOT_HEAD

pytestmark = pytest.mark.gpu

DRIFT, ABS = sc.R("DRIFT"), sc.R("ABS")


@pytest.fixture(scope="module")
def hostlib():
    return sc.build_host()


def make(B, n, reset=True, slots=0):
    from pronto_amd.batch import BatchEstimator
    est = BatchEstimator(B, n_states=n, device=0)
    if slots:
        est.history_reserve(slots)
    if reset:
        vec, quat = np.zeros((n, B)), np.zeros((4, B))
        quat[0] = 1.0
        est.reset(vec, quat, cov_of(n, B))
    return est


def cov_of(n, B):
    P = np.zeros((n, n, B))
    for i in range(n):
        P[i, i] = 0.01 * (i + 1)
    return P


def set_head(est, est7, P):
    """a scripted head: position rows 9..11 and the quaternion from est7, everything else a fixed pattern (no filtering)"""
    vec = np.tile(np.arange(est.n, dtype=np.float64)[:, None] * 0.01, (1, est.B))
    vec[9:12] = est7[:3]
    quat = np.ascontiguousarray(est7[3:])
    rc = est._L.pb_set_head(est._h, vec.ctypes.data, quat.ctypes.data, P.ctypes.data, None, PB_HOST)
    assert rc == 0, est._L.pb_last_error(est._h)


CASES = [  # n, B, mem, valid, per-filter times, distance threshold
    (15, 1, PB_HOST, False, False, 0.0),
    (21, 64, PB_DEVICE, True, True, 0.25),
    (15, 65, PB_HOST, True, True, 0.25),
    (21, 200, PB_DEVICE, False, False, 0.0),
    (15, 200, PB_HOST_BROADCAST, True, True, 0.0),
    (21, 65, PB_HOST_BROADCAST, False, False, 0.25),
]


@pytest.mark.parametrize("n,B,mem,use_valid,times,dthr", CASES)
def test_scorer_alone_against_script_and_host_build(hostlib, n, B, mem, use_valid, times, dthr):
    import torch
    dev = torch.device("cuda:0")
    msgs = sc.scenario(B, 120, seed=5 + B)
    if mem == PB_HOST_BROADCAST:  # one robot's truth for the whole batch: filter 0's
        msgs = [(u, ut, np.ascontiguousarray(np.repeat(p7[:, :1], B, axis=1)), v, e7) for u, ut, p7, v, e7 in msgs]
    ref, ref_closed = sc.run_ref(msgs, B, 10.0, dthr, per_filter_times=times, use_valid=use_valid)
    sc.check_witness(ref)
    host = sc.HostScore(hostlib, B, 10.0, dthr)
    est = make(B, n)
    est.score_init(10.0, dthr)
    P = cov_of(n, B)
    n_before = np.zeros(B, dtype=np.int64)
    for k, (u, ut, p7, v, e7) in enumerate(msgs):
        set_head(est, e7, P)
        a_ut, a_v = (ut if times else None), (v if use_valid else None)
        if mem == PB_DEVICE:
            to = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            est.score_ground_truth(u, to(p7), to(a_v), to(a_ut), absolute=True)
        elif mem == PB_HOST:
            est.score_ground_truth(u, p7, a_v, a_ut, absolute=True)
        else:
            est.score_ground_truth(u, np.ascontiguousarray(p7[:, 0]), a_v, a_ut, absolute=True)
        h_closed = host.message(u, a_ut, p7, a_v, e7, DRIFT | ABS)
        _, counts = est.score_get()  # which messages closed a window: the device's counts behind every message
        np.testing.assert_array_equal(counts[sc.R("N_WINDOWS")] - n_before, ref_closed[k], err_msg="message %d" % k)
        np.testing.assert_array_equal(counts, host.counts, err_msg="message %d" % k)
        np.testing.assert_array_equal(h_closed, ref_closed[k])
        n_before = counts[sc.R("N_WINDOWS")]
    rows, counts = est.score_get()
    print("GPU vs script, worst abs / rel:", sc.compare(ref, rows, counts, "gpu"))
    sc.compare(ref, host.rows, host.counts, "host")
    np.testing.assert_array_equal(counts, host.counts)
    assert int(counts[sc.R("N_WINDOWS")].min()) >= 9
    # pb_score_last = the LAST_* rows and the window's utime
    for b in sorted({0, B - 1, min(sc.STILL, B - 1), min(sc.YAW_CROSS, B - 1)}):
        last = est.score_last(b)
        assert last["utime"] == counts[sc.R("LAST_UTIME"), b]
        got = np.concatenate([last["pos_error"], [last["pos_error_norm"]], last["rpy_error"], [last["distance_travelled"], last["percent_ddt"], last["time_elapsed"]]])
        np.testing.assert_array_equal(got, rows[sc.R("LAST_POS_ERROR"):sc.R("LAST_POS_ERROR") + 10, b])
    # a sub-range read
    if B > 3:
        r2, c2 = est.score_get(1, B - 3)
        np.testing.assert_array_equal(r2, rows[:, 1:B - 2])
        np.testing.assert_array_equal(c2, counts[:, 1:B - 2])
    est.close()


@pytest.mark.parametrize("n", [15, 21])
def test_head_in_a_checkpoint_slot_and_explicit_slot(n):
    from pronto_amd.synth import Workload
    B = 130
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    q4 = w.process_noise()
    msgs = sc.scenario(B, 4, seed=9)
    a = make(B, n, reset=False, slots=3)
    a.reset(vec, quat, P0)
    a.set_output_slot(1)
    a.predict(w.imu_block(0), q4)               # the head now lives in checkpoint slot 1
    assert a._L.pb_head_slot(a._h) == 1
    gv, gq, gP, gll = a.get_head()
    b = make(B, n)                              # the same posterior as a head in the context's own array
    assert b._L.pb_set_head(b._h, gv.ctypes.data, gq.ctypes.data, np.ascontiguousarray(gP).ctypes.data, gll.ctypes.data, PB_HOST) == 0
    assert b._L.pb_head_slot(b._h) == -1
    for e in (a, b):
        e.score_init(0.5, 0.0)
    cs_head, cs_slot = a.state_checksum(-1), a.state_checksum(1)
    a.set_pred_slot(0)
    a.set_output_slot(2)                        # pending while the scorer runs
    for u, ut, p7, v, e7 in msgs:
        a.score_ground_truth(u, p7, v, ut, absolute=True)
        b.score_ground_truth(u, p7, v, ut, absolute=True)
    ra, ca = a.score_get()
    rb, cb = b.score_get()
    np.testing.assert_array_equal(ra, rb)
    np.testing.assert_array_equal(ca, cb)
    assert ca[sc.R("N_WINDOWS")].max() >= 2 and ca[sc.R("ABS_N")].max() == 4
    anchored = ca[sc.R("ANCHOR_UTIME")] >= 0
    np.testing.assert_array_equal(ra[sc.R("ANCHOR_EST"):sc.R("ANCHOR_EST") + 3, anchored], gv[9:12, anchored])
    assert a.state_checksum(-1) == cs_head and a.state_checksum(1) == cs_slot and a._L.pb_head_slot(a._h) == 1
    # the pending slots were neither consumed nor disturbed: the next fused step writes its prediction to 0 and its posterior to 2
    cs0 = a.state_checksum(0)
    lo, mask = w.legodo_block(1)
    a.step_legodo(w.imu_block(1), lo, mask, q4)
    assert a._L.pb_head_slot(a._h) == 2 and a.state_checksum(0) != cs0
    assert a.state_checksum(1) == cs_slot
    # an explicit slot: the head has moved on, slot 1 still holds the first posterior
    a.score_init(0.5, 0.0)
    for u, ut, p7, v, e7 in msgs:
        a.score_ground_truth(u, p7, v, ut, slot=1, absolute=True)
    ra, ca = a.score_get()
    np.testing.assert_array_equal(ra, rb)
    np.testing.assert_array_equal(ca, cb)
    assert a.state_checksum(1) == cs_slot and a._L.pb_head_slot(a._h) == 2
    a.close()
    b.close()


@pytest.mark.parametrize("n", [15, 21])
def test_through_a_filter(hostlib, n):
    """200 filters, 300 fused steps on the synthetic streams, ground truth every 10th step (10 ms): the scorer reads the head the
    filter just wrote; the witnesses get the same head through pb_get_head.  time_threshold_s = 0.035 closes a window every
    4 messages."""
    from pronto_amd.synth import Workload
    B, T = 200, 300
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    q4 = w.process_noise()
    est = make(B, n, reset=False)
    est.reset(vec, quat, P0)
    est.score_init(0.035, 0.0)
    truth = sc.scenario(B, T // 10, seed=21, spacing_us=10_000)
    ref = sc.sr.ScoreRef(B, 0.035, 0.0)
    host = sc.HostScore(hostlib, B, 0.035, 0.0)
    for k in range(T):
        lo, mask = w.legodo_block(k)
        est.step_legodo(w.imu_block(k), lo, mask, q4)
        if k % 10 == 9:
            u, ut, p7, v, _ = truth[k // 10]
            est.score_ground_truth(u, p7, v, ut, absolute=True)
            gv, gq, _, _ = est.get_head(want_cov=False)
            e7 = np.ascontiguousarray(np.concatenate([gv[9:12], gq]))
            r_closed = ref.message(ut, p7[:3], p7[3:], e7[:3], e7[3:], v, True, True)
            np.testing.assert_array_equal(host.message(u, ut, p7, v, e7, DRIFT | ABS), r_closed)
    sc.check_witness(ref)
    rows, counts = est.score_get()
    print("GPU vs script, worst abs / rel:", sc.compare(ref, rows, counts, "gpu"))
    sc.compare(ref, host.rows, host.counts, "host")
    np.testing.assert_array_equal(counts, host.counts)
    assert int(counts[sc.R("N_WINDOWS")].min()) >= 5
    est.close()


def derived_metric(rows, counts, metric):
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == sc.R("MEAN_PDDT"):
            n, v = counts[sc.R("N_DDT")], rows[sc.R("SUM_PDDT")] / counts[sc.R("N_DDT")]
        elif metric == sc.R("RMS_DRIFT"):
            n, v = counts[sc.R("N_WINDOWS")], np.sqrt(rows[sc.R("SUM_ERR_SQ")] / counts[sc.R("N_WINDOWS")])
        else:
            n, v = counts[sc.R("ABS_N")], np.sqrt(rows[sc.R("ABS_SUM_SQ")] / counts[sc.R("ABS_N")])
    return np.where(n > 0, v, np.inf), n > 0


# 257: one filter more than a first-stage workgroup of k_score_best covers (SCORE_BEST_PER_WG = 256)
@pytest.mark.parametrize("B", [1, 64, 200, 257])
def test_best(B):
    n = 15
    est = make(B, n)
    est.score_init(2.5, 0.0)
    for m in (sc.R("MEAN_PDDT"), sc.R("RMS_DRIFT"), sc.R("ATE_RMSE")):
        assert est.score_best(m) == (-1, 0.0)                      # no filter has data
    msgs = sc.scenario(B, 10, seed=31)
    lo_, hi_ = (B // 3, B - 2) if B >= 64 else (0, 0)               # the planted tie: two filters with the same truth and estimate,
    valid = np.ones(B, dtype=np.uint8)
    if B >= 64:
        valid[[1, B - 1]] = 0                                       # two filters never get a message
    P = cov_of(n, B)
    for u, ut, p7, v, e7 in msgs:
        if B >= 64:                                                 # ... and the smallest errors of the batch
            e7[:, lo_] = p7[:, lo_] + 1e-7 * np.array([1, -2, 0.5, 0, 0, 0, 0]) * (u // 1_000_000)
            p7[:, hi_], e7[:, hi_] = p7[:, lo_], e7[:, lo_]
        set_head(est, e7, P)
        est.score_ground_truth(u, p7, valid, None, absolute=True)
    rows, counts = est.score_get()
    for m in (sc.R("MEAN_PDDT"), sc.R("RMS_DRIFT"), sc.R("ATE_RMSE")):
        v, has = derived_metric(rows, counts, m)
        f, val = est.score_best(m)
        if B >= 64:
            assert not has[1] and not has[B - 1] and has[lo_]
            assert v[lo_] == v[hi_] == v.min(), "the planted tie is the minimum"
            assert f == lo_
        else:
            assert has.all()
        assert f == int(np.argmin(v))                               # numpy's argmin also takes the first of equals
        # the same quotient and square root on the device: each within 1 ulp there and half an ulp here, so < 4 ulp = 1e-15 in all
        assert abs(val - v[f]) <= 1e-15 * abs(v[f])
    est.close()


def test_argument_and_state_errors():
    from pronto_amd.batch import PbError
    B = 8
    pose = np.zeros((7, B)); pose[3] = 1.0

    def code(fn, *a, **k):
        with pytest.raises(PbError) as e:
            fn(*a, **k)
        return e.value.code

    est = make(B, 15, reset=False)
    est.score_init()
    assert code(est.score_ground_truth, 0, pose) == PB_ERR_STATE              # before pb_reset
    est.close()
    est = make(B, 15, slots=2)
    assert code(est.score_ground_truth, 0, pose) == PB_ERR_STATE              # before pb_score_init
    assert code(est.score_get) == PB_ERR_STATE
    assert code(est.score_last, 0) == PB_ERR_STATE
    assert code(est.score_best) == PB_ERR_STATE
    L, h = est._L, est._h
    assert L.pb_score_init(h, -1.0, 0.0) == PB_ERR_ARG and L.pb_score_init(h, 10.0, -0.5) == PB_ERR_ARG
    assert L.pb_score_init(h, float("nan"), 0.0) == PB_ERR_ARG
    est.score_init()
    assert code(est.score_ground_truth, 0, pose, slot=2) == PB_ERR_STATE      # slot out of range
    assert code(est.score_ground_truth, 0, pose, slot=-2) == PB_ERR_STATE
    p = pose.ctypes.data
    assert L.pb_score_ground_truth(h, 0, None, None, None, PB_SLOT_HEAD, DRIFT, PB_HOST) == PB_ERR_ARG       # NULL pose
    assert L.pb_score_ground_truth(h, 0, None, p, None, PB_SLOT_HEAD, 0, PB_HOST) == PB_ERR_ARG             # no flags
    assert L.pb_score_ground_truth(h, 0, None, p, None, PB_SLOT_HEAD, 4, PB_HOST) == PB_ERR_ARG             # unknown flags
    assert L.pb_score_ground_truth(h, 0, None, p, None, PB_SLOT_HEAD, DRIFT, 7) == PB_ERR_ARG               # unknown mem
    f, v = C.c_int(), C.c_double()
    assert L.pb_score_best(h, 9, C.byref(f), C.byref(v)) == PB_ERR_ARG                                      # unknown metric
    assert L.pb_score_best(h, 0, None, C.byref(v)) == PB_ERR_ARG
    assert L.pb_score_get(h, 0, B + 1, None, None, PB_HOST) == PB_ERR_ARG
    assert L.pb_score_get(h, 0, B, None, None, PB_HOST_BROADCAST) == PB_ERR_ARG
    ut, out = C.c_int64(), (C.c_double * 10)()
    assert L.pb_score_last(h, B, C.byref(ut), out) == PB_ERR_ARG
    assert L.pb_score_ground_truth(h, 0, None, p, None, 1, DRIFT | ABS, PB_HOST) == 0                       # a valid slot works
    est.score_init(10.0, 0.25)                                                                             # again = reset
    _, counts = est.score_get()
    assert np.all(counts[sc.R("ANCHOR_UTIME")] == -2) and np.all(counts[sc.R("ABS_N")] == 0)
    est.close()
