"""pb_smooth_log_corrected: whole-log RTS smoothing for logs with a sparse stream of corrections (VO position_orient, scan-match
position_yaw) behind some of the IMU + leg-odometry pairs, and what it stands on: pb_set_pred_slot in front of
pb_step_legodo_correct -- the corrected step also keeps its INS posterior (what EKFSmoothBackwardsPass reads at every INS update,
mav_state_est.cpp:98-189; "cur" is the posterior of the LAST measurement behind it).  Runs on the MI355X."""
import numpy as np
import pytest

from smoother_ref import oracle_smooth_step, start_of
from util import embed21, pad_z, rel

from pronto_amd.synth import Workload

TOL = 1e-9          # against the oracle (TOL of tests/test_smooth_log_fused.py)
TOL_PRED21 = 1e-15  # the 21-state predicted slot against pb_predict from the same head (15 states: bit for bit)
TOL_FUSED = 1e-12   # fused against un-fused: the header's bound for pb_step_legodo_correct
IDX = {0: [9, 10, 11, 6, 7, 8], 1: [9, 10, 11, 8]}
PB_ERR_ARG, PB_ERR_STATE = 1, 4

pytestmark = pytest.mark.gpu


def _est(oracle, w, n, B, slots):
    from pronto_amd.batch import BatchEstimator
    est = BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    vec, quat, P0, q4 = start_of(w)
    est.reset(vec, quat, P0)
    est.history_reserve(slots)
    return est, q4


def _corr_block(w, kind, k, B):
    """(z [m,B], R diagonal [m,B], quat [4,B], mask2 [B] with some zeros) of step k: the Workload helpers of the config-3 / config-5
    parity cases"""
    z, qm, Rd = w.vo_block(k) if kind == 0 else w.scanmatch_block(k)
    mask2 = ((np.arange(B) + k) % 7 != 0).astype(np.uint8)
    return pad_z(z, len(IDX[kind])), np.ascontiguousarray(Rd), np.ascontiguousarray(qm), mask2


def _corr_stream(w, kind, ticks, B):
    blocks = [_corr_block(w, kind, k, B) for k in ticks]
    return [np.ascontiguousarray(np.stack([b[i] for b in blocks])) for i in range(4)]


def _corrected_log(est, dev, streams, q4, dt, K, kind, ticks, corr, fused, first_slot=1):
    import torch
    got, order = {}, []

    def sink(step, slot):
        order.append(step)
        got[step] = est.get_slot(slot)
    up = lambda a: torch.from_numpy(a).to(dev)
    z2, R2, qm2, mask2 = corr
    est.smooth_log_corrected(*(up(a) for a in streams), q4, dt, K, kind, ticks, up(z2), up(R2), up(qm2), up(mask2), fused=fused,
                             first_slot=first_slot, sink=sink)
    return got, order


@pytest.mark.parametrize("B", [37, 101])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [15, 21])
def test_corrected_step_keeps_its_prediction(oracle, n, kind, B):
    w = Workload(B, n_states=n)
    imu = w.imu_block(0)
    lo, mask = w.legodo_block(0)
    zz, Rd, qm, mask2 = _corr_block(w, kind, 0, B)
    assert 0 < int(mask2.sum()) < B
    p, f = 1, 3
    est, q4 = _est(oracle, w, n, B, 4)
    est.set_pred_slot(p)
    est.set_output_slot(f)
    est.step_legodo_correct(imu, lo, mask, q4, kind, zz, Rd, qm, mask2)   # (the parent commit: PB_ERR_STATE)
    assert est._L.pb_head_slot(est._h) == f
    pred = est.get_slot(p)
    filt_sum, pred_sum = est.state_checksum(f), est.state_checksum(p)
    assert est.state_checksum() == filt_sum
    # one-shot: the next corrected step writes slot p no more
    lo1, mask1 = w.legodo_block(1)
    est.set_output_slot(2)
    est.step_legodo_correct(w.imu_block(1), lo1, mask1, q4, kind, *_corr_block(w, kind, 1, B))
    assert est.state_checksum(p) == pred_sum and est.state_checksum(f) == filt_sum
    est.close()
    # (a) pb_predict alone from the same head
    ref, _ = _est(oracle, w, n, B, 4)
    ref.predict(imu, q4)
    want = ref.get_head()
    ref.close()
    worst = max(rel(a, b) for a, b in zip(pred, want))
    print("n=%d kind=%d B=%d: predicted slot vs pb_predict %.1e" % (n, kind, B, worst))
    if n == 15:
        assert all(np.array_equal(a, b) for a, b in zip(pred, want))
    else:
        assert worst <= TOL_PRED21, worst
    # (b) the same call without a predicted slot
    ref, _ = _est(oracle, w, n, B, 4)
    ref.set_output_slot(f)
    ref.step_legodo_correct(imu, lo, mask, q4, kind, zz, Rd, qm, mask2)
    assert ref.state_checksum(f) == filt_sum
    ref.close()


TICKS = [0, 6, 7, 20, 34, 48, 49]   # the first step, both sides of a stretch boundary (stride 7), an ordinary one, the newest two


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [15, 21])
def test_corrected_smoothing_equals_the_all_checkpoints_pass_bit_for_bit(oracle, n, kind, fused):
    import torch
    B, T, K, dt = 37, 50, 7, 1e-3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    corr = _corr_stream(w, kind, TICKS, B)
    ref, q4 = _est(oracle, w, n, B, 2 * T + 2)
    for k in range(T):
        c = [a[TICKS.index(k)] for a in corr] if k in TICKS else None
        if fused:
            ref.set_pred_slot(2 * k)
            ref.set_output_slot(2 * k + 1)
            if c:
                ref.step_legodo_correct(imu[k], lo[k], mask[k], q4, kind, *c)
            else:
                ref.step_legodo(imu[k], lo[k], mask[k], q4)
        else:
            ref.set_output_slot(2 * k)
            ref.predict(imu[k], q4)
            ref.set_output_slot(2 * k + 1)
            ref.update_indexed([3, 4, 5], np.ascontiguousarray(lo[k][0:3]), np.ascontiguousarray(lo[k][3:6]), mask=mask[k])
            if c:
                ref.set_output_slot(2 * k + 1)
                ref.update_indexed(IDX[kind], c[0], c[1], mask=c[3], quat_meas=c[2])
    final = ref.get_slot(2 * (T - 1) + 1)
    want, nxt = {}, 2 * (T - 1) + 1
    for k in range(T - 2, -1, -1):
        out = 2 * T + (k % 2)
        ref.smooth_step(2 * (k + 1), nxt, 2 * k + 1, out, dt)
        want[k] = ref.get_slot(out)
        nxt = out
    ref.close()
    est, _ = _est(oracle, w, n, B, 0)
    est.history_reserve(est.smooth_log_slots(T, K) + 1)
    got, order = _corrected_log(est, dev, (imu, lo, mask), q4, dt, K, kind, TICKS, corr, fused)
    assert order == list(range(T - 2, -1, -1))
    for k in range(T - 1):
        for a, b in zip(got[k], want[k]):
            assert np.array_equal(a, b), k
    assert est._L.pb_head_slot(est._h) == -1
    for a, b in zip(est.get_head(), final):     # the newest step is not smoothed, but its tick is filtered
        assert np.array_equal(a, b)
    est.close()


_ORACLE = {}


def _oracle_smoothed(oracle, n, kind, T, B, dt, ticks):
    """The oracle's forward pass (pred after the predict, filtered after the LAST update of the step) and its backward recursion, once
    per (n, T): the stride does not enter."""
    key = (n, kind, T, B)
    if key not in _ORACLE:
        w = Workload(B, n_states=n)
        vec, quat, P0, q4 = start_of(w)
        v21, P21 = embed21(vec, P0)
        ob = oracle.OracleBatch(v21, quat, P21)
        hist = []
        for k in range(T):
            lo, mask = w.legodo_block(k)
            ob.predict(w.imu_block(k), q4)
            pred = (ob.vec.copy(), ob.quat.copy(), ob.cov.copy())
            ob.update_indexed([3, 4, 5], lo[0:3], lo[3:6], mask=mask)
            if k in ticks:
                zz, Rd, qm, mask2 = _corr_block(w, kind, k, B)
                ob.update_indexed(IDX[kind], zz, Rd, quat_meas=qm, mask=mask2)
            hist.append((pred, (ob.vec.copy(), ob.quat.copy(), ob.cov.copy())))
        sm, nxt = {}, hist[T - 1][1]
        for k in range(T - 2, -1, -1):
            nxt = oracle_smooth_step(oracle, hist[k + 1][0], nxt, hist[k][1], dt)
            sm[k] = nxt
        for v in sm.values():
            for a in v:
                a.setflags(write=False)
        _ORACLE[key] = sm
    return _ORACLE[key]


@pytest.mark.parametrize("T,K", [(23, 1), (23, 4), (31, 5), (16, 16)])
@pytest.mark.parametrize("n", [15, 21])
def test_corrected_smoothing_matches_the_oracle(oracle, n, T, K):
    """Config 3 (15 states, position_orient) and config 5 (21 states, position_yaw), a tick on every 5th step; fused and un-fused
    against the oracle and against each other; ragged last stretches."""
    import torch
    B, dt = 29, 1e-3
    kind = 0 if n == 15 else 1
    dev = torch.device("cuda:0")
    ticks = list(range(0, T, 5))
    w = Workload(B, n_states=n)
    streams = w.streams(0, T)
    corr = _corr_stream(w, kind, ticks, B)
    got = {}
    for fused in (0, 1):
        est, q4 = _est(oracle, w, n, B, 0)
        est.history_reserve(est.smooth_log_slots(T, K))
        got[fused], _ = _corrected_log(est, dev, streams, q4, dt, K, kind, ticks, corr, fused, first_slot=0)
        est.close()
    want = _oracle_smoothed(oracle, n, kind, T, B, dt, ticks)
    for fused in (0, 1):
        worst = 0.0
        for k in range(T - 1):
            v, q, P, _ = got[fused][k]
            worst = max(worst, rel(v, want[k][0][:n]), rel(q, want[k][1]), rel(P, want[k][2][:n, :n]))
        print("n=%d T=%d K=%d fused=%d: against the oracle %.1e" % (n, T, K, fused, worst))
        assert worst < TOL, (fused, worst)
    both = max(rel(a, b) for k in range(T - 1) for a, b in zip(got[1][k][:3], got[0][k][:3]))
    print("n=%d T=%d K=%d: fused against un-fused %.1e" % (n, T, K, both))
    assert both <= TOL_FUSED, both


@pytest.mark.parametrize("n", [15, 21])
def test_no_ticks_is_the_plain_smoother(oracle, n):
    import torch
    B, T, K, dt = 37, 20, 4, 1e-3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    streams = [torch.from_numpy(a).to(dev) for a in w.streams(0, T)]
    for fused in (False, True):
        est, q4 = _est(oracle, w, n, B, 0)
        est.history_reserve(est.smooth_log_slots(T, K))
        want = {}
        est.smooth_log(*streams, q4, dt, K, sink=lambda step, slot: want.__setitem__(step, est.state_checksum(slot)), fused=fused)
        want["head"] = est.state_checksum()
        est.close()
        empty = torch.zeros((0, 6, B), dtype=torch.float64, device=dev)
        for steps in (None, []):   # corr = NULL; a stream with n_ticks = 0
            est, q4 = _est(oracle, w, n, B, 0)
            est.history_reserve(est.smooth_log_slots(T, K))
            got = {}
            est.smooth_log_corrected(*streams, q4, dt, K, 0, steps, empty, [1.0] * 6, empty[:, :4], fused=fused,
                                     sink=lambda step, slot: got.__setitem__(step, est.state_checksum(slot)))
            got["head"] = est.state_checksum()
            est.close()
            assert got == want and len(got) == T


def test_corrected_smoothing_errors_leave_the_head_usable(oracle):
    import torch
    from pronto_amd.batch import PbError
    n, B, T, K, dt = 15, 37, 12, 3, 1e-3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    streams = [torch.from_numpy(a).to(dev) for a in (imu, lo, mask)]
    up = lambda a: torch.from_numpy(a).to(dev)
    z2, R2, qm2, mask2 = (up(a) for a in _corr_stream(w, 0, [2, 5], B))
    est, q4 = _est(oracle, w, n, B, 0)
    need = est.smooth_log_slots(T, K)
    est.history_reserve(need + 1)
    spare = need
    cases = [(0, [5, 2], PB_ERR_ARG, 0, z2),         # a decreasing step list
             (0, [5, 5], PB_ERR_ARG, 0, z2),         # ... and one that does not increase
             (0, [2, T], PB_ERR_ARG, 0, z2),         # a step equal to n_steps
             (0, [-1, 5], PB_ERR_ARG, 0, z2),        # ... and one in front of the log
             (7, [2, 5], PB_ERR_ARG, 0, z2),         # an unknown kind
             (0, [2, 5], PB_ERR_ARG, 0, None),       # ticks without their measurement blocks
             (0, [2, 5], PB_ERR_STATE, 2, z2)]       # too few slots
    for fused in (0, 1):
        for kind, steps, code, first_slot, z2 in cases:
            est.set_output_slot(0)
            est.step_legodo(imu[0], lo[0], mask[0], q4)   # the head lives in slot 0, and a predicted slot is pending
            head = est.state_checksum()
            est.set_pred_slot(spare)
            with pytest.raises(PbError) as e:
                est.smooth_log_corrected(*streams, q4, dt, K, kind, steps, z2, R2, qm2, mask2, fused=fused, first_slot=first_slot)
            assert e.value.code == code, (kind, steps, e.value)
            assert est._L.pb_head_slot(est._h) == -1      # back in the context's own array, unchanged
            assert est.state_checksum() == head
            before = est.state_checksum(spare)
            est.step_legodo(imu[1], lo[1], mask[1], q4)   # usable, and no slot left pending
            assert est._L.pb_head_slot(est._h) == -1 and est.state_checksum(spare) == before
    est.close()
