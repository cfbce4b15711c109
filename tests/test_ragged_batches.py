"""Ragged batches -- independent log segments as one batch: filter i follows recording i, so a batched message may leave some filters
without an IMU sample or a joint state, and every filter has its own time stamp and its own number of new KVH packets.  The four
device pieces this rests on, each against "the reference did nothing" for the filters without a message and against the oracle run
on the others alone:
  pb_imu_notch_counts (k_notch_counts), pb_ins_body_block / _reset (k_ins_body), pb_set_imu_valid (k_imu_idle_prepare in front of
  every step launcher of pb_step.hip) and pb_legodo_set_message_times (the odometry wave of the pair kernels).
A filter without a message is compared BIT FOR BIT with its own prior after every call; the filters with one are compared with the
oracle.  Runs on the MI355X."""
import ctypes as C

import numpy as np
import pytest

from noise_block import masked_oracle_step
from util import pad_z, rel, rel_elem

from pronto_amd.synth import Workload

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---------------------------------------------------------------- 1. notch cascade with per-filter packet counts ----
NOTCH_B = 130            # two full waves and a two-lane tail
NOTCH_MAXP = 11          # chunks of 4, 4 and 3: the short last chunk and its clamped prefetch both run
NOTCH_CALLS = 40
NOTCH_VALUES = (-1, 0, 1, 3, 4, 5, 8, 11, 12)   # none (twice), one, inside / exactly / just past a chunk, two chunks, all, too many
NOTCH_WATCHED = (0, 63, 64, 129)                # first / last lane of wave 0, first lane of wave 1, last lane of the tail
NOTCH_SEED = 1           # (chosen so that _notch_counts' assertions hold: see there)
NOTCH_WAVE_IDLE_CALL = 6
POISON = 1e30            # finite: a consumed surplus packet shows as 1e30 in the output, not as a NaN that a max() may swallow
SENTINEL = -4321.0625


def _notch_counts():
    """counts [calls, B] int32: every value of NOTCH_VALUES in each watched lane, one call with a whole wave at 0, and for every
    filter a consuming call behind an idle one (so that a filter state touched by an idle call shows in a later output)."""
    rng = np.random.default_rng(NOTCH_SEED)
    counts = rng.choice(NOTCH_VALUES, size=(NOTCH_CALLS, NOTCH_B)).astype(np.int32)
    counts[NOTCH_WAVE_IDLE_CALL, 64:128] = 0
    for lane in NOTCH_WATCHED:
        assert set(counts[:, lane].tolist()) == set(NOTCH_VALUES), lane
    eff = np.clip(counts, 0, NOTCH_MAXP)
    for b in range(NOTCH_B):
        idle = np.nonzero(eff[:, b] == 0)[0]
        assert len(idle) and np.any(eff[idle[0]:, b] > 0), b
    return counts, eff


def _notch_stream(T, B, seed):
    """the signal of test_notch.py's device test: gravity on z, unit noise, a unit 87 Hz line -- [T, 3, B]"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * 1e-3
    return 9.8 * (np.arange(3) == 2)[None, :, None] + rng.normal(size=(T, 3, B)) + np.sin(2 * np.pi * 87 * t)[:, None, None]


def test_notch_counts_every_filter_every_call(oracle):
    """pb_imu_notch_counts for 130 filters over 40 calls, each filter with its own count per call (including -1, 0, more than
    max_packets, and every mixture inside one wave), PB_HOST and PB_DEVICE alternating.  Reference: oracle.notch_cascade_run on
    exactly the packets the filter should have consumed (12 consumes 11; -1 and 0 none).  After EVERY call, for ALL filters: the
    returned sample within 1e-12 of the reference at the filter's newest consumed packet (the bound and the amplitudes of
    test_device_notch_matches_oracle); a filter without a new packet keeps its accel_out entries (PB_DEVICE) or gets 0 (PB_HOST).
    The packet rows beyond a filter's count hold 1e30."""
    import torch
    from pronto_amd.batch import BatchEstimator
    B, P = NOTCH_B, NOTCH_MAXP
    counts, eff = _notch_counts()
    total = eff.sum(axis=0)
    stream = _notch_stream(int(total.max()), B, seed=4)
    ref = [oracle.notch_cascade_run(np.ascontiguousarray(stream[:total[b], :, b]), 87.0) for b in range(B)]
    est = BatchEstimator(B, n_states=15)
    est.imu_notch_init(87.0, 1000.0)
    pos = np.zeros(B, dtype=np.int64)
    worst = 0.0
    for c in range(NOTCH_CALLS):
        pk = np.full((P, 3, B), POISON)
        for b in range(B):
            pk[:eff[c, b], :, b] = stream[pos[b]:pos[b] + eff[c, b], :, b]
        if c % 2:
            d_out = torch.full((3, B), SENTINEL, dtype=torch.float64, device="cuda:0")
            est.imu_notch_counts(_dev(counts[c]), _dev(pk), d_out)
            out, idle_value = d_out.cpu().numpy(), SENTINEL
        else:
            out, idle_value = np.full((3, B), SENTINEL), 0.0
            est.imu_notch_counts(np.ascontiguousarray(counts[c]), pk, out)
        pos += eff[c]
        got = eff[c] > 0
        assert np.all(out[:, ~got] == idle_value), (c, np.nonzero(np.any(out != idle_value, axis=0) & ~got)[0])
        want = np.stack([ref[b][pos[b] - 1] if got[b] else np.zeros(3) for b in range(B)], axis=1)
        err = np.max(np.abs(out[:, got] - want[:, got]), initial=0.0)
        worst = max(worst, err)
        assert err < 1e-12, (c, err, np.nonzero(np.any(np.abs(out - want) >= 1e-12, axis=0) & got)[0])
    print("notch counts: worst |sample - oracle| over %d calls x %d filters: %.2e" % (NOTCH_CALLS, B, worst))
    est.close()


def test_notch_counts_all_equal_is_pb_imu_notch():
    """pb_imu_notch(n) and pb_imu_notch_counts with every count = n (max_packets 11, 1e30 behind the n-th packet): bit-identical
    outputs, n = 1, 4, 5, 11 in turn, filter state carried across the calls, host and device buffers alternating."""
    import torch
    from pronto_amd.batch import BatchEstimator
    B, P = NOTCH_B, NOTCH_MAXP
    seq = (1, 4, 5, 11) * 3
    stream = _notch_stream(sum(seq), B, seed=5)
    a, b = BatchEstimator(B, n_states=15), BatchEstimator(B, n_states=15)
    a.imu_notch_init(87.0, 1000.0)
    b.imu_notch_init(87.0, 1000.0)
    k = 0
    for call, n in enumerate(seq):
        pk = np.ascontiguousarray(stream[k:k + n])
        pk11 = np.full((P, 3, B), POISON)
        pk11[:n] = pk
        cnt = np.full(B, n, dtype=np.int32)
        if call % 2:
            oa, ob_ = (torch.zeros((3, B), dtype=torch.float64, device="cuda:0") for _ in range(2))
            a.imu_notch(_dev(pk), oa)
            b.imu_notch_counts(_dev(cnt), _dev(pk11), ob_)
            oa, ob_ = oa.cpu().numpy(), ob_.cpu().numpy()
        else:
            oa, ob_ = np.zeros((3, B)), np.zeros((3, B))
            a.imu_notch(pk, oa)
            b.imu_notch_counts(cnt, pk11, ob_)
        assert np.all(np.abs(oa) < 100.0) and oa.tobytes() == ob_.tobytes(), (call, n)
        k += n
    a.close()
    b.close()


# ---------------------------------------------------------------- 2. body-frame block ----
# ins_rotate is about twenty roundings per component on products bounded by |v|: 1e-14 ~ 45 eps leaves a factor two over that.
ROT_TOL = 1e-14          # relative to max |input| of the message; observed 1.4e-16 (Microstrain), 1.5e-16 (Atlas) on an MI355X
INS_B, INS_MSGS, INS_RESET_BEFORE = 130, 12, 8
INS_ROT = np.array([0.8, -0.3, 0.4, 0.2]) / np.linalg.norm([0.8, -0.3, 0.4, 0.2])
INS_TRANS = (0.03, -0.02, 0.5)


def _rot_ld(q):
    """the rotation matrix of the quaternion (w, x, y, z) in long double"""
    w, x, y, z = [np.longdouble(v) for v in q]
    one, two = np.longdouble(1), np.longdouble(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=np.longdouble)


def _ins_validity(rng):
    """about 30 % idle; filter 5 idle on its very first message, filter 7 for four messages in a row, lane 129 alternating"""
    v = (rng.random((INS_MSGS, INS_B)) > 0.3).astype(np.uint8)
    v[0, 5], v[1:3, 5] = 0, 1
    v[2, 7], v[3:7, 7], v[7, 7] = 1, 0, 1
    v[:, 129] = np.arange(INS_MSGS) % 2
    return v


@pytest.mark.parametrize("config", ["microstrain", "atlas", "atlas_scalar_utime"])
def test_ins_body_block(config):
    """pb_ins_body_block over 12 messages with a validity mask (message 2: valid = NULL) and a pb_ins_body_reset in the middle, the
    inputs from the host in one context and from the device in another.  Microstrain: no raw_dt, no translation, dt = dt_default.
    Atlas: gyro = delta_rotation / raw_dt[b], the translation, dt from per-filter utimes with +-40 us jitter (or from the call's scalar
    utime).  Reference in long double.  The six rotated entries within 1e-14 * max|input|; dt EXACTLY float64(ut - prev) * 1e-6
    (dt_default on a filter's first message and after the reset; across idle messages the whole gap); an idle filter's entry is bit
    for bit the six values it last produced with dt == 0.0 (zeros if it never had a message); valid_out == valid; host and device
    inputs give bit-identical blocks."""
    import torch
    from pronto_amd.batch import BatchEstimator
    B = INS_B
    atlas = config != "microstrain"
    rng = np.random.default_rng(21)
    valid = _ins_validity(rng)
    R = _rot_ld(INS_ROT)
    dt_default = 1.0 / 333.0
    trans = INS_TRANS if atlas else None
    eh, ed = BatchEstimator(B, n_states=15), BatchEstimator(B, n_states=15)
    last, prev = np.zeros((6, B)), np.zeros(B, dtype=np.int64)
    worst = 0.0
    for m in range(INS_MSGS):
        if m == INS_RESET_BEFORE:
            eh.ins_body_reset()
            ed.ins_body_reset()
            last[:], prev[:] = 0.0, 0
        accel = np.ascontiguousarray(9.8 * (np.arange(3) == 2)[:, None] + rng.normal(size=(3, B)))
        utime = 1_000_000 + 1000 * (m + 1)
        if atlas:
            gyro = np.ascontiguousarray(1e-3 * rng.normal(size=(3, B)))        # delta_rotation
            raw_dt = np.ascontiguousarray(1e-3 * (1.0 + 0.01 * rng.normal(size=B)))
            utimes = None if config == "atlas_scalar_utime" else (utime + rng.integers(-40, 41, size=B)).astype(np.int64)
        else:
            gyro, raw_dt, utimes = np.ascontiguousarray(rng.normal(size=(3, B))), None, None
        v = None if m == 2 else valid[m]
        on = np.ones(B, dtype=bool) if v is None else v.astype(bool)
        outs = []
        for est, up in ((eh, lambda a: a), (ed, lambda a: None if a is None else _dev(a))):
            blk = torch.full((7, B), SENTINEL, dtype=torch.float64, device="cuda:0")
            vout = torch.full((B,), 7, dtype=torch.uint8, device="cuda:0")
            est.ins_body_block(up(gyro), up(accel), INS_ROT, blk, raw_dt=up(raw_dt), utimes=up(utimes), utime=utime, valid=up(v),
                               trans_vec=trans, dt_default=dt_default, dt_from_utimes=atlas, valid_out=vout)
            outs.append((blk.cpu().numpy(), vout.cpu().numpy()))
        (blk, vout), (blk_d, vout_d) = outs
        assert blk.tobytes() == blk_d.tobytes() and vout.tobytes() == vout_d.tobytes(), m
        assert np.array_equal(vout, on.astype(np.uint8)), m
        # the filters with a message
        g = gyro.astype(np.longdouble) / raw_dt.astype(np.longdouble) if atlas else gyro.astype(np.longdouble)
        want = np.concatenate([R @ g, R @ accel.astype(np.longdouble) + (np.array(trans, dtype=np.longdouble)[:, None] if atlas else 0)])
        scale = float(max(np.max(np.abs(g[:, on])), np.max(np.abs(accel[:, on])), max(abs(t) for t in (trans or (0.0,)))))
        err = float(np.max(np.abs(blk[0:6][:, on].astype(np.longdouble) - want[:, on]), initial=0.0)) / scale
        worst = max(worst, err)
        assert err <= ROT_TOL, (m, err)
        ut = np.full(B, utime, dtype=np.int64) if utimes is None else utimes
        dt_want = np.full(B, dt_default)
        if atlas:
            seen = on & (prev != 0)
            dt_want[seen] = (ut[seen] - prev[seen]).astype(np.float64) * 1e-6
            prev[on] = ut[on]
        assert blk[6, on].tobytes() == dt_want[on].tobytes(), (m, np.nonzero(on & (blk[6] != dt_want))[0])
        # the filters without one
        assert blk[0:6][:, ~on].tobytes() == last[:, ~on].tobytes(), m
        assert np.all(blk[6, ~on] == 0.0) and not np.any(np.signbit(blk[6, ~on])), m
        last[:, on] = blk[0:6][:, on]
    print("ins_body_block %s: worst rotated entry error / max|input| = %.2e (bound %.0e)" % (config, worst, ROT_TOL))
    eh.close()
    ed.close()


# ---------------------------------------------------------------- 3. masked steps against "the reference did nothing" ----
STEP_B, STEP_T = 130, 40
STEP_WAVE_IDLE, STEP_ALL_IDLE, STEP_ONE_SHOT = 7, 13, 20
STEP_CHECKS = (0, 9, 39)          # steps 1, 10 and 40


def _step_validity():
    """about 30 % idle; filter 0 always valid (but for the step where nobody is), filter 1 idle from step 5 on (an ended segment),
    lane 129 alternating, the whole second wave idle at one step, every filter idle at another"""
    rng = np.random.default_rng(33)
    v = (rng.random((STEP_T, STEP_B)) > 0.3).astype(np.uint8)
    v[:, 0] = 1
    v[4:, 1] = 0
    v[:, 129] = np.arange(STEP_T) % 2
    v[STEP_WAVE_IDLE, 64:128] = 0
    v[STEP_ALL_IDLE, :] = 0
    return v


def assert_kept(n, before, after, idle, what=""):
    """the filters `idle` of a state (vec, quat, cov, ll): pose, velocity, biases, quaternion, covariance and log-likelihood bit for
    bit; for 15 states the whole vector; for 21 the angular-velocity / acceleration rows are re-derived through the biases
    (omega + bg - bg) and held to 1e-15 * max(1, max|v|), the bound of test_imu_valid_split.py"""
    v0, q0, P0, l0 = before
    v1, q1, P1, l1 = after
    rows = np.arange(n)
    exact = rows if n == 15 else rows[((rows >= 3) & (rows < 12)) | (rows >= 15)]
    moved = np.nonzero(idle & np.any(v1[exact] != v0[exact], axis=0))[0]
    assert v1[exact][:, idle].tobytes() == v0[exact][:, idle].tobytes(), (what, "vec", moved)
    if idle.any():
        assert np.max(np.abs(v1[:, idle] - v0[:, idle])) <= 1e-15 * max(1.0, np.max(np.abs(v0[:, idle]))), (what, "omega / accel rows")
    assert q1[:, idle].tobytes() == q0[:, idle].tobytes(), (what, "quat")
    assert P1[:, :, idle].tobytes() == P0[:, :, idle].tobytes(), (what, "cov", np.nonzero(idle & np.any(P1 != P0, axis=(0, 1)))[0])
    assert l1[idle].tobytes() == l0[idle].tobytes(), (what, "ll")


def _snapshot(ob):
    return ob.vec.copy(), ob.quat.copy(), ob.cov.copy(), ob.ll.copy()


def _check_against(got, want, n):
    """test_gpu_parity.check for a state that is not the head"""
    from test_gpu_parity import ELEM_TOL, TOL
    pairs = ((got[0], want[0][:n]), (got[1], want[1]), (got[2], want[2][:n, :n]), (got[3], want[3]))
    errs = [rel(a, b) for a, b in pairs]
    assert max(errs) < TOL, errs
    elem = [rel_elem(a, b) for a, b in pairs]
    assert max(elem) < ELEM_TOL, elem


def _masked_cases():
    cases = []
    for n in (15, 21):
        for mapping in ("default", "coop15=0" if n == 15 else "quad21=0"):
            cases += [(entry, n, mapping) for entry in ("predict", "step_host", "step_dev", "step_pred")]
        cases += [("correct_orient", n, "default"), ("correct_yaw", n, "default")]
        cases += [(entry, n, "qblk") for entry in ("predict", "step_dev", "correct_orient")]
    return cases + [("correct_orient_pred", 15, "default"), ("correct_yaw_pred", 15, "default")]


@pytest.mark.parametrize("entry,n,mapping", _masked_cases())
def test_masked_step_idle_filters_keep_their_prior(oracle, monkeypatch, entry, n, mapping):
    """pb_set_imu_valid in front of every entry point that takes an IMU step, on every kernel mapping, 40 steps of 130 filters:
      predict                  k_step_coop<15> / k_step_quad, PRONTO_BATCH_COOP15=0: k_step<15>, PRONTO_BATCH_QUAD21=0: k_step_coop<21>
      step_host / step_dev     pb_step_legodo on the same mappings
      step_pred                the same into an output slot with a predicted slot pending: k_step_coop_pred / k_step_quad_pred, under
                               PRONTO_BATCH_COOP15=0 the two-launch fall-back of step_pred
      correct_orient / _yaw    pb_step_legodo_correct: the fused k_step_coop<..CORR> (15 states), two launches (21)
      correct_*_pred           the same with an output and a predicted slot: k_step_coop_corr_pred (15 states)
    After EVERY step the filters without a message are compared bit for bit with their own prior (assert_kept), the others must have
    moved; at steps 1, 10 and 40 every filter is compared with the oracle, whose idle columns were put back (masked_oracle_step).  A
    predicted slot holds the oracle's state after its masked predict and, for the idle filters, the prior.  One step is followed by an
    unmasked call: the mask is one-shot.
    Mapping "qblk": the default kernels with a per-filter process noise (pb_set_process_noise_block, three different scales across
    the batch) -- what is put back behind the step for an idle filter is measured against the q THAT filter's step used.
    Semantics of the correction rows: the second update has its own mask2, independent of the IMU mask -- a filter without an IMU
    message gets no process step and no leg-odometry update, but may still receive the correction (the reference's VO / scan-match
    handler is independent of its IMU handler): the oracle applies it with mask2 alone, and only the filters with neither are held
    to their prior."""
    from pronto_amd import _lib
    from pronto_amd import batch as pa
    from test_gpu_parity import check, make_pair
    if "=" in mapping:
        monkeypatch.setenv("PRONTO_BATCH_COOP15" if n == 15 else "PRONTO_BATCH_QUAD21", "0")
    B, T = STEP_B, STEP_T
    w = Workload(B, n_states=n)
    est, ob = make_pair(pa, oracle, w, dense_p0=3)
    if "=" in mapping:
        assert ("coop" if n == 15 else "quad") not in est.hot_kernel()
    q4 = w.process_noise()
    valid = _step_validity()
    rng2 = np.random.default_rng(34)
    qscale = None
    if mapping == "qblk":
        qscale = 1.0 + 0.25 * (np.arange(B) % 3)
        q_block = _dev(np.outer(np.asarray(q4, dtype=np.float64), qscale))      # [4, B], alive until est.close()
        est.set_process_noise_block(q_block)

    def oracle_predict(imu, v):
        if qscale is None:
            masked_oracle_step(ob, v, lambda: ob.predict(imu, q4))
            return
        for s in np.unique(qscale):
            masked_oracle_step(ob, v.astype(bool) & (qscale == s), lambda: ob.predict(imu, np.asarray(q4, dtype=np.float64) * s))
    slots = entry.endswith("pred")
    if slots:
        est.history_reserve(3)
    corr = entry.startswith("correct")
    orient = entry.startswith("correct_orient")
    idx2 = [9, 10, 11, 6, 7, 8] if orient else [9, 10, 11, 8]
    state = dict(calls=0, pred=None)

    def call(k, vmask):
        """one call of the entry point on the inputs of step k (vmask None: no pb_set_imu_valid), the oracle alongside; -> mask2"""
        imu = w.imu_block(k)
        lo, mask = w.legodo_block(k)
        v = np.ones(B, dtype=np.uint8) if vmask is None else vmask
        lo_mask = (mask.astype(bool) & v.astype(bool)).astype(np.uint8)     # no message at all: no leg odometry either
        d_valid = None if vmask is None else _dev(vmask)
        if d_valid is not None:
            est.set_imu_valid(d_valid)
        if slots:
            est.set_output_slot(state["calls"] % 2)
            est.set_pred_slot(2)
        state["calls"] += 1
        mask2 = None
        if entry == "predict":
            est.predict(_dev(imu) if k % 2 else imu, q4)
        elif not corr:
            a = (imu, np.ascontiguousarray(lo), lo_mask)
            est.step_legodo(*(tuple(_dev(x) for x in a) if entry == "step_dev" else a), q4)
        else:
            z, qm, Rd = w.vo_block(k) if orient else w.scanmatch_block(k)
            zz, qm, Rd = pad_z(z, len(idx2)), np.ascontiguousarray(qm), np.ascontiguousarray(Rd)
            mask2 = (rng2.random(B) > 0.4).astype(np.uint8)
            est.step_legodo_correct(imu, np.ascontiguousarray(lo), lo_mask, q4, _lib.PB_CORR_POS_ORIENT if orient else _lib.PB_CORR_POS_YAW,
                                    zz, Rd, qm, mask2)
        est.sync()                                                           # (d_valid stays alive until the step has run)
        oracle_predict(imu, v)
        state["pred"] = _snapshot(ob) if slots else None
        if entry != "predict":
            ob.update_indexed([3, 4, 5], lo[0:3], lo[3:6], mask=lo_mask)
        if corr:
            ob.update_indexed(idx2, zz, Rd, quat_meas=qm, mask=mask2)
        return mask2

    before = est.get_head()
    for k in range(T):
        mask2 = call(k, valid[k])
        after = est.get_head()
        no_imu = valid[k] == 0
        idle = no_imu if mask2 is None else no_imu & (mask2 == 0)
        assert_kept(n, before, after, idle, (entry, k))
        assert np.all(np.any(after[2][:, :, ~no_imu] != before[2][:, :, ~no_imu], axis=(0, 1))), (k, "a filter with a message did not move")
        if slots:
            pred = est.get_slot(2)
            assert_kept(n, before, pred, no_imu, (entry, k, "predicted slot"))
        if k in STEP_CHECKS:
            check(est, ob)
            if slots:
                _check_against(pred, state["pred"], n)
        if k == STEP_ONE_SHOT:      # the mask was this call's alone: the same entry point again, without one
            assert no_imu.sum() > 20
            call(T, None)
            again = est.get_head()
            assert np.all(np.any(again[2][:, :, no_imu] != after[2][:, :, no_imu], axis=(0, 1))), "the mask outlived its call"
            after = again
        before = after
    est.close()


# ---------------------------------------------------------------- 4. a broadcast IMU sample under a mask ----
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("entry", ["predict", "split_host", "split_dev", "pair_feet"])
def test_broadcast_imu_sample_honours_the_mask(oracle, n, entry):
    """pb_set_imu_valid in front of pb_predict / pb_step_legodo_split / pb_step_legodo_feet with ONE IMU sample for every filter
    (PB_HOST_BROADCAST: the sample travels as kernel arguments, there is no device block).  The mask used to be dropped on this
    path -- every filter took the step.  Bit-identical to the same call with the sample replicated into a [7][B] device block under
    the same mask; the filters without a message keep their prior, the others move."""
    import torch
    from pronto_amd import batch as pa
    from test_gpu_parity import make_pair
    from test_leg_odometry import R_VXYZ, SCHMITT, gait
    B = 130
    rng = np.random.default_rng(41)
    w = Workload(B, n_states=n, dt_us=2000)
    q4 = w.process_noise()
    ests = [make_pair(pa, oracle, w, dense_p0=3)[0] for _ in range(2)]
    for est in ests:                                                       # (angular-velocity / acceleration entries that are not the initial ones)
        lo, mask = w.legodo_block(0)
        est.step_legodo(w.imu_block(0), lo, mask, q4)
        if entry == "pair_feet":
            est.legodo_init(*SCHMITT, True)
    ticks = gait(B, 12, seed=9) if entry == "pair_feet" else [None] * 3
    before = ests[0].get_head()
    for k, msg in enumerate(ticks, start=1):
        one = np.ascontiguousarray(w.imu_block(k)[:, 0])
        valid = (rng.random(B) > 0.4).astype(np.uint8)
        valid[64:128] = valid[64:128] if k != 2 else 0
        lo, mask = w.legodo_block(k)
        lo_mask = (mask.astype(bool) & valid.astype(bool)).astype(np.uint8)
        heads, outs = [], []
        for est, imu in ((ests[0], one), (ests[1], _dev(np.repeat(one[:, None], B, axis=1)))):
            d_valid = _dev(valid)
            est.set_imu_valid(d_valid)
            if entry == "predict":
                est.predict(imu, q4)
            elif entry == "pair_feet":
                utime, feet, forces, _ = msg
                lo_out = torch.zeros((6, B), dtype=torch.float64, device="cuda:0")
                mk_out = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
                est.legodo_set_message_times(None, valid)
                est.step_legodo_feet(imu, q4, utime, _dev(feet), _dev(forces), *R_VXYZ, lo_out, mk_out)
                outs.append((lo_out.cpu().numpy(), mk_out.cpu().numpy()))
            else:
                a = (np.ascontiguousarray(lo), lo_mask)
                est.step_legodo(imu, *(tuple(_dev(x) for x in a) if entry == "split_dev" else a), q4)
            est.sync()
            heads.append(est.get_head())
        for a, b in zip(*heads):
            assert a.tobytes() == b.tobytes(), (k, "broadcast sample and replicated block differ")
        if outs:
            (lo_a, mk_a), (lo_b, mk_b) = outs
            assert mk_a.tobytes() == mk_b.tobytes() and not np.any(mk_a[valid == 0])
            assert lo_a[:, mk_a == 1].tobytes() == lo_b[:, mk_b == 1].tobytes()
        idle = valid == 0
        assert_kept(n, before, heads[0], idle, (entry, k))
        assert np.all(np.any(heads[0][2][:, :, ~idle] != before[2][:, :, ~idle], axis=(0, 1)))
        before = heads[0]
    for est in ests:
        est.close()


# ---------------------------------------------------------------- 5. pair calls with per-filter validity and clocks ----
PAIR_B, PAIR_T, PAIR_ZERO = 12, 260, 4
PAIR_ACTIVE, PAIR_ENDED, PAIR_JUMPED = 0, 3, 7
PAIR_END_TICK, PAIR_JUMP_TICK, PAIR_JUMP_US = 100, 130, 40_000


@pytest.mark.parametrize("n,kind,mode", [(15, "joints_dev", 0), (15, "feet_dev", 0), (21, "joints_dev", 0), (21, "feet_dev", 0),
                                         (15, "joints_dev", 2)])
def test_pair_call_with_per_filter_validity_and_clocks(oracle, n, kind, mode):
    """test_pair_call_against_the_oracle_chain_on_gpu with a message time and a validity flag PER FILTER: pb_legodo_set_message_times
    (PB_HOST on even ticks, PB_DEVICE on odd ones) and the same flags to pb_set_imu_valid in front of pb_step_legodo_joints / _feet.
    The utimes jitter by +-40 us per filter; one filter's clock jumps by more than 30 ms once (updateOdometry's reset path), one
    filter's segment ends at tick 100, the others miss about 20 % of the ticks.  The oracle filter is stepped through
    masked_oracle_step and OracleLegs.update skips the filters without a message.  Per tick: masks bit-identical, the measurement
    block of the valid filters <= 1e-8, R rows at rtol 1e-14 (1e-13 in mode 2, as the six-row model test); a filter without a message
    has mask 0 and its odometry state (pb_legodo_get: pose and the three info fields) unchanged across the call.  At the end: the
    posterior (check), the odometry state of an active, the ended and the jumped filter <= 1e-9.  mode 2: LegOdoCommon's
    pos_and_lin_rate with its two-row mask."""
    import torch
    import legs
    from pronto_amd import batch as pa
    from test_gpu_parity import check
    from test_leg_odometry import R_VXYZ, SCHMITT, OracleLegs, gait
    from util import embed21
    B, T, ZERO = PAIR_B, PAIR_T, PAIR_ZERO
    R_XYZ, R_VANG, R_VANG_U = 0.05, 0.4, 0.9
    dev = torch.device("cuda:0")
    L = oracle.lib()
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    gain = np.array([7000, 10000, 10000, 10000, 10000, 10000] * 2, dtype=np.float32)
    w = Workload(B, n_states=n, dt_us=2000)
    vec, quat, P0 = w.initial_state()
    v21, P21 = embed21(vec, P0)
    ob = oracle.OracleBatch(v21, quat, P21)
    est = pa.BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    est.reset(vec, quat, P0)
    est.legodo_init(*SCHMITT, True)
    est.legodo_set_chain(*chain, gain)
    est.legodo_set_zero_initial_velocity(ZERO)
    if mode:
        est.legodo_set_measurement_mode(mode, R_XYZ, R_VANG, R_VANG_U)
    orc = OracleLegs(oracle, B, True)
    zc = np.full(B, ZERO)
    q4 = w.process_noise()
    rows = 6 if mode == 0 else 12
    lo = torch.zeros((rows, B), dtype=torch.float64, device=dev)
    mk = torch.zeros((B,) if mode == 0 else (2, B), dtype=torch.uint8, device=dev)
    r, ru = R_VXYZ
    r5 = np.array([R_XYZ, r, R_VANG, ru, R_VANG_U])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(51)
    src = legs.joint_gait(B, T, seed=27) if kind.startswith("joints") else gait(B, T, seed=27)
    n_upd, n_three, seen, n_idle = 0, 0, set(), 0
    for k, msg in enumerate(src):
        has = rng.random(B) > 0.2
        has[PAIR_ACTIVE] = has[PAIR_ACTIVE] or k >= T - 2
        has[PAIR_JUMPED] = True
        has[PAIR_ENDED] = k < PAIR_END_TICK
        v8 = has.astype(np.uint8)
        ut = (msg[0] + rng.integers(-40, 41, size=B)).astype(np.int64)
        if k >= PAIR_JUMP_TICK:
            ut[PAIR_JUMPED] += PAIR_JUMP_US
        idle = np.nonzero(~has)[0]
        n_idle += len(idle)
        leg_before = {b: est.legodo_get(b) for b in idle}
        imu = w.imu_block(k)
        if k % 2:
            d_ut, d_v = _dev(ut), _dev(v8)
            est.legodo_set_message_times(d_ut, d_v)
        else:
            est.legodo_set_message_times(ut, v8)
        d_iv = _dev(v8)
        est.set_imu_valid(d_iv)
        if kind.startswith("joints"):
            utime, jp, je, forces, _ = msg
            est.step_legodo_joints(_dev(imu), q4, utime, _dev(jp), _dev(je), _dev(forces), r, ru, lo, mk)
            ofeet = legs.oracle_feet(L, chain, jp, je, gain)
        else:
            utime, feet, forces, _ = msg
            est.step_legodo_feet(_dev(imu), q4, utime, _dev(feet), _dev(forces), r, ru, lo, mk)
            ofeet = feet
        g_mask, g_lo = mk.cpu().numpy().reshape(-1, B), lo.cpu().numpy()       # (synchronises: the device arrays above have been read)
        for b in idle:
            pose, info = est.legodo_get(b)
            assert pose.tobytes() == leg_before[b][0].tobytes() and info[:3] == leg_before[b][1][:3], (k, b)
        assert not np.any(g_mask[:, ~has]), k
        # the oracle chain on the oracle filter's OWN state; the filters without a message do nothing at all
        masked_oracle_step(ob, v8, lambda: ob.predict(imu, q4))
        oargs = (np.ascontiguousarray(ofeet), forces.astype(np.float64), np.ascontiguousarray(ob.quat))
        wpos = np.ascontiguousarray(ob.vec[9:12]) if mode == 2 else None
        if k == PAIR_JUMP_TICK:    # the same message WITHOUT the jump, on a copy of the oracle's odometry state: it would have been used
            twin = OracleLegs(oracle, B, True)
            for dst, src_ in zip(twin.bufs, orc.bufs):
                C.memmove(dst, src_, len(src_))
            ut_plain = ut.copy()
            ut_plain[PAIR_JUMPED] -= PAIR_JUMP_US
            plain_status = twin.update(ut_plain, *oargs, wpos=wpos, valid=v8)[1][PAIR_JUMPED]
            assert orc.get(PAIR_JUMPED)[2][1] == 1                     # (leg_odo_init: the odometry was running)
        od, os_, op = orc.update(ut, *oargs, wpos=wpos, valid=v8)
        if k == PAIR_JUMP_TICK:    # ... with it, updateOdometry's 30 ms reset is taken: the message re-initialises the odometry, no measurement
            assert ut[PAIR_JUMPED] - op[PAIR_JUMPED] > 30_000 and plain_status >= 0 and os_[PAIR_JUMPED] == -1.0
            assert not np.any(g_mask[:, PAIR_JUMPED])
        ok = os_ >= 0
        assert not np.any(ok & ~has)
        zc[ok] -= 1                                       # rbis_legodo_update.cpp:264-268, reached for a valid status only
        zero = ok & (zc > 0)
        seen.update(np.unique(os_).tolist())
        if mode == 0:
            od[0:3, zero] = 0.0
            elapsed = np.where(ok, (ut - op) * 1e-6, 1.0)
            z = od[0:3] / elapsed
            Rd = np.tile(np.where(os_ >= 0.5, ru * ru, r * r), (3, 1))
            mask = ok.astype(np.uint8)
            assert np.array_equal(g_mask[0], mask), (k, g_mask[0], mask)
            assert np.max(np.abs(g_lo[0:3, ok] - z[:, ok]), initial=0.0) < 1e-8, k
            assert np.allclose(g_lo[3:6, ok], Rd[:, ok], rtol=1e-14, atol=0), k
            ob.update_indexed([3, 4, 5], np.ascontiguousarray(z), np.ascontiguousarray(Rd), mask=mask)
            n_upd += int(ok.sum())
            continue
        z6, R6 = np.zeros((6, B)), np.ones((6, B))
        m_of = np.zeros(B, dtype=int)
        for b in np.nonzero(ok)[0]:
            dt3, dq, cpos = od[0:3, b].copy(), od[3:7, b].copy(), orc.pos[:, b].copy()
            if zero[b]:                                   # odo_delta / odo_position set to identity, the status passed on as it is
                dt3[:] = 0.0
                dq[:] = (1.0, 0.0, 0.0, 0.0)
                cpos[:] = 0.0
            idx = np.zeros(6, dtype=np.int32)
            z, Rd = np.zeros(6), np.zeros(6)
            m_of[b] = L.po_legodo_create_measurement(mode, dp(r5), dp(cpos), dp(dt3), dp(dq), int(ut[b]), int(op[b]), int(orc.pos_ok[b]),
                                                     float(os_[b]), idx.ctypes.data_as(C.POINTER(C.c_int)), dp(z), dp(Rd))
            if m_of[b] == 6:
                assert list(idx) == [9, 10, 11, 3, 4, 5]
                z6[:, b], R6[:, b] = z, Rd
            else:
                assert m_of[b] == 3 and list(idx[:3]) == [3, 4, 5]
                z6[3:6, b], R6[3:6, b] = z[:3], Rd[:3]
        six, three = m_of == 6, m_of == 3
        assert np.array_equal(g_mask[0], six.astype(np.uint8)), (k, g_mask[0], six)
        assert np.array_equal(g_mask[1], three.astype(np.uint8)), (k, g_mask[1], three)
        assert np.max(np.abs(g_lo[0:6][:, six] - z6[:, six]), initial=0.0) < 1e-8, k
        assert np.allclose(g_lo[6:12][:, six], R6[:, six], rtol=1e-13, atol=0), k
        assert np.max(np.abs(g_lo[3:6][:, three] - z6[3:6][:, three]), initial=0.0) < 1e-8, k
        assert np.allclose(g_lo[9:12][:, three], R6[3:6][:, three], rtol=1e-13, atol=0), k
        if six.any():
            ob.update_indexed([9, 10, 11, 3, 4, 5], np.ascontiguousarray(z6), np.ascontiguousarray(R6), mask=six.astype(np.uint8))
        if three.any():
            ob.update_indexed([3, 4, 5], np.ascontiguousarray(z6[3:6]), np.ascontiguousarray(R6[3:6]), mask=three.astype(np.uint8))
        n_upd += int(six.sum() + three.sum())
        n_three += int(three.sum())
    assert n_upd > B * T // 10 and seen == {-1.0, 0.0, 1.0} and n_idle > B * T // 10
    assert mode == 0 or n_three > 0
    check(est, ob)
    for b in (PAIR_ACTIVE, PAIR_ENDED, PAIR_JUMPED):
        pose, info = est.legodo_get(b)
        t, q, oi = orc.get(b)
        assert np.max(np.abs(pose[0:3] - t)) < 1e-9 and info[0] == oi[0] and info[1] == oi[1] and info[2] == oi[2], b
    est.close()
