"""pb_set_process_noise_block -- [4][B] = q_gyro, q_accel, q_gyro_bias, q_accel_bias per filter -- at every kernel that loads it:
k_step, k_step_coop (whole and half tiles, with and without a correction stage), k_step_coop_pred, k_step_coop_corr_pred, k_step_quad,
k_step_quad_pred, k_replay_fused, k_replay_coop, k_replay_quad, the two pair kernels of rbis_legstep.hpp and their parameter-block
siblings, and the launchers that decide which pointer they see (pb_run_legodo's cache-blocked order shifts it per block).

The block of every case is tests/noise_block.py's: seven quadruples whose rows are not proportional (a row read in another's place, or
taken from the call's scalar q, moves the result far beyond the tolerance), assigned so that the filter a wrong offset would read --
a tile back, one to three blocks of 256 back, the other half of the tile -- always carries another quadruple.  The scalar q passed
alongside is the workload's and differs from every quadruple.  References: the oracle run group by group (per_filter_oracle*),
compared through test_gpu_parity.check / test_ragged_batches._check_against with the project's TOL and ELEM_TOL; every start
covariance is dense.  Runs on the MI355X."""
import numpy as np
import pytest

from noise_block import (noise_block, noise_quadruples, oracle_noise_block, per_filter_oracle, per_filter_oracle_columns,
                         per_filter_run_legodo)
from util import pad_z, random_spd, rel

from pronto_amd.synth import Workload

pytestmark = pytest.mark.gpu

DENSE = 3                      # seed of make_pair's dense_p0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _snapshot(ob):
    return ob.vec.copy(), ob.quat.copy(), ob.cov.copy(), ob.ll.copy()


def _pair_with_block(oracle, w):
    """(est with the block set, oracle batch, the block the oracle is stepped with, the device copy -- keep it alive as long as est
    steps --, the scalar q)"""
    from pronto_amd import batch as pa
    from test_gpu_parity import make_pair
    est, ob = make_pair(pa, oracle, w, dense_p0=DENSE)
    blk, _ = noise_block(w.B)
    d_blk = _dev(blk)
    est.set_process_noise_block(d_blk)
    q4 = w.process_noise()
    assert not any(np.array_equal(q4, q) for q in noise_quadruples())
    return est, ob, oracle_noise_block(blk, w.n), d_blk, q4


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- A. the step entry points on every mapping ----
STEP_B, STEP_T = 200, 12          # three tiles and an eight-filter tail
STEP_CHECKS = (0, 5, 11)
MAPPINGS = {  # name -> (n, environment, what pb_hot_kernel must name)
    "n15": (15, {}, "k_step_coop<15"),
    "n15_coop15=0": (15, {"PRONTO_BATCH_COOP15": "0"}, "k_step<15"),
    "n15_half=1": (15, {"PRONTO_BATCH_HALF": "1"}, "k_step_coop<15"),   # (two workgroups per tile; pb_hot_kernel names the kernel alone)
    "n21": (21, {}, "k_step_quad"),
    "n21_quad21=0": (21, {"PRONTO_BATCH_QUAD21": "0"}, "k_step_coop<21"),
}
ENTRIES = ("predict_host", "predict_dev", "step_host", "step_dev", "correct_orient", "correct_yaw", "step_pred", "correct_orient_pred",
           "correct_yaw_pred")


@pytest.mark.parametrize("mapping", list(MAPPINGS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_step_entry_follows_each_filters_own_noise(oracle, monkeypatch, entry, mapping):
    """pb_predict (IMU block from the host / the device), pb_step_legodo (host / device), pb_step_legodo_correct (position + orientation,
    position + yaw) and the last three again with an output slot and a predicted slot pending, 12 steps of 200 filters with the block
    set, on the default kernels, PRONTO_BATCH_COOP15=0 (k_step), PRONTO_BATCH_QUAD21=0 (k_step_coop<21>) and PRONTO_BATCH_HALF=1 (half
    tiles).  At steps 1, 6 and 12 the head equals the oracle whose process step ran with each filter's own quadruple; a predicted slot
    holds the oracle's state behind that per-filter process step.  After pb_set_process_noise_block(NULL) one further call follows the
    scalar q again."""
    from pronto_amd import _lib
    from test_gpu_parity import check
    from test_ragged_batches import _check_against
    n, env, kernel = MAPPINGS[mapping]
    for name in ("PRONTO_BATCH_COOP15", "PRONTO_BATCH_QUAD21", "PRONTO_BATCH_HALF"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    B, T = STEP_B, STEP_T
    w = Workload(B, n_states=n)
    est, ob, blk, d_blk, q4 = _pair_with_block(oracle, w)
    assert est.hot_kernel().startswith(kernel), est.hot_kernel()
    if n == 21:
        assert np.any(blk[2] != 0.0) and np.any(blk[3] != 0.0)
    slots = entry.endswith("pred")
    if slots:
        est.history_reserve(3)
    corr = entry.startswith("correct")
    orient = entry.startswith("correct_orient")
    idx2 = [9, 10, 11, 6, 7, 8] if orient else [9, 10, 11, 8]
    rng = np.random.default_rng(34)
    calls = [0]

    def call(k, q_block):
        """one call of the entry point on the inputs of step k, the oracle alongside (q_block None: the scalar q); -> predicted state"""
        imu = w.imu_block(k)
        lo, mask = w.legodo_block(k)
        lo = np.ascontiguousarray(lo)
        if slots:
            est.set_output_slot(calls[0] % 2)
            est.set_pred_slot(2)
        calls[0] += 1
        if entry.startswith("predict"):
            a = _dev(imu) if entry == "predict_dev" else imu           # (a device block stays alive until est.sync() below)
            est.predict(a, q4)
        elif not corr:
            a = tuple(_dev(x) for x in (imu, lo, mask)) if entry == "step_dev" else (imu, lo, mask)
            est.step_legodo(*a, q4)
        else:
            z, qm, Rd = w.vo_block(k) if orient else w.scanmatch_block(k)
            zz, qm, Rd = pad_z(z, len(idx2)), np.ascontiguousarray(qm), np.ascontiguousarray(Rd)
            mask2 = (rng.random(B) > 0.4).astype(np.uint8)
            est.step_legodo_correct(imu, lo, mask, q4, _lib.PB_CORR_POS_ORIENT if orient else _lib.PB_CORR_POS_YAW, zz, Rd, qm, mask2)
        est.sync()
        if q_block is None:
            ob.predict(imu, q4)
        else:
            per_filter_oracle(ob, q_block, lambda q: ob.predict(imu, q))
        pred = _snapshot(ob)
        if not entry.startswith("predict"):
            ob.update_indexed([3, 4, 5], lo[0:3], lo[3:6], mask=mask)
        if corr:
            ob.update_indexed(idx2, zz, Rd, quat_meas=qm, mask=mask2)
        return pred

    for k in range(T):
        pred = call(k, blk)
        if k in STEP_CHECKS:
            check(est, ob)
            if slots:
                _check_against(est.get_slot(2), pred, n)
    est.set_process_noise_block(None)
    pred = call(T, None)
    check(est, ob)
    if slots:
        _check_against(est.get_slot(2), pred, n)
    est.close()


# ---------------------------------------------------------------- B. 15 states never read rows 2 and 3 ----
@pytest.mark.parametrize("kern", ["k_step", "k_step_coop", "k_replay_coop"])
def test_15_states_ignore_the_bias_noise_rows(oracle, monkeypatch, kern):
    """A 15-state filter has no bias states: the same run with rows 2 and 3 of the block all 0 and all 1e30 is bit-identical, on the
    one-lane step, the two-wave step and the two-wave replay (a bias noise that leaked into the 15 x 15 covariance would show as
    1e30 * dt)."""
    from pronto_amd import batch as pa
    from test_gpu_parity import make_pair
    monkeypatch.setenv("PRONTO_BATCH_COOP15", "0" if kern == "k_step" else "1")
    monkeypatch.delenv("PRONTO_BATCH_HALF", raising=False)
    monkeypatch.setenv("PRONTO_BATCH_REPLAY_ONELANE", "0")
    B, T = STEP_B, STEP_T
    w = Workload(B, n_states=15)
    q4 = w.process_noise()
    d = [_dev(a) for a in w.streams(0, T)]
    heads = []
    for fill in (0.0, 1e30):
        est, _ = make_pair(pa, oracle, w, dense_p0=DENSE)
        assert ("coop" in est.hot_kernel()) == (kern != "k_step")
        blk, _ = noise_block(B)
        blk[2:4] = fill
        d_blk = _dev(blk)
        est.set_process_noise_block(d_blk)
        if kern == "k_replay_coop":
            est.replay_legodo_fused(*d, q4, 5)
        else:
            for k in range(T):
                est.step_legodo(d[0][k], d[1][k], d[2][k], q4)
        heads.append(est.get_head())
        est.close()
    assert all(np.all(np.isfinite(a)) for a in heads[1])
    assert _same(*heads)


# ---------------------------------------------------------------- C. the bulk run, step by step and cache-blocked ----
@pytest.mark.parametrize("n,kern", [(15, "coop"), (15, "lane"), (21, "quad"), (21, "coop")])
def test_cache_blocked_run_with_a_noise_block(oracle, n, kern, monkeypatch):
    """test_cache_blocked_replay_is_bit_identical_to_the_step_by_step_order (test_gpu_parity.py) with the block set: 1 024 filters in
    four blocks of 256, cache policies 0 / 1 / 2, the four step kernels.  The step-by-step order equals the oracle run group by group;
    the blocked order is bit-identical to it.  (pbk_step_range used to shift the state, the inputs and the mask to a block's first
    filter but not the noise block: every block after the first stepped with the noise of filters 0..255 -- quad_id gives those
    filters other quadruples.)"""
    from pronto_amd import batch as pa
    from test_gpu_parity import check, make_pair
    B, T = 1024, 12
    w = Workload(B, n_states=n)
    q4 = w.process_noise()
    imu, lo, mask = w.streams(0, T)
    d = [_dev(a) for a in (imu, lo, mask)]
    blk, _ = noise_block(B)
    d_blk = _dev(blk)
    monkeypatch.setenv("PRONTO_BATCH_COOP15", "1" if kern == "coop" else "0")
    monkeypatch.setenv("PRONTO_BATCH_QUAD21", "1" if kern == "quad" else "0")
    monkeypatch.delenv("PRONTO_BATCH_HALF", raising=False)
    heads = {}
    for blocked in ("0", "1"):
        for hint in (("0", "1", "2") if blocked == "1" else ("0",)):
            monkeypatch.setenv("PRONTO_BATCH_BLOCKED", blocked)
            monkeypatch.setenv("PRONTO_BATCH_BLOCK_FILTERS", "320")
            monkeypatch.setenv("PRONTO_BATCH_MEMHINT", hint)
            est, ob = make_pair(pa, oracle, w, dense_p0=5)
            assert [t for t in ("coop", "quad") if t in est.hot_kernel()] == ([] if kern == "lane" else [kern])
            assert est.run_block() == (256 if blocked == "1" else 0)
            est.set_process_noise_block(d_blk)
            est.run_legodo(*d, q4)
            est.run_legodo(*d, q4)          # (twice: the second call starts from a head the blocked order left)
            heads[(blocked, hint)] = est.get_head()
            if blocked == "0":
                for _ in range(2):
                    per_filter_run_legodo(oracle, ob, imu, lo, mask, oracle_noise_block(blk, n))
                check(est, ob)
            est.close()
    ref = heads[("0", "0")]
    for key, head in heads.items():
        differ = np.nonzero(np.any(head[2] != ref[2], axis=(0, 1)))[0]
        assert _same(head, ref), (key, "filters that differ from the step-by-step order: %d, the first %s" % (len(differ), differ[:4]))


# ---------------------------------------------------------------- D. the time-fused replay ----
REPLAY_T = 14


@pytest.mark.parametrize("n,onelane", [(15, "0"), (15, "1"), (21, "0")])
@pytest.mark.parametrize("T_fuse", [1, 7])
def test_time_fused_replay_with_a_noise_block(oracle, monkeypatch, n, onelane, T_fuse):
    """pb_replay_legodo_fused with the block set: k_replay_coop<15>, k_replay_fused<15> (PRONTO_BATCH_REPLAY_ONELANE=1) and k_replay_quad,
    one and seven steps per launch over 14 steps of 200 filters.  Against the per-step path with the same block 1e-12 (the bound of
    test_time_fused_replay_equals_per_step_path: another kernel, other multiply-add contractions), against the grouped oracle check().
    (The one-lane switch is read by pb_create; as a function-local static it kept the value of the process's first replay call, and a
    test that asked for the one-lane kernel behind any other replay test ran k_replay_coop.)"""
    from pronto_amd import batch as pa
    from test_gpu_parity import check, make_pair
    monkeypatch.setenv("PRONTO_BATCH_REPLAY_ONELANE", onelane)
    for name in ("PRONTO_BATCH_COOP15", "PRONTO_BATCH_QUAD21", "PRONTO_BATCH_HALF"):
        monkeypatch.delenv(name, raising=False)
    B, T = STEP_B, REPLAY_T
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    d = [_dev(a) for a in (imu, lo, mask)]
    est_f, ob, blk, d_blk, q4 = _pair_with_block(oracle, w)
    est_s, _ = make_pair(pa, oracle, w, dense_p0=DENSE)
    est_s.set_process_noise_block(d_blk)
    est_f.replay_legodo_fused(*d, q4, T_fuse)
    est_s.run_legodo(*d, q4)
    per_filter_run_legodo(oracle, ob, imu, lo, mask, blk)
    check(est_f, ob)
    check(est_s, ob)
    worst = max(rel(a, b) for a, b in zip(est_f.get_head(), est_s.get_head()))
    assert worst < 1e-12, worst
    est_f.close()
    est_s.close()


@pytest.mark.parametrize("n", [15, 21])
def test_checkpointed_replay_with_a_noise_block(oracle, monkeypatch, n):
    """pb_replay_legodo_checkpointed with the block set, EVERY slot compared: bit for bit with the same replay kernel launched one step at
    a time, 1e-12 with the per-message path into slots (the header's two statements), check() against the grouped oracle."""
    from pronto_amd import batch as pa
    from test_gpu_parity import make_pair
    from test_ragged_batches import _check_against
    monkeypatch.setenv("PRONTO_BATCH_REPLAY_ONELANE", "0")
    B, T = STEP_B, REPLAY_T
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    d = [_dev(a) for a in (imu, lo, mask)]
    est_c, ob, blk, d_blk, q4 = _pair_with_block(oracle, w)
    est_1, _ = make_pair(pa, oracle, w, dense_p0=DENSE)
    est_s, _ = make_pair(pa, oracle, w, dense_p0=DENSE)
    for e in (est_1, est_s):
        e.set_process_noise_block(d_blk)
    for e in (est_c, est_s):
        e.history_reserve(T + 1)
    est_c.replay_legodo_checkpointed(*d, q4, 5, first_slot=1)       # launches of 5, 5 and 4 steps
    for t in range(T):
        est_1.replay_legodo_fused(d[0][t:t + 1].contiguous(), d[1][t:t + 1].contiguous(), d[2][t:t + 1].contiguous(), q4, 1)
        est_s.set_output_slot(1 + t)
        est_s.step_legodo(d[0][t], d[1][t], d[2][t], q4)
        per_filter_oracle(ob, blk, lambda q: ob.predict(imu[t], q))
        ob.update_indexed([3, 4, 5], np.ascontiguousarray(lo[t][0:3]), np.ascontiguousarray(lo[t][3:6]), mask=mask[t])
        got = est_c.get_slot(1 + t)
        assert _same(got, est_1.get_head()), t
        assert max(rel(a, b) for a, b in zip(got, est_s.get_slot(1 + t))) < 1e-12, t
        _check_against(got, _snapshot(ob), n)
    assert _same(est_c.get_head(), est_1.get_head())
    for e in (est_c, est_1, est_s):
        e.close()


# ---------------------------------------------------------------- E. the pair kernels ----
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("kind,param_block", [("feet_dev", False), ("joints_dev", False), ("joints_dev", True)])
def test_pair_call_with_a_noise_block(oracle, n, kind, param_block):
    """pb_step_legodo_feet / pb_step_legodo_joints with the block set: k_pair_leg / k_pair_quad_leg, and with pb_legodo_set_param_block
    set as well (both per-filter blocks live at once) k_pair_legpar / k_pair_quad_legpar.  The oracle chain of
    test_leg_param_block.pair_chain (per tick the process step, then on the oracle filter's own pose the leg odometry, the lin_rate
    measurement and its update) with the process step made per filter; that file's tolerances.  B = 65: one tile and one filter."""
    from pronto_amd import batch as pa
    from test_leg_param_block import draws, pair_chain, uniform_block
    B = 65
    blk, _ = noise_block(B)
    est = pa.BatchEstimator(B, n_states=n)
    n_upd, _, seen, _ = pair_chain(oracle, n, kind, 0, B, draws(B) if param_block else uniform_block(B), est, q_block=blk, param_block=param_block, dense_p0=DENSE)
    assert n_upd > B * 260 // 10 and seen == {-1.0, 0.0, 1.0}
    est.close()


# ---------------------------------------------------------------- F. the smoothing drivers ----
SM_B, SM_T, SM_K, SM_DT = 37, 50, 7, 1e-3          # the shapes of test_smoother.py's whole-log test
SM_TICKS = [0, 6, 7, 20, 34, 48, 49]               # test_smooth_log_corrected.py's
SM_KIND, SM_IDX = 0, [9, 10, 11, 6, 7, 8]
_SM_ORACLE = {}


def _sm_start(w):
    """start_of(w) with a dense start covariance over the states the process step PROPAGATES (velocity, chi, position, biases).  The
    angular-velocity and acceleration rows stay as start_of leaves them: the process step overwrites their diagonal blocks with
    q_gyro I / q_accel I (rbis.cpp:120-121) and keeps their cross-covariances, so a dense prior THERE (cross terms ~3e-3 against a
    new diagonal of 6e-5 ... 8e-2) makes the first predicted covariances indefinite -- smallest eigenvalue -1e-2 in the oracle's forward
    pass, with the workload's own q as well -- and the RTS step, which factorises the predicted covariance, has no meaning on them
    (the oracle's pivoted and the kernels' unpivoted LDL^T then differ by 1e-9 and more).  _sm_oracle asserts the precondition."""
    from smoother_ref import start_of
    vec, quat, P0, q4 = start_of(w)
    D = random_spd(w.n, w.B, 0.03, DENSE)
    for rows in (slice(0, 3), slice(12, 15)):
        D[rows], D[:, rows] = 0.0, 0.0
    return vec, quat, P0 + D, q4


def _sm_corr(w):
    from test_smooth_log_corrected import _corr_stream
    return _corr_stream(w, SM_KIND, SM_TICKS, w.B)


def _sm_oracle(oracle, n, corrected):
    """the grouped oracle's forward pass and backward recursion, once per (n, corrected): {step: (vec, quat, cov)}"""
    from smoother_ref import oracle_backward_pass, oracle_forward
    key = (n, corrected)
    if key not in _SM_ORACLE:
        w = Workload(SM_B, n_states=n)
        P0 = _sm_start(w)[2]
        blk = oracle_noise_block(noise_block(SM_B, smoothable=True)[0], n)
        corr = (SM_IDX, SM_TICKS, *_sm_corr(w)) if corrected else None
        # the precondition of the RTS step, on the reference alone: every predicted covariance is positive definite
        for pred, _ in per_filter_oracle_columns(blk, lambda cols, q: oracle_forward(oracle, w, n, SM_T, len(cols), q4=q, cols=cols, P0=P0, corr=corr)):
            P = np.moveaxis(pred[2][:n, :n], 2, 0)
            assert np.linalg.eigvalsh(0.5 * (P + np.swapaxes(P, 1, 2))).min() > 0.0
        keep = {0, 1, SM_K - 1, SM_K, 3 * SM_K, SM_T - 3, SM_T - 2}
        _SM_ORACLE[key] = per_filter_oracle_columns(
            blk, lambda cols, q: oracle_backward_pass(oracle, w, n, SM_T, len(cols), SM_DT, keep, q4=q, cols=cols, P0=P0, corr=corr))
    return _SM_ORACLE[key]


@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("driver", ["smooth_log", "smooth_log_fused", "smooth_log_corrected"])
def test_smoothing_driver_with_a_noise_block(oracle, n, driver):
    """pb_smooth_log, pb_smooth_log_fused and pb_smooth_log_corrected (fused, position + orientation ticks) with the block set: the forward
    pass AND the recompute pass step with each filter's own noise.  Bit-identical to the all-checkpoints pass built from the same
    per-message calls under the same block, and within test_smoother.py's TOL of the grouped oracle's backward recursion.
    The RTS step factorises the predicted covariance, so this case keeps it positive definite (asserted on the oracle's forward pass):
    q_gyro, q_accel > 0 (noise_quadruples(smoothable=True)) and the dense part of the start covariance over the propagated states only
    (_sm_start).  With an exact 0 in q_gyro / q_accel the kernels and the oracle differed by 6e-3, with the dense prior over the
    angular-velocity / acceleration rows by 1.4e-9 (15 states) -- both on matrices the reference's own .ldlt() has no answer for."""
    from pronto_amd.batch import BatchEstimator
    from test_smoother import TOL
    B, T, K, dt = SM_B, SM_T, SM_K, SM_DT
    w = Workload(B, n_states=n)
    vec, quat, P0, q4 = _sm_start(w)
    imu, lo, mask = w.streams(0, T)
    blk, qid = noise_block(B, smoothable=True)   # (q_gyro, q_accel > 0: the RTS step inverts the predicted covariance)
    d_blk = _dev(blk)
    corrected = driver == "smooth_log_corrected"
    corr = _sm_corr(w) if corrected else None

    def make(slots):
        e = BatchEstimator(B, n_states=n)
        e.set_constants(*oracle.constants())
        e.reset(vec, quat, P0)
        e.history_reserve(slots)
        e.set_process_noise_block(d_blk)
        return e
    ref = make(2 * T + 2)
    for k in range(T):
        c = [a[SM_TICKS.index(k)] for a in corr] if corrected and k in SM_TICKS else None
        if driver == "smooth_log":
            ref.set_output_slot(2 * k)
            ref.predict(imu[k], q4)
            ref.set_output_slot(2 * k + 1)
            ref.update_indexed([3, 4, 5], np.ascontiguousarray(lo[k][0:3]), np.ascontiguousarray(lo[k][3:6]), mask=mask[k])
        else:
            ref.set_pred_slot(2 * k)
            ref.set_output_slot(2 * k + 1)
            if c:
                ref.step_legodo_correct(imu[k], lo[k], mask[k], q4, SM_KIND, *c)
            else:
                ref.step_legodo(imu[k], lo[k], mask[k], q4)
    final = ref.get_slot(2 * (T - 1) + 1)
    want, nxt = {}, 2 * (T - 1) + 1
    for k in range(T - 2, -1, -1):
        out = 2 * T + (k % 2)
        ref.smooth_step(2 * (k + 1), nxt, 2 * k + 1, out, dt)
        want[k] = ref.get_slot(out)
        nxt = out
    ref.close()
    est = make(0)
    est.history_reserve(est.smooth_log_slots(T, K) + 1)
    got, order = {}, []

    def sink(step, slot):
        order.append(step)
        got[step] = est.get_slot(slot)
    streams = [_dev(a) for a in (imu, lo, mask)]
    if corrected:
        z2, R2, qm2, mask2 = (_dev(a) for a in corr)
        est.smooth_log_corrected(*streams, q4, dt, K, SM_KIND, SM_TICKS, z2, R2, qm2, mask2, fused=True, first_slot=1, sink=sink)
    else:
        est.smooth_log(*streams, q4, dt, K, first_slot=1, sink=sink, fused=driver == "smooth_log_fused")
    assert order == list(range(T - 2, -1, -1))
    for k in range(T - 1):
        assert _same(got[k], want[k]), k
    assert _same(est.get_head(), final)
    est.close()
    ora = _sm_oracle(oracle, n, corrected)
    worst = np.zeros(7)                         # per quadruple: a miss names the noise it came with
    for k, (ov, oq, oP) in ora.items():
        v, q, P, _ = got[k]
        for g in range(7):
            s = qid == g
            worst[g] = max(worst[g], rel(v[:, s], ov[:n][:, s]), rel(q[:, s], oq[:, s]), rel(P[:, :, s], oP[:n, :n][:, :, s]))
    print("%s n=%d: worst error against the grouped oracle per quadruple" % (driver, n), ["%.1e" % x for x in worst])
    assert worst.max() < TOL, worst
