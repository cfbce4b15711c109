"""Every measurement-update kernel against exact arithmetic on an ill-conditioned innovation covariance -- run with `-m gpu` on an
MI355X.  The parity tests hold the kernels to the oracle at 1e-9; from cond(S) ~ 1e9 two correct fp64 updates differ by more than
that, so no parity test goes there, and a pivot clamp or a regulariser in ldlt<M> (rbis_device.hpp) would pass all of them.  Here
the judge is tests/update_exact.py: the reference's update in mpmath at 60 digits, 130 heads (two waves and a two-lane tail) in five
bins of 26 with cond(S) from 1e2 to 1e10, set with pb_reset, one update, read back with pb_get_head.

Bound (update_exact.check_bound; the precedent is test_noise_id.py): per piece -- state vector outside chi, quaternion,
log-likelihood, and the (idx,idx), (other,idx), (other,other) blocks of the covariance, each on its own scale -- and per bin,
kernel error <= 16 x the oracle's worst error in that bin + 1e-13, both against the exact posterior; every output finite.  16 is
the project's precedent, not derived: the unpivoted LDL^T + rank-m downdate and the oracle's pivoted LDL^T + dense P - K C P are
both backward stable on SPD S, and the factor leaves room for the order of operations of each mapping while a lost digit and a half
fails.  The exact posterior is computed for every second filter of each bin (13 of 26: the references of this file take over a
minute otherwise).

Measured on an MI355X, the bin of the worst conditioned filters (cond(S) 2.5e8 ... 8e9), per-filter diagonal R, oracle / kernel,
of each kernel the list with the largest kernel : oracle ratio (every bin of every case: profiles/update_exact.txt; the tests print
them before they assert).  P_oo, the block the update hardly touches, stays at or under 1.7e-15 everywhere:
      kernel                               vec                 quat                ll                  P_mm                P_om
      k_update_lane_rt                     1.1e-07 / 1.7e-07   1.1e-08 / 2.5e-08   4.0e-08 / 1.5e-07   4.1e-07 / 8.2e-07   8.5e-07 / 1.3e-06
      k_update_coop_rt                     2.2e-08 / 1.8e-08   3.8e-09 / 4.7e-09   6.2e-08 / 6.6e-08   3.0e-06 / 2.8e-06   6.5e-06 / 4.5e-06
      k_step_coop<15>                      2.0e-08 / 2.6e-08   3.9e-09 / 5.1e-09   4.0e-08 / 1.5e-07   4.1e-07 / 8.2e-07   8.5e-07 / 1.3e-06
      k_update_lane                        7.8e-08 / 6.5e-08   9.6e-09 / 9.0e-09   8.6e-08 / 1.7e-07   3.8e-06 / 2.1e-06   9.8e-06 / 7.2e-06
      k_update_quad_rt                     8.9e-08 / 2.8e-07   8.4e-09 / 3.4e-08   6.8e-08 / 5.5e-07   4.3e-06 / 9.5e-06   5.0e-06 / 8.9e-06
      k_update_quad                        3.8e-08 / 5.4e-08   1.0e-09 / 3.4e-09   3.1e-08 / 9.5e-08   4.1e-07 / 8.2e-07   1.0e-05 / 1.7e-05
      k_update_quad_list                   5.2e-08 / 3.6e-08   8.9e-09 / 5.0e-09   5.5e-08 / 5.7e-08   2.3e-06 / 3.0e-06   5.8e-06 / 6.0e-06
      k_step_coop<21>                      3.8e-08 / 5.4e-08   1.0e-09 / 3.4e-09   3.1e-08 / 9.5e-08   4.1e-07 / 8.2e-07   1.0e-05 / 1.7e-05
      k_step_coop_pred<15>                 1.0e-09 / 4.6e-10   2.0e-09 / 2.3e-09   1.1e-07 / 3.1e-08   3.6e-06 / 3.4e-06   7.8e-06 / 3.9e-06
      k_step_quad_pred                     1.7e-09 / 7.9e-10   8.1e-09 / 2.5e-09   1.1e-07 / 1.0e-07   3.0e-06 / 1.9e-06   4.9e-06 / 1.8e-06
      k_step_coop_pred<15,CorrPosOrient>   5.4e-09 / 7.3e-09   9.3e-09 / 8.0e-09   5.8e-08 / 8.9e-08   4.6e-06 / 2.2e-06   8.0e-06 / 3.0e-06
      k_step_coop_pred<15,CorrPosYaw>      8.2e-10 / 2.1e-09   1.6e-09 / 5.4e-09   1.3e-07 / 2.4e-07   6.0e-06 / 3.2e-06   5.0e-06 / 3.1e-06
The largest share of the bound any case, piece and bin uses is 0.62 (k_update_quad_rt<3>, [5,8,19], log-likelihood, first bin:
3.9e-13 against the oracle's 3.3e-14); in the last bin the largest kernel : oracle ratio is 8 (k_update_quad_rt, log-likelihood).
"""
import numpy as np
import pytest

import update_exact as ue

pytestmark = pytest.mark.gpu

B = ue.B_GPU
SWITCHES = ("PRONTO_BATCH_GENERIC_UPDATE", "PRONTO_BATCH_QUAD21", "PRONTO_BATCH_COOP15", "PRONTO_BATCH_HALF", "PRONTO_BATCH_MEMHINT")
H = ue.HANDLER_LISTS
# run-time lists for the generic kernels: m = 1 ... 6 without and with an orientation measurement (21 states: bias rows among them)
GENERIC = {15: [H[9], H[6], ([4, 10], False), ([7, 9], True), H[0], ([4, 7, 10], True), H[7], H[4], ([3, 9, 10, 11, 5], False),
                ([9, 10, 11, 7, 8], True), H[2], H[3]],
           21: [([16], False), H[6], ([4, 16], False), ([7, 19], True), H[0], ([5, 8, 19], True), H[7], H[4], ([3, 9, 15, 11, 20], False),
                ([9, 10, 18, 7, 8], True), H[2], ([10, 3, 7, 15, 20, 6], True)]}
FULL_R_LISTS = [H[k] for k in (0, 1, 2, 3, 4, 7, 8, 9, 10)]        # test_full_r_on_the_handler_index_lists' lists
CORR_NAME = ["CorrVel", "CorrPos", "CorrPosVel", "CorrPosOrient", "CorrPosYaw", "CorrVelYaw", "CorrYaw", "CorrGpfYawPos", "CorrGpfChiPos",
             "CorrGpfZ"]


def _cases():
    """(mapping, n, idx, orient, R kind, the kernel the case means to run)"""
    out = []

    def add(mapping, n, lists, kern, host_on):
        for idx, o in lists:
            out.append((mapping, n, idx, o, "diag", kern(idx, o)))
        for idx, o in lists:
            if idx in host_on:
                out.append((mapping, n, idx, o, "host", kern(idx, o)))
        for idx, o in lists:
            # (for m = 1 a full R is the per-filter diagonal)
            if len(idx) > 1 and (mapping.startswith("generic") or (idx, o) in FULL_R_LISTS):
                out.append((mapping, n, idx, o, "full", kern(idx, o)))

    add("generic", 15, GENERIC[15], lambda i, o: "k_update_lane_rt<15,%d,%s>" % (len(i), str(o).lower()) if len(i) <= 4 else "k_update_coop_rt<%d>" % len(i),
        ([4, 10], [3, 9, 10, 11, 5]))
    add("default", 15, H, lambda i, o: "k_step_coop<15,false,.,%s>" % CORR_NAME[H.index((i, o))] if (i, o) != H[10] else "k_update_lane<15,6,IdxVelOmega>",
        ([9, 10, 11, 8], [3, 4, 5, 0, 1, 2]))
    add("generic", 21, GENERIC[21], lambda i, o: "k_update_quad_rt<%d>" % len(i), ([4, 16],))
    add("default", 21, H, lambda i, o: "k_update_quad<%s>" % CORR_NAME[H.index((i, o))] if (i, o) != H[10] else "k_update_quad_list<.,3,4,5,0,1,2>",
        ([9, 10, 11, 6, 7, 8], [3, 4, 5, 0, 1, 2]))
    add("quad21=0", 21, [l for l in H[:10] if len(l[0]) <= 4], lambda i, o: "k_step_coop<21,false,.,%s>" % CORR_NAME[H.index((i, o))], ([9, 10, 11, 8],))
    return out


def _id(v):
    return "-".join(str(i) for i in v) if isinstance(v, list) else None


def _estimator(oracle, monkeypatch, mapping, n, slots=0):
    """an estimator on the mapping a case names; the switches are read in pb_create"""
    from pronto_amd.batch import BatchEstimator
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if mapping == "generic":
        monkeypatch.setenv("PRONTO_BATCH_GENERIC_UPDATE", "1")
    if mapping == "quad21=0":
        monkeypatch.setenv("PRONTO_BATCH_QUAD21", "0")
    est = BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    # pb_hot_kernel names the step kernel of the mapping the context chose; the stand-alone updates follow that choice and the switch
    want = {15: "k_step_coop<15", 21: "k_step_coop<21" if mapping == "quad21=0" else "k_step_quad"}[n]
    assert est.hot_kernel().startswith(want), est.hot_kernel()
    if slots:
        est.history_reserve(slots)
    return est


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _r_arg(case):
    return list(case.R) if case.kind == "host" else case.R


@pytest.mark.parametrize("mapping,n,idx,orient,kind,kernel", _cases(), ids=_id)
def test_stand_alone_update_against_exact_arithmetic(oracle, monkeypatch, mapping, n, idx, orient, kind, kernel):
    """One pb_update_indexed / pb_update_indexed_orient on every kernel that can take it:
      15 states  PRONTO_BATCH_GENERIC_UPDATE=1: k_update_lane_rt<15,M,ORIENT> (m = 1 ... 4, both ORIENT), k_update_coop_rt<M> (m = 5, 6);
                 default: k_step_coop<15,false,.,CORR> for the ten compile-time lists, k_update_lane<15,6,IdxVelOmega> for [3,4,5,0,1,2]
      21 states  PRONTO_BATCH_GENERIC_UPDATE=1: k_update_quad_rt<M> (m = 1 ... 6); default: k_update_quad<CORR> for the ten lists,
                 k_update_quad_list for [3,4,5,0,1,2]; PRONTO_BATCH_QUAD21=0: k_step_coop<21,false,.,CORR> for the lists with m <= 4
      R          a per-filter diagonal everywhere; one host diagonal on one list per kernel; a full R with off-diagonals on the
                 generic kernels and on the handler lists that take one (m > 1)
      mask       the same update again with every second filter masked out: those keep their prior bit for bit, the others meet
                 the same bound
    The case asserts the mapping through pb_hot_kernel and the switch it set; `kernel` in the test id's place names what runs."""
    case = ue.reference(oracle, n, idx, orient, kind)
    h = case.heads
    est = _estimator(oracle, monkeypatch, mapping, n)
    label = "%-8s n=%d %-34s %-18s R=%s" % (mapping, n, kernel, idx, kind)
    est.reset(h["vec"], h["quat"], h["P"])
    prior = est.get_head()
    assert _same_bits(prior, (h["vec"], h["quat"], h["P"], np.zeros(B)))
    est.update_indexed(idx, h["z"], _r_arg(case), quat_meas=case.quat_meas)
    got = est.get_head()
    ue.judge(label, case, got)
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)          # the filters with an exact posterior stay active
    est.reset(h["vec"], h["quat"], h["P"])
    est.update_indexed(idx, h["z"], _r_arg(case), quat_meas=case.quat_meas, mask=mask)
    gm = est.get_head()
    est.close()
    assert all(np.array_equal(a[..., mask == 0], p[..., mask == 0]) for a, p in zip(gm, prior)), "a masked filter moved"
    ue.judge(label + " masked", case, gm, quiet=True)


def _one_log_inputs(oracle, n, idx):
    """well-conditioned heads with a negative R on the first row (filters 1 mod 3: det S < 0) / the first two rows (2 mod 3: det S > 0
    from two negative pivots) -> (heads, R, exact)"""
    h = ue.ill_conditioned_heads(n, idx, B, [n, 2] + idx)
    R = h["R"].copy()
    for b in range(B):
        for row in range(b % 3):
            R[row, b] = -2.0 * h["P"][idx[row], idx[row], b]
    few = np.arange(12)                                      # cond 1e2 ... 5e2
    ex = ue.exact_update(n, ue.take(h["vec"], few), ue.take(h["quat"], few), ue.take(h["P"], few), idx, ue.take(h["z"], few), ue.take(R, few),
                         None, None, oracle.constants())
    return h, np.ascontiguousarray(R), few, ex


@pytest.mark.parametrize("mapping,n,idx", [("generic", 15, [4, 10]), ("generic", 15, [3, 9, 10, 11, 5]), ("default", 15, [9, 10, 11]),
                                           ("default", 15, [3, 4, 5, 0, 1, 2]), ("generic", 21, [5, 8, 19]), ("default", 21, [9, 10, 11, 3, 4, 5]),
                                           ("default", 21, [3, 4, 5, 0, 1, 2]), ("quad21=0", 21, [8, 9, 10, 11])], ids=_id)
def test_one_log_of_the_determinant(oracle, monkeypatch, mapping, n, idx):
    """The reference takes ONE log of S.determinant() (rbis.cpp:142): on an indefinite S a negative determinant gives NaN and two
    negative pivots a finite value, where a sum of logs of |pivots| gives a finite value for both.  One list per kernel; the NaNs sit on
    the filters whose exact determinant is negative and nowhere else; state, covariance and the finite likelihoods of the twelve
    filters with an exact posterior (cond <= 5e2) agree with it to 1e-9."""
    h, R, few, ex = _one_log_inputs(oracle, n, idx)
    est = _estimator(oracle, monkeypatch, mapping, n)
    est.reset(h["vec"], h["quat"], h["P"])
    est.update_indexed(idx, h["z"], R)
    v, q, P, ll = est.get_head()
    est.close()
    neg = np.arange(B) % 3 == 1
    assert np.array_equal(np.isnan(ll), neg) and np.all(np.isfinite(v)) and np.all(np.isfinite(q)) and np.all(np.isfinite(P))
    assert np.array_equal(np.isnan(ex["ll"]), neg[few])
    e = ue.errors((ue.take(v, few), ue.take(q, few), ue.take(P, few), np.where(neg[few], 0.0, ll[few])), dict(ex, ll=np.where(neg[few], 0.0, ex["ll"])), idx)
    assert max(e[p].max() for p in ue.PIECES) < 1e-9, {p: e[p].max() for p in ue.PIECES}


FUSED_DT = 1e-13      # the predict in front of the update must leave the measured block as ill-conditioned as it was set
FUSED_Q4 = [4.0, 4.0, 1e-3, 1e-3]   # the predict overwrites P[omega,omega], P[accel,accel] with these: at or over what was there, P stays SPD


@pytest.mark.parametrize("n,corr", [(15, None), (21, None), (15, 0), (15, 1)])
def test_fused_step_against_exact_arithmetic(oracle, monkeypatch, n, corr):
    """pb_step_legodo (predict + a three-row velocity update: k_step_coop_pred<15>, k_step_quad_pred) and pb_step_legodo_correct
    (+ PB_CORR_POS_ORIENT / PB_CORR_POS_YAW behind it, 15 states) with a predicted-state slot set: the exact update is applied to the
    kernel's OWN stored prediction, read back from the slot, so the predict's rounding is not judged.  dt = 1e-13 and a process noise
    that only replaces the angular-velocity and acceleration blocks by something larger keep the measured block as ill-conditioned
    as pb_reset left it; cond(S) of the bins is asserted from the stored prediction (first bin <= 1e4, last >= 1e8), like the positive
    definiteness of the prediction and of the exact posterior.  The corrected step's velocity update is a weak one (R = 100) in front
    of the ill-conditioned correction, both in exact arithmetic without rounding in between.  The same call without a predicted slot
    leaves the same head bit for bit (test_pred_slot.py ties the plain fused step; the corrected one is tied here)."""
    from pronto_amd import _lib
    from pronto_amd.synth import Workload
    idx = [3, 4, 5] if corr is None else ([9, 10, 11, 6, 7, 8] if corr == _lib.PB_CORR_POS_ORIENT else [9, 10, 11, 8])
    h = ue.ill_conditioned_heads(n, idx, B, [n, 3] + idx)
    imu = Workload(B, n_states=n).imu_block(0)
    imu[6] = FUSED_DT
    lo = np.ascontiguousarray(np.concatenate([h["vec"][3:6] + 1.0, np.full((3, B), 100.0)])) if corr is not None else \
        np.ascontiguousarray(np.concatenate([h["z"], h["R"]]))
    heads = []
    for pred_slot in (True, False):
        est = _estimator(oracle, monkeypatch, "default", n, slots=4)
        est.reset(h["vec"], h["quat"], h["P"])
        if pred_slot:
            est.set_pred_slot(1)
        if corr is None:
            est.step_legodo(imu, lo, None, FUSED_Q4)
        else:
            est.set_output_slot(2)
            est.step_legodo_correct(imu, lo, None, FUSED_Q4, corr, h["z"], h["R"], h["quat_meas"])
        heads.append(est.get_head())
        if pred_slot:
            pred = est.get_slot(1)
        est.close()
    assert _same_bits(heads[0], heads[1]), "the predicted slot changed the filtered head"
    case = ue.Case()
    case.n, case.B = n, B
    stages = [([3, 4, 5], lo[0:3], lo[3:6], None)]
    if corr is not None:
        stages.append((idx, h["z"], h["R"], h["quat_meas"]))
    ue.judge_against(oracle, case, pred, stages)
    kernel = {(15, None): "k_step_coop_pred<15>", (21, None): "k_step_quad_pred", (15, 0): "k_step_coop_pred<15,CorrPosOrient>",
              (15, 1): "k_step_coop_pred<15,CorrPosYaw>"}[(n, corr)]
    ue.judge("%-8s n=%d %-34s %-18s R=%s" % ("fused", n, kernel, idx, "diag"), case, heads[0])
