"""pb_update_indexed_wide -- indexed (+ orientation) updates of seven to nine rows on k_update_wide, the GPF's all_states list
{3 ... 11} among them -- run with `-m gpu` on an MI355X.

  exact       six cases x R full / per-filter diagonal / one host diagonal on 130 pb_reset heads with cond(S) from 1e2 to 1e10, judged by
              tests/update_exact.py against the update in 60-digit arithmetic: per piece and bin, error <= 16 x the oracle's own error
              + 1e-13 (check_bound; the references are shared with tests/test_update_wide_host.py, which runs the same per-lane function
              through g++)
  parity      well-conditioned S against the oracle at the project's bar (1e-9 per block, rel_elem as test_gpu_parity.check)
  chain       20 IMU + leg-odometry steps with an all_states full-R update behind every fifth, against the same chain on the oracle
  identities  masked filters, output slots, the three input spaces, m <= 6 against pb_update_indexed: bit for bit
  edges       refused arguments, a pending predicted slot, ONE log of the determinant
"""
import numpy as np
import pytest

import update_exact as ue
from test_gpu_parity import ELEM_TOL, TOL, pa  # noqa: F401  (pa: the module fixture that builds and imports the package)
from test_update_wide_host import ALL_STATES, CASES, KINDS
from util import embed21, random_spd, rel, rel_elem

from pronto_amd.synth import Workload

pytestmark = pytest.mark.gpu

B = ue.B_GPU
LIST7, LIST8 = [17, 3, 9, 10, 11, 15, 20], [0, 14, 3, 9, 10, 11, 8, 6]


def _id(v):
    return "-".join(str(i) for i in v) if isinstance(v, list) else None


def _estimator(pa, oracle, n, batch=B, slots=0):
    est = pa.BatchEstimator(batch, n_states=n)
    est.set_constants(*oracle.constants())
    if slots:
        est.history_reserve(slots)
    return est


def _r_arg(case):
    return list(case.R) if case.kind == "host" else case.R


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,idx,orient", CASES, ids=_id)
def test_against_exact_arithmetic(pa, oracle, n, idx, orient, kind):
    case = ue.reference(oracle, n, idx, orient, kind)
    h = case.heads
    est = _estimator(pa, oracle, n)
    est.reset(h["vec"], h["quat"], h["P"])
    est.update_indexed_wide(idx, h["z"], _r_arg(case), quat_meas=case.quat_meas)
    got = est.get_head()
    est.close()
    ue.judge("wide     n=%d k_update_wide<%d,%d,%s> %s R=%s" % (n, n, len(idx), str(orient).lower(), idx, kind), case, got)


def _measurement(n, idx, Bn, vec, quat, P, seed):
    """a well-conditioned measurement of rows idx -> z [m,B], full R [m*m,B], quat_meas [4,B]"""
    rng = np.random.default_rng(seed)
    m = len(idx)
    Rd = rng.uniform(0.5, 2.0, size=(m, Bn)) * np.stack([P[i, i] for i in idx])
    z = np.ascontiguousarray(vec[idx] + np.sqrt(Rd) * rng.normal(size=(m, Bn)))
    d = 0.05 * rng.normal(size=(3, Bn))
    a = np.linalg.norm(d, axis=0)
    qm = ue._quat_mul_np(quat, np.concatenate([np.cos(a / 2)[None], np.sin(a / 2) * d / a]))
    return z, ue.full_r(Rd, seed), np.ascontiguousarray(qm)


def _heads(n, Bn, seed=5):
    w = Workload(Bn, n_states=n)
    vec, quat, P0 = w.initial_state()
    if n == 21:
        vec[15:18], vec[18:21] = 0.5 * w.bg, 0.5 * w.ba
    return w, np.ascontiguousarray(vec), np.ascontiguousarray(quat), P0 + random_spd(n, Bn, 0.03, seed)


def _check(got, want):
    errs = {k: rel(g, w) for k, g, w in zip(("vec", "quat", "cov", "ll"), got, want)}
    assert max(errs.values()) < TOL, errs
    elem = {k: rel_elem(g, w) for k, g, w in zip(("vec", "quat", "cov", "ll"), got, want)}
    assert max(elem.values()) < ELEM_TOL, elem


@pytest.mark.parametrize("orient", [False, True])
@pytest.mark.parametrize("n,idx", [(15, ALL_STATES), (21, ALL_STATES), (21, LIST7), (15, LIST8)], ids=_id)
@pytest.mark.parametrize("Bn", [1, 70, 130])
def test_parity_with_the_oracle(pa, oracle, Bn, n, idx, orient):
    _, vec, quat, P = _heads(n, Bn)
    z, R, qm = _measurement(n, idx, Bn, vec, quat, P, [n, Bn] + idx)
    qm = qm if orient else None
    est = _estimator(pa, oracle, n, Bn)
    est.reset(vec, quat, P)
    est.update_indexed_wide(idx, z, R, quat_meas=qm)
    got = est.get_head()
    est.close()
    _check(got, ue.oracle_update(oracle, n, vec, quat, P, idx, z, R, qm))


@pytest.mark.parametrize("n", [15, 21])
def test_chain_with_leg_odometry(pa, oracle, n):
    Bn = 70
    w, vec, quat, P = _heads(n, Bn, seed=7)
    est = _estimator(pa, oracle, n, Bn)
    est.reset(vec, quat, P)
    v21, P21 = embed21(vec, P)
    ob = oracle.OracleBatch(v21, quat, P21)
    q4 = w.process_noise()
    for k in range(20):
        imu = w.imu_block(k)
        lo, mask = w.legodo_block(k)
        est.step_legodo(imu, lo, mask, q4)
        ob.predict(imu, q4)
        ob.update_indexed([3, 4, 5], lo[0:3], lo[3:6], mask=mask)
        if k % 5 == 4:
            v, q, Pm, ll = ob.vec[:n].copy(), ob.quat.copy(), ob.cov[:n, :n].copy(), ob.ll.copy()
            z, R, _ = _measurement(n, ALL_STATES, Bn, v, q, Pm, [n, k])
            est.update_indexed_wide(ALL_STATES, z, R)
            v, q, Pm, ll = ue.oracle_update(oracle, n, v, q, Pm, ALL_STATES, z, R, None, ll=ll)
            v21, P21 = embed21(v, Pm)
            ob = oracle.OracleBatch(v21, q, P21, ll)
    got = est.get_head()
    est.close()
    _check(got, (ob.vec[:n], ob.quat, ob.cov[:n, :n], ob.ll))


@pytest.mark.parametrize("n,idx,orient", [(15, ALL_STATES, True), (21, ALL_STATES, False), (21, LIST7, True)], ids=_id)
def test_mask_and_output_slot_bit_identities(pa, oracle, n, idx, orient):
    _, vec, quat, P = _heads(n, B)
    z, R, qm = _measurement(n, idx, B, vec, quat, P, [n, 1] + idx)
    qm = qm if orient else None
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    est = _estimator(pa, oracle, n, slots=3)
    est.reset(vec, quat, P)
    prior = est.get_head()
    est.update_indexed_wide(idx, z, R, quat_meas=qm)
    plain = est.get_head()
    est.reset(vec, quat, P)
    est.update_indexed_wide(idx, z, R, quat_meas=qm, mask=mask)
    masked = est.get_head()
    assert all(np.array_equal(a[..., mask == 0], p[..., mask == 0]) for a, p in zip(masked, prior)), "a masked filter moved"
    assert all(np.array_equal(a[..., mask == 1], p[..., mask == 1]) for a, p in zip(masked, plain))
    # the posterior through an output slot: the in-place result, the masked filters' rows copied over, the head follows
    est.reset(vec, quat, P)
    est.set_output_slot(1)
    est.update_indexed_wide(idx, z, R, quat_meas=qm, mask=mask)
    assert est._L.pb_head_slot(est._h) == 1
    assert _same_bits(est.get_head(), masked) and _same_bits(est.get_slot(1), masked)
    # a head that lives in a slot: the next update goes back to the context's own array and leaves the slot as it was
    est.update_indexed_wide(idx, z, R, quat_meas=qm, mask=mask)
    assert est._L.pb_head_slot(est._h) == -1 and _same_bits(est.get_slot(1), masked)
    twice = est.get_head()
    est.reset(vec, quat, P)
    est.update_indexed_wide(idx, z, R, quat_meas=qm, mask=mask)
    est.update_indexed_wide(idx, z, R, quat_meas=qm, mask=mask)
    assert _same_bits(est.get_head(), twice)
    est.close()


@pytest.mark.parametrize("kind", ["host", "full"])
@pytest.mark.parametrize("n,idx,orient", [(15, ALL_STATES, False), (21, LIST8[:7], True)], ids=_id)
def test_input_spaces_give_equal_bits(pa, oracle, n, idx, orient, kind):
    """one measurement for every filter as PB_HOST blocks, PB_DEVICE tensors and PB_HOST_BROADCAST values"""
    import torch
    _, vec, quat, P = _heads(n, B)
    z1, R1, q1 = _measurement(n, idx, 1, vec[:, :1], quat[:, :1], P[:, :, :1], [n, 2] + idx)
    m = len(idx)
    z1, q1 = z1[:, 0].copy(), q1[:, 0].copy()
    R1 = R1[:, 0].copy() if kind == "full" else R1[:, 0].reshape(m, m).diagonal().copy()
    tile = lambda a: np.ascontiguousarray(np.tile(a[:, None], (1, B)))
    sums = []
    for space in ("host", "device", "broadcast"):
        est = _estimator(pa, oracle, n)
        est.reset(vec, quat, P)
        if space == "broadcast":
            args = (z1, R1 if kind == "full" else list(R1), q1 if orient else None)
        else:
            args = (tile(z1), tile(R1), tile(q1) if orient else None)
            if space == "device":
                args = tuple(None if a is None else torch.from_numpy(a).cuda() for a in args)
        est.update_indexed_wide(idx, args[0], args[1], quat_meas=args[2])
        sums.append(tuple(est.state_checksum()))
        est.close()
    assert sums[0] == sums[1] == sums[2], sums


@pytest.mark.parametrize("n,idx,orient", [(15, [9, 10, 11, 6, 7, 8], True), (15, [3, 9, 10, 11, 5], False), (15, [4, 7, 10], True),
                                          (21, [9, 10, 11, 3, 4, 5], False), (21, [10, 3, 7, 15, 20, 6], True), (21, [16], False)], ids=_id)
def test_up_to_six_rows_equal_update_indexed(pa, oracle, n, idx, orient):
    _, vec, quat, P = _heads(n, B)
    z, R, qm = _measurement(n, idx, B, vec, quat, P, [n, 3] + idx)
    qm = qm if orient else None
    m = len(idx)
    Rd = np.ascontiguousarray(R.reshape(m, m, B)[np.arange(m), np.arange(m)])
    mask = (np.arange(B) % 4 != 0).astype(np.uint8)
    for Rarg in (R if m > 1 else Rd, Rd, list(Rd[:, 0])):
        for mk in (None, mask):
            sums = []
            for wide in (False, True):
                est = _estimator(pa, oracle, n)
                est.reset(vec, quat, P)
                (est.update_indexed_wide if wide else est.update_indexed)(idx, z, Rarg, mask=mk, quat_meas=qm)
                sums.append(tuple(est.state_checksum()))
                est.close()
            assert sums[0] == sums[1]


def test_refused_arguments_leave_the_head_untouched(pa, oracle):
    _, vec, quat, P = _heads(15, B)
    est = _estimator(pa, oracle, 15, slots=2)
    est.reset(vec, quat, P)
    before = tuple(est.state_checksum())
    for bad in (list(range(10)), [3, 4, 5, 6, 7, 8, 9, 3], [3, 4, 5, 6, 7, 8, 15]):
        with pytest.raises(pa.PbError) as e:
            est.update_indexed_wide(bad, np.zeros((len(bad), B)), [0.1] * len(bad))
        assert e.value.code == 1, bad
    est.set_pred_slot(1)
    with pytest.raises(pa.PbError) as e:                        # as pb_update_indexed: no predicted slot on an update
        est.update_indexed_wide(ALL_STATES, np.zeros((9, B)), [0.1] * 9)
    assert e.value.code == 4
    assert tuple(est.state_checksum()) == before
    est.update_indexed_wide(ALL_STATES, np.ascontiguousarray(vec[3:12]), [0.1] * 9)    # ... and the slot is forgotten
    assert tuple(est.state_checksum()) != before
    est.close()


@pytest.mark.parametrize("n", [15, 21])
def test_one_log_of_the_determinant(pa, oracle, n):
    """diagonal R on a diagonal P: S is diagonal with the pivots R_k + P_kk.  One negative pivot (filters 1 mod 3): det S < 0, NaN;
    two (2 mod 3): det S > 0 and a finite likelihood (rbis.cpp:142 takes ONE log of the determinant); the rest stays finite"""
    w = Workload(B, n_states=n)
    vec, quat, _ = w.initial_state()
    P = np.zeros((n, n, B))
    P[np.arange(n), np.arange(n)] = 0.02 + 0.01 * np.arange(n)[:, None]
    R = np.full((9, B), 0.05)
    for b in range(B):
        for row in range(b % 3):
            R[row, b] = -2.0 * P[ALL_STATES[row], ALL_STATES[row], b]
    z = np.ascontiguousarray(vec[3:12] + 0.01)
    est = _estimator(pa, oracle, n)
    est.reset(np.ascontiguousarray(vec), np.ascontiguousarray(quat), P)
    est.update_indexed_wide(ALL_STATES, z, R)
    v, q, Pp, ll = est.get_head()
    est.close()
    assert np.array_equal(np.isnan(ll), np.arange(B) % 3 == 1)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(q)) and np.all(np.isfinite(Pp))
    S = R + np.stack([P[i, i] for i in ALL_STATES])
    ok = np.arange(B) % 3 != 1
    want = -np.log(np.prod(S[:, ok], axis=0)) - np.sum(0.01 ** 2 / S[:, ok], axis=0)
    assert np.max(np.abs(ll[ok] - want) / np.abs(want)) < 1e-12
