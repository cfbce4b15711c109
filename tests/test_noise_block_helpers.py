"""The helpers of tests/noise_block.py on the CPU: what tests/test_process_noise_block.py concludes from a per-filter process noise
rests on (a) quadruples that tell the rows apart, (b) an assignment no offset alias maps onto itself and (c) a grouped oracle that
is the plain oracle when the groups do not differ."""
import numpy as np
import pytest

from noise_block import (ALIAS_SHIFTS, N_QUADS, noise_block, noise_quadruples, oracle_columns, per_filter_oracle, per_filter_oracle_columns,
                         per_filter_run_legodo, quad_id)
from smoother_ref import oracle_backward_pass
from util import embed21, random_spd

from pronto_amd.synth import Workload


def test_noise_quadruples_tell_the_rows_apart():
    Q = noise_quadruples()       # (asserts its own properties)
    assert Q.shape == (7, 4)
    # a row read in another row's place, or replaced by ANY scalar, changes at least one quadruple by more than a factor of two
    for i in range(4):
        assert np.max(Q[:, i]) > 2.0 * np.min(Q[:, i])
        for j in range(4):
            if i != j:
                a, b = Q[:, i], Q[:, j]
                assert np.any(np.maximum(a, b) > 2.0 * np.minimum(a, b)), (i, j)
    assert np.sum((Q[:, None, :2] == Q[None, :, :2]).all(axis=2)) == N_QUADS + 2    # exactly one pair that rows 0 / 1 do not tell apart


@pytest.mark.parametrize("B", [37, 130, 200, 1024, 1500])
def test_quad_id_has_no_tile_block_or_half_tile_alias(B):
    qid = quad_id(B)
    assert qid.shape == (B,) and set(qid.tolist()) == set(range(N_QUADS))
    for b in range(B):
        assert qid[b] == (b + 2 * (b // 64) + b // 256) % 7
        for s in ALIAS_SHIFTS:
            if b - s >= 0:
                assert qid[b] != qid[b - s], (b, s)
        if (b ^ 32) < B:
            assert qid[b] != qid[b ^ 32], b
    blk, qid2 = noise_block(B)
    assert blk.shape == (4, B) and blk.flags.c_contiguous and np.array_equal(qid, qid2)
    assert np.array_equal(blk[:, B - 1], noise_quadruples()[qid[B - 1]])


def _pair(oracle, w):
    vec, quat, P0 = w.initial_state()
    P0 = P0 + random_spd(w.n, w.B, 0.03, 3)
    if w.n == 21:
        vec[15:18], vec[18:21] = 0.5 * w.bg, 0.5 * w.ba
    v21, P21 = embed21(vec, P0)
    return oracle.OracleBatch(v21, quat, P21), oracle.OracleBatch(v21, quat, P21), P0


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip((a.vec, a.quat, a.cov_cm, a.ll), (b.vec, b.quat, b.cov_cm, b.ll)))


@pytest.mark.parametrize("n", [15, 21])
def test_grouped_oracle_with_equal_quadruples_is_the_plain_oracle(oracle, n):
    """Seven groups (quad_id) that all carry the SAME quadruple: per_filter_oracle (predict), per_filter_run_legodo and the grouped
    backward pass give the whole-batch oracle's results bit for bit -- the grouping itself changes nothing."""
    B, T, dt = 70, 6, 1e-3
    w = Workload(B, n_states=n)
    q4 = noise_quadruples()[0]
    blk = np.repeat(q4[:, None], B, axis=1)
    groups = quad_id(B)
    assert len(set(groups.tolist())) == N_QUADS
    # predict
    plain, grouped, P0 = _pair(oracle, w)
    for k in range(3):
        imu = w.imu_block(k)
        plain.predict(imu, q4)
        per_filter_oracle(grouped, blk, lambda q: grouped.predict(imu, q), groups=groups)
    assert _same(plain, grouped)
    assert not np.array_equal(plain.cov, _pair(oracle, w)[0].cov)
    # run_legodo
    imu, lo, mask = w.streams(0, T)
    plain.run_legodo(imu, lo, mask, q4)
    per_filter_run_legodo(oracle, grouped, imu, lo, mask, blk, groups=groups)
    assert _same(plain, grouped)
    sub = oracle_columns(oracle, plain, np.array([5, 69]))
    assert sub.B == 2 and np.array_equal(sub.cov[:, :, 1], plain.cov[:, :, 69])
    # the smoother's forward and backward pass
    keep = {0, 2, T - 2}
    want = oracle_backward_pass(oracle, w, n, T, B, dt, keep, q4=q4, P0=P0)
    got = per_filter_oracle_columns(blk, lambda cols, q: oracle_backward_pass(oracle, w, n, T, len(cols), dt, keep, q4=q, cols=cols, P0=P0),
                                    groups=groups)
    assert set(got) == keep
    for k in keep:
        for a, b in zip(got[k], want[k]):
            assert not np.any(np.isnan(a)) and a.tobytes() == np.ascontiguousarray(b).tobytes(), k


def test_grouped_oracle_with_different_quadruples_differs_per_group(oracle):
    """... and with the seven quadruples the groups DO differ: each filter equals the whole-batch oracle run with ITS quadruple."""
    B, n = 70, 21
    w = Workload(B, n_states=n)
    blk, qid = noise_block(B)
    _, grouped, _ = _pair(oracle, w)
    imu = w.imu_block(0)
    per_filter_oracle(grouped, blk, lambda q: grouped.predict(imu, q))
    for g, q4 in enumerate(noise_quadruples()):
        plain, _, _ = _pair(oracle, w)
        plain.predict(imu, q4)
        sel = qid == g
        assert np.array_equal(grouped.cov[:, :, sel], plain.cov[:, :, sel])
        assert not np.array_equal(grouped.cov[:, :, ~sel], plain.cov[:, :, ~sel])
