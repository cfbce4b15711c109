"""TEST-ONLY helpers for runs with a per-filter process noise (pb_set_process_noise_block, [4][B] = q_gyro, q_accel, q_gyro_bias,
q_accel_bias per filter): seven quadruples that tell the four rows apart, an assignment of them to filters that no tile, block or
half-tile alias maps onto itself, and the oracle driven group by group -- it takes one q for the whole batch."""
import numpy as np

N_QUADS = 7


def noise_quadruples(smoothable=False):
    """[7, 4]: (q_gyro, q_accel, q_gyro_bias, q_accel_bias).  Across the seven the four rows are pairwise non-proportional (a row read
    in another's place, or taken from a scalar, changes the result), the entries span three decades, every row has an exact 0, and
    quadruples 2 and 3 differ in rows 2 / 3 only (15 states must not tell them apart, 21 states must).
    smoothable: the zeros of q_gyro and q_accel replaced by 2e-4 / 6e-4, for runs that are smoothed afterwards.  The process step SETS
    the angular-velocity and acceleration blocks of the covariance to q_gyro I and q_accel I (rbis.cpp:120-121), and the RTS step
    solves with that predicted covariance (rbis.cpp:244-251, .ldlt().solve): with a zero there it is singular and the smoothed
    posterior is whatever the factorisation's pivoting makes of 0 / 0 -- in the reference, the oracle and the kernels alike."""
    Q = np.array([[6e-5, 1.5e-2, 3e-3, 2e-2],
                  [1e-3, 1e-4, 5e-2, 1e-3],
                  [2e-2, 5e-2, 0.0, 4e-3],
                  [2e-2, 5e-2, 6e-3, 0.0],
                  [0.0, 3e-3, 1e-4, 8e-2],
                  [4e-3, 0.0, 2e-2, 3e-4],
                  [3e-4, 8e-2, 7e-4, 1e-1]])
    assert Q[4, 0] == 0.0 and Q[5, 1] == 0.0
    if smoothable:
        Q[4, 0], Q[5, 1] = 2e-4, 6e-4
    assert Q.shape == (N_QUADS, 4) and np.all(Q >= 0.0)
    for i in range(4):
        assert np.any(Q[:, i] == 0.0) != (smoothable and i < 2), i
        for j in range(i):   # not proportional: the 2 x 2 minors of the two rows do not all vanish
            minors = np.outer(Q[:, i], Q[:, j]) - np.outer(Q[:, j], Q[:, i])
            assert np.max(np.abs(minors)) > 1e-3 * np.max(Q[:, i]) * np.max(Q[:, j]), (i, j)
    nz = Q[Q > 0.0]
    assert 1e3 <= nz.max() / nz.min() <= 1e4
    assert np.array_equal(Q[2, :2], Q[3, :2]) and Q[2, 2] != Q[3, 2] and Q[2, 3] != Q[3, 3]
    assert len({tuple(r) for r in Q}) == N_QUADS
    return Q


ALIAS_SHIFTS = (64, 256, 512, 768)   # a tile; one, two and three blocks of 256 (the cache-blocked order of the bulk run)


def quad_id(B):
    """filter -> quadruple.  A filter and the filter a wrong offset would read in its place -- a tile back, one to three blocks of 256
    back, the other half of its tile (b ^ 32) -- never share a quadruple."""
    b = np.arange(B)
    qid = (b + 2 * (b // 64) + b // 256) % N_QUADS
    for s in ALIAS_SHIFTS:
        assert np.all(qid[s:] != qid[:B - s] if B > s else True), s
    half = b ^ 32
    ok = half < B
    assert np.all(qid[b[ok]] != qid[half[ok]])
    return qid


def noise_block(B, smoothable=False):
    """(q_block [4, B] C-contiguous, quad_id [B]); smoothable: see noise_quadruples"""
    qid = quad_id(B)
    return np.ascontiguousarray(noise_quadruples(smoothable)[qid].T), qid


def oracle_noise_block(q_block, n):
    """the block the ORACLE is stepped with for an n-state filter.  The oracle always carries 21 states; it stands in for a 15-state
    filter only with its bias states switched off -- zero variance (util.embed21) AND zero bias process noise (as
    Workload.process_noise() gives for 15 states): a bias variance grown by rows 2 / 3 would reach chi and the velocity through Ad
    from the second step on (2e-8 of max|P| after six steps with these quadruples).  The device gets the block as it is."""
    q = np.array(q_block, dtype=np.float64)
    if n == 15:
        q[2:4] = 0.0
    return q


def masked_oracle_step(ob, valid, fn):
    """fn() on every column of the oracle batch, then the columns without a message put back: their estimator did nothing"""
    keep = [a.copy() for a in (ob.vec, ob.quat, ob.cov_cm, ob.ll)]
    fn()
    idle = np.asarray(valid) == 0
    ob.vec[:, idle], ob.quat[:, idle], ob.cov_cm[:, :, idle], ob.ll[idle] = keep[0][:, idle], keep[1][:, idle], keep[2][:, :, idle], keep[3][idle]


def _groups(q_block, groups):
    """-> [(q4, member mask [B])]: one entry per group id (default: per distinct column of q_block); a group's columns must agree"""
    q_block = np.asarray(q_block, dtype=np.float64)
    if groups is None:
        groups = np.unique(q_block.T, axis=0, return_inverse=True)[1].reshape(-1)
    out = []
    for g in np.unique(groups):
        sel = np.asarray(groups) == g
        q4 = q_block[:, np.argmax(sel)].copy()
        assert np.all(q_block[:, sel] == q4[:, None]), g
        out.append((q4, sel))
    return out


def per_filter_oracle(ob, q_block, fn, groups=None):
    """One step of the oracle batch `ob` with a process noise per filter: fn(q4) -- a step of the WHOLE batch, e.g.
    lambda q4: ob.predict(imu, q4) -- once per distinct column of q_block [4, B], only that group's columns kept
    (masked_oracle_step).  groups [B]: group ids to use instead of the distinct columns."""
    for q4, sel in _groups(q_block, groups):
        masked_oracle_step(ob, sel, lambda: fn(q4))


def _scatter(dst, src, cols, B):
    """src: ndarrays with the filters (len(cols)) on the last axis, nested in tuples / lists / dicts -> the same nest at B filters"""
    if isinstance(src, dict):
        dst = {} if dst is None else dst
        for k, v in src.items():
            dst[k] = _scatter(dst.get(k), v, cols, B)
        return dst
    if isinstance(src, (tuple, list)):
        dst = [None] * len(src) if dst is None else list(dst)
        return type(src)(_scatter(d, s, cols, B) for d, s in zip(dst, src))
    src = np.asarray(src)
    assert src.shape[-1] == len(cols), src.shape
    if dst is None:
        dst = np.full(src.shape[:-1] + (B,), np.nan, dtype=src.dtype)
    dst[..., cols] = src
    return dst


def per_filter_oracle_columns(q_block, fn, groups=None):
    """A whole-trajectory oracle routine with a process noise per filter: fn(cols, q4) runs the routine on the filters `cols` alone
    (the caller slices its inputs) and returns arrays with those filters on the last axis, nested in tuples / lists / dicts; the
    results of all groups scattered back to B filters.  Every filter is in exactly one group, so nothing is left unset."""
    B = np.asarray(q_block).shape[1]
    out = None
    for q4, sel in _groups(q_block, groups):
        cols = np.nonzero(sel)[0]
        out = _scatter(out, fn(cols, q4), cols, B)
    return out


def oracle_columns(oracle, ob, cols):
    """the filters `cols` of an oracle batch as a batch of their own"""
    return oracle.OracleBatch(ob.vec[:, cols], ob.quat[:, cols], ob.cov[:, :, cols], ob.ll[cols])


def per_filter_run_legodo(oracle, ob, imu, lo, mask, q_block, groups=None):
    """ob.run_legodo over the streams imu [T,7,B], lo [T,6,B], mask [T,B] with q_block's noise per filter, group by group"""
    def run(cols, q4):
        sub = oracle_columns(oracle, ob, cols)
        sub.run_legodo(np.ascontiguousarray(imu[:, :, cols]), np.ascontiguousarray(lo[:, :, cols]), np.ascontiguousarray(mask[:, cols]), q4)
        return sub.vec, sub.quat, sub.cov_cm, sub.ll
    v, q, Pcm, ll = per_filter_oracle_columns(q_block, run, groups)
    ob.vec[:], ob.quat[:], ob.cov_cm[:], ob.ll[:] = v, q, Pcm, ll
