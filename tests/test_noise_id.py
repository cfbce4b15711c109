"""Noise identification (state-estimator/src/noise_id/noise_id.cpp:9-65): windowed predict-only
roll-forward from logged filter states + likelihood of the end-of-window error.  One GPU batch carries the whole
windows x candidate-noise grid (per-filter process noise); by linearity rolled_cov - start_window_cov is the predict
chain from P = 0, which the oracle's literal two-covariance restatement confirms."""
import numpy as np
import pytest

from pronto_amd.synth import Workload

ACTIVE = [3, 4, 5, 6, 7, 8, 9, 10, 11]   # roll_forward.cpp:52-57: velocity, chi, position


def make_history(T, seed=0):
    """A logged 'truth' filter history for one run: vec [T+1,21] (omega, accel filled in), quat [T+1,4]."""
    w = Workload(1, b0=seed, n_states=15)
    vec = np.zeros((T + 1, 21))
    quat = np.zeros((T + 1, 4))
    for k in range(T + 1):
        tr = w.truth(w.time_s(k))
        vec[k, 0:3] = tr["omega"][:, 0]
        vec[k, 3:6] = tr["vel_b"][:, 0]
        vec[k, 9:12] = tr["pos"][:, 0]
        vec[k, 12:15] = tr["f_b"][:, 0]
        quat[k] = tr["quat"][:, 0]
    return vec, quat


def test_oracle_noise_id_linearity_and_likelihood(oracle):
    """rolled_cov - start_window_cov does not depend on the start covariance (it is the accumulated process noise)."""
    vec, quat = make_history(40)
    P0 = np.diag(np.r_[np.zeros(3), np.full(9, 0.01), np.zeros(9)])
    e1, c1, ld1, mh1, ll1 = oracle.noise_id_window(vec, quat, P0, 1e-3, 7.6e-5, 1e-2, ACTIVE)
    e2, c2, ld2, mh2, ll2 = oracle.noise_id_window(vec, quat, np.zeros((21, 21)), 1e-3, 7.6e-5, 1e-2, ACTIVE)
    assert np.max(np.abs(c1 - c2)) < 1e-15 * max(1.0, np.max(np.abs(P0))) + 1e-12 * np.max(np.abs(c2))
    assert np.allclose(e1, e2, atol=0) and abs(ll1 - ll2) < 1e-6 * abs(ll2)
    # likelihood pieces against numpy
    S = c2[np.ix_(ACTIVE, ACTIVE)]
    ea = e2[ACTIVE]
    assert np.isclose(ld2, np.linalg.slogdet(S)[1], rtol=1e-10)
    assert np.isclose(mh2, ea @ np.linalg.solve(S, ea), rtol=1e-8)
    assert np.isclose(ll2, -0.5 * (9 * np.log(2 * np.pi) + ld2 + mh2), rtol=1e-12)


@pytest.mark.gpu
def test_gpu_noise_id_grid_matches_oracle(oracle):
    import torch
    from pronto_amd.batch import BatchEstimator
    T, NW, Nwin = 120, 6, 20                      # 6 windows of 20 steps
    q_grid = [(7.6e-5, 1e-2), (3e-4, 4e-2), (1e-5, 2.5e-3)]
    vec, quat = make_history(T, seed=5)
    B = NW * len(q_grid)
    win = np.repeat(np.arange(NW), len(q_grid))   # filter b -> window
    cand = np.tile(np.arange(len(q_grid)), NW)    # filter b -> candidate
    est = BatchEstimator(B, n_states=15)
    est.set_constants(*oracle.constants())
    start = win * Nwin
    x0 = np.ascontiguousarray(vec[start, :15].T)
    q0 = np.ascontiguousarray(quat[start].T)
    est.reset(x0, q0, np.zeros((15, 15, B)))      # P = 0: the chain IS rolled_cov - start_window_cov
    qblk = np.zeros((4, B))
    qblk[0] = [q_grid[c][0] for c in cand]
    qblk[1] = [q_grid[c][1] for c in cand]
    d_q = torch.from_numpy(qblk).to("cuda:0")
    est.set_process_noise_block(d_q)
    for ii in range(Nwin):
        k = start + ii
        imu = np.zeros((7, B))
        imu[0:3] = vec[k, 0:3].T                  # truth omega and accel drive the roll-forward (noise_id.cpp:26)
        imu[3:6] = vec[k, 12:15].T
        imu[6] = 1e-3
        est.predict(imu, [0, 0, 0, 0])            # scalar q ignored while the block is set
    est.set_process_noise_block(None)
    end = start + Nwin
    out, err = est.window_nll(ACTIVE, np.ascontiguousarray(vec[end, :15].T), np.ascontiguousarray(quat[end].T), want_err=True)
    v, q, P, ll = est.get_head()
    for b in range(B):
        s = start[b]
        P0 = np.diag(np.r_[np.zeros(3), np.full(9, 0.02), np.zeros(9)])   # any start covariance: it cancels
        e, c, ld, mh, lk = oracle.noise_id_window(vec[s:s + Nwin + 1], quat[s:s + Nwin + 1], P0, 1e-3, *q_grid[cand[b]], ACTIVE)
        assert np.max(np.abs(P[:, :, b] - c[:15, :15])) < 1e-9 * np.max(np.abs(c))
        assert np.max(np.abs(err[:, b] - e[:15])) < 1e-9 * max(np.max(np.abs(e)), 1e-6)
        assert np.isclose(out[0, b], ld, rtol=1e-8) and np.isclose(out[1, b], mh, rtol=1e-6) and np.isclose(out[2, b], lk, rtol=1e-6)
    # the candidates rank differently: the likelihood is a usable objective
    tot = [out[2, cand == c].sum() for c in range(len(q_grid))]
    assert len(set(np.round(tot, 6))) == len(q_grid)


# ---------------------------------------------------------------- pb_window_nll against a 60-digit reference ----
NLL_B = 130                 # two waves and a two-lane tail
NLL_BINS = 5                # 26 filters each, one condition-number range per bin (the batch is ordered by condition number)
NLL_IDX = {15: {1: [7], 3: [4, 6, 11], 6: [9, 3, 8, 5, 10, 6], 9: ACTIVE},
           21: {1: [16], 3: [5, 8, 19], 6: [10, 3, 7, 15, 20, 6], 9: [3, 6, 7, 8, 9, 11, 16, 18, 20]}}
NLL_NEAR_PI = np.pi - 1e-6
_NLL_CACHE = {}


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def nll_inputs(n, B=NLL_B):
    """(vec [n,B], quat [4,B], P [n,n,B], truth_vec, truth_quat): dense SPD P = Q diag(lambda) Q^T * scale with condition numbers
    1e2 ... 1e10 in filter order and scales 1e-3 ... 1 (every principal minor of up to nine rows stays a normal number: > 1e-117);
    head and truth quaternions of either sign; truth = head (-) an error of ~0.1 per entry, the rotation between truth and head
    ~0.05 rad, for every 13th filter pi - 1e-6 about a random axis."""
    rng = np.random.default_rng(770 + n)
    vec = rng.normal(size=(n, B))
    quat = rng.normal(size=(4, B))
    quat /= np.linalg.norm(quat, axis=0)
    quat[:, rng.random(B) < 0.5] *= -1.0
    cond = np.geomspace(1e2, 1e10, B)
    P = np.empty((n, n, B))
    for b in range(B):
        Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
        A = (Q * np.geomspace(1.0, 1.0 / cond[b], n)) @ Q.T * 10.0 ** rng.uniform(-3, 0)
        P[:, :, b] = 0.5 * (A + A.T)
    tvec = vec - 0.1 * rng.normal(size=(n, B))
    tquat = np.empty((4, B))
    near_pi = np.arange(B) % 13 == 5
    for b in range(B):
        d = rng.normal(size=3)
        d *= (NLL_NEAR_PI if near_pi[b] else 0.05 * (1 + rng.random())) / np.linalg.norm(d)
        a = np.linalg.norm(d)
        tquat[:, b] = _quat_mul(quat[:, b], np.r_[np.cos(a / 2), -np.sin(a / 2) * d / a])     # truth^-1 * head = exp(d)
    tquat[:, np.arange(B) % 3 == 1] *= -1.0
    return np.ascontiguousarray(vec), np.ascontiguousarray(quat), P, np.ascontiguousarray(tvec), np.ascontiguousarray(tquat), near_pi


def nll_reference(v, q, P, tv, tq, idx):
    """logdet, Mahalanobis distance, -0.5 (m log 2 pi + logdet + maha) and the error vector of every filter in mpmath at 60 digits from
    the float64 inputs as they are: chi = Log(truth^-1 * head) as eigen_utils::subtractQuats (angle = 2 atan2(|vec|, |w|), the axis
    flipped for w < 0).  -> (out [3][B], err [n][B]) as lists of mpf."""
    import mpmath as mp
    n, B = v.shape
    m = len(idx)
    out, err = [[None] * B for _ in range(3)], [[None] * B for _ in range(n)]
    with mp.workdps(60):
        for b in range(B):
            h, t = [mp.mpf(float(x)) for x in q[:, b]], [mp.mpf(float(x)) for x in tq[:, b]]
            t2 = sum(x * x for x in t)
            ti = [t[0] / t2, -t[1] / t2, -t[2] / t2, -t[3] / t2]
            r = [ti[0] * h[0] - ti[1] * h[1] - ti[2] * h[2] - ti[3] * h[3], ti[0] * h[1] + ti[1] * h[0] + ti[2] * h[3] - ti[3] * h[2],
                 ti[0] * h[2] - ti[1] * h[3] + ti[2] * h[0] + ti[3] * h[1], ti[0] * h[3] + ti[1] * h[2] - ti[2] * h[1] + ti[3] * h[0]]
            nv = mp.sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3])
            angle = 2 * mp.atan2(nv, abs(r[0]))
            assert nv > 0 and angle < mp.pi
            f = (-angle if r[0] < 0 else angle) / nv
            e = [mp.mpf(float(v[i, b])) - mp.mpf(float(tv[i, b])) for i in range(n)]
            e[6:9] = [r[1] * f, r[2] * f, r[3] * f]
            for i in range(n):
                err[i][b] = e[i]
            S = mp.matrix(m, m)
            for i in range(m):
                for j in range(m):
                    S[i, j] = mp.mpf(float(P[idx[i], idx[j], b]))
            ea = mp.matrix([e[i] for i in idx])
            det = mp.det(S)
            assert det > mp.mpf(2) ** -1022                               # a normal float64 number
            logdet = mp.log(det)
            maha = (ea.T * mp.lu_solve(S, ea))[0]
            out[0][b], out[1][b], out[2][b] = logdet, maha, -(m * mp.log(2 * mp.pi) + logdet + maha) / 2
    return out, err


def nll_errors(got_out, got_err, ref):
    """per filter: the error of logdet and of the likelihood relative to max(|ref|, 1) (they live in the log domain: a relative error
    delta of the determinant is an absolute delta here), of the Mahalanobis distance relative to |ref|, of the error vector relative to
    its largest entry -> {piece: [B]}"""
    import mpmath as mp
    ref_out, ref_err = ref
    B = len(ref_out[0])
    res = {}
    with mp.workdps(60):
        for row, name, floor in ((0, "logdet", 1), (1, "maha", 0), (2, "nll", 1)):
            res[name] = np.array([float(abs(mp.mpf(float(got_out[row, b])) - ref_out[row][b]) / max(abs(ref_out[row][b]), floor)) for b in range(B)])
        if got_err is not None:
            n = len(ref_err)
            res["err"] = np.array([float(max(abs(mp.mpf(float(got_err[i, b])) - ref_err[i][b]) for i in range(n)) /
                                         max(abs(ref_err[i][b]) for i in range(n))) for b in range(B)])
    return res


def oracle_nll(oracle, v, q, P, tv, tq, idx):
    """the same pieces from the oracle: po_subtract_quats for chi, po_loglike_pieces (pivoted LDL^T solve, LU determinant)"""
    import ctypes as C
    L = oracle.lib()
    n, B = v.shape
    out, err = np.empty((3, B)), np.empty((n, B))
    ia = (C.c_int * len(idx))(*idx)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for b in range(B):
        e = v[:, b] - tv[:, b]
        chi = np.zeros(3)
        L.po_subtract_quats(dp(np.ascontiguousarray(q[:, b])), dp(np.ascontiguousarray(tq[:, b])), dp(chi))
        e[6:9] = chi
        err[:, b] = e
        es, cov = oracle.Rbis(), oracle.Rbim()
        es.vec[:] = list(np.r_[e, np.zeros(21 - n)])
        P21 = np.zeros((21, 21))
        P21[:n, :n] = P[:, :, b]
        cov.m[:] = list(np.ascontiguousarray(P21.T).ravel())
        ld, mh = C.c_double(), C.c_double()
        out[2, b] = L.po_loglike_pieces(len(idx), ia, C.byref(es), C.byref(cov), C.byref(ld), C.byref(mh))
        out[0, b], out[1, b] = ld.value, mh.value
    return out, err


def test_nll_reference_on_a_case_with_a_known_answer():
    """the 60-digit reference itself: P = diag, head = truth rotated by a known angle about z"""
    v, tv = np.zeros((15, 1)), np.zeros((15, 1))
    v[3, 0], tv[3, 0] = 0.5, 0.25
    P = np.zeros((15, 15, 1))
    P[:, :, 0] = np.diag(np.arange(1.0, 16.0))
    q, tq = np.array([[np.cos(0.2)], [0.0], [0.0], [np.sin(0.2)]]), -np.array([[1.0], [0.0], [0.0], [0.0]])
    out, err = nll_reference(v, q, P, tv, tq, [3, 8])
    assert abs(float(err[8][0]) - 0.4) < 1e-15 and float(err[6][0]) == 0.0 and float(err[3][0]) == 0.25     # (truth = -identity: w < 0, the same rotation)
    assert abs(float(out[0][0]) - np.log(4.0 * 9.0)) < 1e-14 and abs(float(out[1][0]) - (0.0625 / 4 + 0.16 / 9)) < 1e-15
    e = nll_errors(np.array([[np.log(36.0)], [0.0625 / 4 + 0.16 / 9], [0.0]]), None, (out, err))
    assert e["logdet"][0] < 1e-15 and e["maha"][0] < 1e-14 and e["nll"][0] > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 3, 6, 9])
@pytest.mark.parametrize("n", [15, 21])
def test_window_nll_against_a_60_digit_reference(oracle, n, m):
    """pb_window_nll on heads set directly (pb_reset): 130 filters with dense SPD covariances of condition number 1e2 ... 1e10, head and
    truth quaternions of either sign, every 13th chi residual at pi - 1e-6; index lists that mix velocity, chi and position (21 states:
    bias rows too), m = 1, 3, 6, 9; truth from the host and from the device; err_out NULL and given.  Reference: mpmath at 60 digits
    on the head as pb_get_head returns it.

    Bound, per piece and per bin of 26 filters (one range of condition numbers each): 16 x the oracle's own worst error in that bin
    against the same reference (po_loglike_pieces: pivoted LDL^T solve, LU determinant; the kernel: unpivoted LDL^T -- both backward
    stable on SPD matrices, the factor covers the operation order for m <= 9) + 1e-13.  logdet and the likelihood are measured
    relative to max(|ref|, 1), the Mahalanobis distance relative to |ref|, the error vector relative to its largest entry.

    Measured on an MI355X, the bin of the worst conditioned filters (cond 2.5e8 ... 1e10), oracle / kernel; host and device buffers
    and both err_out variants gave the same figures:
      n  m   logdet                maha                  likelihood            error vector
      15 1   1.0e-16 / 1.0e-16     2.2e-14 / 3.4e-14     2.2e-14 / 8.5e-15     1.6e-15 / 8.5e-16
      15 3   7.4e-16 / 1.6e-15     1.0e-14 / 4.5e-14     3.9e-14 / 4.5e-14     1.6e-15 / 8.5e-16
      15 6   3.9e-14 / 3.1e-14     1.3e-12 / 1.1e-12     1.3e-12 / 1.1e-12     1.6e-15 / 8.5e-16
      15 9   1.2e-12 / 9.3e-13     4.6e-11 / 1.1e-10     4.6e-11 / 1.1e-10     1.6e-15 / 8.5e-16
      21 1   8.7e-17 / 8.7e-17     1.5e-16 / 1.8e-16     4.3e-16 / 4.3e-16     1.6e-15 / 7.2e-16
      21 3   1.9e-16 / 3.9e-16     3.0e-15 / 9.1e-15     8.7e-15 / 1.6e-14     1.6e-15 / 7.2e-16
      21 6   3.9e-15 / 1.5e-15     4.3e-14 / 8.0e-14     4.3e-14 / 8.0e-14     1.6e-15 / 7.2e-16
      21 9   2.2e-14 / 3.2e-14     2.7e-12 / 2.5e-12     2.8e-12 / 2.5e-12     1.6e-15 / 7.2e-16
    (the test prints every bin of every variant before it asserts)
    """
    import torch
    from pronto_amd.batch import BatchEstimator
    B = NLL_B
    idx = NLL_IDX[n][m]
    assert len(idx) == m and (n == 15 or m == 1 or any(i >= 15 for i in idx))
    vec, quat, P, tvec, tquat, near_pi = nll_inputs(n)
    est = BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    est.reset(vec, quat, P)
    v, q, Ph, _ = est.get_head()
    Ph = np.ascontiguousarray(Ph)
    key = (n, m)
    if key not in _NLL_CACHE:
        ref = nll_reference(v, q, Ph, tvec, tquat, idx)
        o_out, o_err = oracle_nll(oracle, v, q, Ph, tvec, tquat, idx)
        _NLL_CACHE[key] = (ref, nll_errors(o_out, o_err, ref))
    ref, o_e = _NLL_CACHE[key]
    chi = np.array([[float(x) for x in ref[1][i]] for i in (6, 7, 8)])
    assert np.all(np.abs(np.linalg.norm(chi[:, near_pi], axis=0) - NLL_NEAR_PI) < 1e-9) and near_pi.sum() == 10
    bins = np.array_split(np.arange(B), NLL_BINS)
    for mem in ("host", "device"):
        for want_err in (False, True):
            tv, tq = (tvec, tquat) if mem == "host" else (torch.from_numpy(tvec).to("cuda:0"), torch.from_numpy(tquat).to("cuda:0"))
            res = est.window_nll(idx, tv, tq, want_err=want_err)
            est.sync()
            out, err = res if want_err else (res, None)
            if mem == "device":
                out, err = out.cpu().numpy(), (err.cpu().numpy() if want_err else None)
            k_e = nll_errors(out, err, ref)
            for piece, ke in k_e.items():
                for i, sel in enumerate(bins):
                    print("n=%d m=%d %s err_out=%d %-6s bin %d: oracle %.2e kernel %.2e" % (n, m, mem, want_err, piece, i, o_e[piece][sel].max(), ke[sel].max()))
            for piece, ke in k_e.items():
                for i, sel in enumerate(bins):
                    assert ke[sel].max() <= 16.0 * o_e[piece][sel].max() + 1e-13, (mem, want_err, piece, i, ke[sel].max(), o_e[piece][sel].max())
    est.close()
