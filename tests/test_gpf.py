"""The GPF measurement on the device (pb_gpf_*, pronto_amd/csrc/rbis_gpf_kernels.hpp) -- run with `-m gpu` on an MI355X.

  normals      the device's numbers against numpy on the same Philox words (1e-12), moments over 70 x 4096, reproducibility
  sample       pb_gpf_sample against the exact L xi and the composed pose (gpf_ref.check: 16 x the numpy witness's error + 1e-13), one
               filter whose chi perturbation stays below the fold tolerance, one with a zeroed covariance.  The 60-digit judgement
               (of delta, the pose and the chi fold) covers the first 20 and the last 4 samples of every filter -- both sides of the
               16-sample chunk boundary and the ragged last chunk; every other sample is held to the numpy witness at 1e-12
               absolute (both are a few ulps of an m-term product of values below 10; a wrong index moves a sample by order sigma)
  measurement  pb_gpf_measurement against 60-digit arithmetic on the device's own delta block, all three statuses in one batch, a NaN
               log-likelihood, two runs bit for bit; K = 5 and 6 (an empty quarter, a quarter of one sample)
  chain        gpf_update (sample -> torch Gaussian log-likelihood -> measurement -> update_indexed_wide) against the witness's
               posterior through update_exact; a masked-off filter keeps its state bit for bit
  grid         the built-in voxel-grid likelihood with per-filter and with broadcast points against the numpy witness
  edges        refused arguments
B = 70: one full tile and a ragged tail of 6."""
import ctypes as C

import numpy as np
import pytest

import gpf_ref as gr
import update_exact as ue
from test_gpf_host import grid_case
from test_gpu_parity import pa  # noqa: F401  (the module fixture that builds and imports the package)

pytestmark = pytest.mark.gpu

B = 70
BRANCH = {58: "flat", 59: "flat", 60: "spike", 61: "anti", 62: "anti", 63: "nan", 64: "anti", 66: "flat", 68: "anti", 69: "spike"}
NS = [15, 21]
# The seed of each (n, m) draw of the measurement test.  The input conditions (gpf_ref.assert_input_conditions) are asserted on every
# run; these are draws that meet them -- with 70 filters a draw often holds one whose weight sum lies within a few percent of a bound.
# Each is the FIRST seed from 2 upwards whose numpy witness met the conditions with a margin of 5 % on W and a factor 3 on the
# eigenvalues, for all 70 filters: 1 seed tried for seven of the ten cases, 2 for (21, 4), 3 for (15, 6), 7 for (15, 1), 41 for (21, 1).
# One row is the hard case: with a likelihood twice as wide as the prior W / K is 0.89 in expectation, a hair under the 0.9 the issue
# asks for.  Filters AT a weight-sum bound are the subject of test_weight_sum_bounds_are_strict (W = 5 m and W = K exactly).
SEEDS = {(15, 1): 8, (15, 3): 2, (15, 4): 2, (15, 6): 4, (15, 9): 2, (21, 1): 42, (21, 3): 2, (21, 4): 3, (21, 6): 2, (21, 9): 2}


def _estimator(pa, oracle, n, h):
    est = pa.BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    est.reset(h["vec"], h["quat"], np.ascontiguousarray(h["P"]))
    return est


def _np(t):
    return t.cpu().numpy()


def test_normals(pa, oracle):
    import torch
    h = gr.heads(15, [11], B, 1)
    est = _estimator(pa, oracle, 15, h)
    seed = 0xC0FFEE1234567
    small = _np(est.gpf_normals(seed, 5, 7))
    assert np.max(np.abs(small - gr.normals_ref(seed, 5, 7, B))) <= 1e-12
    a = est.gpf_normals(seed, 5, 4096)
    x = _np(a)
    assert np.array_equal(x[:7], small)                         # a row does not depend on how many rows are asked for
    assert abs(x.mean()) < 0.01 and abs(x.var() - 1.0) < 0.01
    assert len(np.unique(x.T, axis=0)) == B and len(np.unique(x, axis=0)) == 4096
    assert torch.equal(a, est.gpf_normals(seed, 5, 4096))
    assert not np.any(_np(est.gpf_normals(seed, 6, 4096)) == x)
    est.close()


def _special_heads(n, idx):
    h = gr.heads(n, idx, B, 1)
    h["P"][:, :, 67] = 0.0                                  # Sigma_bar not positive definite (in the ragged tail)
    h["P"][6:9, :, 33] *= 1e-8                              # chi perturbations below the fold tolerance
    h["P"][:, 6:9, 33] *= 1e-8
    return h


@pytest.mark.parametrize("m,K", gr.CASES + [(3, 5), (3, 6)])
@pytest.mark.parametrize("n", NS)
def test_sample_against_exact_arithmetic(pa, oracle, n, m, K):
    idx = gr.LISTS[m]
    h = _special_heads(n, idx)
    tol = oracle.constants()[1]
    est = _estimator(pa, oracle, n, h)
    xi_t = est.gpf_normals(11, m, K * m).view(K, m, B)
    delta, pose = est.gpf_sample(idx, xi_t)
    xi, gd, gp = _np(xi_t), _np(delta), _np(pose)
    est.close()
    ks = sorted(set(list(range(min(20, K))) + list(range(max(K - 4, 0), K))))
    ed, ep = gr.exact_sample(h, idx, xi, tol, ks)
    wd, wp = gr.witness_sample(h, idx, xi, tol)
    assert np.all(gd[:, :, 67] == 0.0) and np.all(gp[:, :3, 67] == h["vec"][9:12, 67]) and np.all(gp[:, 3:, 67] == h["quat"][:, 67])
    if 6 in idx:
        assert np.all(gp[:, 3:, 33] == h["quat"][:, 33]) and not np.all(gp[:, 3:, 0] == h["quat"][:, 0])
    gr.check("k_gpf_sample<%d,%d> K=%d" % (n, m, K), gr.sample_errors(gd[ks], gp[ks], ed, ep), gr.sample_errors(wd[ks], wp[ks], ed, ep),
             [np.arange(B)])
    assert np.max(np.abs(gd - wd)) <= 1e-12 and np.max(np.abs(gp - wp)) <= 1e-12


@pytest.mark.parametrize("m,K", gr.CASES)
@pytest.mark.parametrize("n", NS)
def test_measurement_against_exact_arithmetic(pa, oracle, n, m, K):
    import torch
    idx = gr.LISTS[m]
    seed = SEEDS[n, m]
    h = gr.heads(n, idx, B, seed)
    est = _estimator(pa, oracle, n, h)
    delta, _ = est.gpf_sample(idx, np.random.default_rng([seed, m, n]).normal(size=(K, m, B)))
    gd = _np(delta)
    ll = gr.gaussian_loglik(h, idx, gd, seed, BRANCH)
    z, R, status = est.gpf_measurement(idx, delta, ll)
    z2, R2, status2 = est.gpf_measurement(idx, delta, torch.as_tensor(ll))
    est.close()
    assert torch.equal(z, z2) and torch.equal(R, R2) and torch.equal(status, status2)
    Sig, xm = gr.sigma_bar(h, idx), np.ascontiguousarray(h["vec"][idx])
    ex = gr.exact_fit(Sig, xm, gd, ll)
    normal = [b for b in range(B) if b not in BRANCH]
    gr.assert_input_conditions(ex, m, K, normal, [b for b, k in BRANCH.items() if k == "anti"])
    assert all(ex["status"][b] == 2 for b, k in BRANCH.items() if k in ("flat", "spike", "nan"))
    assert set(ex["status"]) == {0, 1, 2}
    wz, wR, ws = gr.witness_fit(Sig, xm, gd, ll)
    assert np.array_equal(ws, ex["status"])
    assert np.array_equal(_np(status), ex["status"]), (_np(status), ex["status"])
    Rg = gr.r_cols(_np(R), m)
    assert np.array_equal(Rg, Rg.transpose(0, 2, 1))
    gr.check("k_gpf_fit<%d,%d> K=%d" % (n, m, K), gr.fit_errors(_np(z), Rg, ex), gr.fit_errors(wz, wR, ex), gr.cond_bins(ex))


@pytest.mark.parametrize("K", [5, 6])
def test_measurement_with_an_empty_or_single_sample_quarter(pa, oracle, K):
    """K = 5: the waves hold 2, 2, 1, 0 samples; K = 6: 2, 2, 2, 0.  5 m < W < K needs m = 1 and K = 6."""
    idx = [11]
    h = gr.heads(15, idx, B, 3)
    est = _estimator(pa, oracle, 15, h)
    delta, _ = est.gpf_sample(idx, est.gpf_normals(31, 0, K).view(K, 1, B))
    gd = _np(delta)
    ll = 0.05 * gr.gaussian_loglik(h, idx, gd, 5)
    z, R, status = est.gpf_measurement(idx, delta, ll)
    est.close()
    Sig, xm = gr.sigma_bar(h, idx), np.ascontiguousarray(h["vec"][idx])
    ex = gr.exact_fit(Sig, xm, gd, ll)
    wz, wR, ws = gr.witness_fit(Sig, xm, gd, ll)
    assert np.array_equal(_np(status), ex["status"]) and np.array_equal(ws, ex["status"])
    assert (K == 5 and np.all(ex["status"] == 2)) or (K == 6 and np.any(ex["status"] != 2))
    gr.check("k_gpf_fit<15,1> K=%d" % K, gr.fit_errors(_np(z), gr.r_cols(_np(R), 1), ex), gr.fit_errors(wz, wR, ex), [np.arange(B)])


def test_weight_sum_bounds_are_strict(pa, oracle):
    """flat log-likelihoods: W = K exactly.  K = 5 with one row: W = 5 m, not above it; max_weight_proportion = 1: W = K, not below it"""
    import torch
    h = gr.heads(15, [11], B, 3)
    est = _estimator(pa, oracle, 15, h)
    for K, mwp in ((5, 2.0), (96, 1.0)):
        delta, _ = est.gpf_sample([11], est.gpf_normals(5, 0, K).view(K, 1, B))
        z, R, status = est.gpf_measurement([11], delta, torch.zeros((K, B), dtype=torch.float64, device="cuda"), mwp)
        assert np.all(_np(status) == 2) and np.array_equal(_np(z), h["vec"][[11]]) and np.all(_np(R) == gr.R_FIX)
    est.close()


def test_chain_against_the_witness_posterior(pa, oracle):
    import torch
    n, m, K = 15, 3, 200
    idx = gr.LISTS[m]
    h = gr.heads(n, idx, B, 4)
    rng = np.random.default_rng(9)
    Sig = gr.sigma_bar(h, idx)
    centre, prec = np.empty((3, B)), np.empty((B, 3, 3))
    for b in range(B):
        Q, a = h["Q"][b], h["sigma"][b] * rng.uniform(1.0, 2.0, size=3)
        centre[:, b] = h["vec"][9:12, b] + 0.5 * np.linalg.cholesky(Sig[b]) @ rng.normal(size=3)
        prec[b] = (Q / a ** 2) @ Q.T
    ct, pt = torch.as_tensor(centre).cuda(), torch.as_tensor(prec).cuda()

    def loglik(pose):
        d = pose[:, :3, :] - ct[None]
        return -0.5 * torch.einsum("kib,bij,kjb->kb", d, pt, d).contiguous()

    est = _estimator(pa, oracle, n, h)
    prior = est.get_head()
    delta, pose = est.gpf_sample(idx, est.gpf_normals(77, 3, K * m).view(K, m, B))
    gd, ll = _np(delta), _np(loglik(pose))
    mask = np.ones(B, dtype=np.uint8)
    mask[41] = 0
    z, R, status = est.gpf_update(idx, K, loglik, 77, stream_id=3, mask=mask)
    got = est.get_head()
    est.close()
    assert all(np.array_equal(a[..., 41], p[..., 41]) for a, p in zip(got, prior)), "a masked filter moved"
    xm = np.ascontiguousarray(h["vec"][idx])
    ex = gr.exact_fit(Sig, xm, gd, ll)
    gr.assert_input_conditions(ex, m, K, range(B))
    wz, wR, ws = gr.witness_fit(Sig, xm, gd, ll)
    assert np.all(_np(status) == 0) and np.all(ws == 0)
    cols = lambda Rb: np.ascontiguousarray(Rb.transpose(2, 1, 0).reshape(m * m, B))
    sel = np.flatnonzero(mask)
    t = lambda a: ue.take(a, sel)
    exact = ue.exact_update(n, t(h["vec"]), t(h["quat"]), t(h["P"]), idx, t(ex["z"]), t(cols(ex["R"])), None, None, oracle.constants())
    wit = ue.oracle_update(oracle, n, t(h["vec"]), t(h["quat"]), t(h["P"]), idx, t(wz), t(cols(wR)), None)
    bins = [np.arange(len(sel))]
    ue.check_bound("gpf_update chain", ue.errors(tuple(t(a) for a in got), exact, idx), ue.errors(wit, exact, idx), bins)


@pytest.mark.parametrize("broadcast", [False, True])
def test_grid_likelihood(pa, oracle, broadcast):
    import torch
    g = grid_case(B, 33)
    h = gr.heads(15, [11], B, 1)
    est = _estimator(pa, oracle, 15, h)
    with pytest.raises(pa.PbError, match="pb_gpf_grid_set"):
        est.gpf_grid_loglik(torch.as_tensor(g["pose"]).cuda(), g["points"])
    est.gpf_grid_set(g["origin"], g["res"], g["values"], g["unknown"], g["cov"])
    pts = np.ascontiguousarray(g["points"][:, 0]) if broadcast else g["points"]
    dev_pts = pts if broadcast else torch.as_tensor(pts).cuda()
    got = _np(est.gpf_grid_loglik(torch.as_tensor(g["pose"]).cuda(), dev_pts))
    host = None if broadcast else _np(est.gpf_grid_loglik(g["pose"], pts))
    est.close()
    ll, near, bound = gr.grid_loglik(g["origin"], g["res"], g["values"], g["unknown"], g["cov"], g["pose"], pts)
    assert near.mean() <= 1e-3 and np.ptp(ll) > 1.0
    assert np.all(near | (np.abs(got - ll) <= bound)), np.max(np.abs(got - ll))
    assert broadcast or np.array_equal(host, got)


def test_refused_arguments(pa, oracle):
    import torch
    h = gr.heads(15, [11], B, 1)
    est = _estimator(pa, oracle, 15, h)
    L, hd = est._L, est._h
    buf = torch.zeros(4 * 10 * B + 7 * 4 * B + 200 * B, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    ia = lambda *v: (C.c_int * len(v))(*v)
    for m, idx, K in ((10, ia(*range(10)), 4), (0, ia(3), 4), (2, ia(9, 9), 4), (2, ia(9, 15), 4), (2, ia(-1, 3), 4), (3, ia(9, 10, 11), 0)):
        assert L.pb_gpf_sample(hd, m, idx, K, p, p, p) == pa._lib.PB_ERR_ARG
        assert L.pb_gpf_measurement(hd, m, idx, K, p, p, 0.999, p, p, C.c_void_p(st.data_ptr())) == pa._lib.PB_ERR_ARG
        assert est._L.pb_last_error(hd)
    assert L.pb_gpf_sample(hd, 1, ia(11), 4, None, p, p) == pa._lib.PB_ERR_ARG
    assert L.pb_gpf_measurement(hd, 1, ia(11), 4, p, None, 0.999, p, p, C.c_void_p(st.data_ptr())) == pa._lib.PB_ERR_ARG
    assert L.pb_gpf_normals(hd, 1, 1, 0, p) == pa._lib.PB_ERR_ARG and L.pb_gpf_normals(hd, 1, 1, 4, None) == pa._lib.PB_ERR_ARG
    with pytest.raises(ValueError):
        est.gpf_sample([9, 10, 11], np.zeros((4, 2, B)))
    with pytest.raises(ValueError):
        est.gpf_measurement([11], np.zeros((4, 1, B)), np.zeros((5, B)))
    fresh = pa.BatchEstimator(B, n_states=15)
    assert fresh._L.pb_gpf_sample(fresh._h, 1, ia(11), 4, p, p, p) == pa._lib.PB_ERR_STATE       # before pb_reset
    fresh.close()
    est.close()
