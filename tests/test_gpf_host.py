"""The per-lane arithmetic of the GPF measurement (pronto_amd/csrc/rbis_gpf.hpp) on the CPU: g++ compiles the same PB_HD functions
(tests/cpp/gpf_host.cpp) and tests/gpf_ref.py judges them against 60-digit arithmetic with gpf_ref.check's bound (16 x the numpy
witness's own error + 1e-13, equal status), for M = 1, 3, 4, 6, 9 with all three statuses in one batch.  Of the samples, the first 20
and the last 4 of every filter are judged at 60 digits (delta, the pose, the chi fold); the others are held to the numpy witness at 1e-12
absolute.  The host Philox4x32-10 is
held word for word against the pure-Python one, the normals against numpy on the same words.  The same source with its own main
runs a fixed batch under -fsanitize=address,undefined (a stand-alone program, nothing preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpf_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gpf_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "pronto_amd", "csrc", h) for h in ("rbis_gpf.hpp", "rbis_device.hpp")]
B_HOST = 24
BRANCH = {16: "flat", 17: "flat", 18: "spike", 19: "anti", 20: "anti", 21: "anti", 22: "nan", 23: "spike"}
TOL = 1e-6       # the default chi fold tolerance


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "build", name)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", out, SRC] + flags)
    return out


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(_build("libgpf_host.so", ["-O2", "-fPIC", "-shared"]))
    lib.gpf_host_grid.restype = C.c_double
    return lib


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_sample(lib, h, idx, xi, tol=TOL):
    K, m, B = xi.shape
    Sig = np.ascontiguousarray(gr.sigma_bar(h, idx).transpose(1, 2, 0))
    x6, q = np.ascontiguousarray(h["vec"][6:12]), np.ascontiguousarray(h["quat"])
    delta, pose = np.empty((K, m, B)), np.empty((K, 7, B))
    assert lib.gpf_host_sample(m, (C.c_int * m)(*idx), K, B, dp(Sig), dp(x6), dp(q), dp(np.ascontiguousarray(xi)), C.c_double(tol), dp(delta), dp(pose)) == 0
    return delta, pose


def host_fit(lib, h, idx, delta, ll, mwp=gr.MWP):
    K, m, B = delta.shape
    Sig = np.ascontiguousarray(gr.sigma_bar(h, idx).transpose(1, 2, 0))
    xm = np.ascontiguousarray(h["vec"][idx])
    z, R, status = np.empty((m, B)), np.empty((m * m, B)), np.zeros(B, dtype=np.int32)
    assert lib.gpf_host_fit(m, K, B, dp(Sig), dp(xm), dp(np.ascontiguousarray(delta)), dp(np.ascontiguousarray(ll)), C.c_double(mwp), dp(z), dp(R),
                            status.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return z, gr.r_cols(R, m), status


def test_philox_word_for_word(host):
    rng = np.random.default_rng(1)
    cases = [((0, 0, 0, 0), (0, 0)), ((MASK := 0xFFFFFFFF, MASK, MASK, MASK), (MASK, MASK))]
    cases += [(tuple(int(v) for v in rng.integers(0, 2 ** 32, 4)), tuple(int(v) for v in rng.integers(0, 2 ** 32, 2))) for _ in range(50)]
    for ctr, key in cases:
        out = (C.c_uint32 * 4)()
        host.gpf_host_philox((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == gr.philox4x32_10(ctr, key), (ctr, key)
    # Random123's known answer for an all-zero counter and key
    assert gr.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


def test_host_normals_against_numpy_on_the_same_words(host):
    rows, Bn = 7, 9
    out = np.empty((rows, Bn))
    host.gpf_host_normals(C.c_uint64(0x123456789ABCDEF), C.c_uint32(3), rows, Bn, dp(out))
    assert np.max(np.abs(out - gr.normals_ref(0x123456789ABCDEF, 3, rows, Bn))) <= 1e-12


@pytest.mark.parametrize("m,K", gr.CASES)
def test_sample_lane_functions_against_exact_arithmetic(host, m, K):
    idx, n = gr.LISTS[m], 15
    h = gr.heads(n, idx, B_HOST, 1)
    h["P"][:, :, 5] = 0.0                                   # Sigma_bar not positive definite: every sample is the head
    h["P"][6:9, :, 6] *= 1e-8                               # chi perturbations below the fold tolerance
    h["P"][:, 6:9, 6] *= 1e-8
    xi = np.random.default_rng([2, m]).normal(size=(K, m, B_HOST))
    ks = list(range(20)) + list(range(K - 4, K))
    ed, ep = gr.exact_sample(h, idx, xi, TOL, ks)
    wd, wp = gr.witness_sample(h, idx, xi, TOL)
    gd, gp = host_sample(host, h, idx, xi)
    assert np.all(gd[:, :, 5] == 0.0) and np.all(gp[:, :3, 5] == h["vec"][9:12, 5]) and np.all(gp[:, 3:, 5] == h["quat"][:, 5])
    if 6 in idx:
        assert np.all(gp[:, 3:, 6] == h["quat"][:, 6]) and not np.all(gp[:, 3:, 0] == h["quat"][:, 0])
    gr.check("host sample m=%d" % m, gr.sample_errors(gd[ks], gp[ks], ed, ep), gr.sample_errors(wd[ks], wp[ks], ed, ep), [np.arange(B_HOST)])
    # every other sample: a few ulps of an m-term product of values below 10 against an error of the order of sigma >= 0.02
    assert np.max(np.abs(gd - wd)) <= 1e-12 and np.max(np.abs(gp - wp)) <= 1e-12


_FIT = {}


def fit_case(m, K, B, branch, seed=1):
    """heads, samples (the numpy witness's), log-likelihoods and the exact fit of one (m, K): computed once per process"""
    key = (m, K, B, seed)
    if key not in _FIT:
        idx = gr.LISTS[m]
        h = gr.heads(15, idx, B, seed)
        xi = np.random.default_rng([3, m, seed]).normal(size=(K, m, B))
        delta, _ = gr.witness_sample(h, idx, xi, TOL)
        ll = gr.gaussian_loglik(h, idx, delta, seed, branch)
        _FIT[key] = (idx, h, delta, ll)
    return _FIT[key]


def judge_fit(label, h, idx, delta, ll, got, branch, B):
    """got = (z [m,B], R [B,m,m], status [B]) against the exact fit of the same delta and ll"""
    m, K = len(idx), delta.shape[0]
    Sig, xm = gr.sigma_bar(h, idx), np.ascontiguousarray(h["vec"][idx])
    ex = gr.exact_fit(Sig, xm, delta, ll)
    normal = [b for b in range(B) if b not in branch]
    gr.assert_input_conditions(ex, m, K, normal, [b for b, k in branch.items() if k == "anti"])
    assert all(ex["status"][b] == 2 for b, k in branch.items() if k in ("flat", "spike", "nan"))
    wz, wR, ws = gr.witness_fit(Sig, xm, delta, ll)
    assert np.array_equal(ws, ex["status"])
    z, R, status = got
    assert np.array_equal(np.asarray(status), ex["status"]), (status, ex["status"])
    gr.check(label, gr.fit_errors(z, R, ex), gr.fit_errors(wz, wR, ex), gr.cond_bins(ex))
    return ex


@pytest.mark.parametrize("m,K", gr.CASES)
def test_fit_lane_functions_against_exact_arithmetic(host, m, K):
    idx, h, delta, ll = fit_case(m, K, B_HOST, BRANCH)
    judge_fit("host fit m=%d K=%d" % (m, K), h, idx, delta, ll, host_fit(host, h, idx, delta, ll), BRANCH, B_HOST)


@pytest.mark.parametrize("K", [5, 6])
def test_fit_with_an_empty_or_single_sample_quarter(host, K):
    """K = 5: the quarters hold 2, 2, 1, 0 samples; K = 6: 2, 2, 2, 0.  One row: 5 m < W can hold only for m = 1 and K = 6"""
    idx, h, delta, ll = fit_case(1, K, B_HOST, {}, seed=4)
    ll = 0.05 * ll
    Sig, xm = gr.sigma_bar(h, idx), np.ascontiguousarray(h["vec"][idx])
    ex = gr.exact_fit(Sig, xm, delta, ll)
    wz, wR, ws = gr.witness_fit(Sig, xm, delta, ll)
    z, R, status = host_fit(host, h, idx, delta, ll)
    assert np.array_equal(status, ex["status"]) and np.array_equal(ws, ex["status"])
    assert (K == 5 and np.all(status == 2)) or (K == 6 and np.any(status != 2))
    gr.check("host fit K=%d" % K, gr.fit_errors(z, R, ex), gr.fit_errors(wz, wR, ex), [np.arange(B_HOST)])


def test_weight_sum_bounds_are_strict(host):
    """flat log-likelihoods: W = K exactly.  K = 5 with one row: W = 5 m, not above it; max_weight_proportion = 1: W = K, not below it"""
    idx, h, delta, _ = fit_case(1, 5, B_HOST, {}, seed=4)
    assert np.all(host_fit(host, h, idx, delta, np.zeros((5, B_HOST)), mwp=2.0)[2] == 2)
    idx, h, delta, _ = fit_case(1, 96, B_HOST, BRANCH)
    z, R, status = host_fit(host, h, idx, delta, np.zeros((96, B_HOST)), mwp=1.0)
    assert np.all(status == 2) and np.array_equal(z, h["vec"][idx]) and np.all(R == gr.R_FIX)


def grid_case(B, K, seed=7):
    """a 12 x 10 x 8 grid of random values, 37 points with three non-finite, poses in and around the map"""
    rng = np.random.default_rng(seed)
    values = rng.uniform(-3.0, 0.5, size=(8, 10, 12))
    origin, res = np.array([-3.0, -2.5, -1.0]), 0.5
    pose = np.empty((K, 7, B))
    pose[:, :3] = (origin + 0.5 * res * np.array([12, 10, 8]))[None, :, None] + rng.normal(size=(K, 3, B)) * np.array([1.5, 1.2, 0.8])[None, :, None]
    pose[::5, 0] += 6.0                                        # pushed outside the map
    q = rng.normal(size=(K, 4, B))
    pose[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    pts = rng.uniform(-2.0, 2.0, size=(37 * 3, B))
    pts[[3 * 4, 3 * 17, 3 * 30]] = np.array([np.nan, np.inf, -np.inf])[:, None]
    return dict(values=values, origin=origin, res=res, unknown=-12.0, cov=2.25, pose=pose, points=np.ascontiguousarray(pts))


def test_grid_lane_function_and_the_witness_exclusions(host):
    g = grid_case(6, 33)
    for pts in (g["points"], np.ascontiguousarray(g["points"][:, 0])):
        ll, near, bound = gr.grid_loglik(g["origin"], g["res"], g["values"], g["unknown"], g["cov"], g["pose"], pts)
        assert near.mean() <= 1e-3                             # the cap on excluded pairs, for the witness
        dims = (C.c_int * 3)(12, 10, 8)
        for b in range(6):
            p = np.ascontiguousarray((pts if pts.ndim == 1 else pts[:, b]))
            for k in range(33):
                got = host.gpf_host_grid(dp(g["origin"]), C.c_double(g["res"]), dims, dp(g["values"]), C.c_double(g["unknown"]), C.c_double(g["cov"]),
                                         dp(np.ascontiguousarray(g["pose"][k, :, b])), 37, dp(p))
                assert near[k, b] or abs(got - ll[k, b]) <= bound[k, b], (k, b, got, ll[k, b])
    assert np.ptp(ll) > 1.0


def test_stand_alone_program_under_sanitizers():
    exe = _build("gpf_host_san", ["-O1", "-g", "-DGPF_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-2000:])
