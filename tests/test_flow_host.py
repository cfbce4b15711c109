"""The per-lane arithmetic of the optical-flow sigma-point update (pronto_amd/csrc/rbis_flow.hpp) on the CPU: g++ compiles the same
PB_HD function the kernel runs (tests/cpp/flow_host.cpp) and tests/flow_ref.py judges it against 60-digit arithmetic under the
project's exact-arithmetic bound (flow_ref.judge), for 15 and 21 states and both flags, with the special filters of the GPU tests in the
batch.  Beside it: the reduced form (12 columns, 25 points) against the unreduced one at 60 digits, a 15-state context against the
21-state filter with zero bias blocks, the EKF limit of the gain, the five weights, and the same source with its own main under
-fsanitize=address,undefined (a stand-alone program, nothing preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flow_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "pronto_amd", "csrc", h) for h in ("rbis_flow.hpp", "rbis_device.hpp")]


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "build", name)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", out, SRC] + flags)
    return out


@pytest.fixture(scope="module")
def host():
    return C.CDLL(_build("libflow_host.so", ["-O2", "-fPIC", "-shared"]))


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def r_full(R, B):
    """any of the three encodings -> [16,B] column-major"""
    return np.ascontiguousarray(np.stack([fr.r_matrix(R, b).T.ravel() for b in range(B)], axis=1))


def host_update(lib, h, R, cam, wts, flags, tol=fr.TOL):
    n, B = h["vec"].shape
    vec, quat, ll, P, flow = (np.ascontiguousarray(h[k], dtype=np.float64) for k in ("vec", "quat", "ll", "P", "flow"))
    out = dict(vec=np.empty((n, B)), quat=np.empty((4, B)), ll=np.empty(B), P=np.empty((n, n, B)), zhat=np.empty((4, B)),
               status=np.zeros(B, dtype=np.int32))
    camv, w = np.concatenate(cam), np.array(wts)
    assert lib.flow_host_update(n, B, dp(vec), dp(quat), dp(ll), dp(P), dp(flow), dp(r_full(R, B)), dp(camv), dp(w), C.c_double(tol), flags,
                                dp(out["vec"]), dp(out["quat"]), dp(out["ll"]), dp(out["P"]), dp(out["zhat"]),
                                out["status"].ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return out


def test_weights_are_the_references_expressions(host):
    w = np.empty(5)
    host.flow_host_weights(dp(w))
    assert tuple(w) == fr.weights()
    lam, Ws0, Wc0, Wi, s = fr.weights()
    assert abs((21 + lam) / 2.1e-5 - 1) < 2e-10 and Ws0 < -9e5 and 2.3e4 < Wi < 2.4e4        # the cancellation the bound is about


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n", [15, 21])
def test_lane_function_against_exact_arithmetic(host, n, flags):
    c = fr.reference(n, flags)
    print("heads(%d): %d draws for %d filters" % (n, c.h["tried"], c.B))
    fr.assert_input_conditions(c)
    got = host_update(host, c.h, c.R, c.cam, c.wts, flags)
    assert np.array_equal(got["quat"], c.h["quat"]) and np.array_equal(got["ll"], c.h["ll"])     # the prior's bits
    assert np.array_equal(got["P"], np.swapaxes(got["P"], 0, 1))
    st = c.wit["status"]
    assert set(st[list(fr.SPECIAL["zero"])]) == {2} and set(st[list(fr.SPECIAL["col7"])]) == {9} and set(st[list(fr.SPECIAL["fold"])]) == {0}
    fr.judge("host n=%d flags=%d" % (n, flags), c, got)
    # the flag matters: the head's attitude moves zhat by far more than the bound
    other = fr.reference(n, 1 - flags)
    assert np.nanmax(np.abs(c.wit["zhat"] - other.wit["zhat"])) > 1e-3


@pytest.mark.parametrize("n", [15, 21])
def test_second_batch_with_the_negative_pivot_in_the_tail(host, n):
    """the special filters at other places (pivot 7 negative at 70 and at 129): the statuses follow, the skipped filters keep their
    bits, and every filter that is the same in both batches gets the same bits"""
    h1, h2 = fr.add_specials(fr.heads(n)), fr.add_specials(fr.heads(n), fr.SPECIAL_TAIL7)
    g1, g2 = (host_update(host, h, h["R"], fr.camera(), fr.weights(), 0) for h in (h1, h2))
    fr.check_second_batch(h2, g1, g2)


def test_fold_filter_sees_the_identity_everywhere(host):
    """every sigma point's |chi| below the tolerance: the chi rows of the factor cannot reach the measurement, flags 0"""
    c = fr.reference(21, 0)
    for b in fr.SPECIAL["fold"]:
        k = int(np.flatnonzero(c.sel == b)[0])
        assert max(float(v) for v in c.exact["raw"][k]["chi_norms"]) < fr.TOL / 2


@pytest.mark.parametrize("flags", [0, 1])
def test_reduced_equals_unreduced_at_60_digits(flags):
    import mpmath as mp
    h, sel = fr.heads(21), [0, 40, 90]
    full = fr.exact_update(h, h["R"], fr.camera(), fr.weights(), fr.TOL, flags, sel)
    red = fr.exact_update(h, h["R"], fr.camera(), fr.weights(), fr.TOL, flags, sel, reduced=True)
    for a, b in zip(full["raw"], red["raw"]):
        err = max([abs(u - v) for u, v in zip(a["vec"], b["vec"])] + [abs(u - v) for ra, rb in zip(a["P"], b["P"]) for u, v in zip(ra, rb)]
                  + [abs(u - v) for u, v in zip(a["zhat"], b["zhat"])])
        assert err < mp.mpf(10) ** -45, err


@pytest.mark.parametrize("flags", [0, 1])
def test_15_states_are_the_first_rows_of_21_with_zero_bias_blocks(host, flags):
    h15 = fr.add_specials(fr.heads(15))
    B = h15["vec"].shape[1]
    h21 = dict(h15, vec=np.zeros((21, B)), P=np.zeros((21, 21, B)))
    h21["vec"][:15], h21["P"][:15, :15] = h15["vec"], h15["P"]
    # (a zero bias block has zero pivots at columns 15 ... 20 only: the twelve columns the update factors are the same)
    g15 = host_update(host, h15, h15["R"], fr.camera(), fr.weights(), flags)
    g21 = host_update(host, h21, h15["R"], fr.camera(), fr.weights(), flags)
    assert np.array_equal(g15["status"], g21["status"]) and (g15["status"] == 0).sum() >= B - 3
    assert np.array_equal(g21["vec"][:15], g15["vec"]) and np.array_equal(g21["P"][:15, :15], g15["P"])
    assert np.array_equal(g21["zhat"], g15["zhat"], equal_nan=True)
    assert np.all(g21["vec"][15:] == 0) and np.all(g21["P"][15:] == 0) and np.all(g21["P"][:, 15:] == 0)


def test_gain_approaches_the_ekf_gain_for_a_tiny_covariance():
    """With P -> 0 the sigma points sample h linearly and K -> P H^T (H P H^T + R)^-1.  H by central differences with step d: its
    relative truncation error is ~ d^2 |h'''| / |h'| <= 1e-6 x O(10) at d = 1e-3, its rounding error ~ 1e-16 / d = 1e-13.  The
    unscented gain differs from the EKF's by the second-order terms, O(sigma^2) relative = 1e-8 at sigma <= 1e-4.  Tolerance 1e-4."""
    cam, wts = fr.camera(), fr.weights()
    h = fr.heads(21)
    b = 3
    hs = {k: (v[..., b:b + 1].copy() if isinstance(v, np.ndarray) else v) for k, v in h.items()}
    hs["P"] *= (1e-4 / 3.0) ** 2 / np.max(np.diag(hs["P"][:, :, 0]) / fr.SIGMA ** 2)
    hs["vec"][6:9] = 0.0
    w = fr.witness_update(hs, hs["R"], cam, wts, 1e-12, 0)         # (tolerance below every sigma point's |chi|: h is smooth in chi)
    K = np.array([[float(v) for v in row] for row in w["raw"][0]["K"]])
    x, q, msg = hs["vec"][:, 0], list(hs["quat"][:, 0]), list(hs["flow"][4:, 0])
    camc = tuple(list(v) for v in cam)
    H, d = np.zeros((4, 21)), 1e-3
    for j in range(12):
        xp, xn = x.copy(), x.copy()
        xp[j] += d
        xn[j] -= d
        H[:, j] = (np.array(fr.measure(fr._NP, list(xp), q, camc, msg, 1e-12, 0)) - np.array(fr.measure(fr._NP, list(xn), q, camc, msg, 1e-12, 0))) / (2 * d)
    P = hs["P"][:, :, 0]
    Kekf = P @ H.T @ np.linalg.inv(H @ P @ H.T + np.diag(hs["R"][:, 0]))
    assert np.max(np.abs(K - Kekf)) <= 1e-4 * np.max(np.abs(Kekf)), np.max(np.abs(K - Kekf)) / np.max(np.abs(Kekf))


def test_stand_alone_program_under_sanitizers():
    exe = _build("flow_host_san", ["-O1", "-g", "-DFLOW_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-2000:])
