"""wide_update_lane (pronto_amd/csrc/rbis_update_wide.hpp), the per-lane arithmetic of k_update_wide, on the CPU: g++ compiles the
same PB_HD function over an in-memory tile (tests/cpp/wide_update_host.cpp) and tests/update_exact.py judges it against the exact
posterior on ill-conditioned S -- the six cases of pb_update_indexed_wide's GPU test, R full, per-filter diagonal and one host diagonal,
with update_exact.check_bound's bound (16 x the oracle's own error in the bin + 1e-13), no other tolerance.  The same file is also
built as a stand-alone program under -fsanitize=address,undefined and run once."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import update_exact as ue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "wide_update_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "pronto_amd", "csrc", h) for h in ("rbis_update_wide.hpp", "rbis_device.hpp")]
ALL_STATES = list(range(3, 12))
# (n, index list, orientation measurement): pb_update_indexed_wide's cases
CASES = [(15, ALL_STATES, False), (15, ALL_STATES, True), (21, ALL_STATES, True), (21, [17, 3, 9, 10, 11, 15, 20], False),
         (15, [0, 14, 3, 9, 10, 11, 8, 6], True), (21, [9, 10, 11, 6, 7, 8, 15, 16, 17], True)]
KINDS = ("full", "diag", "host")
R_KIND = {"host": 0, "diag": 1, "full": 2}     # enum pb_rkind


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "build", name)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", out, SRC] + flags)
    return out


@pytest.fixture(scope="module")
def host():
    return C.CDLL(_build("libwide_update_host.so", ["-O2", "-fPIC", "-shared"]))


def host_update(lib, constants, n, idx, vec, quat, P, z, R, quat_meas, mask=None):
    """one update through the g++ build -> (vec, quat, P [n,n,B], ll)"""
    B, m = vec.shape[1], len(idx)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    v, q, ll = np.array(vec), np.array(quat), np.zeros(B)
    cov = np.ascontiguousarray(np.swapaxes(P, 0, 1)).reshape(n * n, B).copy()      # column-major: flat index c * n + r
    Rn = np.ascontiguousarray(R, dtype=np.float64)
    kind = R_KIND["host"] if Rn.ndim == 1 else (R_KIND["diag"] if Rn.shape[0] == m else R_KIND["full"])
    mk = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.wide_host_update(n, B, m, (C.c_int * m)(*idx), dp(np.ascontiguousarray(z)), dp(Rn), kind, dp(quat_meas), mk,
                              C.c_double(constants[0]), C.c_double(constants[1]), dp(v), dp(q), dp(cov), dp(ll))
    assert rc == 0
    return v, q, np.swapaxes(cov.reshape(n, n, B), 0, 1).copy(), ll


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,idx,orient", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else None)
def test_lane_function_against_exact_arithmetic(oracle, host, n, idx, orient, kind):
    case = ue.reference(oracle, n, idx, orient, kind)
    h = case.heads
    got = host_update(host, oracle.constants(), n, idx, h["vec"], h["quat"], h["P"], h["z"], case.R, case.quat_meas)
    ue.judge("host     n=%d wide_update_lane<%d,%d,%s> %s R=%s" % (n, n, len(idx), str(orient).lower(), idx, kind), case, got)
    # every second filter masked off: those keep their prior bit for bit, the others do not move
    mask = (np.arange(case.B) % 2 == 0).astype(np.uint8)
    gm = host_update(host, oracle.constants(), n, idx, h["vec"], h["quat"], h["P"], h["z"], case.R, case.quat_meas, mask)
    low = np.tril(np.ones((n, n), bool))
    prior = (h["vec"], h["quat"], np.where(low[:, :, None], h["P"], np.swapaxes(h["P"], 0, 1)), np.zeros(case.B))
    assert all(np.array_equal(a[..., mask == 0], p[..., mask == 0]) for a, p in zip(gm, prior)), "a masked filter moved"
    assert all(np.array_equal(a[..., mask == 1], p[..., mask == 1]) for a, p in zip(gm, got))


def test_stand_alone_program_under_sanitizers():
    exe = _build("wide_update_host_san", ["-O1", "-g", "-DWIDE_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-2000:])
