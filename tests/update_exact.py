"""The measurement update in exact arithmetic, and heads whose innovation covariance S is ill-conditioned (plain Python, no GPU).

The device factorises S = P[idx,idx] + R without pivoting and downdates P by W D^-1 W^T (ldlt<M>, measurement_update_cols in
rbis_device.hpp); the oracle pivots like Eigen's .ldlt() and forms P - K C P densely (oracle/pronto_oracle.c).  The parity tests
hold one fp64 statement against the other at 1e-9, which says nothing once cond(S) passes ~1e9: both are then further than that
from the truth.  exact_update() is the truth: the reference's update (rbis.cpp:124-143, 199-226) in mpmath at 60 digits on the
fp64 inputs as given; errors() measures a result against it per block, because the max-norm of the whole covariance is dominated
by the block the update hardly touches."""
import numpy as np

DPS = 60
BINS = 5
B_GPU = 130            # two full waves and a two-lane tail; 5 bins of 26 filters, one range of condition numbers each

# the index lists with a compile-time kernel (pb_update_ct.hip), in its order: (idx, orientation measurement)
HANDLER_LISTS = [([3, 4, 5], False), ([9, 10, 11], False), ([9, 10, 11, 3, 4, 5], False), ([9, 10, 11, 6, 7, 8], True),
                 ([9, 10, 11, 8], True), ([3, 4, 5, 8], True), ([8], True), ([8, 9, 10, 11], False), ([6, 7, 8, 9, 10, 11], False),
                 ([11], False), ([3, 4, 5, 0, 1, 2], False)]
# lists no handler produces, for the run-time-index kernels: the m the handlers leave out, chi rows beside others, 21 states' bias rows
EXTRA_LISTS = {15: [([4, 10], False), ([7, 9], True), ([4, 7, 10], True), ([3, 9, 10, 11, 5], False), ([9, 10, 11, 7, 8], True)],
               21: [([16], False), ([4, 16], False), ([7, 19], True), ([5, 8, 19], True), ([3, 9, 15, 11, 20], False),
                    ([9, 10, 18, 7, 8], True), ([10, 3, 7, 15, 20, 6], True)]}
PIECES = ("vec", "quat", "ll", "P_mm", "P_om", "P_oo")


def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _ldl(A, n, pd=True):
    """A = L D L^T of a symmetric matrix given as a list of rows (lower part read) -> (L, d).  pd: stop at the first d[j] <= 0, which
    shows that A is not positive definite; otherwise negative pivots are taken as they come (exact arithmetic needs no pivoting)"""
    from mpmath import fdot
    L = [[0] * n for _ in range(n)]
    d = [0] * n
    for j in range(n):
        t = [L[j][k] * d[k] for k in range(j)]
        d[j] = A[j][j] - fdot(L[j][:j], t)
        if d[j] == 0 or (pd and d[j] < 0):
            return L, d
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - fdot(L[i][:j], t)) / d[j]
    return L, d


def _ldl_solve(L, d, rhs, n):
    y = list(rhs)
    for i in range(n):
        for j in range(i):
            y[i] -= L[i][j] * y[j]
    y = [y[i] / d[i] for i in range(n)]
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= L[j][i] * y[j]
    return y


def r_matrix(R, m, b):
    """R of filter b as [m,m] from any of the three encodings: one host diagonal (length m), a per-filter diagonal [m,B], a full
    column-major [m*m,B] (for m = 1 the last two are the same thing)"""
    R = np.asarray(R, dtype=np.float64)
    if R.ndim == 1:
        assert R.shape == (m,)
        return np.diag(R)
    if R.shape[0] == m:
        return np.diag(R[:, b])
    assert R.shape[0] == m * m
    return R[:, b].reshape(m, m).T


def exact_update(n, vec, quat, P, idx, z, R, quat_meas, mask, constants, ll=None, then=()):
    """RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement::updateFilter for every filter of a batch, in mpmath at 60 digits.
    vec [n,B], quat [4,B], P [n,n,B] (the lower triangle is read, as the device stores it), z [m,B], R in any of the three encodings,
    quat_meas [4,B] or None, mask [B] or None (0: the filter keeps its prior), constants = (g, chi tolerance), ll [B] the prior
    log-likelihood (default 0).
      residual   z - x[idx]; with quat_meas the chi rows take subtractQuats(quat_meas, quat) = Log(quat^-1 quat_meas), angle
                 2 atan2(|v|, |w|) about v / (sign(w) |v|) (rbis.cpp:199-208)
      S = R + P[idx,idx], K = P[:,idx] S^-1, dx = K residual, P - K C P, ll - log(det S) - residual^T S^-1 residual: ONE log (:124-143)
      apply      RBIS(dx) folds its chi into a quaternion when |chi| > tol; vec += dx; the state's chi is folded likewise; the two
                 rotations are composed (rbisApplyDelta, :219-227)
    then: further measurements (idx, z, R, quat_meas, mask) applied one after the other to the unrounded posterior (a fused step's
    second update).
    -> dict: vec, quat, P, ll rounded to fp64; cond = cond_2(S) of the last update; p_over_r = P[idx,idx] / R for m = 1 (what varies
    there, NaN otherwise); prior_pd, post_pd, s_pd: P as given, the exact posterior and every S are positive definite."""
    import mpmath as mp
    B = vec.shape[1]
    tol = constants[1]
    stages = [([int(i) for i in s[0]],) + tuple(s[1:]) for s in [(idx, z, R, quat_meas, mask)] + list(then)]
    out = dict(vec=np.array(vec, dtype=np.float64), quat=np.array(quat, dtype=np.float64), P=np.empty((n, n, B)),
               ll=np.zeros(B) if ll is None else np.array(ll, dtype=np.float64), cond=np.full(B, np.nan), p_over_r=np.full(B, np.nan),
               prior_pd=np.zeros(B, bool), post_pd=np.zeros(B, bool), s_pd=np.zeros(B, bool))
    with mp.workdps(DPS):
        f = lambda a: mp.mpf(float(a))
        for b in range(B):
            Pm = [[f(P[max(i, j), min(i, j), b]) for j in range(n)] for i in range(n)]
            for i in range(n):
                for j in range(n):
                    out["P"][i, j, b] = float(Pm[i][j])
            x, q, llv = [f(a) for a in vec[:, b]], [f(a) for a in quat[:, b]], f(out["ll"][b])
            out["prior_pd"][b] = out["s_pd"][b] = True
            first = True
            for idx, z, R, quat_meas, mask in stages:
                if mask is not None and not mask[b]:
                    continue
                m = len(idx)
                if first:
                    out["prior_pd"][b] = all(dk > 0 for dk in _ldl(Pm, n)[1])
                    first = False
                x, q, Pm, llv, info = _update_one(mp, f, n, tol, x, q, Pm, llv, idx, [z[k, b] for k in range(m)], r_matrix(R, m, b),
                                                  None if quat_meas is None else quat_meas[:, b])
                out["s_pd"][b] &= info["s_pd"]
                out["cond"][b], out["p_over_r"][b] = info["cond"], info["p_over_r"]
            if first:                      # masked out of every update: the prior, as rounded above
                out["post_pd"][b] = True
                continue
            out["post_pd"][b] = all(dk > 0 for dk in _ldl(Pm, n)[1])
            for i in range(n):
                for j in range(n):
                    out["P"][i, j, b] = float(Pm[i][j])
            out["vec"][:, b] = [float(a) for a in x]
            out["quat"][:, b] = [float(a) for a in q]
            out["ll"][b] = np.nan if llv is None else float(llv)
    return out


def _update_one(mp, f, n, tol, x, q, Pm, llv, idx, zb, Rm, qmb):
    """one update of one filter, every quantity an mpf (llv None: a NaN likelihood) -> (x, q, P, llv, info)"""
    m = len(idx)
    resid = [f(zb[k]) - x[idx[k]] for k in range(m)]
    if qmb is not None:
        n2 = sum(a * a for a in q)
        r = _qmul([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2], [f(a) for a in qmb])
        nv = mp.sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3])
        dq = [mp.mpf(0)] * 3
        if nv != 0:
            angle = 2 * mp.atan2(nv, abs(r[0]))
            assert angle < mp.pi           # (the wrap of an angle of exactly pi is not exercised here)
            s = (-angle if r[0] < 0 else angle) / nv
            dq = [r[1] * s, r[2] * s, r[3] * s]
        for k in range(m):
            if 6 <= idx[k] <= 8:
                resid[k] = dq[idx[k] - 6]
    S = [[f(Rm[i, j]) + Pm[idx[i]][idx[j]] for j in range(m)] for i in range(m)]
    L, d = _ldl(S, m, pd=False)
    assert all(dk != 0 for dk in d), "S is singular"
    info = dict(s_pd=all(dk > 0 for dk in d))
    det = mp.mpf(1)
    for dk in d:
        det *= dk
    sol = _ldl_solve(L, d, resid, m)
    # (the reference takes log(S.determinant()): NaN for a negative determinant, finite for an even number of negative pivots)
    llv = llv - mp.log(det) - sum(resid[k] * sol[k] for k in range(m)) if det > 0 and llv is not None else None
    # K^T = S^-1 (C P): one solve per state row
    K = [_ldl_solve(L, d, [Pm[idx[k]][i] for k in range(m)], m) for i in range(n)]
    dx = [mp.fdot(K[i], resid) for i in range(n)]
    post = [[None] * n for _ in range(n)]
    cols = [[Pm[idx[k]][j] for k in range(m)] for j in range(n)]
    for i in range(n):
        for j in range(i + 1):
            post[i][j] = post[j][i] = Pm[i][j] - mp.fdot(K[i], cols[j])

    def fold(chi, qq):
        nn = mp.sqrt(chi[0] * chi[0] + chi[1] * chi[1] + chi[2] * chi[2])
        assert nn == 0 or not (tol / 2 < nn < 2 * tol), "chi within a factor two of the fold tolerance: the branch is not decided by the inputs"
        if nn > tol:
            sh = mp.sin(nn / 2) / nn
            return [mp.mpf(0)] * 3, _qmul(qq, [mp.cos(nn / 2), sh * chi[0], sh * chi[1], sh * chi[2]])
        return chi, qq
    dchi, dquat = fold(dx[6:9], [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)])
    dx[6:9] = dchi
    x = [x[i] + dx[i] for i in range(n)]
    chi, q = fold(x[6:9], q)
    x[6:9] = chi
    q = _qmul(q, dquat)
    if m == 1:
        info["cond"], info["p_over_r"] = 1.0, float(Pm[idx[0]][idx[0]] / f(Rm[0, 0]))
    else:
        ev = [abs(e) for e in mp.eigsy(mp.matrix(S), eigvals_only=True)]
        info["cond"], info["p_over_r"] = float(max(ev) / min(ev)), np.nan
    return x, q, post, llv, info


def _quat_mul_np(a, b):
    return np.stack([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def ill_conditioned_heads(n, idx, B, seed):
    """B heads and one measurement of rows idx for each, ordered by condition number -> dict(vec, quat, P, z, R, quat_meas).
      P[idx,idx]      Q diag(geomspace(1, 1/cond_b, m)) Q^T * 1e-2 with cond_b = geomspace(1e2, 1e10, B) in filter order
      P[other,idx]    G P[idx,idx], G ~ N(0,1);  P[other,other] = G P[idx,idx] G^T + A A^T + 1e-5 I: P is positive definite (the Schur
                      complement of the measured block is A A^T + 1e-5 I), the rows the update does not measure move with the measured
      R [m,B]         0.05 ... 0.2 x lambda_min of the measured block, per row
      m = 1           there is no condition number to vary: P[idx,idx] = 1e-2 and R = 1e-2 / cond_b, P / R over the same range
      vec, quat       Workload.initial_state(), 21 states with nonzero bias rows
      z               x[idx] + N(0,1) sqrt(S_ii); quat_meas = quat * Exp(d), |d| in 0.02 ... 0.2 rad"""
    from pronto_amd.synth import Workload
    rng = np.random.default_rng(seed)
    idx = [int(i) for i in idx]
    m = len(idx)
    other = [i for i in range(n) if i not in idx]
    no = len(other)
    w = Workload(B, n_states=n)
    vec, quat, _ = w.initial_state()
    if n == 21:
        vec[15:18], vec[18:21] = 0.5 * w.bg, 0.5 * w.ba
    cond = np.geomspace(1e2, 1e10, B)
    P, R = np.empty((n, n, B)), np.empty((m, B))
    for b in range(B):
        if m > 1:
            Q = np.linalg.qr(rng.normal(size=(m, m)))[0]
            lam = np.geomspace(1.0, 1.0 / cond[b], m) * 1e-2
            Pmm = (Q * lam) @ Q.T
            Pmm = 0.5 * (Pmm + Pmm.T)
            R[:, b] = rng.uniform(0.05, 0.2, size=m) * lam[-1]
        else:
            Pmm = np.array([[1e-2]])
            R[0, b] = 1e-2 / cond[b]
        G, A = rng.normal(size=(no, m)), 0.03 * rng.normal(size=(no, no))
        Pb = np.empty((n, n))
        Pb[np.ix_(idx, idx)] = Pmm
        Pb[np.ix_(other, idx)] = G @ Pmm
        Pb[np.ix_(idx, other)] = (G @ Pmm).T
        Poo = G @ Pmm @ G.T + A @ A.T + 1e-5 * np.eye(no)
        Pb[np.ix_(other, other)] = 0.5 * (Poo + Poo.T)
        P[:, :, b] = Pb
    sig = np.sqrt(np.stack([P[i, i] for i in idx]) + R)
    z = np.ascontiguousarray(vec[idx] + sig * rng.normal(size=(m, B)))
    d = rng.normal(size=(3, B))
    d *= rng.uniform(0.02, 0.2, size=B) / np.linalg.norm(d, axis=0)
    a = np.linalg.norm(d, axis=0)
    qm = _quat_mul_np(quat, np.concatenate([np.cos(a / 2)[None], np.sin(a / 2) * d / a]))
    return dict(vec=np.ascontiguousarray(vec), quat=np.ascontiguousarray(quat), P=P, z=z, R=np.ascontiguousarray(R),
                quat_meas=np.ascontiguousarray(qm))


def full_r(Rd, seed):
    """a full R with off-diagonals from the per-filter diagonal Rd [m,B]: D^1/2 C D^1/2 with C = I + off-diagonals of at most
    0.6 / (m - 1) (eigenvalues of C within 0.4 ... 1.6: lambda_min(R) stays within 0.02 ... 0.32 x lambda_min of the measured block)
    -> [m*m,B] column-major"""
    rng = np.random.default_rng(seed)
    m, B = Rd.shape
    out = np.empty((m * m, B))
    for b in range(B):
        Cm = np.eye(m)
        for i in range(m):
            for j in range(i):
                Cm[i, j] = Cm[j, i] = rng.uniform(-1, 1) * 0.6 / (m - 1)
        s = np.sqrt(Rd[:, b])
        out[:, b] = (Cm * np.outer(s, s)).T.ravel()
    return out


def r_of_kind(heads, kind, seed=0):
    """'diag': the per-filter diagonal; 'host': one diagonal for every filter, that of the last (worst conditioned) one -- R is then
    below 0.2 lambda_min everywhere and cond(S) still follows the measured block; 'full': full_r()"""
    if kind == "diag":
        return heads["R"]
    if kind == "host":
        return np.ascontiguousarray(heads["R"][:, -1])
    assert kind == "full"
    return full_r(heads["R"], seed)


def regime(ex, m):
    """what orders the batch: cond_2(S), for m = 1 P / R"""
    return ex["cond"] if m > 1 else ex["p_over_r"]


def assert_input_conditions(ex, m, sel, bins):
    """conditions on the inputs (not tolerances): every P as rounded to fp64 and every exact posterior is positive definite; the first
    bin stays at or under 1e4, the last at or over 1e8.  sel: the filters exact_update was given; bins: index arrays into sel."""
    assert ex["prior_pd"].all() and ex["post_pd"].all() and ex["s_pd"].all()
    reg = regime(ex, m)
    assert np.all(np.isfinite(reg))
    assert reg[bins[0]].max() <= 1e4 and reg[bins[-1]].min() >= 1e8, (reg[bins[0]].max(), reg[bins[-1]].min())


def errors(got, exact, idx):
    """per filter -> {piece: [B]}.  got = (vec [n,B], quat [4,B], P [n,n,B], ll [B]), exact = exact_update()'s dict.
      vec    rows outside 6-8 (chi is folded into the quaternion), relative to max |exact vec|
      quat   absolute (unit quaternions);  ll relative to max(|exact|, 1)
      P_mm, P_om, P_oo   the (idx,idx), (other,idx) and (other,other) blocks of the lower triangle, each relative to max |exact block|
                         of that filter"""
    v, q, P, ll = got
    n, B = v.shape
    idx = [int(i) for i in idx]
    other = [i for i in range(n) if i not in idx]
    rows = [i for i in range(n) if not 6 <= i <= 8]
    low = np.tril(np.ones((n, n), bool))
    Pl = np.where(low[:, :, None], P, np.swapaxes(P, 0, 1))      # the lower triangle, mirrored
    ex = exact
    res = dict(vec=np.max(np.abs(v[rows] - ex["vec"][rows]), axis=0) / np.max(np.abs(ex["vec"][rows]), axis=0),
               quat=np.max(np.abs(q - ex["quat"]), axis=0), ll=np.abs(ll - ex["ll"]) / np.maximum(np.abs(ex["ll"]), 1.0))
    for name, r, c in (("P_mm", idx, idx), ("P_om", other, idx), ("P_oo", other, other)):
        g, e = Pl[np.ix_(r, c)], ex["P"][np.ix_(r, c)]
        res[name] = np.max(np.abs(g - e), axis=(0, 1)) / np.max(np.abs(e), axis=(0, 1))
    return res


def oracle_update(po, n, vec, quat, P, idx, z, R, quat_meas, mask=None, ll=None):
    """the same update from the oracle -> (vec [n,B], quat, P [n,n,B], ll): OracleBatch.update_indexed for the two diagonal encodings,
    the single-filter entry points (po_indexed_update / po_indexed_orient_update) for a full R"""
    import ctypes as C
    B, m = vec.shape[1], len(idx)
    v21, P21 = np.zeros((21, B)), np.zeros((21, 21, B))
    v21[:n], P21[:n, :n] = vec, P
    ob = po.OracleBatch(v21, quat, P21, ll)
    Rn = np.asarray(R, dtype=np.float64)
    if Rn.ndim == 1 or Rn.shape[0] == m:
        Rd = np.tile(Rn[:, None], (1, B)) if Rn.ndim == 1 else Rn
        ob.update_indexed(idx, z, Rd, quat_meas=quat_meas, mask=mask)
        return ob.vec[:n].copy(), ob.quat.copy(), ob.cov[:n, :n].copy(), ob.ll.copy()
    L = po.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ov, oq, oP, oll = ob.vec.copy(), ob.quat.copy(), ob.cov.copy(), ob.ll.copy()
    ia = (C.c_int * m)(*idx)
    for b in range(B):
        if mask is not None and not mask[b]:
            continue
        x, Pm, post_ll = po.Rbis(), po.Rbim(), C.c_double(0)
        x.vec[:], x.quat[:] = list(ob.vec[:, b]), list(ob.quat[:, b])
        Pm.m[:] = list(np.ascontiguousarray(ob.cov[:, :, b].T).ravel())
        zz, Rb = np.ascontiguousarray(z[:, b]), np.ascontiguousarray(Rn[:, b])
        if quat_meas is not None:
            qq = np.ascontiguousarray(quat_meas[:, b])
            L.po_indexed_orient_update(m, ia, dp(zz), dp(Rb), dp(qq), C.byref(x), C.byref(Pm), float(ob.ll[b]), C.byref(x), C.byref(Pm), C.byref(post_ll))
        else:
            L.po_indexed_update(m, ia, dp(zz), dp(Rb), C.byref(x), C.byref(Pm), float(ob.ll[b]), C.byref(x), C.byref(Pm), C.byref(post_ll))
        ov[:, b], oq[:, b], oll[b] = x.vec[:], x.quat[:], post_ll.value
        oP[:, :, b] = np.array(Pm.m[:]).reshape(21, 21).T
    return ov[:n], oq, oP[:n, :n], oll


def take(a, sel):
    """the filters sel of a per-filter array (filter index last); None passes through"""
    return None if a is None else np.ascontiguousarray(np.asarray(a)[..., sel])


def take_r(R, sel):
    """the same for R: one host diagonal (1-d) serves every filter"""
    return R if np.ndim(R) == 1 else take(R, sel)


def check_bound(label, got_err, oracle_err, bins, quiet=False):
    """the bound of the exact-arithmetic tests, per piece and per bin: error <= 16 x the oracle's worst error in that bin + 1e-13,
    both against exact_update() (the project's precedent, test_noise_id.py: both factorisations are backward stable on SPD matrices,
    the factor covers the operation order).  Prints every bin of every piece (oracle/kernel, bins in the order of the condition
    number) before it asserts anything; returns the lines."""
    lines, bad = [], []
    for piece in PIECES:
        cells = []
        for i, sel in enumerate(bins):
            k, o = float(np.max(got_err[piece][sel])), float(np.max(oracle_err[piece][sel]))
            cells.append("%.1e/%.1e" % (o, k))
            if not (np.all(np.isfinite(got_err[piece][sel])) and k <= 16.0 * o + 1e-13):
                bad.append("%s %s bin %d: oracle %.2e kernel %.2e" % (label, piece, i, o, k))
        lines.append("%s | %-4s | %s" % (label, piece, "  ".join(cells)))
    if not quiet or bad:
        print("\n".join(lines))
    assert not bad, "\n".join(bad)
    return lines


class Case:
    """one (n, idx, orientation, R kind): the heads, the measurement, the exact posterior of every second filter and the oracle's errors"""


_CASES = {}


def reference(po, n, idx, orient, kind, B=B_GPU):
    """The inputs and the exact reference of one (n, idx, orientation, R kind), computed once per process and shared by every
    kernel mapping that takes this input (and by the CPU and the GPU tests).  The exact posterior is computed for every second
    filter (sel; 13 per bin of 26): 60 digits without a compiled big-number backend cost 5 ... 20 ms per filter and update.
    -> Case: heads, R, quat_meas (None without orientation), sel, bins (index arrays into sel), exact, oracle_err"""
    key = (n, tuple(idx), bool(orient), kind, B)
    if key not in _CASES:
        c = Case()
        c.n, c.idx, c.orient, c.kind, c.B = n, [int(i) for i in idx], bool(orient), kind, B
        c.heads = ill_conditioned_heads(n, idx, B, [n] + c.idx)
        c.R = r_of_kind(c.heads, kind, [n, 1] + c.idx)
        c.quat_meas = c.heads["quat_meas"] if orient else None
        h = c.heads
        judge_against(po, c, (h["vec"], h["quat"], h["P"], None), [(c.idx, h["z"], c.R, c.quat_meas)])
        _CASES[key] = c
    return _CASES[key]


def judge_against(po, c, prior, stages):
    """fills c.sel, c.bins, c.exact and c.oracle_err: the updates stages = [(idx, z, R, quat_meas), ...] applied one after the other to
    prior = (vec, quat, P, ll) -- in exact arithmetic without rounding in between, and by the oracle -- for every second filter.  The
    conditions on the inputs are those of the LAST update; its idx names the blocks of errors()."""
    v, q, P, ll = prior
    c.idx = [int(i) for i in stages[-1][0]]
    c.sel = np.arange(0, c.B, 2)
    c.bins = [np.flatnonzero(np.isin(c.sel, part)) for part in np.array_split(np.arange(c.B), BINS)]
    st = [(i, take(z, c.sel), take_r(R, c.sel), take(qm, c.sel), None) for i, z, R, qm in stages]
    c.exact = exact_update(c.n, take(v, c.sel), take(q, c.sel), take(P, c.sel), *st[0], po.constants(), ll=take(ll, c.sel), then=st[1:])
    assert_input_conditions(c.exact, len(c.idx), c.sel, c.bins)
    o = (take(v, c.sel), take(q, c.sel), take(P, c.sel), take(ll, c.sel))
    for i, z, R, qm, _ in st:
        o = oracle_update(po, c.n, o[0], o[1], o[2], i, z, R, qm, ll=o[3])
    c.oracle_err = errors(o, c.exact, c.idx)


def judge(label, case, got, quiet=False):
    """got = (vec, quat, P, ll) of the whole batch from the code under test: finite everywhere, and within check_bound() of the
    exact posterior on the filters that have one"""
    assert all(np.all(np.isfinite(a)) for a in got), label
    return check_bound(label, errors(tuple(take(a, case.sel) for a in got), case.exact, case.idx), case.oracle_err, case.bins, quiet)
