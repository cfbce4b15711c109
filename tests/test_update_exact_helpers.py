"""The exact-arithmetic reference of the measurement update (tests/update_exact.py) against the oracle where S is well conditioned,
and the kernels' per-lane update arithmetic, compiled for the host by the test-only harness, against that reference on
ill-conditioned S (cond 1e2 ... 1e10).  No GPU; the same inputs and references serve tests/test_update_ill_conditioned.py."""
import ctypes as C

import numpy as np
import pytest

import update_exact as ue
from test_host_math import P as dptr, pack, unpack

ALL_LISTS = {n: ue.HANDLER_LISTS + ue.EXTRA_LISTS[n] for n in (15, 21)}
KIND_OF = {tuple(idx): k for k, (idx, _) in enumerate(ue.HANDLER_LISTS[:10])}      # hh_update_quad / hh_update_coop's numbering


def lid(v):
    return "-".join(str(i) for i in v) if isinstance(v, list) else None


def test_exact_update_on_cases_with_known_answers():
    """the reference itself.  (a) diagonal P, one row: the scalar Kalman update.  (b) an orientation measurement a known angle about z
    away, P = p I on chi and nothing else: chi correction p / (p + r) * angle, folded into the quaternion.  (c) one log of det S: a
    negative determinant gives NaN like the reference's log(S.determinant()), two negative pivots a finite value."""
    n = 15
    vec, quat, P = np.zeros((n, 1)), np.array([[1.0], [0.0], [0.0], [0.0]]), np.zeros((n, n, 1))
    P[:, :, 0] = np.diag(np.arange(1.0, n + 1))
    vec[9, 0] = 0.5
    ex = ue.exact_update(n, vec, quat, P, [9], np.array([[1.25]]), np.array([[2.5]]), None, None, (9.8, 1e-6))
    k = 10.0 / 12.5
    assert abs(ex["vec"][9, 0] - (0.5 + k * 0.75)) < 1e-15 and abs(ex["P"][9, 9, 0] - 2.0) < 1e-15 and ex["P"][8, 8, 0] == 9.0
    assert abs(ex["ll"][0] - (-np.log(12.5) - 0.75 ** 2 / 12.5)) < 1e-15 and ex["p_over_r"][0] == 4.0 and np.all(ex["quat"] == quat)
    assert ex["prior_pd"][0] and ex["post_pd"][0] and ex["s_pd"][0]
    # (b) quat_meas = -(rotation by 0.4 about z): the same rotation, w < 0
    qm = -np.array([[np.cos(0.2)], [0.0], [0.0], [np.sin(0.2)]])
    P[:, :, 0] = np.diag(np.r_[np.full(6, 1e-3), np.full(3, 0.03), np.full(6, 1e-3)])
    ex = ue.exact_update(n, vec, quat, P, [8], np.array([[123.0]]), [0.01], qm, None, (9.8, 1e-6))
    a = 0.75 * 0.4
    assert np.max(np.abs(ex["quat"][:, 0] - [np.cos(a / 2), 0, 0, np.sin(a / 2)])) < 1e-16 and np.all(ex["vec"][6:9] == 0)
    assert abs(ex["P"][8, 8, 0] - 0.0075) < 1e-17 and abs(ex["ll"][0] - (-np.log(0.04) - 0.16 / 0.04)) < 1e-14
    # a chi correction under the tolerance stays in the vector
    ex = ue.exact_update(n, vec, quat, P, [8], np.array([[123.0]]), [0.01], qm, None, (9.8, 1.0))
    assert abs(ex["vec"][8, 0] - a) < 1e-16 and np.all(ex["quat"] == quat)
    # a masked filter keeps its prior
    ex = ue.exact_update(n, vec, quat, P, [8], np.array([[123.0]]), [0.01], qm, np.zeros(1, np.uint8), (9.8, 1e-6))
    assert np.all(ex["vec"] == vec) and np.all(ex["P"] == P) and ex["ll"][0] == 0.0
    # (c)
    P[:, :, 0] = np.diag(np.arange(1.0, n + 1))
    z2 = np.array([[1.0], [2.0]])
    ex = ue.exact_update(n, vec, quat, P, [3, 4], z2, [-6.0, 1.0], None, None, (9.8, 1e-6))       # S = diag(-2, 6)
    assert np.isnan(ex["ll"][0]) and not ex["s_pd"][0] and abs(ex["vec"][3, 0] - 4.0 / -2.0) < 1e-15
    ex = ue.exact_update(n, vec, quat, P, [3, 4], z2, [-6.0, -8.0], None, None, (9.8, 1e-6))      # S = diag(-2, -3)
    assert abs(ex["ll"][0] - (-np.log(6.0) + 0.5 + 4.0 / 3.0)) < 1e-15 and abs(ex["cond"][0] - 1.5) < 1e-12
    # a full R: S = [[5, 1], [1, 6]] -> det 29
    ex = ue.exact_update(n, vec, quat, P, [3, 4], z2, np.array([[1.0], [1.0], [1.0], [1.0]]), None, None, (9.8, 1e-6))
    assert abs(ex["ll"][0] - (-np.log(29.0) - (6.0 - 4.0 + 20.0) / 29.0)) < 1e-14


def test_errors_measure_each_block_on_its_own_scale():
    """a wrong entry of the measured block is invisible in the max-norm of the whole covariance and plain in P_mm"""
    n, idx = 15, [9, 10, 11]
    h = ue.ill_conditioned_heads(n, idx, 4, 1)
    h["P"][np.ix_(idx, idx)] *= 1e-6                      # (a measured block after an accurate measurement)
    ex = dict(vec=h["vec"], quat=h["quat"], P=h["P"], ll=np.zeros(4))
    Pw = h["P"].copy()
    Pw[10, 9, 3] *= 1.0 + 1e-3
    e = ue.errors((h["vec"], h["quat"], Pw, np.zeros(4)), ex, idx)
    assert e["P_mm"][3] > 1e-5 and e["P_om"][3] == 0 and e["P_oo"][3] == 0 and np.all(e["vec"] == 0) and np.all(e["P_mm"][:3] == 0)
    assert np.max(np.abs(Pw - h["P"])) / np.max(np.abs(h["P"])) < 1e-6
    Pu = h["P"].copy()
    Pu[9, 10, 3] = 7.0                                    # the upper triangle is not read
    assert ue.errors((h["vec"], h["quat"], Pu, np.zeros(4)), ex, idx)["P_mm"][3] == 0


@pytest.mark.parametrize("kind", ["diag", "full"])
@pytest.mark.parametrize("n,idx,orient", [(n, idx, o) for n in (15, 21) for idx, o in ALL_LISTS[n]], ids=lid)
def test_reference_agrees_with_the_oracle_where_s_is_well_conditioned(oracle, n, idx, orient, kind):
    """exact_update against the oracle's update on the first bin of ill_conditioned_heads (cond(S) <= 1e4): every handler index
    list of pb_update_ct.hip plus lists with m = 2 and 5, m = 1 ... 6 with and without orientation, 15 and 21 states, diagonal and
    full R.  Bound: 1e-12 on the state vector, the quaternion and the log-likelihood in errors()'s measure (1e4 x the 1e-16 two fp64
    statements differ by at cond 1e2).  The covariance blocks get the same 1e-12 plus what fp64 itself leaves of them: the update
    subtracts from a measured block of size |P-| a term that leaves 0.05 ... 0.2 lambda_min of it, up to 5 cond(S) times smaller, and
    each of the m products and the subtraction rounds relative to |P-|; relative to the block that is left that is
    (m + 2) 2^-53 |P- block| / |P+ block| (for m = 3 at cond 3.5e3: 6e-12 with the 1e-12, where the oracle is at 3.5e-12, the largest
    share of this bound any case uses: 0.59).  No implementation in fp64 can do better in that measure, so a flat 1e-12 there would
    test the inputs, not the reference."""
    case = ue.reference(oracle, n, idx, orient, kind)
    first = case.bins[0]
    assert ue.regime(case.exact, len(idx))[first].max() <= 1e4
    m = len(idx)
    other = [i for i in range(n) if i not in idx]
    prior = ue.take(case.heads["P"], case.sel)
    for piece in ue.PIECES:
        e = case.oracle_err[piece][first]
        bound = np.full(len(first), 1e-12)
        if piece.startswith("P_"):
            r, c = {"P_mm": (idx, idx), "P_om": (other, idx), "P_oo": (other, other)}[piece]
            scale = np.max(np.abs(prior[np.ix_(r, c)]), axis=(0, 1)) / np.max(np.abs(case.exact["P"][np.ix_(r, c)]), axis=(0, 1))
            bound = bound + (m + 2) * 2.0 ** -53 * scale[first]
        print("n=%d idx=%s %s %-5s oracle against exact %.2e (bound %.2e)" % (n, idx, kind, piece, e.max(), bound[np.argmax(e)]))
        assert np.all(e <= bound), (piece, e.max())


def harness_state(H, case, n):
    h = case.heads
    return pack(H, n, h["vec"], h["quat"], h["P"], np.zeros(case.B))


def run_entry(H, oracle, entry, case, mask=None):
    """one update of case's heads through a harness entry -> (vec, quat, P, ll)"""
    n, B, idx, h = case.n, case.B, case.idx, case.heads
    g, tol = oracle.constants()
    gd, td = C.c_double(g), C.c_double(tol)
    st = harness_state(H, case, n)
    qm = h["quat_meas"]               # (entries with an orientation template parameter read it; the others ignore it)
    mk = None if mask is None else mask.ctypes.data_as(C.c_void_p)
    z, R = h["z"], case.R
    if entry == "vo":
        H.hh_update_vo(n, dptr(st), C.c_long(B), B, dptr(z), dptr(R), dptr(qm), gd, td)
    elif entry == "posyaw":
        H.hh_update_posyaw(n, dptr(st), C.c_long(B), B, dptr(z), dptr(R), dptr(qm), gd, td)
    elif entry == "quad":
        H.hh_update_quad(KIND_OF[tuple(idx)], dptr(st), C.c_long(B), B, dptr(z), dptr(R), dptr(qm), mk, gd, td)
    elif entry == "coop":
        assert H.hh_update_coop(n, KIND_OF[tuple(idx)], dptr(st), C.c_long(B), B, dptr(z), dptr(R), dptr(qm), mk, gd, td) == 0
    elif entry == "coop_correct":
        imu, lo, q4 = np.zeros((7, B)), np.ones((6, B)), np.zeros(4)
        H.hh_step_coop_correct(n, 0 if len(idx) == 6 else 1, 2, dptr(st), C.c_long(B), B, dptr(imu), dptr(lo), None, dptr(q4), gd, td,
                               dptr(z), dptr(R), dptr(qm), mk)
    else:
        assert entry == "rt"
        ia = (C.c_int * len(idx))(*idx)
        assert H.hh_update_rt(n, len(idx), ia, dptr(st), C.c_long(B), B, dptr(z), dptr(R), 1 if case.kind == "full" else 0,
                              dptr(qm) if case.orient else None, mk, gd, td) == 0
    v, q, cov, ll = unpack(H, n, st)
    return v, q, cov, ll


def harness_cases():
    out = []
    for n in (15, 21):
        out += [("vo", n, [9, 10, 11, 6, 7, 8], True, "diag"), ("posyaw", n, [9, 10, 11, 8], True, "diag"),
                ("coop_correct", n, [9, 10, 11, 6, 7, 8], True, "diag"), ("coop_correct", n, [9, 10, 11, 8], True, "diag")]
        for idx, o in ue.HANDLER_LISTS[:10]:
            if n == 15 or len(idx) <= 4:
                out.append(("coop", n, idx, o, "diag"))
            if n == 21:
                out.append(("quad", n, idx, o, "diag"))
        for idx, o in ALL_LISTS[n]:
            out.append(("rt", n, idx, o, "diag"))
        for idx, o in ([([3, 4, 5, 0, 1, 2], False)] + ue.EXTRA_LISTS[n]):
            out.append(("rt", n, idx, o, "full"))
    return out


@pytest.mark.parametrize("entry,n,idx,orient,kind", harness_cases(), ids=lambda v: lid(v) if isinstance(v, list) else None)
def test_per_lane_maths_against_exact(oracle, harness, entry, n, idx, orient, kind):
    """The update arithmetic of every mapping the harness models, one update of 130 ill-conditioned heads each, all five bins, against
    the 60-digit reference: measurement_update with a compile-time list (vo, posyaw), the two-role mapping with its hand-off for each
    of the ten handler lists (coop; coop_correct is the same through the fused step's entry), the four-wave mapping (quad), and the
    one-lane update with a run-time list (rt: k_update_lane_rt's order of operations, any list, diagonal and full R).
    Bound: update_exact.check_bound -- per piece and bin 16 x the oracle's worst error + 1e-13.  A masked half keeps its prior bit for
    bit where the entry takes a mask."""
    case = ue.reference(oracle, n, idx, orient, kind)
    got = run_entry(harness, oracle, entry, case)
    ue.judge("%s n=%d idx=%s %s" % (entry, n, idx, kind), case, got)
    if entry in ("quad", "coop", "rt"):
        mask = (np.arange(case.B) % 2 == 0).astype(np.uint8)
        prior = unpack(harness, n, harness_state(harness, case, n))
        gm = run_entry(harness, oracle, entry, case, mask)
        for a, b, p in zip(gm, got, prior):
            assert np.array_equal(a[..., mask == 1], b[..., mask == 1]) and np.array_equal(a[..., mask == 0], p[..., mask == 0])


@pytest.mark.parametrize("entry,n,idx", [("rt", 15, [4, 10]), ("rt", 21, [5, 8, 19]), ("coop", 15, [9, 10, 11]), ("coop", 21, [8, 9, 10, 11]),
                                         ("quad", 21, [3, 4, 5]), ("quad", 21, [9, 10, 11, 3, 4, 5])], ids=lid)
def test_one_log_of_the_determinant(oracle, harness, entry, n, idx):
    """The reference takes ONE log of S.determinant() (rbis.cpp:142).  On a positive definite S a sum of logs of the pivots is the same
    number; the two part where S is indefinite: a negative determinant gives NaN, an even number of negative pivots a finite value.
    A negative R on the first row (filters 1 mod 3) / the first two rows (2 mod 3) of well-conditioned heads makes such S; the state,
    the covariance and the finite likelihoods agree with the exact update to 1e-9, the NaNs sit where the exact determinant is
    negative and nowhere else."""
    B, m = 12, len(idx)
    case = ue.Case()
    case.n, case.idx, case.B, case.orient, case.kind = n, idx, B, False, "diag"
    h = case.heads = ue.ill_conditioned_heads(n, idx, 130, [n, 2] + idx)
    for k in h:
        h[k] = ue.take(h[k], np.arange(B))          # cond 1e2 ... 5e2
    R = h["R"].copy()
    for b in range(B):
        for row in range(b % 3):
            R[row, b] = -2.0 * h["P"][idx[row], idx[row], b]
    case.R = np.ascontiguousarray(R)
    ex = ue.exact_update(n, h["vec"], h["quat"], h["P"], idx, h["z"], case.R, None, None, oracle.constants())
    neg = np.arange(B) % 3 == 1
    assert np.array_equal(np.isnan(ex["ll"]), neg) and np.array_equal(ex["s_pd"], np.arange(B) % 3 == 0)
    v, q, cov, ll = run_entry(harness, oracle, entry, case)
    assert np.array_equal(np.isnan(ll), neg), ll
    e = ue.errors((v, q, cov, np.where(neg, 0.0, ll)), dict(ex, ll=np.where(neg, 0.0, ex["ll"])), idx)
    assert max(e[p].max() for p in ue.PIECES) < 1e-9, {p: e[p].max() for p in ue.PIECES}
