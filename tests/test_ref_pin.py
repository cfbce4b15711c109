"""The ONE piece of this path that is pinned to the reference itself: TorqueAdjustment::processSample
(estimate_tools/src/backlash_filter_tools/torque_adjustment.cpp:27-62), compiled UNMODIFIED from the reference tree by `make -C
oracle ref` into oracle/_ref/libref_torque_adjustment.so (no Eigen / boost / LCM / libbot2 / KDL: every other reference file is
unbuildable, SURVEY.md 8c, and stays "parity unpinned").

Held to the reference's own object code, bit for bit (float arithmetic):
  * po_torque_adjust (oracle/leg_odometry.c),
  * oracle/leg_numpy.py's torque_adjust (the second witness),
  * the device function torque_adjust of rbis_legodo.hpp as compiled for the host harness,
  * the committed vectors ta_in / ta_out of tests/golden/leg_fk.npz,
  * the effort path of the golden leg-odometry fixtures: joint positions adjusted by the REFERENCE class, pushed through po_fk,
    give the fixtures' foot poses exactly.
CPU tier.  The reference's outputs on every input used here are recorded in tests/golden/ref_torque.npz (tests/golden/make_golden.py
ref_torque, from that .so), so the tests stand without the reference tree: each one holds the code under test to the record, and
where oracle/_ref is built (build() makes it when the reference tree is present) also the record to the reference class itself."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_torque_adjustment.so")
RECORD = os.path.join(ROOT, "tests", "golden", "ref_torque.npz")
LEG_FIXTURES = ("legodo_alt", "legodo_standing", "legodo_ctrl")
TICK_STRIDE = 7   # every 7th tick of a leg fixture goes through the reference class


def load_ref():
    """The reference class (oracle/_ref), or None where it is not built."""
    if not os.path.exists(REF_SO):
        return None
    L = C.CDLL(REF_SO)
    L.ref_torque_adjustment.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_char_p),
                                        C.POINTER(C.c_float), C.POINTER(C.c_float)]
    return L


@pytest.fixture(scope="module")
def ref():
    return load_ref()


@pytest.fixture(scope="module")
def recorded():
    return np.load(RECORD)


def ref_adjust(L, names, positions, efforts, adjust_names, gains):
    """One TorqueAdjustment(adjust_names, gains).processSample(names, positions, efforts) of the reference -> adjusted positions."""
    n, na = len(names), len(adjust_names)
    nm = (C.c_char_p * n)(*[s.encode() for s in names])
    an = (C.c_char_p * na)(*[s.encode() for s in adjust_names])
    pos = np.ascontiguousarray(positions, dtype=np.float32).copy()
    eff = np.ascontiguousarray(efforts, dtype=np.float32)
    g = np.ascontiguousarray(gains, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ref_torque_adjustment(na, an, fp(g), n, nm, fp(pos), fp(eff)) == 0
    return pos


def cases(n=4000, seed=11):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 1.0, n).astype(np.float32)
    e = (rng.normal(0, 300.0, n) * rng.choice([1.0, 10.0, 0.01], n)).astype(np.float32)
    g = rng.choice(np.array([7000, 10000, 1000, 50, 1e-3, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -2500, 3e38], dtype=np.float32), n)
    # the clamp edges: effort / gain exactly at, just below and just above +-0.1
    p[:6] = 0.25
    g[:6] = 1000.0
    e[:6] = np.array([100.0, np.nextafter(np.float32(100.0), np.float32(0)), np.nextafter(np.float32(100.0), np.float32(200)),
                      -100.0, np.nextafter(np.float32(-100.0), np.float32(0)), np.nextafter(np.float32(-100.0), np.float32(-200))], dtype=np.float32)
    return p, e, g


def one_by_one(L, p, e, g):
    """every case as its own single-joint robot through the reference class (stdout of the constructors silenced)"""
    out = np.empty_like(p)
    fd = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        for i in range(len(p)):
            out[i] = ref_adjust(L, ["j"], p[i:i + 1], e[i:i + 1], ["j"], g[i:i + 1])[0]
    finally:
        os.dup2(fd, 1)
        os.close(fd)
        os.close(null)
    return out


def leg_effort_path(L, g, names, chain_names):
    """Every robot of every TICK_STRIDE-th tick of leg fixture g: ONE processSample call of the reference class on the whole
    16-joint message with the fixture's adjustment joints / gains -> adjusted positions [ticks, B, rows]."""
    T, _, B = g["jpos"].shape
    fd = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        return np.array([[ref_adjust(L, names, g["jpos"][k][:, b], g["jeff"][k][:, b], chain_names, g["gain"]) for b in range(B)]
                         for k in range(0, T, TICK_STRIDE)], dtype=np.float32)
    finally:
        os.dup2(fd, 1)
        os.close(fd)
        os.close(null)


def leg_names():
    """(message joint names: the chain joints at their rows, clutter elsewhere; the chain's joint names in chain order)"""
    import legs
    nl, nr, ty, rows, org, ax = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    names = ["other_%d" % r for r in range(legs.N_ROWS)]
    chain_names = [j[0] for j in legs.ATLAS_LEFT + legs.ATLAS_RIGHT]
    for j, r in enumerate(rows):
        names[r] = chain_names[j]
    return names, chain_names


def record(L):
    """The reference's outputs on every input of these tests (tests/golden/make_golden.py ref_torque writes them)."""
    p, e, g = cases()
    fk = np.load(os.path.join(ROOT, "tests", "golden", "leg_fk.npz"))
    out = {"cases_in": np.stack([p, e, g]), "cases_out": one_by_one(L, p, e, g), "ta_out": one_by_one(L, *fk["ta_in"])}
    names, chain_names = leg_names()
    for name in LEG_FIXTURES:
        out["adjusted_" + name] = leg_effort_path(L, np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")), names, chain_names)
    return out


def test_oracle_witness_and_device_function_equal_the_reference_bit_for_bit(ref, recorded, oracle, harness):
    from oracle import leg_numpy as ln
    L = oracle.lib()
    L.po_torque_adjust.restype = C.c_float
    L.po_torque_adjust.argtypes = [C.c_float, C.c_float, C.c_float]
    harness.hh_torque_adjust.restype = C.c_float
    harness.hh_torque_adjust.argtypes = [C.c_float, C.c_float, C.c_float]
    p, e, g = recorded["cases_in"]
    want = recorded["cases_out"]
    if ref is not None:
        assert one_by_one(ref, p, e, g).tobytes() == want.tobytes()
    po = np.array([L.po_torque_adjust(a, b, c) for a, b, c in zip(p, e, g)], dtype=np.float32)
    # the device function is branch-free on gain == 0; the chain table stores 0 for a gain that is not std::isnormal
    # (leg_chain_set, rbis_legodo.hpp:197 = torque_adjustment.cpp:52) -- the same mapping here
    tiny = np.finfo(np.float32).tiny
    g_tab = np.where(np.isfinite(g) & (np.abs(g) >= tiny), g, np.float32(0.0)).astype(np.float32)
    hh = np.array([harness.hh_torque_adjust(a, b, c) for a, b, c in zip(p, e, g_tab)], dtype=np.float32)
    wit = np.array([ln.torque_adjust(a, b, c) for a, b, c in zip(p, e, g)], dtype=np.float32)
    assert po.tobytes() == want.tobytes(), np.nonzero(po.view(np.uint32) != want.view(np.uint32))[0][:10]
    assert hh.tobytes() == want.tobytes(), np.nonzero(hh.view(np.uint32) != want.view(np.uint32))[0][:10]
    assert wit.tobytes() == want.tobytes(), np.nonzero(wit.view(np.uint32) != want.view(np.uint32))[0][:10]
    assert (want != p).sum() > len(p) // 3 and (want == p).sum() > len(p) // 10    # both branches of isnormal(gain) were taken


def test_committed_vectors_are_the_reference_outputs(ref, recorded):
    g = np.load(os.path.join(ROOT, "tests", "golden", "leg_fk.npz"))
    want = recorded["ta_out"]
    if ref is not None:
        assert one_by_one(ref, *g["ta_in"]).tobytes() == want.tobytes()
    assert g["ta_out"].tobytes() == want.tobytes()


@pytest.mark.parametrize("name", LEG_FIXTURES)
def test_effort_path_of_the_leg_fixtures_is_the_reference_class(ref, recorded, oracle, name):
    """Every robot of every TICK_STRIDE-th tick of the fixture: ONE processSample call of the reference class on the whole 16-joint
    message with the fixture's adjustment joints / gains (joints looked up by NAME, as the reference does), then po_fk on the
    adjusted chain angles -> the fixture's foot poses, exactly."""
    import legs
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    adjusted = recorded["adjusted_" + name]
    if ref is not None:
        assert leg_effort_path(ref, g, *leg_names()).tobytes() == adjusted.tobytes()
    L = oracle.lib()
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    nl, nr, ty, rows, org, ax = chain
    assert adjusted.shape[:2] == (len(range(0, g["jpos"].shape[0], TICK_STRIDE)), g["jpos"].shape[2])
    worst = 0.0
    for i, k in enumerate(range(0, g["jpos"].shape[0], TICK_STRIDE)):
        for b, adj in enumerate(adjusted[i]):
            for side, (lo, n) in enumerate(((0, nl), (nl, nr))):
                ang = np.array([float(adj[rows[lo + j]]) for j in range(n)])
                t, q = legs.oracle_fk(L, chain, side, ang)
                worst = max(worst, float(np.max(np.abs(t - g["feet"][k][7 * side:7 * side + 3, b]))),
                            float(np.max(np.abs(q - g["feet"][k][7 * side + 3:7 * side + 7, b]))))
    assert worst == 0.0, worst
