"""Per-filter leg-odometry noises and contact thresholds (pb_legodo_set_param_block, rbis_legpar.hpp): the parameter block read by
k_odo_legpar (stand-alone odometry) and k_pair_legpar / k_pair_quad_legpar (IMU step + odometry + update in one kernel) against B
independent oracle robots, each po_leg_init'ed / po_leg_set_contact_mode'd with its own float-rounded values.

Tolerances are those of the sibling tests in test_leg_odometry.py: statuses and masks bit-identical, the measurement z <= 1e-8, R to
rtol 1e-14 (1e-13 in the six-row modes, as there), the final posterior through test_gpu_parity.check.

Parameter draws: thresholds default_rng(3).uniform(300, 500) low, uniform(520, 700) high; delays whole numbers in [3000, 9000] us;
r_vxyz = linspace(5, 12, B), r_vxyz_uncertain = linspace(20, 10, B) -- not below the (5, 10) the closed-loop tests of
test_leg_odometry.py found stable."""
import ctypes as C

import numpy as np
import pytest

from pronto_amd import _lib
from pronto_amd.synth import Workload
from test_leg_odometry import OracleLegs, SCHMITT, R_VXYZ, STANDING, gait, same_rotation

R6 = (0.05, 0.4, 0.9)   # r_xyz, r_vang, r_vang_uncertain of test_pair_call_in_the_six_row_modes_against_the_oracle_chain_on_gpu


def draws(B, thresholds=True, delays=True, noises=True, six=True, standing=False):
    """the block [PB_LEGPAR_ROWS, B]: the rows named vary per filter, the others hold the sibling tests' scalars"""
    rng = np.random.default_rng(3)
    low, high = rng.uniform(300, 500, B), rng.uniform(520, 700, B)
    ld, hd = rng.integers(3000, 9001, B), rng.integers(3000, 9001, B)
    tf, lvl = rng.uniform(700, 1100, B), rng.uniform(0.5, 0.8, B)
    blk = np.zeros((_lib.PB_LEGPAR_ROWS, B))
    blk[_lib.PB_LEGPAR_R_VXYZ] = np.linspace(5, 12, B) if noises else R_VXYZ[0]
    blk[_lib.PB_LEGPAR_R_VXYZ_UNCERTAIN] = np.linspace(20, 10, B) if noises else R_VXYZ[1]
    f = np.geomspace(0.5, 2.0, B) if six else np.ones(B)    # 0.5x ... 2x the six-row test's values
    blk[_lib.PB_LEGPAR_R_XYZ] = R6[0] * f
    blk[_lib.PB_LEGPAR_R_VANG] = R6[1] * f[::-1]
    blk[_lib.PB_LEGPAR_R_VANG_UNCERTAIN] = R6[2] * f
    blk[_lib.PB_LEGPAR_SCHMITT_LOW] = low if thresholds else SCHMITT[0]
    blk[_lib.PB_LEGPAR_SCHMITT_HIGH] = high if thresholds else SCHMITT[1]
    blk[_lib.PB_LEGPAR_SCHMITT_LOW_DELAY] = ld if delays else SCHMITT[2]
    blk[_lib.PB_LEGPAR_SCHMITT_HIGH_DELAY] = hd if delays else SCHMITT[3]
    blk[_lib.PB_LEGPAR_TOTAL_FORCE] = tf if standing else STANDING[0]
    blk[_lib.PB_LEGPAR_STANDING_SCHMITT_LEVEL] = lvl if standing else STANDING[1]
    return np.ascontiguousarray(blk)


def uniform_block(B, schmitt=SCHMITT, r=R_VXYZ, r6=R6, standing=STANDING):
    blk = np.zeros((_lib.PB_LEGPAR_ROWS, B))
    for row, v in zip(range(_lib.PB_LEGPAR_ROWS), (r[0], r[1], r6[1], r6[2], r6[0], *schmitt, *standing)):
        blk[row] = v
    return blk


class PerFilterLegs(OracleLegs):
    """B oracle robots, each with the float-rounded values of its own column of the block"""

    def __init__(self, oracle, blk, standing=False):
        B = blk.shape[1]
        OracleLegs.__init__(self, oracle, B, True)
        f32 = lambda v: float(np.float32(v))
        for b, buf in enumerate(self.bufs):
            self.L.po_leg_init(buf, f32(blk[_lib.PB_LEGPAR_SCHMITT_LOW, b]), f32(blk[_lib.PB_LEGPAR_SCHMITT_HIGH, b]),
                               int(blk[_lib.PB_LEGPAR_SCHMITT_LOW_DELAY, b]), int(blk[_lib.PB_LEGPAR_SCHMITT_HIGH_DELAY, b]), 1)
            if standing:
                self.L.po_leg_set_contact_mode(buf, 1, f32(blk[_lib.PB_LEGPAR_TOTAL_FORCE, b]), f32(blk[_lib.PB_LEGPAR_STANDING_SCHMITT_LEVEL, b]), 0)


def lin_rate(od, os_, op, utime, blk):
    """LegOdoCommon's lin_rate measurement (rbis_legodo_common.cpp:99-169) with each filter's own noises: z [3,B], R diagonal [3,B], mask"""
    r, ru = blk[_lib.PB_LEGPAR_R_VXYZ], blk[_lib.PB_LEGPAR_R_VXYZ_UNCERTAIN]
    z = od[0:3] / ((utime - op) * 1e-6)
    return z, np.tile(np.where(os_ >= 0.5, ru * ru, r * r), (3, 1)), (os_ >= 0).astype(np.uint8)


# ---- 1. open loop, k_odo_legpar ----------------------------------------------------------------------------------------------
_open_loop = {}


def open_loop_oracle(oracle, blk, wq):
    """the per-filter oracles on the broadcast log gait(1, 500, seed=27), made once for both state sizes (the same head orientation)"""
    key = wq.tobytes()
    if key not in _open_loop:
        B = blk.shape[1]
        orc = PerFilterLegs(oracle, blk)
        out = []
        for utime, feet, forces, _ in gait(1, 500, seed=27):
            od, os_, op = orc.update(utime, np.repeat(feet, B, axis=1), np.repeat(forces, B, axis=1), wq)
            out.append((od, os_, op))
        _open_loop[key] = out
    return _open_loop[key]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
def test_open_loop_odometry_with_per_filter_thresholds_on_gpu(oracle, n):
    """pb_legodo_update with a block: one robot's foot-pose log for 100 filters that were reset to the same state and differ in the
    block alone.  Every tick: status, increment, lin_rate measurement against the per-filter oracles.  The log must tell the filters
    apart: on at least 3 ticks the increment of two filters differs by more than 1e-6 (the oracle alone: 9 such ticks with thresholds
    and delays varied, B = 65; none with uniform parameters).  The statuses are uniform across the filters on such a log -- the
    classifier's strike / break triggers have fixed levels -- and are not asserted to vary."""
    import torch
    from pronto_amd import batch as pa
    B = 100
    dev = torch.device("cuda:0")
    vec, quat, P0 = Workload(B, n_states=n, dt_us=2000).initial_state()
    vec, quat, P0 = (np.ascontiguousarray(np.repeat(a[..., :1], B, axis=-1)) for a in (vec, quat, P0))
    blk = draws(B)
    est = pa.BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    est.reset(vec, quat, P0)
    est.legodo_init(*SCHMITT, True)
    est.legodo_set_param_block(blk)
    wq = np.ascontiguousarray(est.get_head()[1])
    want = open_loop_oracle(oracle, blk, wq)
    d_delta = torch.zeros((7, B), dtype=torch.float64, device=dev)
    d_status = torch.zeros(B, dtype=torch.float64, device=dev)
    d_lo = torch.zeros((6, B), dtype=torch.float64, device=dev)
    d_mask = torch.zeros(B, dtype=torch.uint8, device=dev)
    apart = 0
    for k, (utime, feet, forces, _) in enumerate(gait(1, 500, seed=27)):
        est.legodo_update(utime, np.ascontiguousarray(feet[:, 0]), np.ascontiguousarray(forces[:, 0]), -1.0, -1.0, d_delta, d_status, d_lo, d_mask)
        od, os_, op = want[k]
        g_delta, g_status, g_lo, g_mask = (t.cpu().numpy() for t in (d_delta, d_status, d_lo, d_mask))
        assert np.array_equal(g_status, os_), k
        assert np.max(np.abs(g_delta[0:3] - od[0:3])) < 1e-11 and same_rotation(g_delta[3:7], od[3:7]) < 1e-12, k
        z, Rd, mask = lin_rate(od, os_, op, utime, blk)
        assert np.array_equal(g_mask, mask), k
        on = mask.astype(bool)
        assert np.max(np.abs(g_lo[0:3, on] - z[:, on]), initial=0.0) < 1e-8 and np.allclose(g_lo[3:6, on], Rd[:, on], rtol=1e-14, atol=0), k
        apart += int(np.max(np.max(od[0:3], axis=1) - np.min(od[0:3], axis=1)) > 1e-6)
    print("ticks on which the increment tells two filters apart:", apart)
    assert apart >= 3
    est.close()


# ---- 2, 3. the pair kernels against the oracle chain -------------------------------------------------------------------------
def pair_chain(oracle, n, kind, mode, B, blk, est=None, q_block=None, param_block=True, dense_p0=None):
    """test_pair_call_against_the_oracle_chain_on_gpu / ..._in_the_six_row_modes_... with a parameter block: per tick po_imu_process_step,
    then on the ORACLE filter's own pose after that step po_torque_adjust -> po_fk -> po_leg_update_wc of THAT filter's robot ->
    LegOdoCommon's measurement with THAT filter's noises -> po_indexed_update, the zero_initial_velocity counter per filter.  est = None:
    the oracle chain alone (what it yields must stay finite and reach the counts before a kernel is held against it).
    q_block [4, B]: a process noise per filter (pb_set_process_noise_block), the oracle's process step made per filter; param_block =
    False: blk is uniform_block(B) and the context gets its values as the scalars of pb_legodo_init and of the pair call; dense_p0: the
    seed of a dense SPD matrix added to the start covariance (test_gpu_parity.make_pair's).
    -> (updates applied, three-row fall-backs, statuses seen, the oracle filter)"""
    import legs
    from noise_block import oracle_noise_block, per_filter_oracle
    from util import embed21
    T, ZERO = 260, 4
    L = oracle.lib()
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    gain = np.array([7000, 10000, 10000, 10000, 10000, 10000] * 2, dtype=np.float32)
    w = Workload(B, n_states=n, dt_us=2000)
    vec, quat, P0 = w.initial_state()
    if dense_p0:
        from util import random_spd
        P0 = P0 + random_spd(n, B, 0.03, dense_p0)
    v21, P21 = embed21(vec, P0)
    ob = oracle.OracleBatch(v21, quat, P21)
    orc = PerFilterLegs(oracle, blk)
    zc = np.full(B, ZERO)
    q4 = w.process_noise()
    if est is not None:
        import torch
        dev = torch.device("cuda:0")
        est.set_constants(*oracle.constants())
        est.reset(vec, quat, P0)
        est.legodo_init(*SCHMITT, True)
        est.legodo_set_chain(*chain, gain)
        est.legodo_set_zero_initial_velocity(ZERO)
        if mode:
            est.legodo_set_measurement_mode(mode, 7.0, 8.0, 9.0)   # (the three noises: replaced by the block)
        r_call = (-1.0, -1.0)                                  # (the two noises: ignored with a block)
        if param_block:
            est.legodo_set_param_block(blk)
        else:
            assert mode == 0 and np.array_equal(blk, uniform_block(B))
            r_call = R_VXYZ
        if q_block is not None:
            d_q = torch.from_numpy(np.ascontiguousarray(q_block)).to(dev)   # (alive until the last call below has been read back)
            est.set_process_noise_block(d_q)
        lo = torch.zeros((6 if mode == 0 else 12, B), dtype=torch.float64, device=dev)
        mk = torch.zeros((2, B) if mode == 2 else (B,), dtype=torch.uint8, device=dev)
    bcast = kind.endswith("bcast")
    W = 1 if bcast else B
    src = legs.joint_gait(W, T, seed=27 if mode == 0 else 29) if kind.startswith("joints") else gait(W, T, seed=27)
    r5 = np.ascontiguousarray(blk[[_lib.PB_LEGPAR_R_XYZ, _lib.PB_LEGPAR_R_VXYZ, _lib.PB_LEGPAR_R_VANG, _lib.PB_LEGPAR_R_VXYZ_UNCERTAIN,
                                   _lib.PB_LEGPAR_R_VANG_UNCERTAIN]].T)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    n_upd = n_three = 0
    seen = set()
    for k, msg in enumerate(src):
        imu = w.imu_block(k)
        if bcast:
            imu = np.ascontiguousarray(np.repeat(imu[:, :1], B, axis=1))
        if kind.startswith("joints"):
            utime, jp, je, forces, _ = msg
            ofeet = legs.oracle_feet(L, chain, jp, je, gain)
        else:
            utime, ofeet, forces, _ = msg
        if est is not None:
            imu_in = np.ascontiguousarray(imu[:, 0]) if bcast else torch.from_numpy(imu).to(dev)
            if kind.startswith("joints"):
                a = (np.ascontiguousarray(jp[:, 0]), np.ascontiguousarray(je[:, 0]), np.ascontiguousarray(forces[:, 0])) if bcast else \
                    tuple(torch.from_numpy(x).to(dev) for x in (jp, je, forces))
                est.step_legodo_joints(imu_in, q4, utime, *a, *r_call, lo, mk)
            else:
                est.step_legodo_feet(imu_in, q4, utime, torch.from_numpy(ofeet).to(dev), torch.from_numpy(forces).to(dev), *r_call, lo, mk)
            g_mask, g_lo = mk.cpu().numpy().reshape(-1, B), lo.cpu().numpy()
        if bcast:
            ofeet, forces = np.repeat(ofeet, B, axis=1), np.repeat(forces, B, axis=1)
        if q_block is None:
            ob.predict(imu, q4)
        else:
            per_filter_oracle(ob, oracle_noise_block(q_block, n), lambda q: ob.predict(imu, q))
        od, os_, op = orc.update(utime, np.ascontiguousarray(ofeet), forces.astype(np.float64), np.ascontiguousarray(ob.quat),
                                 wpos=np.ascontiguousarray(ob.vec[9:12]) if mode == 2 else None)
        valid = os_ >= 0
        zc[valid] -= 1                                    # rbis_legodo_update.cpp:264-268, reached for a valid status only
        zero = valid & (zc > 0)
        if mode == 0:
            od[0:3, zero] = 0.0
            z, Rd, mask = lin_rate(od, os_, op, utime, blk)
            if est is not None:
                assert np.array_equal(g_mask[0], mask), (k, g_mask[0], mask)
                assert np.max(np.abs(g_lo[0:3, valid] - z[:, valid]), initial=0.0) < 1e-8, k
                assert np.allclose(g_lo[3:6, valid], Rd[:, valid], rtol=1e-14, atol=0), k
            ob.update_indexed([3, 4, 5], np.ascontiguousarray(z), np.ascontiguousarray(Rd), mask=mask)
            n_upd += int(valid.sum())
        else:
            z6, R6_ = np.zeros((6, B)), np.ones((6, B))
            m_of = np.zeros(B, dtype=int)
            idx6 = None
            for b in np.nonzero(valid)[0]:
                dt3, dq, cpos = od[0:3, b].copy(), od[3:7, b].copy(), orc.pos[:, b].copy()
                if zero[b]:
                    dt3[:] = 0.0
                    dq[:] = (1.0, 0.0, 0.0, 0.0)
                    cpos[:] = 0.0
                idx = np.zeros(6, dtype=np.int32)
                z, Rd = np.zeros(6), np.zeros(6)
                m = L.po_legodo_create_measurement(mode, dp(np.ascontiguousarray(r5[b])), dp(cpos), dp(dt3), dp(dq), int(utime), int(op[b]),
                                                   int(orc.pos_ok[b]), float(os_[b]), idx.ctypes.data_as(C.POINTER(C.c_int)), dp(z), dp(Rd))
                m_of[b] = m
                if m == 6:
                    assert idx6 is None or list(idx) == idx6
                    idx6 = list(idx)
                    z6[:, b], R6_[:, b] = z, Rd
                else:
                    assert mode == 2 and m == 3 and list(idx[:3]) == [3, 4, 5]
                    z6[3:6, b], R6_[3:6, b] = z[:3], Rd[:3]
            six, three = m_of == 6, m_of == 3
            if est is not None:
                assert np.array_equal(g_mask[0], six.astype(np.uint8)), (k, g_mask[0], six)
                if mode == 2:
                    assert np.array_equal(g_mask[1], three.astype(np.uint8)), (k, g_mask[1], three)
                assert np.max(np.abs(g_lo[0:6][:, six] - z6[:, six]), initial=0.0) < 1e-8, k
                assert np.allclose(g_lo[6:12][:, six], R6_[:, six], rtol=1e-13, atol=0), k
                assert np.max(np.abs(g_lo[3:6][:, three] - z6[3:6][:, three]), initial=0.0) < 1e-8, k
                assert np.allclose(g_lo[9:12][:, three], R6_[3:6][:, three], rtol=1e-13, atol=0), k
            if six.any():
                ob.update_indexed(idx6, np.ascontiguousarray(z6), np.ascontiguousarray(R6_), mask=six.astype(np.uint8))
            if three.any():
                ob.update_indexed([3, 4, 5], np.ascontiguousarray(z6[3:6]), np.ascontiguousarray(R6_[3:6]), mask=three.astype(np.uint8))
            n_upd += int(six.sum()) + int(three.sum())
            n_three += int(three.sum())
        seen.update(np.unique(os_).tolist())
    assert np.all(np.isfinite(ob.vec)) and np.all(np.isfinite(ob.cov))
    if est is not None:
        from test_gpu_parity import check
        check(est, ob)
        pose, info = est.legodo_get(B - 1)
        t, q, oi = orc.get(B - 1)
        assert np.max(np.abs(pose[0:3] - t)) < 1e-9 and info[0] == oi[0] and info[1] == oi[1] and info[2] == oi[2]
    return n_upd, n_three, seen, ob


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("kind", ["joints_dev", "joints_bcast", "feet_dev"])
def test_pair_call_with_a_parameter_block_against_the_oracle_chain_on_gpu(oracle, n, kind):
    """k_pair_legpar (n = 15) / k_pair_quad_legpar (n = 21), lin_rate, all eleven rows per filter; B = 100 is one full and one ragged
    tile.  (The oracle chain alone with the wider noise ranges [4, 12] / [8, 20]: 25 432-25 900 of 26 000 updates, all three statuses,
    everything finite.)"""
    from pronto_amd import batch as pa
    B = 100
    est = pa.BatchEstimator(B, n_states=n)
    n_upd, _, seen, _ = pair_chain(oracle, n, kind, 0, B, draws(B, standing=True), est)
    print("updates applied:", n_upd, "of", B * 260)
    assert n_upd > B * 260 // 10 and seen == {-1.0, 0.0, 1.0}
    est.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind", ["joints_dev", "joints_bcast"])
def test_pair_call_in_the_six_row_modes_with_a_parameter_block_on_gpu(oracle, n, mode, kind):
    """the same in LegOdoCommon's six-row modes: r_vang, r_vang_uncertain and r_xyz per filter, 0.5x ... 2x the values of
    test_pair_call_in_the_six_row_modes_against_the_oracle_chain_on_gpu, which also sets the counts asked for here."""
    from pronto_amd import batch as pa
    B = 65
    est = pa.BatchEstimator(B, n_states=n)
    n_upd, n_three, seen, _ = pair_chain(oracle, n, kind, mode, B, draws(B), est)
    print("updates applied:", n_upd, "of", B * 260, "three-row fall-backs:", n_three)
    assert n_upd > B * 260 // 10 and n_upd - n_three > B * 260 // 20 and seen == {-1.0, 0.0, 1.0}
    assert mode == 1 or n_three > 0
    est.close()


# ---- 4. a uniform block is the scalar path, bit for bit -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("standing", [False, True])
def test_a_uniform_block_is_the_scalar_path_bit_for_bit_on_gpu(n, mode, standing):
    """50 ticks of the stand-alone odometry call (even ticks) and the pair call (odd ticks) on per-filter joint blocks, B = 130: the
    head's checksum after every tick and every filter's odometry state at the end are those of a context driven with the scalars when
    (a) a block that holds one value per row is set (and the calls' own noises are garbage), (b) the block is dropped (NULL) and set
    again half way, (c) another block was set before pb_legodo_init, which drops it."""
    import torch
    import legs
    from pronto_amd import batch as pa
    B, T = 130, 50
    dev = torch.device("cuda:0")
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    w = Workload(B, n_states=n, dt_us=2000)
    x0, q4 = w.initial_state(), w.process_noise()
    msgs = [tuple(torch.from_numpy(x).to(dev) for x in m[1:4]) + (m[0],) for m in legs.joint_gait(B, T, seed=31)]
    imus = [torch.from_numpy(w.imu_block(k)).to(dev) for k in range(T)]
    blk = uniform_block(B)

    def run(variant):
        est = pa.BatchEstimator(B, n_states=n)
        est.reset(*x0)
        if variant == "init_drops":
            est.legodo_init(300.0, 600.0, 1000, 2000, True)
            est.legodo_set_param_block(draws(B, standing=True))
        est.legodo_init(*SCHMITT, True)
        est.legodo_set_chain(*chain, None)
        est.legodo_set_contact_mode(standing, *STANDING)
        if mode:
            est.legodo_set_measurement_mode(mode, *R6)
        lo = torch.zeros((6 if mode == 0 else 12, B), dtype=torch.float64, device=dev)
        mk = torch.zeros((2, B) if mode == 2 else (B,), dtype=torch.uint8, device=dev)
        with_block = variant in ("block", "toggle")
        if with_block:
            est.legodo_set_param_block(blk)
        sums = []
        for k, (jp, je, ff, utime) in enumerate(msgs):
            if variant == "toggle" and k == 20:
                est.legodo_set_param_block(None)
                with_block = False
            if variant == "toggle" and k == 33:
                est.legodo_set_param_block(blk)
                with_block = True
            r, ru = (123.0, 456.0) if with_block else R_VXYZ
            if k % 2 == 0:
                est.legodo_update_joints(utime, jp, None, ff, r, ru, lo_out=lo, mask_out=mk)
                est.predict(imus[k], q4)
            else:
                est.step_legodo_joints(imus[k], q4, utime, jp, None, ff, r, ru, lo, mk)
            sums.append((est.state_checksum(), lo.cpu().numpy().tobytes(), mk.cpu().numpy().tobytes()))
        odo = [(p.tobytes(), tuple(i)) for p, i in (est.legodo_get(b) for b in (0, 63, 64, B - 1))]
        est.close()
        return sums, odo

    want = run("scalars")
    assert len({s[0] for s in want[0]}) == T    # every tick moves the state
    for variant in ("block", "toggle", "init_drops"):
        got = run(variant)
        assert got[0] == want[0] and got[1] == want[1], variant


# ---- 5. the "standing" contact mode with per-filter total_force / standing_schmitt_level ---------------------------------------
@pytest.mark.gpu
def test_standing_mode_with_per_filter_force_and_level_on_gpu(oracle):
    """open loop, B = 65, per-filter foot poses and forces: status and increment against per-robot po_leg_set_contact_mode"""
    import torch
    from pronto_amd import batch as pa
    B, n, T = 65, 15, 300
    dev = torch.device("cuda:0")
    vec, quat, P0 = Workload(B, n_states=n, dt_us=2000).initial_state()
    blk = draws(B, standing=True)
    est = pa.BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    est.reset(vec, quat, P0)
    est.legodo_init(*SCHMITT, True)
    est.legodo_set_contact_mode(True, 1.0, 0.0)     # (the two values: replaced by the block)
    est.legodo_set_param_block(blk)
    orc = PerFilterLegs(oracle, blk, standing=True)
    wq = np.ascontiguousarray(est.get_head()[1])
    d_delta = torch.zeros((7, B), dtype=torch.float64, device=dev)
    d_status = torch.zeros(B, dtype=torch.float64, device=dev)
    seen, feet_seen = set(), set()
    for k, (utime, feet, forces, _) in enumerate(gait(B, T, seed=9)):
        est.legodo_update(utime, torch.from_numpy(feet).to(dev), torch.from_numpy(forces).to(dev), -1.0, -1.0, d_delta, d_status)
        od, os_, op = orc.update(utime, feet, forces, wq)
        g_delta, g_status = d_delta.cpu().numpy(), d_status.cpu().numpy()
        assert np.array_equal(g_status, os_), k
        assert np.max(np.abs(g_delta[0:3] - od[0:3])) < 1e-11 and same_rotation(g_delta[3:7], od[3:7]) < 1e-12, k
        seen.update(np.unique(os_).tolist())
    for b in (0, 31, B - 1):
        pose, info = est.legodo_get(b)
        t, q, oi = orc.get(b)
        assert np.max(np.abs(pose[0:3] - t)) < 1e-10 and info[0] == oi[0] and info[1] == oi[1] and info[2] == oi[2]
        feet_seen.add(int(info[0]))
    assert seen == {-1.0, 0.0, 1.0}
    est.close()


# ---- 6. argument checks ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_parameter_block_argument_checks_on_gpu():
    import torch
    from pronto_amd import batch as pa
    B = 70
    est = pa.BatchEstimator(B, n_states=15)
    L, h = est._L, est._h
    good = draws(B, standing=True)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    err = lambda: (L.pb_last_error(h) or b"").decode()
    assert L.pb_legodo_set_param_block(h, ptr(good), _lib.PB_HOST) == _lib.PB_ERR_STATE and "pb_legodo_init" in err()
    est.legodo_init(*SCHMITT, True)
    assert L.pb_legodo_set_param_block(h, ptr(good), _lib.PB_HOST_BROADCAST) == _lib.PB_ERR_ARG
    assert L.pb_legodo_set_param_block(h, ptr(good), 7) == _lib.PB_ERR_ARG
    assert L.pb_legodo_set_param_block(h, ptr(good), _lib.PB_HOST) == _lib.PB_OK

    # a twin context takes the same good calls and none of the refused ones: both then make the same of the same messages
    twin = pa.BatchEstimator(B, n_states=15)
    twin.legodo_init(*SCHMITT, True)
    twin.legodo_set_param_block(good)
    x0 = Workload(B, n_states=15).initial_state()
    est.reset(*x0)
    twin.reset(*x0)
    dev = torch.device("cuda:0")
    log = [(u, torch.from_numpy(f).to(dev), torch.from_numpy(z).to(dev)) for u, f, z, _ in gait(B, 40, seed=4)]
    calls = [0]

    def odometry(e):
        """40 messages more: what the block in force makes of them"""
        lo = torch.zeros((6, B), dtype=torch.float64, device=dev)
        mk = torch.zeros(B, dtype=torch.uint8, device=dev)
        out = []
        for utime, feet, forces in log:
            e.legodo_update(utime + calls[0] * 100_000, feet, forces, 1.0, 2.0, lo_out=lo, mask_out=mk)
            out.append((lo.cpu().numpy().tobytes(), mk.cpu().numpy().tobytes()))
        return out

    def same():
        got, want = odometry(est), odometry(twin)
        calls[0] += 1
        return got == want

    assert same()
    bad_entries = [(_lib.PB_LEGPAR_R_VXYZ, 5, -0.1), (_lib.PB_LEGPAR_R_VXYZ_UNCERTAIN, 68, np.nan), (_lib.PB_LEGPAR_R_VANG, 0, np.inf),
                   (_lib.PB_LEGPAR_R_VANG_UNCERTAIN, 1, -1.0), (_lib.PB_LEGPAR_R_XYZ, 2, np.nan),
                   (_lib.PB_LEGPAR_SCHMITT_HIGH, 64, 100.0),                     # below its low threshold
                   (_lib.PB_LEGPAR_SCHMITT_LOW_DELAY, 3, 1000.5), (_lib.PB_LEGPAR_SCHMITT_LOW_DELAY, 3, -1.0),
                   (_lib.PB_LEGPAR_SCHMITT_HIGH_DELAY, 67, 2.5e9), (_lib.PB_LEGPAR_SCHMITT_HIGH_DELAY, 67, np.nan)]
    for row, b, v in bad_entries:
        bad = good.copy()
        bad[row, b] = v
        bad[row, b + 1] = v                  # the FIRST offending filter is the one named
        assert L.pb_legodo_set_param_block(h, ptr(bad), _lib.PB_HOST) == _lib.PB_ERR_ARG, (row, b, v)
        assert "filter %d, row %d " % (b, row) in err(), err()
    assert same()                            # the block set before the refused calls is still in force
    # no block: the scalars, which make something else of the messages; a refused call leaves them in force
    est.legodo_set_param_block(None)
    assert not same()
    bad = good.copy()
    bad[0, 0] = -1.0
    assert L.pb_legodo_set_param_block(h, ptr(bad), _lib.PB_HOST) == _lib.PB_ERR_ARG
    twin.legodo_set_param_block(None)
    for e in (est, twin):                    # (the two odometry states went apart: start them over, which keeps "no block")
        e.legodo_init(*SCHMITT, True)
    assert same()
    # a device block is copied (unvalidated): the caller's tensor is free on return
    d = torch.from_numpy(good).to(dev)
    est.legodo_set_param_block(d)
    d.zero_()
    del d
    twin.legodo_set_param_block(good)
    assert same()
    twin.close()
    with pytest.raises(ValueError):
        est.legodo_set_param_block(good[:, :-1].copy())
    est.close()


# ---- 7. ownership ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
def test_the_block_is_the_contexts_and_leaves_the_state_alone_on_gpu(n):
    """in the manner of test_context_memory.py: its fixed call sequence S on a fresh context, and on one whose parameter block is set
    (host and device blocks in turn), dropped and set again between the steps of S, five times in all -- the head's checksum after
    every step is the same -- then pb_destroy; a context created after that computes S again."""
    import torch
    import test_context_memory as tcm
    inp = tcm.Inputs(n)

    def run(between):
        est = tcm.new_estimator(n)
        est.legodo_init(*SCHMITT, True)
        sums = []
        for k, step in enumerate(tcm.steps_of_s(est, inp)):
            step()
            sums.append(est.state_checksum())
            between(est, k)
            assert est.state_checksum() == sums[-1], k
        est.close()
        return sums

    want = run(lambda est, k: None)
    blk = draws(tcm.B, standing=True)

    def reset_block(est, k):
        if k == 2:
            est.legodo_set_param_block(None)
        est.legodo_set_param_block(torch.from_numpy(blk).to("cuda:0") if k % 2 else blk)

    assert run(reset_block) == want
    assert run(lambda est, k: None) == want
