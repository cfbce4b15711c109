"""GPU tier of the yaw-lock handler (pb_step_yawlock_joints / pb_yawlock_update_joints, k_step_yawlock / k_yawlock_form).

Per case one batch of filters with different initial states runs IMU predicts and joint-state messages three ways:
  fused     pb_predict + pb_step_yawlock_joints
  composed  pb_predict + pb_yawlock_update_joints + pb_update_indexed_orient / pb_update_indexed with the two masks
  oracle    oracle/po.py predict + tests/yawlock_ref.py on the oracle's own head + the oracle's indexed update
(a) fused vs oracle: discrete state identical, posterior within 1e-9 (the project's bound for long runs against the oracle);
(b) fused vs composed: <= 1e-12 relative; (c) a filter without an update on a message is bit-identical before and after;
(d) a run through pb_set_output_slot gives the same head."""
import numpy as np
import pytest

import legs
import yawlock_ref as yr
from util import rel

pytestmark = pytest.mark.gpu

B, T = 2048, 1500
PERIOD, THRESHOLD_DEG, DISABLE_S = 25, 1.5, 0.2
R_BIAS_DEG, R_YAW_DEG = 0.05, 1.0


def joints(B, seed):
    """standing robots in joint space: base pose + slow sway per robot; at message 600 a third of them turn the left hip yaw by
    2.0 deg (above the slip threshold), a third by 1.4 deg (below it)"""
    rng = np.random.default_rng(seed)
    rows = legs.ATLAS_ROWS
    base = 0.3 * rng.normal(size=(legs.N_ROWS, B))
    for side, sgn in ((0, 1.0), (1, -1.0)):
        for j, (c, s) in enumerate(((0.05 * sgn, 0.02), (0.03 * sgn, 0.01), (-0.35, 0.05), (0.7, 0.05), (-0.35, 0.05), (-0.03 * sgn, 0.01))):
            base[rows[6 * side + j]] = c + s * rng.normal(size=B)
    f = rng.uniform(0.5, 1.5, B)
    grp = np.arange(B) % 3

    def at(k):
        jp = base.copy()
        t = k * 1e-3
        for side in (0, 1):
            jp[rows[6 * side + 2]] += 0.02 * np.sin(f * t)
            jp[rows[6 * side + 3]] -= 0.02 * np.sin(f * t)
        if k >= 600:
            jp[rows[0]] += np.where(grp == 0, np.radians(2.0), np.where(grp == 1, np.radians(1.4), 0.0))
        return np.ascontiguousarray(jp, dtype=np.float32)
    return at


def make(n, mode, chain):
    import torch
    from pronto_amd.batch import BatchEstimator
    from pronto_amd.synth import Workload
    from oracle import po
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    if n == 21:
        vec[15:18] = 1e-3 * np.random.default_rng(1).normal(size=(3, B))
    g, tol = po.constants()
    ests = []
    for _ in range(2):
        e = BatchEstimator(B, n_states=n, device=0)
        e.set_constants(g, tol)
        e.reset(vec, quat, P0)
        e.legodo_set_chain(*chain)
        e.yawlock_init(mode, PERIOD, True, THRESHOLD_DEG, DISABLE_S, R_BIAS_DEG, R_YAW_DEG)
        ests.append(e)
    v21 = np.zeros((21, B)); v21[:n] = vec
    P21 = np.zeros((21, 21, B)); P21[:n, :n] = P0
    return w, ests[0], ests[1], po.OracleBatch(v21, quat, P21), torch


def discrete(est, ref, who):
    for b in list(range(0, B, 97)) + [1, 2, B - 1]:
        _, info = est.yawlock_get(b)
        want = dict(counter=int(ref.counter[b]), lock_init=int(ref.lock_init[b]), disable_until=int(ref.disable_until[b]),
                    outcome=int(ref.outcome[b]), slips=int(ref.slips[b]))
        assert info == want, "%s filter %d: %s != %s" % (who, b, info, want)


@pytest.mark.parametrize("n,mode,per_filter", [(15, yr.YAW, False), (21, yr.YAWBIAS, False), (21, yr.YAW, True), (21, yr.YAWBIAS_YAW, False)])
def test_fused_step_against_oracle_and_composed(n, mode, per_filter):
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    w, fused, comp, ob, torch = make(n, mode, chain)
    dev = torch.device("cuda:0")
    ref = yr.YawLockRef(B, chain, mode, PERIOD, True, THRESHOLD_DEG, DISABLE_S, R_BIAS_DEG, R_YAW_DEG)
    q4 = w.process_noise()
    jp_at = joints(B, seed=7)
    rng = np.random.default_rng(5)
    zf, qf, mf = torch.zeros((2, B), dtype=torch.float64, device=dev), torch.zeros((4, B), dtype=torch.float64, device=dev), torch.zeros((2, B), dtype=torch.uint8, device=dev)
    zc, qc, mc = torch.zeros_like(zf), torch.zeros_like(qf), torch.zeros_like(mf)
    m = len(ref.idx)
    n_upd = n_idle_all = n_mixed = 0
    min_margin = np.inf
    for k in range(T):
        utime = (k + 1) * 1000
        imu = w.imu_block(k)
        standing_all = not (k < 50 or 800 <= k < 900)
        if per_filter:
            standing = np.full(B, standing_all, dtype=np.uint8)
            standing[(np.arange(B) % 5 == 1) & (k >= 1000)] = 0
            gyro = 0.01 * rng.normal(size=B)
            valid = np.ones(B, dtype=np.uint8)
            if k % 4 == 1:
                valid[np.arange(B) % 7 == 3] = 0
            utimes = utime + (np.arange(B, dtype=np.int64) % 11)
            d_ut, d_valid = torch.from_numpy(utimes).to(dev), torch.from_numpy(valid).to(dev)
        else:
            standing, gyro, valid, utimes, d_ut, d_valid = standing_all, float(0.01 * rng.normal()), None, utime, None, None
        jp = jp_at(k)
        d_jp = torch.from_numpy(jp).to(dev)
        for e in (fused, comp):
            e.predict(imu, q4)
            e.yawlock_set_standing(standing)
            e.yawlock_set_gyro(gyro)
        ob.predict(imu, q4)
        z, q, mask = ref.process(standing, gyro, ob.vec, ob.quat, utimes, jp, valid)
        min_margin = min(min_margin, ref.last_slip_margin_deg.min())
        ref.apply_oracle(ob, z, q, mask)
        any_upd = bool(mask.any())
        check_lanes = any_upd and not mask.any(axis=0).all() and n_mixed < 6
        if not any_upd or check_lanes:
            before = fused.state_checksum() if not any_upd else fused.get_head()
        fused.step_yawlock_joints(utime, d_jp, utimes=d_ut, valid=d_valid, z_out=zf, quat_out=qf, mask_out=mf)
        comp.yawlock_update_joints(utime, d_jp, utimes=d_ut, valid=d_valid, z_out=zc, quat_out=qc, mask_out=mc)
        if mask[0].any():
            comp.update_indexed(ref.idx, zc[:m].contiguous(), ref.R, mask=mc[0], quat_meas=qc)
        if mask[1].any():
            comp.update_indexed([17], zc[:1], [ref.r_bias], mask=mc[1])
        # the masks the kernels formed are the reference's (every message)
        assert np.array_equal(mf.cpu().numpy(), mask) and np.array_equal(mc.cpu().numpy(), mask), "message %d: masks differ" % k
        if not any_upd:      # (c) nobody gets an update: the whole state array is untouched
            assert fused.state_checksum() == before, "message %d: an idle message changed the state" % k
            n_idle_all += 1
        elif check_lanes:    # (c) the lanes without an update in a message where others have one
            after = fused.get_head()
            idle = ~mask.any(axis=0).astype(bool)
            for a, b_ in zip(before, after):
                assert np.array_equal(a[..., idle].view(np.uint64), b_[..., idle].view(np.uint64)), "message %d: an idle lane changed" % k
            assert not np.array_equal(before[0][..., ~idle], after[0][..., ~idle])
            n_mixed += 1
        n_upd += any_upd
        if any_upd and (n_upd % 8 == 1):
            discrete(fused, ref, "fused"), discrete(comp, ref, "composed")
            assert np.max(np.minimum(np.abs(qf.cpu().numpy() - q).max(axis=0), np.abs(qf.cpu().numpy() + q).max(axis=0))) <= 1e-9
    assert min_margin > 1e-6
    assert n_upd > 20 and (mode != yr.YAW or n_idle_all > T // 2)   # (only mode yaw has messages without any update)
    assert ref.slips.sum() > 0 or mode == yr.YAWBIAS
    assert n_mixed > 0 or not per_filter
    discrete(fused, ref, "fused"), discrete(comp, ref, "composed")
    fv, fq, fP, fll = fused.get_head()
    cv, cq, cP, cll = comp.get_head()
    errs_o = dict(vec=rel(fv, ob.vec[:n]), quat=rel(fq, ob.quat), cov=rel(fP, ob.cov[:n, :n]), ll=rel(fll, ob.ll))
    errs_c = dict(vec=rel(fv, cv), quat=rel(fq, cq), cov=rel(fP, cP), ll=rel(fll, cll))
    print("n=%d mode=%d: fused vs oracle %s; fused vs composed %s" % (n, mode, errs_o, errs_c))
    assert max(errs_o.values()) <= 1e-9, errs_o      # (a)
    assert max(errs_c.values()) <= 1e-12, errs_c     # (b)
    fused.close(), comp.close()


@pytest.mark.parametrize("n,mode", [(15, yr.YAW), (21, yr.YAWBIAS_YAW)])
def test_output_slot_run_gives_the_same_head(n, mode):
    """(d) every yaw-lock step writes into a checkpoint slot named with pb_set_output_slot (idle lanes are carried over to it)"""
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    w, plain, slots, _ob, torch = make(n, mode, chain)
    dev = torch.device("cuda:0")
    slots.history_reserve(3)
    q4 = w.process_noise()
    jp_at = joints(B, seed=7)
    for k in range(120):
        imu = w.imu_block(k)
        d_jp = torch.from_numpy(jp_at(k)).to(dev)
        for e in (plain, slots):
            e.predict(imu, q4)
            e.yawlock_set_standing(k >= 10)
            e.yawlock_set_gyro(0.001 * k)
        plain.step_yawlock_joints((k + 1) * 1000, d_jp)
        slots.set_output_slot(k % 3)
        slots.step_yawlock_joints((k + 1) * 1000, d_jp)
        assert slots._L.pb_head_slot(slots._h) == k % 3
    for a, b_ in zip(plain.get_head(), slots.get_head()):
        assert np.array_equal(a, b_)
    assert plain.yawlock_get(5)[1] == slots.yawlock_get(5)[1] and plain.yawlock_get(5)[1]["outcome"] != 0
    plain.close(), slots.close()


def test_argument_checks():
    """modes that measure the gyro bias are refused on 15 states; no chain -> PB_ERR_STATE; a pending predicted slot is refused"""
    import torch
    from pronto_amd import _lib, batch as pa
    chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS)
    w, e15, e21, _ob, _ = make(15, yr.YAW, chain)
    for mode in (yr.YAWBIAS, yr.YAWBIAS_YAW, 3):
        with pytest.raises(pa.PbError) as ei:
            e15.yawlock_init(mode, 1, False, 1.0, 1.0, 1.0, 1.0)
        assert ei.value.code == _lib.PB_ERR_ARG
    with pytest.raises(pa.PbError):
        e15.yawlock_init(yr.YAW, 0, False, 1.0, 1.0, 1.0, 1.0)
    jp = torch.zeros((legs.N_ROWS, B), dtype=torch.float32, device="cuda:0")
    e15.history_reserve(2)
    e15.set_pred_slot(1)
    with pytest.raises(pa.PbError) as ei:
        e15.step_yawlock_joints(1000, jp)
    assert ei.value.code == _lib.PB_ERR_STATE
    e15.step_yawlock_joints(1000, jp)     # the refusal forgot the slot
    from pronto_amd.batch import BatchEstimator
    bare = BatchEstimator(B, n_states=15, device=0)
    vec, quat, P0 = w.initial_state()
    bare.reset(vec, quat, P0)
    bare.yawlock_init(yr.YAW, 1, False, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(pa.PbError) as ei:
        bare.step_yawlock_joints(1000, jp)
    assert ei.value.code == _lib.PB_ERR_STATE
    bare.close(), e15.close(), e21.close()
