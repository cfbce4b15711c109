"""CPU tier of the ground-truth scorer: the per-lane functions of pronto_amd/csrc/rbis_score.hpp, compiled with g++
(tests/score_host.cpp), against the numpy restatement of drift_per_distance.py (tests/score_ref.py).

Pass condition (score_common.compare): window counts, n_ddt, which messages closed a window and the utimes IDENTICAL; lengths in
metres and angles in degrees to 1e-12 absolute; percent_ddt and its sums to 1e-9 relative over windows with dist >= 0.1 m."""
import numpy as np
import pytest

import score_common as sc
import score_ref as sr

B, N = 200, 120
DRIFT, ABS = sc.R("DRIFT"), sc.R("ABS")


@pytest.fixture(scope="module")
def lib():
    return sc.build_host()


@pytest.fixture(scope="module")
def msgs():
    return sc.scenario(B, N)


@pytest.mark.parametrize("distance_threshold", [0.0, 0.25])
@pytest.mark.parametrize("per_filter_times", [False, True])
def test_scenario_against_the_script(lib, msgs, distance_threshold, per_filter_times):
    ref, ref_closed = sc.run_ref(msgs, B, 10.0, distance_threshold, per_filter_times=per_filter_times)
    sc.check_witness(ref)
    host = sc.HostScore(lib, B, 10.0, distance_threshold)
    for k, (u, ut, p7, v, e7) in enumerate(msgs):
        closed = host.message(u, ut if per_filter_times else None, p7, v, e7, DRIFT | ABS)
        np.testing.assert_array_equal(closed, ref_closed[k], err_msg="message %d" % k)
    print("worst abs / rel difference:", sc.compare(ref, host.rows, host.counts))
    # the scenario does what it is for
    nw = ref.n_windows
    assert nw.min() >= 9 and (distance_threshold == 0 or nw.max() > 20)
    assert nw[sc.STILL] > 0 and ref.n_ddt[sc.STILL] == 0 and np.isinf(ref.percent_ddt[sc.STILL])       # truth that does not move
    assert np.all(np.delete(ref.n_ddt, sc.STILL) == np.delete(nw, sc.STILL))
    assert ref.abs_n[0] == N - 5 and ref.abs_n[1] == N                                                  # the first 5 messages invalid
    if distance_threshold == 0 and not per_filter_times:
        # every window of YAW_CROSS spans 11 messages: truth yaws by 178.2 deg, the estimate by 182.6 = -177.4 deg
        assert abs(ref.rpy_error[2, sc.YAW_CROSS] - (-177.4 - 178.2)) < 0.1
        assert abs(np.sqrt(ref.sum_yaw_sq[sc.YAW_CROSS] / nw[sc.YAW_CROSS]) - 4.4) < 0.1


def test_pose_algebra_against_botpy_restatement(lib):
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = rng.normal(size=7) * 3, rng.normal(size=7) * 3  # quaternions NOT normalised, as the script takes them
        out = np.zeros(7)
        lib.sh_transform_relative(sc.ptr(a), sc.ptr(b), sc.ptr(out))
        t, q = sr.transform_relative(a[:3, None], a[3:, None], b[:3, None], b[3:, None])
        scale = max(1.0, float(np.max(np.abs(np.concatenate([t[:, 0], q[:, 0]])))))
        assert np.max(np.abs(out - np.concatenate([t[:, 0], q[:, 0]]))) <= 1e-12 * scale
    for a, want in ((180.0, 180.0), (-180.0, 180.0), (181.0, -179.0), (-355.6, 4.4), (540.0, 180.0), (0.0, 0.0)):
        assert abs(lib.sh_wrap_deg(a) - want) < 1e-12 and abs(float(sr.wrap_deg(a)) - want) < 1e-12


def analytic(lib, p_of, q_of, ep_of, eq_of, n=34, Bn=3):
    host = sc.HostScore(lib, Bn, 10.0, 0.0)
    for k in range(n):
        pose = np.repeat(np.concatenate([p_of(k), q_of(k)])[:, None], Bn, axis=1)
        est = np.repeat(np.concatenate([ep_of(k), eq_of(k)])[:, None], Bn, axis=1)
        host.message((k + 1) * 1_000_000, None, pose, None, est, DRIFT | ABS)
    assert np.all(host.counts[sc.R("N_WINDOWS")] == 3)
    return host


def yaw_quat(deg):
    return sc.rpy_quat(0.0, 0.0, np.radians(deg))


def test_estimate_equal_to_truth_has_zero_error(lib):
    p = lambda k: np.array([0.3 * k, 0.1 * k * k / 30, 0.5])  # noqa: E731
    q = lambda k: sc.rpy_quat(0.1, -0.05, 0.02 * k)           # noqa: E731
    h = analytic(lib, p, q, p, q)
    for name in ("LAST_POS_ERROR_NORM", "SUM_ERR", "SUM_ERR_SQ", "MAX_ERR", "SUM_YAW_SQ", "LAST_PERCENT_DDT", "SUM_PDDT", "ABS_SUM_SQ", "ABS_MAX",
                 "ABS_SUM_YAW_SQ"):
        np.testing.assert_array_equal(h.rows[sc.R(name)], 0.0, err_msg=name)
    pe = sc.R("LAST_POS_ERROR")
    np.testing.assert_array_equal(h.rows[pe:pe + 7], 0.0)  # pos_error, its norm, rpy_error


def test_two_percent_translation_drift(lib):
    """truth 1 m per message along x, the estimate 1.02 m per message, identity rotations: every window has percent_ddt = 2"""
    ident = lambda k: np.array([1.0, 0, 0, 0])  # noqa: E731
    h = analytic(lib, lambda k: np.array([0.25 * k, 0.0, 0.0]), ident, lambda k: np.array([0.25 * k * 1.02, 0.0, 0.0]), ident)
    assert np.max(np.abs(h.rows[sc.R("LAST_PERCENT_DDT")] - 2.0)) <= 1e-12
    assert np.max(np.abs(h.rows[sc.R("SUM_PDDT")] / 3 - 2.0)) <= 1e-12
    assert np.max(np.abs(h.rows[sc.R("LAST_DISTANCE")] - 11 * 0.25)) <= 1e-12
    np.testing.assert_array_equal(h.rows[sc.R("LAST_TIME_ELAPSED")], -11.0)  # the script's sign


def test_one_degree_per_window_yaw_drift(lib):
    """the estimate yaws 1 deg per window (11 messages) faster than truth: rpy_error[2] = 1"""
    p = lambda k: np.array([0.1 * k, 0.0, 0.0])  # noqa: E731
    h = analytic(lib, p, lambda k: yaw_quat(2.0 * k), p, lambda k: yaw_quat((2.0 + 1.0 / 11) * k))
    assert np.max(np.abs(h.rows[sc.R("LAST_RPY_ERROR") + 2] - 1.0)) <= 1e-12
    assert np.max(np.abs(np.sqrt(h.rows[sc.R("SUM_YAW_SQ")] / 3) - 1.0)) <= 1e-12


def test_metric_and_no_data(lib, msgs):
    host = sc.HostScore(lib, B, 10.0, 0.0)
    for m in (sc.R("MEAN_PDDT"), sc.R("RMS_DRIFT"), sc.R("ATE_RMSE")):
        assert not host.metric(m)[1].any()
    for u, ut, p7, v, e7 in msgs[:40]:
        host.message(u, None, p7, v, e7, DRIFT | ABS)
    v, has = host.metric(sc.R("MEAN_PDDT"))
    assert not has[sc.STILL] and has.sum() == B - 1
    np.testing.assert_allclose(v[has], host.rows[sc.R("SUM_PDDT")][has] / host.counts[sc.R("N_DDT")][has], rtol=1e-15)
    v, has = host.metric(sc.R("ATE_RMSE"))
    assert has.all()
    np.testing.assert_allclose(v, np.sqrt(host.rows[sc.R("ABS_SUM_SQ")] / host.counts[sc.R("ABS_N")]), rtol=1e-15)
