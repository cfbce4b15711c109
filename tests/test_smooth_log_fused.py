"""pb_smooth_log_fused: whole-log RTS smoothing with bounded memory where every forward and recompute step is ONE fused launch
(pb_step_legodo's semantics; the recompute step writes the window's predicted and filtered slots together, pb_set_pred_slot +
pb_set_output_slot).  Runs on the MI355X."""
import numpy as np
import pytest

from smoother_ref import oracle_forward, oracle_smooth_step, start_of
from util import rel

from pronto_amd.synth import Workload

TOL = 1e-9
pytestmark = pytest.mark.gpu


def _est(oracle, w, n, B, slots):
    from pronto_amd.batch import BatchEstimator
    est = BatchEstimator(B, n_states=n)
    est.set_constants(*oracle.constants())
    vec, quat, P0, q4 = start_of(w)
    est.reset(vec, quat, P0)
    est.history_reserve(slots)
    return est, q4


def _fused_log(est, streams, q4, dt, K, first_slot=1):
    got, order = {}, []

    def sink(step, slot):
        order.append(step)
        got[step] = est.get_slot(slot)
    est.smooth_log_fused(*streams, q4, dt, K, first_slot=first_slot, sink=sink)
    return got, order


@pytest.mark.parametrize("n", [15, 21])
def test_smooth_log_fused_equals_the_all_checkpoints_fused_pass_bit_for_bit(oracle, n):
    import torch
    B, T, K, dt = 37, 50, 7, 1e-3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    ref, q4 = _est(oracle, w, n, B, 2 * T + 2)
    for k in range(T):
        ref.set_pred_slot(2 * k)
        ref.set_output_slot(2 * k + 1)
        ref.step_legodo(imu[k], lo[k], mask[k], q4)
    want, nxt = {}, 2 * (T - 1) + 1
    for k in range(T - 2, -1, -1):
        out = 2 * T + (k % 2)
        ref.smooth_step(2 * (k + 1), nxt, 2 * k + 1, out, dt)
        want[k] = ref.get_slot(out)
        nxt = out
    ref.close()
    # the head afterwards: T plain pb_step_legodo calls
    plain, _ = _est(oracle, w, n, B, 1)
    for k in range(T):
        plain.step_legodo(imu[k], lo[k], mask[k], q4)
    final = plain.get_head()
    plain.close()
    est, _ = _est(oracle, w, n, B, 0)
    est.history_reserve(est.smooth_log_slots(T, K) + 1)
    got, order = _fused_log(est, [torch.from_numpy(a).to(dev) for a in (imu, lo, mask)], q4, dt, K)
    assert order == list(range(T - 2, -1, -1))
    for k in range(T - 1):
        for a, b in zip(got[k], want[k]):
            assert np.array_equal(a, b), k
    for a, b in zip(est.get_head(), final):
        assert np.array_equal(a, b)
    # against pb_smooth_log (the process step and the update as two launches: another rounding)
    est2, _ = _est(oracle, w, n, B, est.smooth_log_slots(T, K) + 1)
    old = {}
    est2.smooth_log(*(torch.from_numpy(a).to(dev) for a in (imu, lo, mask)), q4, dt, K, first_slot=1,
                    sink=lambda step, slot: old.__setitem__(step, est2.get_slot(slot)))
    worst = max(rel(a, b) for k in range(T - 1) for a, b in zip(got[k][:3], old[k][:3]))
    print("n=%d: pb_smooth_log_fused vs pb_smooth_log %.1e" % (n, worst))
    assert worst <= 1e-12, worst
    est2.close()
    est.close()


@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("T,K", [(23, 1), (23, 4), (31, 5), (16, 16)])
def test_smooth_log_fused_matches_the_oracle(oracle, n, T, K):
    """Every smoothed step against the oracle's recursion over its own forward pass; ragged last stretches."""
    import torch
    B, dt = 29, 1e-3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    est, q4 = _est(oracle, w, n, B, 0)
    est.history_reserve(est.smooth_log_slots(T, K))
    got, _ = _fused_log(est, [torch.from_numpy(a).to(dev) for a in (imu, lo, mask)], q4, dt, K, first_slot=0)
    est.close()
    hist = oracle_forward(oracle, w, n, T, B)
    nxt, worst = hist[T - 1][1], 0.0
    for k in range(T - 2, -1, -1):
        nxt = oracle_smooth_step(oracle, hist[k + 1][0], nxt, hist[k][1], dt)
        v, q, P, _ = got[k]
        worst = max(worst, rel(v, nxt[0][:n]), rel(q, nxt[1]), rel(P, nxt[2][:n, :n]))
    assert worst < TOL, worst


def test_smooth_log_fused_too_few_slots_leaves_the_head_usable(oracle):
    import torch
    from pronto_amd.batch import PbError
    n, B, T, K = 15, 64, 12, 3
    dev = torch.device("cuda:0")
    w = Workload(B, n_states=n)
    imu, lo, mask = w.streams(0, T)
    est, q4 = _est(oracle, w, n, B, 4)
    est.set_output_slot(0)
    est.step_legodo(imu[0], lo[0], mask[0], q4)   # the head lives in slot 0 now
    head = est.get_head()
    est.set_pred_slot(2)
    with pytest.raises(PbError) as e:
        est.smooth_log_fused(*(torch.from_numpy(a).to(dev) for a in (imu, lo, mask)), q4, 1e-3, K)
    assert e.value.code == 4
    assert est._L.pb_head_slot(est._h) == -1          # back in the context's own array
    for a, b in zip(est.get_head(), head):
        assert np.array_equal(a, b)
    before = est.state_checksum(2)
    est.step_legodo(imu[1], lo[1], mask[1], q4)      # usable, and no slot left pending
    assert est.state_checksum(2) == before
    est.close()
