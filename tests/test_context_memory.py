"""The context's device memory (dev_alloc / dev_release, pb_ctx.hpp): buffers that are re-made while the context is in use, and
whole life cycles.  Every device buffer of a context has one owner, so a buffer that is released must neither take a live one with it
nor leave its contents behind, and pb_destroy must free exactly what the families allocated.

A fixed call sequence S runs on a fresh context and on contexts whose checkpoint slots, staging buffers and joint-filter state are
re-made -- and whose handler families are initialised twice -- between its steps: the head's checksum after every step of S is the
same, bit for bit.  B = 100 leaves the last 64-filter tile ragged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 100
ROWS = 33   # joint rows of one message (the Atlas chain reads rows below 28)


class Inputs:
    """the inputs of S and the joint-state messages, made once per state size"""

    def __init__(self, n):
        from pronto_amd.synth import Workload
        w = Workload(B, n_states=n)
        self.n = n
        self.x0 = w.initial_state()
        self.q4 = w.process_noise()
        self.imu, self.lo, self.mask = w.streams(0, 2)
        rng = np.random.default_rng(11)
        self.z1 = 0.01 * rng.normal(size=(1, B))
        self.r1 = np.full((1, B), 0.05 ** 2)
        self.z6 = 0.01 * rng.normal(size=(6, B))
        a = rng.normal(size=(6, 6, B))
        r6 = np.einsum("ikb,jkb->ijb", a, a) * 1e-3 + np.eye(6)[:, :, None] * 0.02   # SPD, full, per filter
        self.r6 = np.ascontiguousarray(r6.reshape(36, B))
        self.jp = [(0.4 * np.sin(0.3 * k + np.arange(ROWS)[:, None] + 0.1 * np.arange(B)[None, :])).astype(np.float32) for k in range(4)]
        self.jv = [rng.normal(size=(ROWS, B)).astype(np.float32) for _ in range(4)]


def steps_of_s(est, inp):
    """S, one callable per step: reset, predict, a host update with m = 1, a host update with m = 6 and a full R (the host staging
    grows from call to call), the fused step"""
    return [lambda: est.reset(*inp.x0),
            lambda: est.predict(inp.imu[0], inp.q4),
            lambda: est.update_indexed([3], inp.z1, inp.r1),
            lambda: est.update_indexed([3, 4, 5, 0, 1, 2], inp.z6, inp.r6),
            lambda: est.step_legodo(inp.imu[1], inp.lo[1], inp.mask[1], inp.q4)]


def new_estimator(n):
    import legs
    from pronto_amd import batch as pa
    est = pa.BatchEstimator(B, n_states=n)
    est.legodo_set_chain(*legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, legs.ATLAS_ROWS), None)
    return est


def joint_filter_msg(est, inp, mode, k, utime):
    """pb_joint_filter_init (which releases the filters' device state) and one message on device arrays"""
    import torch
    dev = torch.device("cuda:0")
    est.joint_filter_init(mode)
    out = torch.zeros((ROWS, B), dtype=torch.float32, device=dev)
    est.joint_filter(utime, torch.from_numpy(inp.jp[k]).to(dev), torch.from_numpy(inp.jv[k]).to(dev), None, out)
    return out


def init_families(est):
    """every handler family's init, twice: the second call finds its buffers allocated"""
    from pronto_amd import _lib
    for _ in range(2):
        est.legodo_init(0.3, 0.6, 5000, 5000)
        est.yawlock_init("yawbias_yaw" if est.n == 21 else "yaw", 1, True, 1.5, 0.5, 0.01, 1.0)
        est.yawlock_set_standing(np.ones(B, dtype=np.uint8))   # (per-filter arrays the context keeps)
        est.yawlock_set_gyro(np.zeros(B))
        est.score_init(10.0, 0.0)
        est.imu_notch_init(90.0, 1000.0)
        assert est._L.pb_ins_body_reset(est._h) == _lib.PB_OK


@pytest.fixture(scope="module", params=[15, 21])
def reference(request):
    """S alone on a fresh context: the checksum after each step; the joint filters' answer to messages 2, 3 as a fresh context's
    first two"""
    inp = Inputs(request.param)
    est = new_estimator(inp.n)
    sums = []
    for step in steps_of_s(est, inp):
        step()
        sums.append(est.state_checksum())
    first = joint_filter_msg(est, inp, "lowpass", 2, 7_000_000).cpu().numpy()
    import torch
    dev = torch.device("cuda:0")
    out = torch.zeros((ROWS, B), dtype=torch.float32, device=dev)
    est.joint_filter(7_001_000, torch.from_numpy(inp.jp[3]).to(dev), torch.from_numpy(inp.jv[3]).to(dev), None, out)
    second = out.cpu().numpy()
    est.close()
    assert len(set(sums)) == len(sums)   # every step of S moves the state
    return inp, sums, first, second


def test_remade_buffers_leave_the_state_and_each_other_alone(reference):
    import torch
    inp, want, jf_first, jf_second = reference
    est = new_estimator(inp.n)
    dev = torch.device("cuda:0")

    def between(k):
        if k == 0:
            est.history_reserve(3)
            joint_filter_msg(est, inp, "lowpass", 0, 5_000_000)
        elif k == 1:
            est.history_reserve(5)
            init_families(est)
            joint_filter_msg(est, inp, "kalman", 1, 6_000_000)
        elif k == 2:
            est.get_head()          # a host read-back: the staging area grows
            init_families(est)
        elif k == 3:
            est.history_reserve(0)
            got = joint_filter_msg(est, inp, "lowpass", 2, 7_000_000).cpu().numpy()
            assert np.array_equal(got, jf_first)    # released filter state does not linger
            out = torch.zeros((ROWS, B), dtype=torch.float32, device=dev)
            est.joint_filter(7_001_000, torch.from_numpy(inp.jp[3]).to(dev), torch.from_numpy(inp.jv[3]).to(dev), None, out)
            assert np.array_equal(out.cpu().numpy(), jf_second)

    for k, step in enumerate(steps_of_s(est, inp)):
        step()
        assert est.state_checksum() == want[k], "after step %d of S" % k
        between(k)
        assert est.state_checksum() == want[k], "after the calls behind step %d of S" % k
    est.close()


def test_life_cycles(reference):
    """ten contexts created, every family initialised, closed; the next context computes what the first one did"""
    inp, want, _, _ = reference
    for _ in range(10):
        est = new_estimator(inp.n)
        est.reset(*inp.x0)
        est.history_reserve(2)
        init_families(est)
        joint_filter_msg(est, inp, "lowpass", 0, 5_000_000)
        joint_filter_msg(est, inp, "kalman", 1, 6_000_000)
        est.get_head()
        est.close()
    est = new_estimator(inp.n)
    for k, step in enumerate(steps_of_s(est, inp)):
        step()
        assert est.state_checksum() == want[k], "after step %d of S" % k
    est.close()
