"""pb_smooth_step_masked: pb_smooth_step for the filters with step[b] = 1, slot_out <- slot_next for step[b] = 0 (no INS update at k+1:
the smoothed posterior at k is the one at k+1), bit for bit -- against pb_smooth_step on the same slots and against slot_next.  The
posteriors are those of a forward pass that keeps every update's (smoother_ref.py's style); step = NULL is pb_smooth_step exactly.
Under the default smoother kernels and under PRONTO_SMOOTH_KERNEL=lane, each in a fresh process (the switch is read once)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def check(n, B, dt=1e-3):
    import torch
    from pronto_amd.batch import BatchEstimator
    from smoother_ref import start_of
    from pronto_amd.synth import Workload
    w = Workload(B, n_states=n)
    vec, quat, P0, q4 = start_of(w)
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    est.history_reserve(8)
    for k in range(2):   # slots 2k: the INS update's posterior, 2k + 1: the filtered posterior of step k
        est.predict(w.imu_block(k), q4)
        est.state_save(2 * k)
        lo, mask = w.legodo_block(k)
        est.update_indexed([3, 4, 5], np.ascontiguousarray(lo[0:3]), np.ascontiguousarray(lo[3:6]), mask=mask)
        est.state_save(2 * k + 1)
    PRED, NEXT, CUR = 2, 3, 1
    est.smooth_step(PRED, NEXT, CUR, 4, dt)
    est.sync()
    ref, nxt = est.get_slot(4), est.get_slot(NEXT)
    rng = np.random.default_rng(n * B)
    step = (rng.random(B) < 0.6).astype(np.uint8)
    step[0] = 0
    sel = step != 0
    d_step = torch.from_numpy(step).to("cuda:0")
    torch.cuda.synchronize()
    for out, mask in ((5, step), (6, d_step), (7, None)):
        est.smooth_step_masked(PRED, NEXT, CUR, out, dt, mask)
        est.sync()
        got = est.get_slot(out)
        for g, r, x in zip(got, ref, nxt):
            want = r if mask is None else np.where(sel, r, x)
            assert g.tobytes() == want.tobytes(), (out, n, B)
    # in place (slot_out = slot_cur), as the shim's pass may run it: a copy of slot_cur in slot 5 becomes the result
    est.state_restore(CUR)
    est.state_save(5)
    est.smooth_step_masked(PRED, NEXT, 5, 5, dt, step)
    est.sync()
    for g, r, x in zip(est.get_slot(5), ref, nxt):
        assert g.tobytes() == np.where(sel, r, x).tobytes(), ("in place", n, B)
    est.close()
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["default", "lane"])
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("B", [1, 100, 4096])
def test_masked_smoother_step_is_select_after_the_step(n, B, kernel):
    env = dict(os.environ)
    env.pop("PRONTO_SMOOTH_KERNEL", None)
    env.pop("PRONTO_SMOOTH_PIVOT", None)
    if kernel == "lane":
        env["PRONTO_SMOOTH_KERNEL"] = "lane"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(B)], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    check(int(sys.argv[1]), int(sys.argv[2]))
    print("PASS")
