"""EKFSmoothBackwardsPass through the C++ shim with state_estimator.fuse_ins_legodo = true (tests/cpp/test_smooth_fused.cpp): the
INS half of a fused pair has no checkpoint, and the pass re-applies the pair with a predicted slot (pb_set_pred_slot).  Every smoothed
step against the oracle; sparse checkpoints against a checkpoint per update, bit for bit.  Runs on the MI355X."""
import subprocess

import pytest

from test_cpp_shim import build_exe


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("every", [1, 3, 7])
def test_smooth_backwards_pass_with_fused_pairs_on_gpu(oracle, n, every):
    exe = build_exe(oracle, "test_smooth_fused")
    r = subprocess.run([exe, str(n), str(every)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 21])
def test_smooth_backwards_pass_with_leg_pair_kernel_on_gpu(oracle, n):
    """Joint states through LegOdoHandler::processMessage(joint_state_t*): with fusion the odometry runs inside the pair kernel
    (leg_kernel_pairs > 0); the pass re-applies those pairs from their kept measurement blocks.  The smoothed posteriors must agree
    with the same run with fusion off to 1e-9."""
    exe = build_exe(oracle, "test_smooth_fused")
    r = subprocess.run([exe, str(n), "1", "joints"], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
