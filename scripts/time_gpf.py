"""Times of the GPF measurement's kernels (pb_gpf_*, pronto_amd/csrc/rbis_gpf_kernels.hpp) and of the whole gpf_update chain:
4 096 and 65 536 filters of 15 states, K = 256 samples, the substates pos_chi {6..11} and all_states {3..11}, the built-in grid
likelihood with 180 broadcast points.  HIP events on the stream the context launches on, warm-up, three rounds per row.  Beside every
time: the bytes the kernel must move (inputs read once, outputs written once) and that rate as a fraction of the copy rate
pb_calib_copy reports in the same run.  Not part of the test suite or of bench.py.  Writes profiles/gpf.txt (argv[1] = another path)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth import Workload  # noqa: E402

assert torch.cuda.is_available(), "time_gpf.py measures on the GPU; there is no CPU path"
K, N_POINTS, ROUNDS, MIN_S = 256, 180, 3, 0.1
LISTS = (("pos_chi", [6, 7, 8, 9, 10, 11]), ("all_states", [3, 4, 5, 6, 7, 8, 9, 10, 11]))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gpf.txt")


def timed(fn, min_s):
    """mean microseconds per call over at least min_s seconds"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, total_ms, n = 10, 0.0, 0
    while total_ms < min_s * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        n += reps
    return total_ms * 1e3 / n


rng = np.random.default_rng(3)
lines = ["# scripts/time_gpf.py: 15 states, K = %d samples, %d broadcast points; us per call: mean of %d rounds (min .. max)" % (K, N_POINTS, ROUNDS),
         "# bytes = what the kernel must move (inputs once, outputs once); copy = that rate / the rate of pb_calib_copy in this run",
         "# the 4 096-filter fractions are NOT fractions of an HBM rate: at that size the state (4.6 MB) and the blocks stay in the caches, for pb_calib_copy too"]
for B in (4096, 65536):
    w = Workload(B, n_states=15)
    vec, quat, P0 = w.initial_state()
    est = BatchEstimator(B, n_states=15)
    est.reset(vec, quat, P0)
    state_bytes = (15 + 5 + 120) * 8
    copy_rate = 10 * 2 * state_bytes * B / (est.calib_copy(10) * 1e-3)      # bytes per second
    lines.append("B=%d pb_calib_copy: %.0f GB/s" % (B, copy_rate / 1e9))
    values = rng.uniform(-3.0, 0.5, size=(40, 200, 200))
    est.gpf_grid_set([-50.0, -50.0, -2.0], 0.5, values, -12.0, 4.0)
    pts = np.ascontiguousarray(rng.uniform(-20.0, 20.0, size=(N_POINTS, 3)) * np.array([1.0, 1.0, 0.1])).ravel()
    for name, idx in LISTS:
        m = len(idx)
        xi = est.gpf_normals(1, 0, K * m).view(K, m, B)
        delta, pose = est.gpf_sample(idx, xi)
        ll = est.gpf_grid_loglik(pose, pts)
        prior = 8 * (m * (m + 1) // 2 + m + 10)
        rows = [("k_gpf_normals [%d][B]" % (K * m), lambda m=m: est.gpf_normals(1, 0, K * m), 8 * K * m),
                ("k_gpf_sample<15,%d>" % m, lambda idx=idx, xi=xi: est.gpf_sample(idx, xi), 8 * K * (2 * m + 7) + prior),
                ("k_gpf_grid_loglik", lambda pose=pose: est.gpf_grid_loglik(pose, pts), 8 * K * 8),
                ("k_gpf_fit<15,%d>" % m, lambda idx=idx, delta=delta, ll=ll: est.gpf_measurement(idx, delta, ll), 8 * K * (m + 2) + prior + 8 * (m + m * m) + 4),
                ("gpf_update chain (normals, sample, grid likelihood, fit, update_indexed_wide)",
                 lambda idx=idx: est.gpf_update(idx, K, lambda p: est.gpf_grid_loglik(p, pts), 1), None)]
        res = [[] for _ in rows]
        for _ in range(ROUNDS):
            for k, (_, fn, _) in enumerate(rows):
                res[k].append(timed(fn, MIN_S))
        for (label, _, nbytes), r in zip(rows, res):
            us = float(np.mean(r))
            tail = "" if nbytes is None else "; %d bytes per filter, %.1f %% of copy" % (nbytes, 100.0 * nbytes * B / (us * 1e-6) / copy_rate)
            lines.append("B=%d %s %s: %.1f us (%.1f .. %.1f)%s" % (B, name, label, us, min(r), max(r), tail))
    est.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
