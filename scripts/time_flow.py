"""Times of the optical-flow sigma-point update (pb_update_optical_flow, pronto_amd/csrc/rbis_flow_kernels.hpp): 65 536 filters of 15
and of 21 states, device inputs, HIP events on the stream the context launches on, warm-up, three alternating rounds.  In the same
run: the six-row pb_update_indexed of profiles/update_wide.txt as the yardstick, pb_calib_copy's rate, and the only way to run this
update without the kernel: get_head, the update on the host, set_head (RBISHostUpdate's path).  The host update is timed as the numpy
witness of tests/flow_ref.py on 32 filters and scaled to the batch -- a compiled host loop would be faster; the two copies are timed
on the whole batch.  Not part of the test suite or of bench.py.  Writes profiles/optical_flow.txt (argv[1] = another path)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import flow_ref as fr  # noqa: E402
from pronto_amd.batch import BatchEstimator  # noqa: E402

assert torch.cuda.is_available(), "time_flow.py measures on the GPU; there is no CPU path"
B, ROUNDS, MIN_S, N_HOST = 65536, 3, 0.1, 32
SIX = [9, 10, 11, 3, 4, 5]
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "optical_flow.txt")


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


lines = ["# scripts/time_flow.py: %d filters, device inputs; us per call: mean of %d alternating rounds (min .. max)" % (B, ROUNDS),
         "# bytes = the state read once and written once; copy = that rate / the rate of pb_calib_copy in this run"]
for n in (15, 21):
    h = fr.heads(n)                                          # the tests' 130 heads (dense positive definite P, heights 0.6 ... 5 m), repeated
    reps = (B + fr.B_GPU - 1) // fr.B_GPU
    vec, quat, P0 = (np.ascontiguousarray(np.tile(h[k], (1,) * (h[k].ndim - 1) + (reps,))[..., :B]) for k in ("vec", "quat", "P"))
    est = BatchEstimator(B, n_states=n)
    est.flow_set_camera(*fr.camera())
    est.reset(vec, quat, P0)
    state_bytes = (n + 5 + n * (n + 1) // 2) * 8
    copy_rate = 10 * 2 * state_bytes * B / (est.calib_copy(10) * 1e-3)      # bytes per second
    lines.append("n=%d pb_calib_copy: %.0f GB/s" % (n, copy_rate / 1e9))
    dev = torch.device("cuda:0")
    flow = torch.from_numpy(np.tile(np.array([0.1, -0.2, 0.05, -0.4, 1.02, 0.97, 1.05])[:, None], (1, B))).to(dev)
    # (a wide R: thousands of repeated updates leave P where it is, so no filter drops out at a pivot while the clock runs)
    R4 = torch.full((4, B), 1e4, dtype=torch.float64, device=dev)
    z6, R6 = torch.from_numpy(np.ascontiguousarray(vec[SIX])).to(dev), torch.full((6, B), 1e4, dtype=torch.float64, device=dev)
    rows = [("pb_update_optical_flow (k_update_flow<%d>)" % n, lambda: est.update_optical_flow(flow, R4)),
            ("pb_update_optical_flow with zhat_out and status_out", lambda: est.update_optical_flow(flow, R4, want_zhat=True, want_status=True)),
            ("pb_update_indexed, six rows %s" % SIX, lambda: est.update_indexed(SIX, z6, R6))]
    res = [[] for _ in rows]
    for _ in range(ROUNDS):
        for k, (_, fn) in enumerate(rows):
            res[k].append(timed(fn, MIN_S))
    for (label, _), r in zip(rows, res):
        us = float(np.mean(r))
        lines.append("n=%d %s: %.1f us (%.1f .. %.1f); %d bytes per filter, %.1f %% of copy"
                     % (n, label, us, min(r), max(r), 2 * state_bytes, 100.0 * 2 * state_bytes * B / (us * 1e-6) / copy_rate))
    _, status = est.update_optical_flow(flow, R4, want_status=True)
    applied = int((status == 0).sum())
    lines.append("n=%d filters applied after the timed runs: %d of %d" % (n, applied, B))
    assert applied == B, "the timed runs did not time the update"
    # the host path: both copies on the whole batch, the update on N_HOST filters
    t = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        v, q, P, ll = est.get_head()
        t1 = time.perf_counter()
        part = dict(vec=np.ascontiguousarray(v[:, :N_HOST]), quat=np.ascontiguousarray(q[:, :N_HOST]), P=np.ascontiguousarray(P[:, :, :N_HOST]),
                    flow=flow[:, :N_HOST].cpu().numpy())
        fr.witness_update(part, np.full((4, N_HOST), 1e4), fr.camera(), fr.weights())
        t2 = time.perf_counter()
        vc, qc, Pc, llc = (np.ascontiguousarray(a, dtype=np.float64) for a in (v, q, P, ll))
        assert est._L.pb_set_head(est._h, vc.ctypes.data, qc.ctypes.data, Pc.ctypes.data, llc.ctypes.data, 0) == 0
        est.sync()
        t3 = time.perf_counter()
        t.append((t1 - t0, (t2 - t1) * B / N_HOST, t3 - t2))
    g, u, s = (float(np.mean([x[k] for x in t])) for k in range(3))
    lines.append("n=%d host path: get_head %.1f ms + numpy witness %.0f s (%.1f ms per filter on %d filters, scaled) + set_head %.1f ms"
                 % (n, g * 1e3, u, u / B * 1e3, N_HOST, s * 1e3))
    est.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
