"""Rates of the yaw-lock step at 64k filters with per-filter device-resident joint states: the fused call
(pb_step_yawlock_joints, k_step_yawlock) on a correction message and on an idle one, against the composed pair of launches
(pb_yawlock_update_joints + pb_update_indexed_orient with the mask) in the same process -- the baseline: existing update
kernels.  15 and 21 states, mode yaw, correction_period 1 (every message corrects) and 333 (idle between corrections).
HIP events on the context's stream (torch's current stream), warm-up, >= 2 s timed per row, fused and composed alternated in
rounds so that the spread of the script is visible.  Writes profiles/yawlock_rate.txt (argv[1] = another path)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import legs  # noqa: E402
from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth import Workload  # noqa: E402

assert torch.cuda.is_available(), "yawlock_rate.py measures on the GPU; there is no CPU path"
dev = torch.device("cuda:0")
B = 65536
HBM_PEAK = 8.0e12   # bytes/s (spec)
ROUNDS, MIN_S = 3, 0.7   # rounds x 0.7 s >= 2 s timed per row
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "yawlock_rate.txt")


def timed(fn, min_s):
    """mean microseconds per call over at least min_s seconds, by events on the stream the context launches on"""
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    reps, total_ms, n = 200, 0.0, 0
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


chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, list(range(12)))
rng = np.random.default_rng(2)
jp = np.zeros((12, B))
for side, sgn in ((0, 1.0), (1, -1.0)):
    for j, c in enumerate((0.05 * sgn, 0.03 * sgn, -0.35, 0.7, -0.35, -0.03 * sgn)):
        jp[6 * side + j] = c + 0.02 * rng.normal(size=B)
d_jp = torch.from_numpy(jp.astype(np.float32)).to(dev)
lines = ["# scripts/yawlock_rate.py: B = %d filters, mode yaw, per-filter joint states [12][B] float32 on the device" % B,
         "# us per message: mean of %d rounds (min .. max); bytes per filter by the DESIGN.md 8d accounting" % ROUNDS]
for n in (15, 21):
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    state_bytes = (n + 5 + n * (n + 1) // 2) * 8
    yaw_state = (18 + 4) * 8
    inputs = 12 * 4
    small = 8 * 8   # head position + quaternion (+ bias z) read by the form
    for period in (1, 333):
        est = BatchEstimator(B, n_states=n)
        est.reset(vec, quat, P0)
        est.legodo_set_chain(*chain)
        est.yawlock_init("yaw", period, True, 1.5, 1.5, 0.05, 1.0)
        est.yawlock_set_standing(True)
        z = torch.zeros((2, B), dtype=torch.float64, device=dev)
        q = torch.zeros((4, B), dtype=torch.float64, device=dev)
        m = torch.zeros((2, B), dtype=torch.uint8, device=dev)
        ut = [0]

        def fused():
            ut[0] += 1000
            est.step_yawlock_joints(ut[0], d_jp, z_out=z, quat_out=q, mask_out=m)   # the handler keeps the block for replays

        def composed():
            ut[0] += 1000
            est.yawlock_update_joints(ut[0], d_jp, z_out=z, quat_out=q, mask_out=m)
            est.update_indexed([8], z[:1], [est_r], mask=m[0], quat_meas=q)

        est_r = np.radians(1.0) ** 2
        fused()   # the capture: from here on every tick is a correction
        res = {"fused": [], "composed": []}
        for _ in range(ROUNDS):
            res["fused"].append(timed(fused, MIN_S))
            res["composed"].append(timed(composed, MIN_S))
        # a correction message: one state round trip + inputs + yaw-lock state (read; the state words written back);
        # an idle message: inputs + yaw-lock state + the small read only
        corr_bytes = 2 * state_bytes + inputs + yaw_state + 4 * 8
        idle_bytes = inputs + small + yaw_state + 4 * 8
        frac_corr = 1.0 / period
        per_msg = frac_corr * corr_bytes + (1 - frac_corr) * idle_bytes
        for name in ("fused", "composed"):
            r = res[name]
            us = float(np.mean(r))
            lines.append("n=%d period=%d %s: %.2f us per message (%.2f .. %.2f); %.0f useful B per filter-message -> %.3f of the HBM roofline (%.1f TB/s peak)"
                         % (n, period, name, us, min(r), max(r), per_msg, per_msg * B / (us * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12))
        kind = "correction message" if period == 1 else "idle message (332 of 333; the correction's share included)"
        lines.append("n=%d period=%d: %s; correction = %d B per filter, idle = %d B per filter" % (n, period, kind, corr_bytes, idle_bytes))
        est.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
