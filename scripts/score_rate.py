"""Cost of one ground-truth message at 64k filters: the device scorer (pb_score_ground_truth, k_score_gt) against what a caller
needed without it -- pb_sync + pb_get_head of every filter's vector and quaternion to the host (the arithmetic of
drift_per_distance.py in a host loop would come on top).  15 and 21 states, in one process.

The scorer rows are PER-CALL times, back to back: HIP events on the context's stream (torch's current stream) around 200 calls of
the Python binding at a time, after a warm-up, three rounds of 0.7 s per row alternated with the download so that the spread of
the script is visible.  At 5-9 us a call this can be the rate at which the host enqueues as much as the kernel's duration, and the
23 MB of score state stay in the memory-side cache between calls: it is what one more message costs a running replay, not a kernel
time and not a bandwidth figure (no rocprofv3 kernel trace of it has been taken).  Rows:
  closing / broadcast   every message closes a window (time threshold 0): the whole score state moves; truth = 7 kernel arguments
  closing / device      the same with a per-filter [7][B] truth block in HBM
  idle / broadcast      no message closes a window (threshold 1e9 s): anchor position and time are read, only PB_SCORE_ABS rows move
The download is timed by the host clock around pb_sync + pb_get_head (it ends in a synchronise): it is a PCIe copy and a
synchronisation, not a kernel.  Writes profiles/score_rate.txt (argv[1] = another path)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pronto_amd import _lib  # noqa: E402
from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth import Workload  # noqa: E402

assert torch.cuda.is_available(), "score_rate.py measures on the GPU; there is no CPU path"
dev = torch.device("cuda:0")
B = 65536
ROUNDS, MIN_S = 3, 0.7
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_rate.txt")


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


def wall(fn, min_s):
    """mean microseconds per call by the host clock; fn ends in a synchronise"""
    for _ in range(5):
        fn()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < min_s:
        fn()
        n += 1
    return (time.perf_counter() - t0) * 1e6 / n


lines = ["# python scripts/score_rate.py: B = %d filters; one ground-truth message" % B,
         "# us per message: mean of %d rounds (min .. max).  scorer rows: per-call time, back to back, score state cache-warm (HIP events around 200 calls); download row: host clock" % ROUNDS,
         "# around pb_sync + pb_get_head(vec, quat -> host), which ends in a synchronise"]
rng = np.random.default_rng(4)
truth = np.concatenate([rng.uniform(-5, 5, (3, B)), np.tile(np.array([[1.0], [0], [0], [0]]), (1, B))])
d_truth = torch.from_numpy(np.ascontiguousarray(truth)).to(dev)
one = np.ascontiguousarray(truth[:, 0])
for n in (15, 21):
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    hv, hq = np.empty((n, B)), np.empty((4, B))
    ut = [0]

    def score(pose):
        def fn():
            ut[0] += 1000
            est.score_ground_truth(ut[0], pose, absolute=True)
        return fn

    def download():
        est.sync()
        rc = est._L.pb_get_head(est._h, 0, B, C.c_void_p(hv.ctypes.data), C.c_void_p(hq.ctypes.data), None, None, _lib.PB_HOST)
        assert rc == 0

    rows = [("scorer, closing / broadcast", 0.0, one), ("scorer, closing / device", 0.0, d_truth), ("scorer, idle / broadcast", 1e9, one)]
    res = {name: [] for name, _, _ in rows}
    res["download"] = []
    for _ in range(ROUNDS):
        for name, thr, pose in rows:
            est.score_init(thr, 0.0)
            res[name].append(timed(score(pose), MIN_S))
        res["download"].append(wall(download, MIN_S))
    # bytes per filter of a closing message with both flags: the estimate (7 doubles); the anchors and their time read and written
    # back (2 x 15 words); 11 sums / maxima and 3 counts read and written; the newest window's 10 fields and its time written
    closing = (7 + 2 * 15 + 2 * (11 + 3) + 11) * 8
    for name, _, pose in rows:
        r = res[name]
        lines.append("n=%d %s: %.2f us per message (%.2f .. %.2f)" % (n, name, float(np.mean(r)), min(r), max(r)))
    r = res["download"]
    lines.append("n=%d download, pb_sync + pb_get_head(vec, quat) to the host: %.2f us per message (%.2f .. %.2f); %d B per filter over PCIe"
                 % (n, float(np.mean(r)), min(r), max(r), (n + 4) * 8))
    lines.append("n=%d: a closing message moves %d B per filter of score state, anchors and estimate (+ 56 B of truth from a device block)" % (n, closing))
    est.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
