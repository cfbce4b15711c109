"""Rates of pb_update_indexed_wide (k_update_wide) at 64k filters: 15 and 21 states, m = 7, 8, 9 rows, a full per-filter R and one
broadcast diagonal, with 0 %, 2 % and 100 % of the filters masked in -- and, in the SAME run, the six-row free-form list
[0, 4, 8, 12, n-5, n-1] through pb_update_indexed (k_update_coop_rt<6> / k_update_quad_rt<6>; profiles/r05_others.txt recorded 31.9 / 48.1 us),
the yardstick: no time is fixed in advance, a wide row is read against that row scaled by algorithmic bytes.
Device-resident inputs, HIP events on the stream the context launches on, warm-up, three rounds per row with the rows alternating inside a
round.  Algorithmic bytes per updated filter: two state images + 8 (m + m^2) or 8 m bytes of measurement + the mask byte.
Writes profiles/update_wide.txt (argv[1] = another path)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth import Workload  # noqa: E402

assert torch.cuda.is_available(), "update_wide_rate.py measures on the GPU; there is no CPU path"
dev = torch.device("cuda:0")
B = 65536
ROUNDS, MIN_S = 3, 0.15
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "update_wide.txt")


def timed(fn, min_s):
    """mean microseconds per call over at least min_s seconds, by events on the stream the context launches on"""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    reps, total_ms, n = 100, 0.0, 0
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


def full_r(m, rng):
    """[m*m, B] column-major: a diagonal of 0.05 ... 0.2 with small symmetric off-diagonals"""
    R = np.zeros((m, m, B))
    R[np.arange(m), np.arange(m)] = rng.uniform(0.05, 0.2, size=(m, B))
    for i in range(m):
        for j in range(i):
            R[i, j] = R[j, i] = 0.01 * rng.uniform(-1, 1, size=B)
    return np.ascontiguousarray(np.swapaxes(R, 0, 1).reshape(m * m, B))


rng = np.random.default_rng(4)
lines = ["# scripts/update_wide_rate.py: B = %d filters, device-resident inputs; us per call: mean of %d rounds (min .. max)" % (B, ROUNDS),
         "# bytes = algorithmic bytes per UPDATED filter (two state images + measurement + mask byte); us/B(six) = time per algorithmic byte",
         "# relative to the six-row row of the same state size and run (rows with 100 % of the filters masked in)"]
for n in (15, 21):
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    state_bytes = (n + 5 + n * (n + 1) // 2) * 8
    rows = []          # (label, callable, bytes per updated filter, fraction masked in)
    six = [0, 4, 8, 12, n - 5, n - 1]
    z6 = torch.from_numpy(np.ascontiguousarray(vec[six])).to(dev)
    R6 = torch.from_numpy(full_r(6, rng)).to(dev)
    rows.append(("m=6 %s full R, pb_update_indexed" % six, lambda z6=z6, R6=R6: est.update_indexed(six, z6, R6), 2 * state_bytes + 8 * 42, 1.0))
    masks = {}
    for frac in (0.0, 0.02, 1.0):
        mk = np.zeros(B, np.uint8)
        mk[rng.permutation(B)[: int(round(frac * B))]] = 1
        masks[frac] = torch.from_numpy(mk).to(dev)
    for m in (7, 8, 9):
        idx = list(range(3, 3 + m))
        z = torch.from_numpy(np.ascontiguousarray(vec[idx])).to(dev)
        Rf = torch.from_numpy(full_r(m, rng)).to(dev)
        Rb = [0.1] * m
        for rname, R, rbytes in (("full R", Rf, 8 * (m + m * m)), ("broadcast diagonal", Rb, 8 * m)):
            for frac in (0.0, 0.02, 1.0):
                rows.append(("m=%d %s, %3.0f %% masked in" % (m, rname, 100 * frac),
                             lambda idx=idx, z=z, R=R, mk=masks[frac]: est.update_indexed_wide(idx, z, R, mask=mk), 2 * state_bytes + rbytes + 1, frac))
    res = [[] for _ in rows]
    for _ in range(ROUNDS):
        for k, (_, fn, _, _) in enumerate(rows):
            res[k].append(timed(fn, MIN_S))
    six_us_per_byte = float(np.mean(res[0])) / rows[0][2]
    for (label, _, nbytes, frac), r in zip(rows, res):
        us = float(np.mean(r))
        rel = "" if frac < 1.0 else "; us/B(six) = %.2f" % (us / nbytes / six_us_per_byte)
        lines.append("n=%d %s: %.2f us (%.2f .. %.2f); %d bytes%s" % (n, label, us, min(r), max(r), nbytes, rel))
    est.close()
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
