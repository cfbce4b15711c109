"""The pair call (pb_step_legodo_joints: IMU step + leg odometry + update in one kernel) at 64k filters with the odometry's noises and
contact thresholds as scalars (k_step_leg / k_step_quad_leg) and as a per-filter block (pb_legodo_set_param_block: k_pair_legpar /
k_pair_quad_legpar), in the three measurement modes, for one robot's joint state (broadcast) and per-filter joint blocks.  The two
variants of a row alternate, ROUNDS times; every time and the minimum are printed.  Wall clock around back-to-back launches.

    python scripts/leg_par_rates.py [B] [scalars]      "scalars": the scalar rows only (A/B of two builds: PRONTO_BATCH_LIB)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import legs  # noqa: E402
from pronto_amd import _lib  # noqa: E402
from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth import Workload  # noqa: E402

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
SCALARS_ONLY = len(sys.argv) > 2 and sys.argv[2] == "scalars"
ROUNDS = 3


def timeit(fn, reps=400):
    for _ in range(100):  # (long enough for the clocks to settle, scripts/leg_rates.py)
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


chain = legs.chain_arrays(legs.ATLAS_LEFT, legs.ATLAS_RIGHT, list(range(12)))
gain = np.array([7000, 10000, 10000, 10000, 10000, 10000] * 2, dtype=np.float32)
msgs = legs.joint_gait(B, 8, seed=1, n_rows=12, rows=list(range(12)))
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
rng = np.random.default_rng(3)
blk = np.zeros((_lib.PB_LEGPAR_ROWS, B))
blk[_lib.PB_LEGPAR_R_VXYZ], blk[_lib.PB_LEGPAR_R_VXYZ_UNCERTAIN] = np.linspace(5, 12, B), np.linspace(20, 10, B)
blk[_lib.PB_LEGPAR_R_VANG], blk[_lib.PB_LEGPAR_R_VANG_UNCERTAIN], blk[_lib.PB_LEGPAR_R_XYZ] = 0.4, 0.9, 0.05
blk[_lib.PB_LEGPAR_SCHMITT_LOW], blk[_lib.PB_LEGPAR_SCHMITT_HIGH] = rng.uniform(300, 500, B), rng.uniform(520, 700, B)
blk[_lib.PB_LEGPAR_SCHMITT_LOW_DELAY], blk[_lib.PB_LEGPAR_SCHMITT_HIGH_DELAY] = rng.integers(3000, 9001, B), rng.integers(3000, 9001, B)
blk[_lib.PB_LEGPAR_TOTAL_FORCE], blk[_lib.PB_LEGPAR_STANDING_SCHMITT_LEVEL] = 900.0, 0.65
print("library:", _lib.LIB_PATH)
for n in (15, 21):
    w = Workload(B, n_states=n, dt_us=2000)
    est = BatchEstimator(B, n_states=n)
    est.reset(*w.initial_state())
    est.legodo_init(475.0, 525.0, 7000, 7000, True)
    est.legodo_set_chain(*chain, gain)
    q4 = w.process_noise()
    imu = up(w.imu_block(0))
    imu1 = np.ascontiguousarray(w.imu_block(0)[:, 0])
    jm = [(m[0], up(m[1]), up(m[2]), up(m[3])) for m in msgs]
    j1 = [(m[0],) + tuple(np.ascontiguousarray(a[:, 0]) for a in m[1:4]) for m in msgs]
    st = (n + 5 + n * (n + 1) // 2) * 8     # bytes of one filter's state, read and written once
    k = [0]

    def nxt(lst):
        k[0] += 1
        return lst[k[0] % len(lst)]

    for mode, name in ((0, "lin_rate"), (1, "lin_rot_rate"), (2, "pos_and_lin_rate")):
        est.legodo_set_measurement_mode(mode, 0.05, 0.4, 0.9)
        nrows = 4 + (2, 4, 3)[mode]         # block rows a filter loads: Schmitt rows + the mode's noises
        for kind, call, inputs in (("one robot (broadcast)", lambda: (lambda m: est.step_legodo_joints(imu1, q4, m[0], m[1], m[2], m[3], 5.0, 10.0))(nxt(j1)), 0),
                                   ("per-filter joint blocks", lambda: (lambda m: est.step_legodo_joints(imu, q4, m[0], m[1], m[2], m[3], 5.0, 10.0))(nxt(jm)), 56 + 104)):
            ts = {"scalars": [], "block": []}
            for _ in range(ROUNDS):
                for variant in (("scalars",) if SCALARS_ONLY else ("scalars", "block")):
                    if not SCALARS_ONLY:   # (a build from before the block has no such entry point)
                        est.legodo_set_param_block(blk if variant == "block" else None)
                    ts[variant].append(timeit(call) * 1e6)
            nb = 2 * st + 2 * 136 + inputs + (48 if mode == 2 else 0)
            line = "n=%d B=%d %-16s %-24s scalars %s min %6.1f us" % (n, B, name, kind, " ".join("%6.1f" % t for t in ts["scalars"]), min(ts["scalars"]))
            if not SCALARS_ONLY:
                line += " | block %s min %6.1f us | time x%.3f, bytes x%.3f (+%d B on %d)" % (
                    " ".join("%6.1f" % t for t in ts["block"]), min(ts["block"]), min(ts["block"]) / min(ts["scalars"]), (nb + 8 * nrows) / nb, 8 * nrows, nb)
            print(line, flush=True)
    est.close()
