#!/usr/bin/env python3
"""bench.py -- EKF predict+update steps/s on MI355X (BASELINE.json metric, configs[1] at N=1).

One step = one IMU predict (RBISIMUProcessStep) + one 3-DoF leg-odometry update (RBISIndexedMeasurement on
idx 3..5) for every filter of the batch = ONE kernel launch; the posterior is written back to HBM after every
step (T = 1 accounting).  Inputs (IMU + leg-odometry streams for warmup+steps) are resident
in HBM before the timed region.  N > 1: one process per GPU (torch.distributed / RCCL), the batch is split by
filter range with NO data-path collective; the only collective is the end-of-run summary all-reduce.  --scaling weak (default:
--batch-per-gpu filters on every GPU) or strong (--total-batch filters, default BASELINE config 4's 262 144, split over the
GPUs); the line's "scaling" and config.workload say which one ran.  `python bench.py --gpus N` starts its N ranks itself (child processes, the parent never
touches the GPU); under torch.distributed.run (WORLD_SIZE set) it is one of the ranks.

The timed region is exactly --steps launches (`timed_steps`), after --warmup untimed ones from the same initial state;
`value`, `ms_per_step` and the roofline figures are over those K launches (a longer window is a larger --steps).

A plain run does only what that line needs: set up, warm up, time the K steps, dump (--dump-outputs), print.  --full adds, at
N=1 and after the timed steps, what takes runs of its own: a second leg that times the same step on 1 M filters (state 1.17 GB,
nothing cache-resident) -> roofline.frac_cache_busting, the same 1 M filters in the library's blocked order ->
roofline.frac_cache_blocked (each leg repeats its 24 steps until it lasts >= --min-timed-ms, resp. half of it), and the CPU
baselines with the HIP path's parity on their sample -> cpu_baseline.  None of it changes the timed steps or the dumped outputs.

--dump-outputs DIR writes what the timed path left for its caller after the last timed step -- the head state of rank 0's
filters as getHeadState returns it -- as DIR/<name>.npy (float64); the inputs depend on the arguments only, so two builds
run with the same arguments can be compared output for output.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "EKF predict+update steps/sec (batched filters), 15-state, 1000 Hz IMU"
HBM_PEAK_GBPS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def bytes_per_step(n):
    """Algorithmic bytes per filter-step, T=1, symmetric-packed P (SURVEY.md 8d / BASELINE.md section 3)."""
    s_x = (n + 4) * 8
    s_p = n * (n + 1) // 2 * 8
    return 2 * (s_x + s_p + 8) + 56 + 48


def cpu_baseline(n, dt_us, target_s, est_cls):
    """Dense op-for-op oracle (kind "port") on this box's host cores, on a bounded sample of the same workload;
    the HIP path is run on the same sample to report the parity of what was just timed."""
    from oracle import po
    from pronto_amd.synth import Workload
    # a GPU box gives one GPU's job a 16-core CPU share whatever nproc says: more OpenMP threads only oversubscribe it
    threads = max(1, min(po.lib().po_max_threads(), int(os.environ.get("PRONTO_CPU_THREADS", "16"))))
    T = 100

    def run(Bs, nthreads=threads):
        w = Workload(Bs, n_states=n, dt_us=dt_us)
        vec, quat, P0 = w.initial_state()
        v21 = np.zeros((21, Bs)); v21[:n] = vec
        P21 = np.zeros((21, 21, Bs)); P21[:n, :n] = P0
        ob = po.OracleBatch(v21, quat, P21)
        imu, lo, mask = w.streams(0, T)
        sec = ob.run_legodo(imu, lo, mask, w.process_noise(), nthreads=nthreads)
        return sec, ob, (w, vec, quat, P0, imu, lo, mask)

    sec1, _, _ = run(256, nthreads=1)  # BASELINE.md section 4 "cpu-dense-1t"
    sec, _, _ = run(4 * threads)  # calibration
    rate = 4 * threads * T / max(sec, 1e-9)
    Bs = int(max(4 * threads, min(262144, rate * target_s / T)))
    Bs = (Bs + threads - 1) // threads * threads
    sec, ob, (w, vec, quat, P0, imu, lo, mask) = run(Bs)
    out = {"value": Bs * T / sec, "unit": "steps/s", "cores": threads, "kind": "port",
           "sample": "%d filters x %d steps of the same synthetic workload, dense 21-state oracle "
                     "(oracle/pronto_oracle.c, gcc -O2 -fopenmp), %.1f s" % (Bs, T, sec),
           "value_1thread": 256 * T / sec1}
    # parity of the HIP path on the very same sample
    import torch
    est = est_cls(Bs, n_states=n, device=torch.cuda.current_device())
    est.set_constants(*po.constants())
    est.reset(vec, quat, P0)
    dev = torch.device("cuda", torch.cuda.current_device())
    est.run_legodo(torch.from_numpy(imu).to(dev), torch.from_numpy(lo).to(dev), torch.from_numpy(mask).to(dev),
                   w.process_noise())
    gv, gq, gP, gll = est.get_head()
    est.close()

    def rel(a, b):
        return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))

    out["parity_max_rel_err"] = max(rel(gv, ob.vec[:n]), rel(gq, ob.quat), rel(gP, ob.cov[:n, :n]), rel(gll, ob.ll))
    try:
        out.update(cpu_structured(n, dt_us, threads, min(3.0, target_s)))
    except Exception as e:  # a reported extra, never a reason to lose the bench line
        out["structured_error"] = repr(e)
    return out


def cpu_structured(n, dt_us, threads, target_s):
    """SURVEY.md 8d asks for the structured CPU figure next to the dense one, so that the GPU/CPU ratio is not inflated
    by the reference's dense waste: the kernels' own per-filter arithmetic (block-sparse Ad, rank-3 downdate, packed P)
    compiled for the host by the TEST harness (tests/host_harness.cpp, g++ -O2), one filter range per host thread."""
    import ctypes as C
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    from pronto_amd.synth import Workload
    so = os.path.join(ROOT, "tests", "build", "libhost_harness.so")
    src = os.path.join(ROOT, "tests", "host_harness.cpp")
    hdr = os.path.join(ROOT, "pronto_amd", "csrc", "rbis_device.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
    hh = C.CDLL(so)
    from oracle import po
    g, tol = po.constants()
    T, Bt = 50, 512
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def prepare(t):
        w = Workload(Bt, b0=t * Bt, n_states=n, dt_us=dt_us)
        vec, quat, P0 = w.initial_state()
        nc = hh.hh_nc(n)
        st = np.zeros((nc, Bt))
        st[:n], st[n:n + 4] = vec, quat
        for i in range(n):
            for j in range(i + 1):
                st[n + 5 + hh.hh_pk(i, j)] = P0[i, j]
        imu, lo, mask = w.streams(0, T)
        return st, np.ascontiguousarray(imu), np.ascontiguousarray(lo), np.ascontiguousarray(mask), \
            np.ascontiguousarray(w.process_noise(), dtype=np.float64)

    def work(job, reps):
        st, imu, lo, mask, q4 = job
        for _ in range(reps):
            for k in range(T):
                hh.hh_step(C.c_int(n), dp(st), C.c_long(Bt), C.c_int(Bt), dp(imu[k]), dp(lo[k]),
                           mask[k].ctypes.data_as(C.POINTER(C.c_uint8)), dp(q4), C.c_double(g), C.c_double(tol), C.c_int(1))

    jobs = [prepare(t) for t in range(threads)]
    t0 = time.perf_counter(); work(jobs[0], 1); one = time.perf_counter() - t0
    reps = max(1, int(target_s / max(one, 1e-6)))
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda j: work(j, reps), jobs))
        sec = time.perf_counter() - t0
    return {"value_structured": threads * Bt * T * reps / sec, "value_structured_1thread": Bt * T / one,
            "structured_sample": "%d threads x %d filters x %d steps, the kernels' block-structured arithmetic compiled "
                                 "for the host (tests/host_harness.cpp), %.1f s" % (threads, Bt, T * reps, sec)}


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILD processes (one per GPU) and relay rank 0's
    JSON line.  This parent never touches the GPU (no torch import, no HIP call), children are fresh interpreters, nothing
    is re-exec'ed; a failing rank makes the whole run fail."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    # rank 0's stdout is drained on a thread; ALL children are polled, and the first one that fails takes the others down at
    # once (a rank that dies before the rendezvous would otherwise leave the rest in init_process_group until its timeout)
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    rcs = [None] * n
    deadline = time.time() + float(os.environ.get("PRONTO_BENCH_TIMEOUT_S", "1500"))
    while any(rc is None for rc in rcs):
        for r, p in enumerate(procs):
            if rcs[r] is None:
                rcs[r] = p.poll()
        failed = [r for r, rc in enumerate(rcs) if rc not in (None, 0)]
        if failed or time.time() > deadline:
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    p.terminate()
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    try:
                        rcs[r] = p.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        rcs[r] = -9
            break
        time.sleep(0.05)
    reader.join(timeout=5)
    sys.stdout.write(b"".join(c for c in chunks if c).decode())
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        raise SystemExit("bench.py: rank(s) failed: %s" % bad)


def cache_busting(BatchEstimator, dev, local_rank, n, d_imu, d_lo, d_mask, vec, quat, P0, q4, min_ms, blocked=False):
    """The same step on 1 M filters (state 1.17 GB >> the 256 MB Infinity Cache): the true-HBM figure next to the
    cache-resident 64k headline.  Inputs: the 64k workload's first blocks tiled 16x along the filter axis (a bandwidth
    measurement; parity is tested elsewhere), 24 distinct blocks cycled.
    blocked = False: step by step over the WHOLE batch (PRONTO_BATCH_BLOCKED=0) -- every launch streams 2.4 GB through DRAM: the
    DRAM-rate evidence.  blocked = True: the library's default order for such a state (pb_run_legodo: filter range outer, time
    inner, blocks that stay cache-resident) -- reported beside it, never as the headline."""
    import torch
    reps_f = (1 << 20) // d_imu.shape[2]
    if reps_f < 1 or (1 << 20) % d_imu.shape[2]:
        return None
    Bb, Tb = 1 << 20, min(24, d_imu.shape[0])
    prev = os.environ.get("PRONTO_BATCH_BLOCKED")
    if not blocked:
        os.environ["PRONTO_BATCH_BLOCKED"] = "0"
    try:
        est = BatchEstimator(Bb, n_states=n, device=local_rank)
    finally:
        if not blocked:
            if prev is None:
                os.environ.pop("PRONTO_BATCH_BLOCKED", None)
            else:
                os.environ["PRONTO_BATCH_BLOCKED"] = prev
    est.reset(torch.from_numpy(vec).to(dev).repeat(1, reps_f).contiguous(),
              torch.from_numpy(quat).to(dev).repeat(1, reps_f).contiguous(),
              torch.from_numpy(P0).to(dev).repeat(1, 1, reps_f).contiguous())
    imu = d_imu[:Tb].repeat(1, 1, reps_f).contiguous()
    lo = d_lo[:Tb].repeat(1, 1, reps_f).contiguous()
    mask = d_mask[:Tb].repeat(1, reps_f).contiguous()
    est.run_legodo(imu, lo, mask, q4)
    ms = est.run_legodo(imu, lo, mask, q4, timed=True)
    R = max(1, int(np.ceil(min_ms / max(ms, 1e-3))))
    tot = 0.0
    for _ in range(R):
        tot += est.run_legodo(imu, lo, mask, q4, timed=True)
    torch.cuda.synchronize()
    kern = est.hot_kernel()
    run_block = est.run_block()
    s = est.summary()
    est.close()
    del imu, lo, mask
    us = tot / (R * Tb) * 1e3
    bps = bytes_per_step(n)
    return {"batch": Bb, "kernel": kern, "order": ("blocks of %d filters, time inner" % run_block) if run_block else "step by step over the whole batch",
            "step_avg_us": us, "kernel_avg_us": us, "launches_timed": R * Tb,
            "algorithmic_bytes_per_launch": bps * Bb, "achieved": bps * Bb / (us * 1e-6) / 1e9,
            "frac": bps * Bb / (us * 1e-6) / 1e9 / HBM_PEAK_GBPS, "value": Bb / (us * 1e-6), "nonfinite": float(s[3])}


DUMP_BYTES = 60_000_000   # --dump-outputs budget (<= 64 MB in all, .npy headers included)
DUMP_SEED = 20251015     # the fixed filter sample of a batch whose head state does not fit the budget


def dump_outputs(est, summary, out_dir):
    """The head state after the last timed step, as a caller of run_legodo receives it (get_head: vec [n,c], quat [4,c],
    cov [n,n,c], loglik [c]), for every filter if it fits DUMP_BYTES, else for a fixed seeded sample of filters
    (filter_index.npy says which, in increasing order); summary.npy is pb_summary over the whole batch."""
    B, n = est.B, est.n
    per_filter = (n + 4 + n * n + 1 + 1) * 8
    c = min(B, DUMP_BYTES // per_filter)
    idx = np.arange(B) if c == B else np.sort(np.random.default_rng(DUMP_SEED).choice(B, c, replace=False))
    vec, quat, cov, ll = np.empty((n, c)), np.empty((4, c)), np.empty((n, n, c)), np.empty(c)
    CH = 65536   # get_head in chunks: host memory stays bounded whatever the batch
    for f0 in range(0, B, CH):
        lo, hi = np.searchsorted(idx, [f0, min(B, f0 + CH)])
        if lo == hi:
            continue
        gv, gq, gP, gll = est.get_head(f0, min(CH, B - f0))
        sel = idx[lo:hi] - f0
        vec[:, lo:hi], quat[:, lo:hi], cov[:, :, lo:hi], ll[lo:hi] = gv[:, sel], gq[:, sel], gP[:, :, sel], gll[sel]
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"vec": vec, "quat": quat, "cov": cov, "loglik": ll, "filter_index": idx.astype(np.float64),
              "summary": np.asarray(summary, dtype=np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return {"dir": out_dir, "filters": int(c), "of": int(B), "files": sorted(k + ".npy" for k in arrays)}


def workload_name(n, Bper, total, world, scaling):
    """config.workload: BASELINE.json's own wording where the run IS one of its configs, a plain description otherwise."""
    k = lambda v: "%dk" % (v // 1024) if v % 1024 == 0 else str(v)
    what = "IMU predict + 3-DoF leg-odom update"
    if world == 1:
        if n == 15 and total == 65536:
            return "64k batched 15-state filters, %s, 1 MI355X" % what          # BASELINE.json configs[1]
        return "%s batched %d-state filters, %s, 1 MI355X" % (k(total), n, what)
    if scaling == "strong":
        tag = " (BASELINE.json configs[3])" if (n == 15 and total == 262144 and world == 8) else ""
        return "%s batched %d-state filters sharded %dxMI355X, %s per GPU, %s, strong scaling%s" % (k(total), n, world, k(Bper), what, tag)
    return "%s batched %d-state filters per GPU x %d MI355X = %s filters, %s, weak scaling (per-GPU batch fixed)" % (k(Bper), n, world, k(total), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-per-gpu", type=int, default=65536)
    ap.add_argument("--n-states", type=int, default=15, choices=[15, 21])
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="N > 1: weak = --batch-per-gpu filters on EVERY GPU (the default; the line says so); strong = --total-batch "
                         "filters split over the N GPUs -- with the default 262 144 that is BASELINE config 4 (32 768 per GPU at N = 8)")
    ap.add_argument("--total-batch", type=int, default=262144, help="--scaling strong: filters of the whole job")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs the headline does not need (N = 1): the 1 M-filter cache-busting and cache-blocked "
                         "legs and the CPU baselines with their parity check; a plain run only sets up, warms up, times --steps "
                         "and prints the line")
    ap.add_argument("--cpu-seconds", type=float, default=6.0,
                    help="--full: target wall time of the dense CPU baseline sample (the structured one adds <= 3 s: <= 10 s of CPU work in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-cache-busting", action="store_true", help="--full: skip the 1 M-filter legs (N=1 only)")
    ap.add_argument("--min-timed-ms", type=float, default=6000.0,
                    help="--full: the 1 M-filter legs repeat their steps until they last at least this long (6 s by default: an "
                         "external GPU-busy sampler with a 5 s period must see them); the headline leg times exactly --steps")
    ap.add_argument("--host-streams", action="store_true",
                    help="generate the input streams with the numpy generator on the host (pronto_amd/synth.py) instead of "
                         "on the device (pronto_amd/synth_device.py: the same counter-based samples)")
    ap.add_argument("--fused", type=int, default=0, metavar="T",
                    help="also time the time-fused replay kernel (T steps per launch, state resident in registers) and "
                         "report it under its own accounting in a 'fused' object; never the headline value")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write rank 0's head state (vec, quat, cov, loglik of every filter, or of a "
                         "fixed seeded sample if that exceeds 60 MB; filter_index; the batch summary) as DIR/<name>.npy, float64")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)

    import torch
    import torch.distributed as dist
    from pronto_amd.batch import BatchEstimator
    from pronto_amd.shard import allreduce_summary, shard_range
    from pronto_amd.synth import Workload

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # Rehearsals of the N > 1 code on a box with ONE GPU (or none):
    #   PRONTO_BENCH_FORCE_DIST=1  the RCCL path with a single rank;
    #   PRONTO_BENCH_REHEARSE=1    N ranks that all use GPU 0 and rendezvous over gloo (RCCL refuses two ranks on one
    #                              device): everything but the collective's transport is the real path;
    #   PRONTO_BENCH_REHEARSE=dry  no GPU at all: rendezvous + one all-reduce over gloo, rank 0 prints a stub line (the
    #                              CPU test of the self-spawn logic, tests/test_shard_dist.py).
    rehearse = os.environ.get("PRONTO_BENCH_REHEARSE", "")
    import datetime
    RDV_TIMEOUT = datetime.timedelta(seconds=float(os.environ.get("PRONTO_BENCH_RDV_TIMEOUT_S", "300")))
    if rehearse == "dry":
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=RDV_TIMEOUT)
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "rank_sum": float(t[0])}), flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no GPU visible; the HIP path has no CPU fallback")
    if rehearse == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or os.environ.get("PRONTO_BENCH_FORCE_DIST") == "1"
    cdev = torch.device("cpu") if rehearse == "1" else dev   # where collective payloads live
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if rehearse == "1":
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=RDV_TIMEOUT)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=RDV_TIMEOUT)

    n, K, W = args.n_states, args.steps, args.warmup
    if args.scaling == "strong":
        total = args.total_batch
        Bper = (total + world - 1) // world   # (shard_range hands the remainder to the first ranks)
    else:
        Bper = args.batch_per_gpu
        total = Bper * world
    b0, b1 = shard_range(total, rank, world)
    B = b1 - b0
    dt_us = 1000

    # ---- synthetic streams for this shard, resident in HBM before the timed region ----
    t_gen = time.perf_counter()
    w = Workload(B, b0=b0, n_states=n, dt_us=dt_us)
    vec, quat, P0 = w.initial_state()
    q4 = w.process_noise()
    T = W + K
    d_imu = torch.empty((T, 7, B), dtype=torch.float64, device=dev)
    d_lo = torch.empty((T, 6, B), dtype=torch.float64, device=dev)
    d_mask = torch.empty((T, B), dtype=torch.uint8, device=dev)
    CH = 16
    if args.host_streams:
        for s in range(0, T, CH):
            e = min(T, s + CH)
            imu, lo, mask = w.streams(s, e - s)
            d_imu[s:e].copy_(torch.from_numpy(imu))
            d_lo[s:e].copy_(torch.from_numpy(lo))
            d_mask[s:e].copy_(torch.from_numpy(mask))
    else:
        # the same counter-based samples made on this rank's GPU: N ranks on one host do not queue up behind numpy
        from pronto_amd.synth_device import DeviceWorkload
        dw = DeviceWorkload(B, b0=b0, n_states=n, dt_us=dt_us, device=dev)
        for s in range(0, T, CH):
            e = min(T, s + CH)
            d_imu[s:e], d_lo[s:e], d_mask[s:e] = dw.streams(s, e - s)
        del dw
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t_gen

    est = BatchEstimator(B, n_states=n, device=local_rank)
    est.reset(vec, quat, P0)
    est.sync()

    def barrier():
        if use_dist and rehearse == "1":
            dist.barrier()
        elif use_dist:
            dist.barrier(device_ids=[local_rank])

    # ---- warmup (untimed): W steps and one pass over the K timed input blocks (every launch the timed region makes, at
    # steady clocks), then a restart from x0 and the W steps again, so that the timed steps continue a plain W-step run ----
    if W:
        est.run_legodo(d_imu[:W], d_lo[:W], d_mask[:W], q4)
    if K:
        est.run_legodo(d_imu[W:], d_lo[W:], d_mask[W:], q4)
        est.reset(vec, quat, P0)
        if W:
            est.run_legodo(d_imu[:W], d_lo[:W], d_mask[:W], q4)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    # ---- timed: K steps = K launches of the hot kernel ----
    ev_ms = 0.0
    t0 = time.perf_counter()
    if K:
        ev_ms = est.run_legodo(d_imu[W:], d_lo[W:], d_mask[W:], q4, timed=True)
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    wall = torch.tensor([t1 - t0, ev_ms * 1e-3], dtype=torch.float64, device=cdev)
    # per-rank spread of the HIP-event time of the timed launches and of the stream generation: (max, -min) through one MAX
    spread = torch.tensor([ev_ms, -ev_ms, t_gen, -t_gen], dtype=torch.float64, device=cdev)
    if use_dist:
        dist.all_reduce(wall, op=dist.ReduceOp.MAX)
        dist.all_reduce(spread, op=dist.ReduceOp.MAX)
    wall_s, ev_s = float(wall[0]), float(wall[1])

    local_summary = est.summary()
    dumped = dump_outputs(est, local_summary, args.dump_outputs) if args.dump_outputs and rank == 0 else None
    summary = allreduce_summary(local_summary, dist if use_dist else None, cdev)

    fused = None
    if args.fused > 0:  # (15 and 21 states: the cooperative replay kernel)
        # secondary accounting: bytes_step(T) = 2*(S_x+S_P+8)/T + 56 + 48; the bound is fp64 VALU issue
        Tf = args.fused
        est.reset(vec, quat, P0)
        est.replay_legodo_fused(d_imu[:W], d_lo[:W], d_mask[:W], q4, Tf)
        torch.cuda.synchronize()
        fms = est.replay_legodo_fused(d_imu[W:], d_lo[W:], d_mask[W:], q4, Tf, timed=True)
        torch.cuda.synchronize()
        bst = 2 * ((n + 4) * 8 + n * (n + 1) // 2 * 8 + 8) / Tf + 56 + 48
        fused = {"steps_per_launch": Tf, "value_per_gpu": B * K / (fms * 1e-3), "unit": "steps/s",
                 "bytes_per_filter_step": bst, "achieved_GBps": bst * B * K / (fms * 1e-3) / 1e9,
                 "frac_of_hbm_roofline_under_this_accounting": bst * B * K / (fms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                 "note": "posterior written once per launch; not the plugin path, not the headline metric"}

    hot = est.hot_kernel()
    est.close()
    busting = busting_blocked = None
    if args.full and world == 1 and not args.no_cache_busting and Bper <= (1 << 19):
        try:
            busting = cache_busting(BatchEstimator, dev, local_rank, n, d_imu, d_lo, d_mask, vec, quat, P0, q4,
                                    args.min_timed_ms)
            busting_blocked = cache_busting(BatchEstimator, dev, local_rank, n, d_imu, d_lo, d_mask, vec, quat, P0, q4,
                                            args.min_timed_ms / 2, blocked=True)
        except Exception as e:  # a reported extra, never a reason to lose the bench line
            busting = busting or {"error": repr(e)}

    if rank == 0:
        bps = bytes_per_step(n)
        value = total * K / wall_s
        launch_s = ev_s / K                       # HIP events on the launch stream around the launches
        achieved = bps * B / launch_s / 1e9       # algorithmic bytes of ONE launch (this rank's shard) / its duration
        state_mb = (n + 5 + n * (n + 1) // 2) * 8 * B / 1e6
        out = {
            "metric": METRIC, "value": value, "unit": "steps/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": wall_s / K * 1e3, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "timed_steps": K, "timed_region_ms": wall_s * 1e3,
            "per_rank_ms": {"kernel_time_max": float(spread[0]), "kernel_time_min": -float(spread[1]),
                            "stream_generation_max": float(spread[2]) * 1e3, "stream_generation_min": -float(spread[3]) * 1e3,
                            "streams": "host numpy" if args.host_streams else "device (pronto_amd/synth_device.py)"},
            "config": {"workload": workload_name(n, Bper, total, world, args.scaling),
                       "batch_per_gpu": Bper, "total_batch": total, "n_states": n, "imu_dt_us": dt_us, "kernel": hot,
                       "launches_per_step": 1, "bytes_per_filter_step": bps, "parallelism": "filter-range split x%d" % world},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": None, "traffic_source": None,
                         "kernel_avg_us": launch_s * 1e6, "algorithmic_bytes_per_launch": bps * B,
                         "resident": ("infinity_cache: the %.0f MB state stays in the 256 MB memory-side cache between "
                                      "launches, so `frac` is NOT an HBM-DRAM rate; see frac_cache_busting (--full)" % state_mb)
                         if state_mb < 256 else "hbm"},
            "summary": {"sum_loglik": float(summary[0]), "checksum_abs": float(summary[1]),
                        "max_quat_norm_dev": float(summary[2]), "nonfinite": float(summary[3])},
        }
        if busting is not None:
            out["roofline"]["frac_cache_busting"] = busting.get("frac")
            out["roofline"]["cache_busting"] = busting
            if busting_blocked is not None:   # the same 1 M filters in the library's default launch order for such a state
                out["roofline"]["frac_cache_blocked"] = busting_blocked.get("frac")
                out["roofline"]["cache_blocked"] = busting_blocked
        tr = os.path.join(ROOT, "profiles", "traffic.json")  # HBM bytes per launch from a separate --pmc pass
        if os.path.exists(tr):
            try:
                rec = json.load(open(tr))
                key = "%s@%d" % (hot, B)
                if key in rec:
                    out["roofline"]["traffic"] = rec[key]["hbm_bytes_per_launch"]
                    out["roofline"]["traffic_source"] = (
                        "NOT measured in this run: profiles/traffic.json, round %s, separate rocprofv3 --pmc FETCH_SIZE / "
                        "WRITE_SIZE passes of this command (scripts/profile.sh), counter scales from profiles/%s_pmc.json"
                        % (rec[key].get("source"), rec[key].get("source")))
            except Exception:
                pass
        if fused is not None:
            out["fused"] = fused
        if dumped is not None:
            out["dumped_outputs"] = dumped
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(n, dt_us, args.cpu_seconds, BatchEstimator)
        print(json.dumps(out), flush=True)
    if use_dist:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
