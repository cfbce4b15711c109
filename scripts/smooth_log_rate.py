"""Whole-log RTS smoothing with bounded memory (pb_smooth_log: checkpoint and recompute): device time per smoothed filter-step,
forward pass + recompute + smoother steps, and the slots it took against the 2 T a posterior per update would need.  With
SMOOTH_LOG_FUSED=1 every case is timed a second time on pb_smooth_log_fused (one fused launch per step) in the same run.
  python scripts/smooth_log_rate.py            env: SMOOTH_LOG_CASES="n,B,T,K;..."  SMOOTH_LOG_FUSED=0|1
  python scripts/smooth_log_rate.py --corrected
--corrected: pb_smooth_log_corrected on the BASELINE correction schedules -- 15 states: config 3, a VO position_orient correction on
every 32nd tick; 21 states: config 5, a scan-match position_yaw correction on every 25th -- with fused = 0 and fused = 1, next to
pb_smooth_log_fused on the same streams without ticks and the headline step (pb_run_legodo) in the same run.  Every figure is repeated
until at least SMOOTH_LOG_MIN_S (default 2) seconds of device time are on the clock, at least three times: median [min .. max]. """
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pronto_amd.batch import BatchEstimator  # noqa: E402
from pronto_amd.synth_device import DeviceWorkload  # noqa: E402



def corrected_cases(cases):
    import torch
    from pronto_amd import _lib
    min_ms = 1e3 * float(os.environ.get("SMOOTH_LOG_MIN_S", "2"))

    def figure(name, T, call):
        call()   # warm-up
        ms = [call()]
        while len(ms) < 3 or sum(ms) < min_ms:
            ms.append(call())
        us = np.array(ms) * 1e3 / T
        print("  %-34s %8.2f us per step of the batch  [%.2f .. %.2f], %d repeats of %.0f ms" % (name, np.median(us), us.min(), us.max(), len(ms), np.median(ms)),
              flush=True)

    for case in cases.split(";"):
        n, B, T, K = (int(v) for v in case.split(","))
        every, kind, label = (32, _lib.PB_CORR_POS_ORIENT, "config 3: position_orient") if n == 15 else (25, _lib.PB_CORR_POS_YAW, "config 5: position_yaw")
        dw = DeviceWorkload(B, n_states=n, device="cuda:0")
        vec, quat, P0 = dw.host.initial_state()
        q4 = dw.host.process_noise()
        imu, lo, mask = dw.streams(0, T)
        steps = [k for k in range(T) if k % every == every - 1]
        m = 6 if kind == _lib.PB_CORR_POS_ORIENT else 4
        z2 = torch.zeros((len(steps), m, B), dtype=torch.float64, device="cuda:0")   # (entries at chi indices are ignored)
        qm2 = torch.empty((len(steps), 4, B), dtype=torch.float64, device="cuda:0")
        for t, k in enumerate(steps):
            z, qm, Rd = dw.host.vo_block(k) if kind == _lib.PB_CORR_POS_ORIENT else dw.host.scanmatch_block(k)
            z2[t, :3] = torch.from_numpy(z)
            qm2[t] = torch.from_numpy(np.ascontiguousarray(qm))
        R2 = [float(Rd[i, 0]) for i in range(m)]
        est = BatchEstimator(B, n_states=n)
        est.reset(vec, quat, P0)
        est.history_reserve(est.smooth_log_slots(T, K))
        print("n=%d, %s on every %dth of %d steps (%d ticks) x %d filters, stride %d" % (n, label, every, T, len(steps), B, K), flush=True)

        def fresh(call):
            def run():
                est.reset(vec, quat, P0)
                return call()
            return run
        figure("pb_run_legodo (headline step)", T, fresh(lambda: est.run_legodo(imu, lo, mask, q4, timed=True)))
        figure("pb_smooth_log_fused, no ticks", T, fresh(lambda: est.smooth_log(imu, lo, mask, q4, 1e-3, K, timed=True, fused=True)))
        if hasattr(est._L, "pb_smooth_log_corrected"):   # (an older build named by PRONTO_BATCH_LIB: the two figures above only)
            for fused in (0, 1):
                figure("pb_smooth_log_corrected fused=%d" % fused, T,
                       fresh(lambda: est.smooth_log_corrected(imu, lo, mask, q4, 1e-3, K, kind, steps, z2, R2, qm2, fused=fused, timed=True)))
        s = est.summary()
        print("  nonfinite %d" % int(s[3]), flush=True)
        est.close()
        del imu, lo, mask, z2, qm2


if "--corrected" in sys.argv[1:]:
    corrected_cases(os.environ.get("SMOOTH_LOG_CASES", "15,65536,1000,22;21,65536,1000,22"))
    sys.exit(0)

cases = os.environ.get("SMOOTH_LOG_CASES", "15,4096,10000,64;21,4096,10000,64;15,65536,1000,22;21,65536,1000,22")
for case in cases.split(";"):
    n, B, T, K = (int(v) for v in case.split(","))
    dw = DeviceWorkload(B, n_states=n, device="cuda:0")
    vec, quat, P0 = dw.host.initial_state()
    q4 = dw.host.process_noise()
    imu, lo, mask = dw.streams(0, T)
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    need = est.smooth_log_slots(T, K)
    est.history_reserve(need)
    for fused in ((False, True) if os.environ.get("SMOOTH_LOG_FUSED", "0") == "1" else (False,)):
        est.reset(vec, quat, P0)
        est.smooth_log(imu[:2 * K], lo[:2 * K], mask[:2 * K], q4, 1e-3, K, fused=fused)   # warm-up
        est.reset(vec, quat, P0)
        ms = est.smooth_log(imu, lo, mask, q4, 1e-3, K, timed=True, fused=fused)
        per_slot = (n + 5 + n * (n + 1) // 2) * 8 * B / 1e6
        s = est.summary()
        print("%s n=%d: %d steps x %d filters, stride %d: %d slots (%.1f GB; a posterior per update: %d slots, %.0f GB): %.1f ms = %.2f us per "
              "smoothed step of the batch = %.4f us per smoothed filter-step; nonfinite %d"
              % ("pb_smooth_log_fused" if fused else "pb_smooth_log", n, T, B, K, need, need * per_slot / 1e3, 2 * T, 2 * T * per_slot / 1e3, ms,
                 ms * 1e3 / T, ms * 1e3 / (T * B), int(s[3])), flush=True)
    est.close()
    del imu, lo, mask
