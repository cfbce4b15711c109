"""Thin Python binding of the C ABI (include/pronto_batch.h) -- test/bench plumbing, not the product.

`BatchEstimator` mirrors the reference's estimator entry points for B filters at once
(state-estimator/src/mav_state_est/mav_state_est.hpp:20-22: addUpdate / getHeadState /
getMeasurementsLogLikelihood) by forwarding to pb_* one-to-one.  Arrays may be numpy (host, staged over
PCIe) or torch CUDA tensors (HBM-resident, read in place).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PB_DEVICE, PB_HOST, PB_HOST_BROADCAST, PB_R_DIAG, PB_R_DIAG_BROADCAST, PB_R_FULL


class PbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pronto_batch error %d: %s" % (code, msg))
        self.code = code


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a, dtype=np.float64, shape=None):
    """(pointer, mem) of a numpy array or a torch tensor; None -> (NULL, None).  The C ABI takes no lengths (it reads
    rows x batch elements), so a mis-shaped array would be an out-of-bounds read: `shape` is checked here."""
    if a is None:
        return None, None
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected an array of shape %s, got %s" % (tuple(shape), tuple(a.shape)))
    if _is_torch(a):
        import torch
        want = {np.float64: torch.float64, np.uint8: torch.uint8, np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        if a.dtype != want or not a.is_contiguous():
            raise TypeError("expected a contiguous %s tensor" % want)
        return C.c_void_p(a.data_ptr()), (PB_DEVICE if a.is_cuda else PB_HOST)
    if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("expected a C-contiguous numpy array of %s" % np.dtype(dtype))
    return C.c_void_p(a.ctypes.data), PB_HOST


def _ptr_block(a, rows=None, B=None, dtype=np.float64):
    """Like _ptr for a [rows, B] data block; a 1-D numpy array of `rows` values means ONE message for every filter of the
    batch (PB_HOST_BROADCAST: expanded on the device, nothing of batch size crosses PCIe)."""
    if isinstance(a, np.ndarray) and a.ndim == 1:
        p, _ = _ptr(a, dtype, shape=None if rows is None else (rows,))
        return p, PB_HOST_BROADCAST
    return _ptr(a, dtype, shape=None if rows is None else (rows, B))


def _same_mem(*mems):
    ms = {m for m in mems if m is not None}
    if len(ms) != 1:
        raise ValueError("all buffers of one call must live in the same memory space")
    return ms.pop()


class BatchEstimator:
    def __init__(self, batch, n_states=15, device=0, n_snapshots=1):
        self._L = _lib.load()
        h = C.c_void_p()
        rc = self._L.pb_create(C.byref(h), n_states, batch, device, n_snapshots)
        if rc:
            raise PbError(rc, (self._L.pb_last_error(None) or b"").decode())
        self._h = h
        self._pinned = []
        self.B, self.n, self.device = batch, n_states, device
        # Launch on torch's current stream of that device (usually the null stream): device tensors handed to this
        # object are produced by torch kernels/copies on that stream, so stream order makes them visible.
        try:
            import torch
            if torch.cuda.is_available():
                self.set_stream(torch.cuda.current_stream(device).cuda_stream)
        except ImportError:
            pass

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self._L.pb_host_free(self._h, p)
            self._pinned = []
            self._L.pb_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            raise PbError(rc, (self._L.pb_last_error(self._h) or b"").decode())

    # --- plumbing ---
    def set_stream(self, stream_ptr):
        """hipStream_t handle, taken literally (0 = the null stream = torch's default stream)."""
        self._chk(self._L.pb_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_own_stream(self):
        self._chk(self._L.pb_use_own_stream(self._h))

    def set_constants(self, g, chi_tol):
        self._chk(self._L.pb_set_constants(self._h, g, chi_tol))

    def sync(self):
        self._chk(self._L.pb_sync(self._h))

    def hot_kernel(self):
        return self._L.pb_hot_kernel(self._h).decode()

    def run_block(self):
        """filters per block of run_legodo's cache-blocked order (0: the whole batch per launch)"""
        return self._L.pb_run_block(self._h)

    # --- posterior checkpoints, RTS smoother ---
    def history_reserve(self, n_slots):
        self._chk(self._L.pb_history_reserve(self._h, n_slots))

    def pinned_empty(self, shape, dtype=np.float64):
        """A numpy array in page-locked host memory (pb_host_alloc): PB_HOST blocks copied from it move at link rate.
        Freed when the estimator is closed."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self._L.pb_host_alloc(self._h, nbytes, C.byref(p)))
        self._pinned.append(p)
        buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def set_output_slot(self, slot):
        """The next update writes its posterior straight into checkpoint `slot` (which becomes the head): a checkpoint
        per update without a copy.  -1 cancels."""
        self._chk(self._L.pb_set_output_slot(self._h, int(slot)))

    def set_pred_slot(self, slot):
        """The next step_legodo / step_legodo_split -- or step_legodo_correct with an output slot pending as well -- also writes its INS
        posterior (the prediction, before the leg-odometry update) into checkpoint `slot`.  One-shot: that call consumes it whatever
        its outcome.  -1 cancels."""
        self._chk(self._L.pb_set_pred_slot(self._h, int(slot)))

    def state_save(self, slot):
        self._chk(self._L.pb_state_save(self._h, slot))

    def state_restore(self, slot):
        self._chk(self._L.pb_state_restore(self._h, slot))

    def smooth_step(self, slot_next_pred, slot_next, slot_cur, slot_out, dt):
        self._chk(self._L.pb_smooth_step(self._h, slot_next_pred, slot_next, slot_cur, slot_out, dt))

    def smooth_step_masked(self, slot_next_pred, slot_next, slot_cur, slot_out, dt, step=None):
        """pb_smooth_step for the filters with step[b] = 1; slot_out <- slot_next for step[b] = 0.  step: [B] uint8 (numpy or a
        device tensor) or None (= every filter)."""
        p, m = _ptr(step, np.uint8, shape=(self.B,))
        self._chk(self._L.pb_smooth_step_masked(self._h, slot_next_pred, slot_next, slot_cur, slot_out, dt, p, PB_HOST if m is None else m))

    def slot_select(self, dst, src, mask, when=1):
        """dst <- src for the filters whose mask entry equals `when` (0 / 1); dst / src: checkpoint slots or _lib.PB_SLOT_HEAD."""
        p, m = _ptr(mask, np.uint8, shape=(self.B,))
        self._chk(self._L.pb_slot_select(self._h, int(dst), int(src), p, int(when), PB_HOST if m is None else m))

    def smooth_log_slots(self, n_steps, stride):
        return self._L.pb_smooth_log_slots(n_steps, stride)

    def smooth_log(self, imu_stream, lo_stream, mask_stream, q4, dt, stride, first_slot=0, sink=None, timed=False, fused=False):
        """Whole-log RTS smoothing with bounded memory (checkpoint and recompute): sink(step, slot) is called newest step first; read the
        slot with get_slot before returning from the sink.  Returns device ms if timed.  fused: pb_smooth_log_fused (one fused launch
        per step, as step_legodo) instead of pb_smooth_log (the process step and the update as two launches)."""
        T = imu_stream.shape[0]
        pi, m1 = _ptr(imu_stream, shape=(T, 7, self.B))
        pl, m2 = _ptr(lo_stream, shape=(T, 6, self.B))
        pm, m3 = _ptr(mask_stream, np.uint8, shape=(T, self.B))
        if _same_mem(m1, m2, m3) != PB_DEVICE:
            raise ValueError("smooth_log needs device-resident streams")
        q = (C.c_double * 4)(*q4)
        ms = C.c_float(0)
        SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)
        cb = SINK((lambda user, step, slot: sink(step, slot))) if sink is not None else None
        fn = self._L.pb_smooth_log_fused if fused else self._L.pb_smooth_log
        self._chk(fn(self._h, T, stride, pi, pl, pm, q, dt, first_slot, C.cast(cb, C.c_void_p) if cb else None, None,
                     C.byref(ms) if timed else None))
        return ms.value if timed else None

    def smooth_log_fused(self, imu_stream, lo_stream, mask_stream, q4, dt, stride, first_slot=0, sink=None, timed=False):
        """smooth_log on pb_smooth_log_fused: every forward and recompute step is ONE fused launch (step_legodo's semantics)."""
        return self.smooth_log(imu_stream, lo_stream, mask_stream, q4, dt, stride, first_slot, sink, timed, fused=True)

    def smooth_log_corrected(self, imu_stream, lo_stream, mask_stream, q4, dt, stride, corr_kind, corr_steps, z2, R2, quat_meas2, mask2=None,
                             fused=True, first_slot=0, sink=None, timed=False):
        """smooth_log / smooth_log_fused for a log with corrections behind some of its pairs (pb_smooth_log_corrected): corr_kind as
        step_legodo_correct (m = 6 / 4), corr_steps the strictly increasing steps that carry one, z2 [n_ticks, m, B], quat_meas2
        [n_ticks, 4, B], mask2 [n_ticks, B] or None (device tensors), R2 a device tensor [n_ticks, m, B] or a length-m list (one
        diagonal for every tick and filter).  corr_steps = None or empty: no correction stream at all."""
        T = imu_stream.shape[0]
        pi, m1 = _ptr(imu_stream, shape=(T, 7, self.B))
        pl, m2 = _ptr(lo_stream, shape=(T, 6, self.B))
        pm, m3 = _ptr(mask_stream, np.uint8, shape=(T, self.B))
        if _same_mem(m1, m2, m3) != PB_DEVICE:
            raise ValueError("smooth_log_corrected needs device-resident streams")
        cs, keep = None, []
        if corr_steps is not None:
            steps = np.ascontiguousarray(corr_steps, dtype=np.int32).reshape(-1)
            nt = steps.shape[0]
            m = {_lib.PB_CORR_POS_ORIENT: 6, _lib.PB_CORR_POS_YAW: 4}.get(corr_kind)   # (None: an unknown kind is the library's to refuse)
            cs = _lib.CorrStream(kind=int(corr_kind), n_ticks=nt, step=steps.ctypes.data)
            keep.append(steps)
            mems = []
            if nt > 0:
                pz, mz = _ptr(z2, shape=m and (nt, m, self.B))
                pq, mq = _ptr(quat_meas2, shape=(nt, 4, self.B))
                pk, mk = _ptr(mask2, np.uint8, shape=(nt, self.B))
                mems = [mz, mq, mk]
                if _is_torch(R2):
                    pr, mr = _ptr(R2, shape=m and (nt, m, self.B))
                    mems.append(mr)
                    cs.r_kind2 = _lib.PB_R_DIAG
                else:
                    rb = np.ascontiguousarray(R2, dtype=np.float64)
                    if m and rb.shape != (m,):
                        raise ValueError("R2: a device tensor [n_ticks, m, B] or m values")
                    keep.append(rb)
                    pr = C.c_void_p(rb.ctypes.data)
                    cs.r_kind2 = _lib.PB_R_DIAG_BROADCAST
                if any(x is not None and x != PB_DEVICE for x in mems):
                    raise ValueError("smooth_log_corrected needs device-resident correction blocks")
                cs.z2, cs.R2, cs.quat_meas2, cs.mask2 = pz, pr, pq, pk
        q = (C.c_double * 4)(*q4)
        ms = C.c_float(0)
        SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)
        cb = SINK((lambda user, step, slot: sink(step, slot))) if sink is not None else None
        self._chk(self._L.pb_smooth_log_corrected(self._h, T, stride, pi, pl, pm, q, dt, first_slot, C.byref(cs) if cs is not None else None,
                                                  1 if fused else 0, C.cast(cb, C.c_void_p) if cb else None, None,
                                                  C.byref(ms) if timed else None))
        return ms.value if timed else None

    def get_slot(self, slot, first=0, count=None, want_cov=True):
        """get_head for a posterior that lives in a checkpoint slot."""
        count = self.B - first if count is None else count
        n = self.n
        vec = np.empty((n, count))
        quat = np.empty((4, count))
        ll = np.empty(count)
        cov = np.empty((n, n, count)) if want_cov else None
        self._chk(self._L.pb_get_slot(self._h, slot, first, count, C.c_void_p(vec.ctypes.data), C.c_void_p(quat.ctypes.data),
                                      C.c_void_p(cov.ctypes.data) if want_cov else None, C.c_void_p(ll.ctypes.data), PB_HOST))
        if want_cov:
            cov = np.swapaxes(cov, 0, 1)
        return vec, quat, cov, ll

    # --- noise identification ---
    def set_process_noise_block(self, q_block):
        """q_block: torch CUDA tensor [4,B] (kept alive by the caller) or None."""
        if q_block is None:
            self._chk(self._L.pb_set_process_noise_block(self._h, None))
            return
        p, m = _ptr(q_block, shape=(4, self.B))
        if m != PB_DEVICE:
            raise ValueError("the process-noise block must be device memory")
        self._chk(self._L.pb_set_process_noise_block(self._h, p))

    def window_nll(self, idx, truth_vec, truth_quat, want_err=False):
        """(logdet, maha, nll) [3,B] (+ error vector [n,B]) of head (-) truth over the active indices.  Truth arrays in numpy: numpy
        results (PB_HOST); torch CUDA tensors: the results are CUDA tensors written by the kernel in place (PB_DEVICE, stream-ordered on
        the context's stream -- sync() before reading them on another)."""
        m = len(idx)
        ia = (C.c_int * m)(*[int(i) for i in idx])
        pv, m1 = _ptr(truth_vec, shape=(self.n, self.B))
        pq, m2 = _ptr(truth_quat, shape=(4, self.B))
        mem = _same_mem(m1, m2)
        if mem == PB_DEVICE:
            import torch
            out = torch.empty((3, self.B), dtype=torch.float64, device=truth_vec.device)
            err = torch.empty((self.n, self.B), dtype=torch.float64, device=truth_vec.device) if want_err else None
        else:
            out = np.empty((3, self.B))
            err = np.empty((self.n, self.B)) if want_err else None
        po, _ = _ptr(out)
        pe, _ = _ptr(err)
        self._chk(self._L.pb_window_nll(self._h, m, ia, pv, pq, po, pe, mem))
        return (out, err) if want_err else out

    # --- leg kinematic odometry ---
    def legodo_init(self, schmitt_low, schmitt_high, low_delay_us, high_delay_us, filter_contact_events=True):
        self._chk(self._L.pb_legodo_init(self._h, schmitt_low, schmitt_high, int(low_delay_us), int(high_delay_us),
                                         int(bool(filter_contact_events))))
        self._leg_mode = 0

    def legodo_update(self, utime, feet, forces, r_vxyz, r_vxyz_uncertain, delta_out=None, status_out=None, lo_out=None,
                      mask_out=None, zero_delta=False, after_predict=None):
        """leg_estimate::updateOdometry for every filter.  feet [14,B] (or [14] broadcast), forces [2,B] (or [2]);
        outputs are torch CUDA tensors: delta [7,B], status [B] (float64), lo block [6,B] + mask [B] (uint8).
        after_predict = an IMU block ([7,B] or [7]): the odometry is slaved to the orientation the filter WILL have after
        predict(that block), which is then run fused with the measurement produced here (step_legodo)."""
        pf, m1 = _ptr_block(feet, 14, self.B)
        pz, m2 = _ptr_block(forces, 2, self.B)
        outs = []
        for a, dt, shp in ((delta_out, np.float64, (7, self.B)), (status_out, np.float64, (self.B,)),
                           (lo_out, np.float64, self._leg_shapes()[0]), (mask_out, np.uint8, self._leg_shapes()[1])):
            p, m = _ptr(a, dt, shape=shp)
            if a is not None and m != PB_DEVICE:
                raise ValueError("legodo_update outputs must be device tensors")
            outs.append(p)
        if after_predict is not None:
            pi, mi = _ptr_block(after_predict, 7, self.B)
            self._chk(self._L.pb_legodo_update_after_predict(self._h, pi, mi, int(utime), pf, pz, _same_mem(m1, m2),
                                                             int(bool(zero_delta)), r_vxyz, r_vxyz_uncertain, *outs))
            return
        self._chk(self._L.pb_legodo_update(self._h, int(utime), pf, pz, _same_mem(m1, m2), int(bool(zero_delta)), r_vxyz,
                                           r_vxyz_uncertain, *outs))

    def legodo_set_contact_mode(self, standing=False, total_force=0.0, standing_schmitt_level=0.0, use_controller_input=False):
        self._chk(self._L.pb_legodo_set_contact_mode(self._h, int(bool(standing)), total_force, standing_schmitt_level,
                                                     int(bool(use_controller_input))))

    def legodo_set_zero_initial_velocity(self, ticks):
        self._chk(self._L.pb_legodo_set_zero_initial_velocity(self._h, int(ticks)))

    def legodo_set_control_contacts(self, n_contacts):
        """[2] int32 (every filter) or [2,B] int32 (numpy or torch CUDA)."""
        p, m = _ptr_block(n_contacts, 2, self.B, dtype=np.int32)
        self._chk(self._L.pb_legodo_set_control_contacts(self._h, p, m))

    def legodo_set_message_times(self, utimes=None, valid=None):
        """Per-filter message times [B] int64 and / or validity [B] uint8 of the NEXT odometry or pair call (pb_legodo_set_message_times):
        numpy arrays (copied) or device tensors (read in place by that call: keep them alive until it has run)."""
        pu, m1 = _ptr(utimes, np.int64, shape=(self.B,))
        pv, m2 = _ptr(valid, np.uint8, shape=(self.B,))
        self._chk(self._L.pb_legodo_set_message_times(self._h, pu, pv, PB_HOST if utimes is None and valid is None else _same_mem(m1, m2)))

    def legodo_set_chain(self, n_left, n_right, joint_type, joint_row, origin_xyz_rpy, axis, adjustment_gain=None):
        n = n_left + n_right
        ty = (C.c_int * n)(*[int(v) for v in joint_type])
        rw = (C.c_int * n)(*[int(v) for v in joint_row])
        org = np.ascontiguousarray(origin_xyz_rpy, dtype=np.float64).reshape(n, 6)
        ax = np.ascontiguousarray(axis, dtype=np.float64).reshape(n, 3)
        gain = None if adjustment_gain is None else np.ascontiguousarray(adjustment_gain, dtype=np.float32).reshape(n)
        dp = C.POINTER(C.c_double)
        self._chk(self._L.pb_legodo_set_chain(self._h, n_left, n_right, ty, rw, org.ctypes.data_as(dp), ax.ctypes.data_as(dp),
                                              None if gain is None else gain.ctypes.data_as(C.POINTER(C.c_float))))

    def legodo_set_measurement_mode(self, mode, r_xyz=0.0, r_vang=0.0, r_vang_uncertain=0.0):
        """LegOdoCommon's mode for the odometry and pair calls: 0 lin_rate (lo [6,B], mask [B]), 1 lin_rot_rate (lo [12,B], mask [B]),
        2 pos_and_lin_rate (lo [12,B], masks [2,B])."""
        self._chk(self._L.pb_legodo_set_measurement_mode(self._h, int(mode), float(r_xyz), float(r_vang), float(r_vang_uncertain)))
        self._leg_mode = int(mode)

    def legodo_set_param_block(self, block):
        """The odometry's noises and contact thresholds PER FILTER (pb_legodo_set_param_block): block [PB_LEGPAR_ROWS, B] float64 in
        the .cfg's units, rows _lib.PB_LEGPAR_* -- a numpy array (checked per filter by the library) or a device tensor (copied
        unchecked); None switches back to the scalars.  The block is copied: the caller's array is free on return."""
        if block is None:
            self._chk(self._L.pb_legodo_set_param_block(self._h, None, PB_HOST))
            return
        shape = tuple(getattr(block, "shape", ()))
        if shape != (_lib.PB_LEGPAR_ROWS, self.B):   # (before any call into the library: it takes no lengths)
            raise ValueError("expected a parameter block of shape %s, got %s" % ((_lib.PB_LEGPAR_ROWS, self.B), shape))
        p, m = _ptr(block, shape=shape)
        self._chk(self._L.pb_legodo_set_param_block(self._h, p, m))

    def _leg_shapes(self):
        mode = getattr(self, "_leg_mode", 0)
        return ((6, self.B), (self.B,)) if mode == 0 else ((12, self.B), (self.B,) if mode == 1 else (2, self.B))

    def legodo_update_joints(self, utime, joint_position, joint_effort, forces, r_vxyz, r_vxyz_uncertain, delta_out=None,
                             status_out=None, lo_out=None, mask_out=None, zero_delta=False, after_predict=None, position_out=None,
                             position_status_out=None):
        """leg_estimate::updateOdometry from a joint state: joint_position [rows,B] float32 (or [rows] broadcast),
        joint_effort the same or None, forces [2,B] float32 (or [2]).  Outputs as legodo_update."""
        rows = joint_position.shape[0]
        pj, m1 = _ptr_block(joint_position, rows, self.B, dtype=np.float32)
        pe, m2 = (None, None) if joint_effort is None else _ptr_block(joint_effort, rows, self.B, dtype=np.float32)
        pz, m3 = _ptr_block(forces, 2, self.B, dtype=np.float32)
        outs = []
        for a, dt, shp in ((delta_out, np.float64, (7, self.B)), (status_out, np.float64, (self.B,)),
                           (lo_out, np.float64, self._leg_shapes()[0]), (mask_out, np.uint8, self._leg_shapes()[1]),
                           (position_out, np.float64, (3, self.B)), (position_status_out, np.uint8, (self.B,))):
            p, m = _ptr(a, dt, shape=shp)
            if a is not None and m != PB_DEVICE:
                raise ValueError("legodo_update_joints outputs must be device tensors")
            outs.append(p)
        pi, mi = (None, PB_DEVICE) if after_predict is None else _ptr_block(after_predict, 7, self.B)
        self._chk(self._L.pb_legodo_update_joints(self._h, pi, mi, int(utime), rows, pj, pe, pz, _same_mem(m1, m2, m3),
                                                  int(bool(zero_delta)), r_vxyz, r_vxyz_uncertain, *outs))

    def step_legodo_joints(self, imu_block, q4, utime, joint_position, joint_effort, forces, r_vxyz, r_vxyz_uncertain, lo_out=None,
                           mask_out=None):
        """One call (one kernel where the context has it) per IMU + joint-state pair: pb_step_legodo_joints."""
        pi, mi = _ptr_block(imu_block, 7, self.B)
        rows = joint_position.shape[0]
        pj, m1 = _ptr_block(joint_position, rows, self.B, dtype=np.float32)
        pe, m2 = (None, None) if joint_effort is None else _ptr_block(joint_effort, rows, self.B, dtype=np.float32)
        pz, m3 = _ptr_block(forces, 2, self.B, dtype=np.float32)
        pl, _ = _ptr(lo_out, shape=self._leg_shapes()[0])
        pm, _ = _ptr(mask_out, np.uint8, shape=self._leg_shapes()[1])
        q = (C.c_double * 4)(*q4)
        self._chk(self._L.pb_step_legodo_joints(self._h, pi, mi, q, int(utime), rows, pj, pe, pz, _same_mem(m1, m2, m3), r_vxyz,
                                                r_vxyz_uncertain, pl, pm))

    def step_legodo_feet(self, imu_block, q4, utime, feet, forces, r_vxyz, r_vxyz_uncertain, lo_out=None, mask_out=None):
        pi, mi = _ptr_block(imu_block, 7, self.B)
        pf, m1 = _ptr_block(feet, 14, self.B)
        pz, m2 = _ptr_block(forces, 2, self.B)
        pl, _ = _ptr(lo_out, shape=self._leg_shapes()[0])
        pm, _ = _ptr(mask_out, np.uint8, shape=self._leg_shapes()[1])
        q = (C.c_double * 4)(*q4)
        self._chk(self._L.pb_step_legodo_feet(self._h, pi, mi, q, int(utime), pf, pz, _same_mem(m1, m2), r_vxyz, r_vxyz_uncertain, pl, pm))

    def calib_copy_checksum(self, reps=1):
        out = (C.c_uint64 * 2)()
        self._chk(self._L.pb_calib_copy_checksum(self._h, int(reps), out))
        return int(out[0]), int(out[1])

    def legodo_fk(self, joint_position, joint_effort, feet_out):
        rows = joint_position.shape[0]
        pj, m1 = _ptr_block(joint_position, rows, self.B, dtype=np.float32)
        pe, m2 = (None, None) if joint_effort is None else _ptr_block(joint_effort, rows, self.B, dtype=np.float32)
        po, mo = _ptr(feet_out, shape=(14, self.B))
        if mo != PB_DEVICE:
            raise ValueError("legodo_fk output must be a device tensor")
        self._chk(self._L.pb_legodo_fk(self._h, rows, pj, pe, _same_mem(m1, m2), po))

    def joint_filter_init(self, mode, process_noise_pos=0.01, process_noise_vel=0.01, observation_noise=5e-4):
        """mode: "lowpass" | "kalman" (state_estimator.legodo.filter_joint_positions, leg_estimate.cpp:43-61); the noise
        defaults are SimpleKalmanFilter's constructor defaults."""
        self._chk(self._L.pb_joint_filter_init(self._h, {"lowpass": 1, "kalman": 2}[mode], process_noise_pos, process_noise_vel,
                                               observation_noise))

    def joint_filter(self, utime, joint_position, joint_velocity, joint_effort, joint_position_out):
        """One joint-state message through the joint filters.  Per-robot [rows, B] blocks (numpy or device tensors) ->
        joint_position_out must be a device tensor [rows, B]; one robot's 1-D [rows] numpy arrays -> a 1-D numpy output."""
        rows = joint_position.shape[0]
        pj, m1 = _ptr_block(joint_position, rows, self.B, dtype=np.float32)
        pv, m2 = (None, None) if joint_velocity is None else _ptr_block(joint_velocity, rows, self.B, dtype=np.float32)
        pe, m3 = (None, None) if joint_effort is None else _ptr_block(joint_effort, rows, self.B, dtype=np.float32)
        mem = _same_mem(m1, m2, m3)
        if mem == PB_HOST_BROADCAST:
            po, mo = _ptr(joint_position_out, np.float32, shape=(rows,))
            if mo != PB_HOST:
                raise ValueError("one robot's message: the output is a numpy array [rows]")
        else:
            po, mo = _ptr(joint_position_out, np.float32, shape=(rows, self.B))
            if mo != PB_DEVICE:
                raise ValueError("per-robot blocks: the output must be a device tensor [rows, B]")
        self._chk(self._L.pb_joint_filter(self._h, int(utime), rows, pj, pv, pe, mem, po))

    def legodo_get(self, b):
        pose = (C.c_double * 7)()
        info = (C.c_int64 * 4)()
        self._chk(self._L.pb_legodo_get(self._h, b, pose, info))
        return np.array(pose), [int(v) for v in info]

    # --- yaw lock (YawLockHandler) ---
    YAWLOCK_MODES = {"yawbias": 0, "yaw": 1, "yawbias_yaw": 2}

    def yawlock_init(self, mode, correction_period, yaw_slip_detect, yaw_slip_threshold_degrees, yaw_slip_disable_period_s, r_yaw_bias_deg=0.0,
                     r_yaw_deg=0.0):
        """mode: "yawbias" | "yaw" | "yawbias_yaw" (or 0 / 1 / 2); resets every filter's yaw-lock state."""
        self._chk(self._L.pb_yawlock_init(self._h, int(self.YAWLOCK_MODES.get(mode, mode)), int(correction_period), int(bool(yaw_slip_detect)),
                                          float(yaw_slip_threshold_degrees), float(yaw_slip_disable_period_s), float(r_yaw_bias_deg),
                                          float(r_yaw_deg)))

    def yawlock_set_standing(self, standing):
        """one bool for every filter, or a [B] uint8 array / tensor"""
        if np.isscalar(standing) or isinstance(standing, bool):
            v = (C.c_uint8 * 1)(1 if standing else 0)
            self._chk(self._L.pb_yawlock_set_standing(self._h, v, PB_HOST_BROADCAST))
        else:
            p, m = _ptr(standing, np.uint8, shape=(self.B,))
            self._chk(self._L.pb_yawlock_set_standing(self._h, p, m))

    def yawlock_set_gyro(self, body_gyro_z):
        """the body-frame gyro z YawLockHandler::insHandler keeps: one value for every filter, or [B]"""
        if np.isscalar(body_gyro_z):
            v = (C.c_double * 1)(float(body_gyro_z))
            self._chk(self._L.pb_yawlock_set_gyro(self._h, v, PB_HOST_BROADCAST))
        else:
            p, m = _ptr(body_gyro_z, shape=(self.B,))
            self._chk(self._L.pb_yawlock_set_gyro(self._h, p, m))

    def _yawlock_call(self, fn, utime, joint_position, utimes, valid, z_out, quat_out, mask_out):
        rows = joint_position.shape[0]
        pj, mj = _ptr_block(joint_position, rows, self.B, dtype=np.float32)
        pu = None if utimes is None else C.c_void_p(utimes.data_ptr())
        pv = None if valid is None else C.c_void_p(valid.data_ptr())
        for t, shape in ((utimes, (self.B,)), (valid, (self.B,))):
            if t is not None and (tuple(t.shape) != shape or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("utimes / valid must be contiguous device tensors of shape [B]")
        pz, m1 = _ptr(z_out, shape=(2, self.B))
        pq, m2 = _ptr(quat_out, shape=(4, self.B))
        pm, m3 = _ptr(mask_out, np.uint8, shape=(2, self.B))
        if any(m is not None and m != PB_DEVICE for m in (m1, m2, m3)):
            raise ValueError("yaw-lock outputs must be device tensors")
        self._chk(fn(self._h, int(utime), pu, pv, rows, pj, mj, pz, pq, pm))

    def yawlock_update_joints(self, utime, joint_position, utimes=None, valid=None, z_out=None, quat_out=None, mask_out=None):
        """YawLockHandler::processMessage, form only: z_out [2,B], quat_out [4,B], mask_out [2,B] device tensors."""
        self._yawlock_call(self._L.pb_yawlock_update_joints, utime, joint_position, utimes, valid, z_out, quat_out, mask_out)

    def step_yawlock_joints(self, utime, joint_position, utimes=None, valid=None, z_out=None, quat_out=None, mask_out=None):
        """the same, formed and applied in one kernel: pb_step_yawlock_joints"""
        self._yawlock_call(self._L.pb_step_yawlock_joints, utime, joint_position, utimes, valid, z_out, quat_out, mask_out)

    def yawlock_get(self, b):
        """(poses [14], dict(counter, lock_init, disable_until, outcome, slips)) of filter b"""
        poses = (C.c_double * 14)()
        info = (C.c_int64 * 4)()
        self._chk(self._L.pb_yawlock_get(self._h, int(b), poses, info))
        return np.array(poses), dict(counter=int(info[0]), lock_init=int(info[1]), disable_until=int(info[2]), outcome=int(info[3]) & 255,
                                     slips=int(info[3]) >> 8)

    # --- accuracy against ground truth (drift_per_distance.py) ---
    SCORE_METRICS = {"mean_pddt": _lib.PB_SCORE_MEAN_PDDT, "rms_drift": _lib.PB_SCORE_RMS_DRIFT, "ate_rmse": _lib.PB_SCORE_ATE_RMSE}

    def score_init(self, time_threshold_s=10.0, distance_threshold=0.0):
        """the script's State for every filter (again = reset); the defaults are the script's"""
        if not (time_threshold_s >= 0 and distance_threshold >= 0):
            raise ValueError("score_init: thresholds must be >= 0")
        self._chk(self._L.pb_score_init(self._h, float(time_threshold_s), float(distance_threshold)))

    def score_ground_truth(self, utime, pose7, valid=None, utimes=None, slot=_lib.PB_SLOT_HEAD, drift=True, absolute=False):
        """on_pose_gt for every filter.  pose7 = pos[3], orientation[4] (w, x, y, z): [7, B] (numpy or device tensor) or a 1-D numpy
        array of 7 values, one robot's truth for every filter.  valid [B] uint8 / utimes [B] int64 live where pose7 lives (numpy for
        the 7-value form)."""
        flags = (_lib.PB_SCORE_DRIFT if drift else 0) | (_lib.PB_SCORE_ABS if absolute else 0)
        if not flags:
            raise ValueError("score_ground_truth: drift and / or absolute")
        pp, mp = _ptr_block(pose7, 7, self.B)
        if pp is None:
            raise ValueError("score_ground_truth: pose7 is required")
        pv, mv = _ptr(valid, np.uint8, shape=(self.B,))
        pu, mu = _ptr(utimes, np.int64, shape=(self.B,))
        _same_mem(PB_HOST if mp == PB_HOST_BROADCAST else mp, mv, mu)
        self._chk(self._L.pb_score_ground_truth(self._h, int(utime), pu, pp, pv, int(slot), flags, mp))

    def score_get(self, first=0, count=None):
        """(rows [PB_SCORE_ROWS, count] float64, counts [PB_SCORE_COUNTS, count] int64), host"""
        count = self.B - first if count is None else count
        if first < 0 or count < 0 or first + count > self.B:
            raise ValueError("score_get: range [%d, +%d) outside batch %d" % (first, count, self.B))
        rows, counts = np.empty((_lib.PB_SCORE_ROWS, count)), np.empty((_lib.PB_SCORE_COUNTS, count), dtype=np.int64)
        self._chk(self._L.pb_score_get(self._h, int(first), int(count), C.c_void_p(rows.ctypes.data), C.c_void_p(counts.ctypes.data), PB_HOST))
        return rows, counts

    def score_last(self, b):
        """the newest error_metrics_t of filter b (utime = -2: no window yet)"""
        if not 0 <= b < self.B:
            raise ValueError("score_last: filter %d of %d" % (b, self.B))
        ut, out = C.c_int64(), (C.c_double * 10)()
        self._chk(self._L.pb_score_last(self._h, int(b), C.byref(ut), out))
        o = np.array(out)
        return dict(utime=ut.value, pos_error=o[0:3], pos_error_norm=o[3], rpy_error=o[4:7], distance_travelled=o[7], percent_ddt=o[8],
                    time_elapsed=o[9])

    def score_best(self, metric="mean_pddt"):
        """(filter, value) with the smallest metric among the filters that have data; filter = -1: none has"""
        m = self.SCORE_METRICS.get(metric, metric)
        if m not in self.SCORE_METRICS.values():
            raise ValueError("score_best: metric must be one of %s" % sorted(self.SCORE_METRICS))
        f, v = C.c_int(), C.c_double()
        self._chk(self._L.pb_score_best(self._h, int(m), C.byref(f), C.byref(v)))
        return f.value, v.value

    # --- IMU front end ---
    def imu_notch_init(self, notch_freq, fs=1000.0):
        self._chk(self._L.pb_imu_notch_init(self._h, notch_freq, fs))

    def imu_notch(self, accel_packets, accel_out):
        """accel_packets [n_packets,3,B] oldest first -> accel_out [3,B] (newest filtered sample)."""
        if accel_packets.ndim != 3:
            raise ValueError("accel_packets must be [n_packets, 3, B]")
        pi, m1 = _ptr(accel_packets, shape=(accel_packets.shape[0], 3, self.B))
        po_, m2 = _ptr(accel_out, shape=(3, self.B))
        self._chk(self._L.pb_imu_notch(self._h, accel_packets.shape[0], pi, po_, _same_mem(m1, m2)))

    def imu_notch_counts(self, counts, accel_packets, accel_out):
        """imu_notch with a packet count per filter (pb_imu_notch_counts): counts [B] int32, accel_packets [max_packets,3,B]; a filter
        without a new packet keeps its accel_out entries (device tensors) or gets 0 (numpy)."""
        if accel_packets.ndim != 3:
            raise ValueError("accel_packets must be [max_packets, 3, B]")
        pc, m0 = _ptr(counts, np.int32, shape=(self.B,))
        pi, m1 = _ptr(accel_packets, shape=(accel_packets.shape[0], 3, self.B))
        po_, m2 = _ptr(accel_out, shape=(3, self.B))
        self._chk(self._L.pb_imu_notch_counts(self._h, accel_packets.shape[0], pc, pi, po_, _same_mem(m0, m1, m2)))

    def ins_body_block(self, gyro, accel, rot_quat, imu_block_out, raw_dt=None, utimes=None, utime=0, valid=None, trans_vec=None,
                       dt_default=0.0, dt_from_utimes=False, valid_out=None):
        """InsHandler's per-message arithmetic (pb_ins_body_block): gyro / accel [3,B], raw_dt [B], utimes [B] int64, valid [B] uint8 live
        in one space (numpy or device tensors); rot_quat (w, x, y, z) and trans_vec are 4 / 3 values; imu_block_out [7,B] and valid_out
        [B] uint8 are device tensors."""
        pg, m1 = _ptr(gyro, shape=(3, self.B))
        pa, m2 = _ptr(accel, shape=(3, self.B))
        pr, m3 = _ptr(raw_dt, shape=(self.B,))
        pu, m4 = _ptr(utimes, np.int64, shape=(self.B,))
        pv, m5 = _ptr(valid, np.uint8, shape=(self.B,))
        po_, mo = _ptr(imu_block_out, shape=(7, self.B))
        pvo, mvo = _ptr(valid_out, np.uint8, shape=(self.B,))
        if mo != PB_DEVICE or (valid_out is not None and mvo != PB_DEVICE):
            raise ValueError("ins_body_block outputs must be device tensors")
        rq = (C.c_double * 4)(*rot_quat)
        tv = None if trans_vec is None else (C.c_double * 3)(*trans_vec)
        self._chk(self._L.pb_ins_body_block(self._h, pg, pa, pr, pu, int(utime), pv, rq, tv, float(dt_default), int(bool(dt_from_utimes)),
                                            _same_mem(m1, m2, m3, m4, m5), po_, pvo))

    def ins_body_reset(self):
        """forget every filter's last body-frame sample and previous message time (pb_ins_body_reset)"""
        self._chk(self._L.pb_ins_body_reset(self._h))

    def set_imu_valid(self, valid_dev):
        """valid_dev [B] uint8 device tensor (0 = no IMU message), or None: for the NEXT call that takes an IMU step (pb_set_imu_valid);
        the tensor must stay alive until that step has run."""
        p, m = _ptr(valid_dev, np.uint8, shape=(self.B,))
        if valid_dev is not None and m != PB_DEVICE:
            raise ValueError("the IMU validity mask must be a device tensor")
        self._chk(self._L.pb_set_imu_valid(self._h, p))

    # --- update objects ---
    def reset(self, vec, quat, cov, broadcast=False):
        """RBISResetUpdate.  vec [n,B], quat [4,B], cov [n,n,B] indexed [row,col,b] (or [n],[4],[n,n] broadcast)."""
        if _is_torch(cov):
            cov_cm = cov.transpose(0, 1).contiguous()
        else:
            cov_cm = np.ascontiguousarray(np.swapaxes(cov, 0, 1))  # column-major flat index c*n+r
        n, B = self.n, self.B
        pv, m1 = _ptr(vec, shape=(n,) if broadcast else (n, B))
        pq, m2 = _ptr(quat, shape=(4,) if broadcast else (4, B))
        pc, m3 = _ptr(cov_cm, shape=(n, n) if broadcast else (n, n, B))
        self._chk(self._L.pb_reset(self._h, pv, pq, pc, int(broadcast), _same_mem(m1, m2, m3)))

    def predict(self, imu_block, q4):
        p, m = _ptr_block(imu_block, 7, self.B)
        q = (C.c_double * 4)(*q4)
        self._chk(self._L.pb_predict(self._h, p, q, m))

    def _r(self, R, m):
        if isinstance(R, (list, tuple)) or (isinstance(R, np.ndarray) and R.ndim == 1):
            arr = np.ascontiguousarray(R, dtype=np.float64)
            if arr.shape == (m * m,) and m > 1:  # one full column-major R for every filter
                return arr, C.c_void_p(arr.ctypes.data), PB_R_FULL, PB_HOST_BROADCAST
            assert arr.shape == (m,)
            return arr, C.c_void_p(arr.ctypes.data), PB_R_DIAG_BROADCAST, None
        kind = PB_R_DIAG if R.shape[0] == m and len(R.shape) == 2 else PB_R_FULL
        p, mem = _ptr(R, shape=(m, self.B) if kind == PB_R_DIAG else (m * m, self.B))
        return R, p, kind, mem

    def update_indexed(self, idx, z, R, mask=None, quat_meas=None):
        """RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement.  z [m,B];
        R: length-m list (broadcast diag), [m,B] per-filter diag, or [m*m,B] full column-major."""
        m = len(idx)
        ia = (C.c_int * m)(*[int(i) for i in idx])
        pz, mz = _ptr_block(z, m, self.B)
        _keep, pr, kind, mr = self._r(R, m)
        pm, mm = _ptr(mask, np.uint8, shape=(self.B,))
        if quat_meas is None:
            self._chk(self._L.pb_update_indexed(self._h, m, ia, pz, pr, kind, pm, _same_mem(mz, mr, mm)))
        else:
            pq, mq = _ptr_block(quat_meas, 4, self.B)
            self._chk(self._L.pb_update_indexed_orient(self._h, m, ia, pz, pr, kind, pq, pm, _same_mem(mz, mr, mm, mq)))

    def update_indexed_wide(self, idx, z, R, mask=None, quat_meas=None):
        """update_indexed for index lists of up to nine rows (pb_update_indexed_wide: the GPF's all_states list, velocity + chi +
        position).  Up to six rows run exactly what update_indexed runs; z and R as there."""
        m = len(idx)
        ia = (C.c_int * m)(*[int(i) for i in idx])
        pz, mz = _ptr_block(z, m, self.B)
        _keep, pr, kind, mr = self._r(R, m)
        pm, mm = _ptr(mask, np.uint8, shape=(self.B,))
        pq, mq = (None, None) if quat_meas is None else _ptr_block(quat_meas, 4, self.B)
        self._chk(self._L.pb_update_indexed_wide(self._h, m, ia, pz, pr, kind, pq, pm, _same_mem(mz, mr, mm, mq)))

    # --- optical-flow sigma-point update (pb_flow_set_camera, pb_update_optical_flow) ---
    def flow_set_camera(self, body_to_cam_trans, zeta1, zeta2, eta):
        """The camera of update_optical_flow: its position in the body frame and zeta1, zeta2, eta as RBISOpticalFlowMeasurement's
        constructor takes them, the rows of the body -> camera rotation (pb_flow_set_camera)."""
        args = []
        for v in (body_to_cam_trans, zeta1, zeta2, eta):
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.shape != (3,):
                raise ValueError("expected 3 values, got shape %s" % (a.shape,))
            args.append((C.c_double * 3)(*a))
        self._chk(self._L.pb_flow_set_camera(self._h, *args))

    def update_optical_flow(self, flow_block, R, mask=None, flags=0, want_zhat=False, want_status=False):
        """RBISOpticalFlowMeasurement: the four-row unscented update of every filter (pb_update_optical_flow).  flow_block [7,B] (or a
        1-D numpy array of 7 values: one message for every filter): ux, uy, theta, scale, alpha1, alpha2, gamma; R: length-4 list
        (broadcast diagonal), [4,B] or [16,B] full column-major; flags: PB_FLOW_HEAD_QUAT.  Returns (zhat [4,B] or None, status [B]
        int32 or None), device tensors: the predicted measurement (filters with status 0 only; NaN elsewhere) and 0 applied /
        1 masked off / 2 + k pivot k of the factor of P not positive."""
        import torch
        pf, mf = _ptr_block(flow_block, 7, self.B)
        _keep, pr, kind, mr = self._r(R, 4)
        pm, mm = _ptr(mask, np.uint8, shape=(self.B,))
        dev = "cuda:%d" % self.device
        zhat = torch.full((4, self.B), float("nan"), dtype=torch.float64, device=dev) if want_zhat else None
        status = torch.empty((self.B,), dtype=torch.int32, device=dev) if want_status else None
        self._chk(self._L.pb_update_optical_flow(self._h, pf, pr, kind, pm, _same_mem(mf, mr, mm), int(flags),
                                                 C.c_void_p(zhat.data_ptr()) if want_zhat else None,
                                                 C.c_void_p(status.data_ptr()) if want_status else None))
        return zhat, status

    # --- Gaussian particle filter measurement (pb_gpf_*) ---
    def _gpf_dev(self, a, shape, dtype=np.float64):
        """a device tensor of `shape` from a torch tensor or a numpy array (uploaded); the shape is checked before any ABI call"""
        import torch
        if tuple(a.shape) != tuple(shape):
            raise ValueError("expected an array of shape %s, got %s" % (tuple(shape), tuple(a.shape)))
        want = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
        t = torch.as_tensor(a) if not _is_torch(a) else a
        if t.dtype != want:
            raise TypeError("expected %s values" % want)
        return t.to("cuda:%d" % self.device).contiguous()

    def _gpf_empty(self, shape, dtype=None):
        import torch
        return torch.empty(shape, dtype=dtype or torch.float64, device="cuda:%d" % self.device)

    @staticmethod
    def _gpf_idx(idx, K):
        m = len(idx)
        if not 1 <= m <= 9:
            raise ValueError("the GPF takes 1..9 rows (got %d)" % m)
        if int(K) < 1:
            raise ValueError("K must be at least 1")
        return m, (C.c_int * m)(*[int(i) for i in idx])

    def gpf_normals(self, seed, stream_id, rows):
        """[rows, B] standard normals on the device, counter-based: Philox4x32-10 keyed by seed over (filter, row pair, stream_id),
        Box-Muller (pb_gpf_normals).  The same arguments give the same bits."""
        if int(rows) < 1:
            raise ValueError("rows must be at least 1")
        out = self._gpf_empty((int(rows), self.B))
        self._chk(self._L.pb_gpf_normals(self._h, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1), int(rows), C.c_void_p(out.data_ptr())))
        return out

    def gpf_sample(self, idx, xi):
        """xi [K, m, B] standard normals -> (delta [K, m, B], pose [K, 7, B]) device tensors: K draws from the marginal of the rows idx
        of every filter and the poses (position xyz, quaternion wxyz) of the sampled states (pb_gpf_sample)."""
        K = xi.shape[0]
        m, ia = self._gpf_idx(idx, K)
        x = self._gpf_dev(xi, (K, m, self.B))
        delta, pose = self._gpf_empty((K, m, self.B)), self._gpf_empty((K, 7, self.B))
        self._chk(self._L.pb_gpf_sample(self._h, m, ia, K, C.c_void_p(x.data_ptr()), C.c_void_p(delta.data_ptr()), C.c_void_p(pose.data_ptr())))
        return delta, pose

    def gpf_measurement(self, idx, delta, loglik, max_weight_proportion=0.999):
        """delta [K, m, B], loglik [K, B] -> (z_eff [m, B], R_eff [m*m, B], status int32 [B]) device tensors, the blocks
        update_indexed_wide takes (pb_gpf_measurement).  status 0: as computed, 1: negative eigenvalues of R_eff replaced, 2: the weights
        are ill-conditioned, R_eff = 1e4 I and z_eff = x[idx]."""
        import torch
        K = delta.shape[0]
        m, ia = self._gpf_idx(idx, K)
        d, l = self._gpf_dev(delta, (K, m, self.B)), self._gpf_dev(loglik, (K, self.B))
        z, R, status = self._gpf_empty((m, self.B)), self._gpf_empty((m * m, self.B)), self._gpf_empty((self.B,), torch.int32)
        self._chk(self._L.pb_gpf_measurement(self._h, m, ia, K, C.c_void_p(d.data_ptr()), C.c_void_p(l.data_ptr()), float(max_weight_proportion),
                                             C.c_void_p(z.data_ptr()), C.c_void_p(R.data_ptr()), C.c_void_p(status.data_ptr())))
        return z, R, status

    def gpf_grid_set(self, origin, resolution, values, unknown_loglike, cov_scaling):
        """The built-in likelihood's map: values [nz, ny, nx] (numpy; what -node->getLogOdds() would return), origin (3), resolution."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 3 or len(origin) != 3:
            raise ValueError("values must be [nz, ny, nx] and origin have three entries")
        o = (C.c_double * 3)(*[float(a) for a in origin])
        dims = (C.c_int * 3)(v.shape[2], v.shape[1], v.shape[0])
        self._chk(self._L.pb_gpf_grid_set(self._h, o, float(resolution), dims, C.c_void_p(v.ctypes.data), float(unknown_loglike), float(cov_scaling)))

    def gpf_grid_loglik(self, pose, points):
        """pose [K, 7, B] -> loglik [K, B] (device tensor) of the scan `points`: [3 n, B] per filter (torch device tensor or numpy), or a
        1-D numpy array of 3 n values, one robot's scan for every filter (pb_gpf_grid_loglik).  Points with a non-finite x are skipped."""
        K = pose.shape[0]
        if K < 1:
            raise ValueError("K must be at least 1")
        p = self._gpf_dev(pose, (K, 7, self.B))
        if points.shape[0] % 3:
            raise ValueError("points must have 3 n rows")
        n = points.shape[0] // 3
        pp, mem = _ptr_block(points, 3 * n, self.B)
        out = self._gpf_empty((K, self.B))
        self._chk(self._L.pb_gpf_grid_loglik(self._h, K, C.c_void_p(p.data_ptr()), n, pp, mem, C.c_void_p(out.data_ptr())))
        return out

    def gpf_update(self, idx, K, loglik_fn, seed, stream_id=0, max_weight_proportion=0.999, mask=None):
        """One whole GPF update: normals -> samples -> loglik_fn(pose [K, 7, B]) -> [K, B] (any torch function of the poses, or
        self.gpf_grid_loglik) -> the effective measurement -> update_indexed_wide.  Returns (z_eff, R_eff, status)."""
        m = len(idx)
        xi = self.gpf_normals(seed, stream_id, int(K) * m).view(int(K), m, self.B)
        delta, pose = self.gpf_sample(idx, xi)
        z, R, status = self.gpf_measurement(idx, delta, loglik_fn(pose), max_weight_proportion)
        if mask is not None and not _is_torch(mask):      # (z and R are device blocks: the mask goes where they are)
            import torch
            mask = torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8)).to(z.device)
        self.update_indexed_wide(idx, z, R, mask=mask)
        return z, R, status

    def step_legodo(self, imu_block, lo_block, mask, q4):
        """IMU block and leg-odometry block (+ mask) may live in different spaces (e.g. a broadcast [7] IMU message and a
        per-filter device measurement from legodo_update(..., after_predict=imu)): pb_step_legodo_split."""
        pi, m1 = _ptr_block(imu_block, 7, self.B)
        pl, m2 = _ptr_block(lo_block, 6, self.B)
        pm, m3 = _ptr(mask, np.uint8, shape=(self.B,))
        q = (C.c_double * 4)(*q4)
        mlo = _same_mem(m2, m3)
        if m1 == mlo:
            self._chk(self._L.pb_step_legodo(self._h, pi, pl, pm, q, m1))
        else:
            self._chk(self._L.pb_step_legodo_split(self._h, pi, m1, pl, pm, mlo, q))

    def step_legodo_correct(self, imu_block, lo_block, mask, q4, corr_kind, z2, R2, quat_meas2, mask2=None):
        """predict + leg-odometry update + one more orientation update (corr_kind: _lib.PB_CORR_POS_ORIENT m=6 idx
        9,10,11,6,7,8 / PB_CORR_POS_YAW m=4 idx 9,10,11,8) in one state round trip.  R2: length-m list or [m,B]."""
        pi, m1 = _ptr_block(imu_block, 7, self.B)
        pl, m2 = _ptr_block(lo_block, 6, self.B)
        pm, m3 = _ptr(mask, np.uint8, shape=(self.B,))
        if corr_kind not in (_lib.PB_CORR_POS_ORIENT, _lib.PB_CORR_POS_YAW):
            raise ValueError("corr_kind must be PB_CORR_POS_ORIENT or PB_CORR_POS_YAW")
        m = 6 if corr_kind == _lib.PB_CORR_POS_ORIENT else 4
        pz, m4 = _ptr_block(z2, m, self.B)
        _keep, pr, kind, m5 = self._r(R2, m)
        pq, m6 = _ptr_block(quat_meas2, 4, self.B)
        pm2, m7 = _ptr(mask2, np.uint8, shape=(self.B,))
        q = (C.c_double * 4)(*q4)
        self._chk(self._L.pb_step_legodo_correct(self._h, pi, pl, pm, q, _same_mem(m1, m2, m3), int(corr_kind), pz, pr, kind,
                                                 pq, pm2, _same_mem(m4, m5, m6, m7)))

    def run_legodo(self, imu_stream, lo_stream, mask_stream, q4, timed=False):
        """n_steps fused steps from device-resident streams [T,7,B], [T,6,B], [T,B]; returns device ms if timed."""
        T = imu_stream.shape[0]
        pi, m1 = _ptr(imu_stream, shape=(T, 7, self.B))
        pl, m2 = _ptr(lo_stream, shape=(T, 6, self.B))
        pm, m3 = _ptr(mask_stream, np.uint8, shape=(T, self.B))
        if _same_mem(m1, m2, m3) != PB_DEVICE:
            raise ValueError("run_legodo needs device-resident streams")
        q = (C.c_double * 4)(*q4)
        ms = C.c_float(0)
        self._chk(self._L.pb_run_legodo(self._h, T, pi, pl, pm, q, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def replay_legodo_fused(self, imu_stream, lo_stream, mask_stream, q4, steps_per_launch, timed=False):
        """Time-fused replay (P resident in registers for steps_per_launch steps); same results as run_legodo."""
        T = imu_stream.shape[0]
        pi, m1 = _ptr(imu_stream, shape=(T, 7, self.B))
        pl, m2 = _ptr(lo_stream, shape=(T, 6, self.B))
        pm, m3 = _ptr(mask_stream, np.uint8, shape=(T, self.B))
        if _same_mem(m1, m2, m3) != PB_DEVICE:
            raise ValueError("replay_legodo_fused needs device-resident streams")
        q = (C.c_double * 4)(*q4)
        ms = C.c_float(0)
        self._chk(self._L.pb_replay_legodo_fused(self._h, T, steps_per_launch, pi, pl, pm, q, C.byref(ms) if timed else None))
        return ms.value if timed else None

    def replay_legodo_checkpointed(self, imu_stream, lo_stream, mask_stream, q4, steps_per_launch, first_slot=0, timed=False):
        """The time-fused replay as a forward pass that keeps every posterior: step t also lands in checkpoint slot first_slot + t
        (history_reserve first), the state stays in registers -- pb_replay_legodo_checkpointed."""
        T = imu_stream.shape[0]
        pi, m1 = _ptr(imu_stream, shape=(T, 7, self.B))
        pl, m2 = _ptr(lo_stream, shape=(T, 6, self.B))
        pm, m3 = _ptr(mask_stream, np.uint8, shape=(T, self.B))
        if _same_mem(m1, m2, m3) != PB_DEVICE:
            raise ValueError("replay_legodo_checkpointed needs device-resident streams")
        q = (C.c_double * 4)(*q4)
        ms = C.c_float(0)
        self._chk(self._L.pb_replay_legodo_checkpointed(self._h, T, steps_per_launch, pi, pl, pm, q, int(first_slot), C.byref(ms) if timed else None))
        return ms.value if timed else None

    # --- fovis history ---
    def snapshot(self, slot=0):
        self._chk(self._L.pb_snapshot(self._h, slot))

    def compose_delta(self, slot, t, q, z_out, quat_out):
        pt, m1 = _ptr_block(t, 3, self.B)
        pq, m2 = _ptr_block(q, 4, self.B)
        pz, m3 = _ptr(z_out, shape=(3, self.B))
        po_, m4 = _ptr(quat_out, shape=(4, self.B))
        if m3 != PB_DEVICE or m4 != PB_DEVICE:
            raise ValueError("compose_delta outputs must be device tensors")
        self._chk(self._L.pb_compose_delta(self._h, slot, pt, pq, pz, po_, _same_mem(m1, m2)))

    # --- queries ---
    def get_head(self, first=0, count=None, want_cov=True):
        """getHeadState: (vec [n,c], quat [4,c], cov [n,n,c] indexed [row,col,b] or None, ll [c]) as numpy."""
        count = self.B - first if count is None else count
        n = self.n
        vec = np.empty((n, count))
        quat = np.empty((4, count))
        ll = np.empty(count)
        cov = np.empty((n, n, count)) if want_cov else None
        self._chk(self._L.pb_get_head(self._h, first, count, C.c_void_p(vec.ctypes.data), C.c_void_p(quat.ctypes.data),
                                      C.c_void_p(cov.ctypes.data) if want_cov else None, C.c_void_p(ll.ctypes.data),
                                      PB_HOST))
        if want_cov:
            cov = np.swapaxes(cov, 0, 1)  # stored [col,row,b] -> [row,col,b]
        return vec, quat, cov, ll

    def filter_state(self, b):
        q = (C.c_double * 4)()
        s = (C.c_double * 21)()
        c = (C.c_double * 441)()
        self._chk(self._L.pb_get_filter_state(self._h, b, q, s, c))
        return np.array(q), np.array(s), np.array(c).reshape(21, 21).T  # cov col-major -> [row,col]

    def calib_copy(self, reps=10):
        """device ms for `reps` plain copies of the state array (counter calibration / copy-rate probe)."""
        ms = C.c_float(0)
        self._chk(self._L.pb_calib_copy(self._h, reps, C.byref(ms)))
        return ms.value

    def state_checksum(self, slot=-1):
        """(sum, xor) over every 64-bit word of the device state (slot < 0: the head)."""
        out = (C.c_uint64 * 2)()
        self._chk(self._L.pb_state_checksum(self._h, int(slot), out))
        return int(out[0]), int(out[1])

    def summary(self):
        out = (C.c_double * 4)()
        self._chk(self._L.pb_summary(self._h, out))
        return np.array(out)
