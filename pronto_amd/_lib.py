"""Build / load libpronto_batch.so (the C ABI of include/pronto_batch.h).

There is no CPU fallback: if the shared library is missing or no gfx950 device is visible, the
product path raises.  The library is kept IN-TREE (pronto_amd/lib/) so it travels with the repo
snapshot and shows up as a loaded native module.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("PRONTO_BATCH_LIB") or os.path.join(_HERE, "lib", "libpronto_batch.so")  # env: A/B builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pronto_batch.h")

PB_OK, PB_ERR_ARG, PB_ERR_HIP, PB_ERR_NO_DEVICE, PB_ERR_STATE = range(5)
PB_HOST, PB_DEVICE, PB_HOST_BROADCAST = 0, 1, 2
PB_R_DIAG_BROADCAST, PB_R_DIAG, PB_R_FULL = 0, 1, 2
PB_CORR_POS_ORIENT, PB_CORR_POS_YAW = 0, 1
PB_SLOT_HEAD = -1
PB_FLOW_HEAD_QUAT = 1
PB_SCORE_DRIFT, PB_SCORE_ABS = 1, 2
PB_SCORE_ROWS, PB_SCORE_COUNTS = 35, 5
PB_SCORE_MEAN_PDDT, PB_SCORE_RMS_DRIFT, PB_SCORE_ATE_RMSE = 0, 1, 2
(PB_LEGPAR_R_VXYZ, PB_LEGPAR_R_VXYZ_UNCERTAIN, PB_LEGPAR_R_VANG, PB_LEGPAR_R_VANG_UNCERTAIN, PB_LEGPAR_R_XYZ, PB_LEGPAR_SCHMITT_LOW,
 PB_LEGPAR_SCHMITT_HIGH, PB_LEGPAR_SCHMITT_LOW_DELAY, PB_LEGPAR_SCHMITT_HIGH_DELAY, PB_LEGPAR_TOTAL_FORCE,
 PB_LEGPAR_STANDING_SCHMITT_LEVEL, PB_LEGPAR_ROWS) = range(12)


def sources():
    """every file the library is made from: all of csrc/ (a superset; the Makefile keeps the exact dependencies) and the header"""
    return [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp")) or f == "Makefile"] + [HEADER]


def is_stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > t for s in sources())


def build(force=False):
    """hipcc --offload-arch=gfx950 -shared (cross-compiles without a GPU)."""
    if force or is_stale():
        # (the translation units are independent: a serial from-scratch build takes ~10 minutes, -j8 ~2.5)
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j%d" % max(1, min(8, os.cpu_count() or 1))] + (["-B"] if force else []))
    return LIB_PATH


class CorrStream(C.Structure):
    """pb_corr_stream (pb_smooth_log_corrected)"""
    _fields_ = [("kind", C.c_int), ("n_ticks", C.c_int), ("step", C.c_void_p), ("z2", C.c_void_p), ("R2", C.c_void_p), ("r_kind2", C.c_int),
                ("quat_meas2", C.c_void_p), ("mask2", C.c_void_p)]


_lib = None

_dp = C.POINTER(C.c_double)
_SIGS = {
    "pb_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "pb_destroy": (C.c_int, [C.c_void_p]),
    "pb_last_error": (C.c_char_p, [C.c_void_p]),
    "pb_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pb_use_own_stream": (C.c_int, [C.c_void_p]),
    "pb_set_constants": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "pb_sync": (C.c_int, [C.c_void_p]),
    "pb_hot_kernel": (C.c_char_p, [C.c_void_p]),
    "pb_batch": (C.c_int, [C.c_void_p]),
    "pb_run_block": (C.c_int, [C.c_void_p]),
    "pb_n_states": (C.c_int, [C.c_void_p]),
    "pb_malloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "pb_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pb_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "pb_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "pb_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "pb_fence_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pb_fence_record": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_fence_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_upload_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]),
    "pb_upload_join": (C.c_int, [C.c_void_p]),
    "pb_upload_sync": (C.c_int, [C.c_void_p]),
    "pb_imu_notch_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_ins_body_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, _dp, _dp,
                                    C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pb_set_imu_valid": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pb_ins_body_reset": (C.c_int, [C.c_void_p]),
    "pb_get_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_smooth_log_slots": (C.c_int, [C.c_int, C.c_int]),
    "pb_smooth_log": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_float)]),
    "pb_smooth_log_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_double, C.c_int, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_float)]),
    "pb_smooth_log_corrected": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_double, C.c_int, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "pb_set_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_predict": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_int]),
    "pb_update_indexed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int]),
    "pb_update_indexed_orient": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int]),
    "pb_update_indexed_wide": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int]),
    "pb_gpf_normals": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]),
    "pb_gpf_sample": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pb_gpf_measurement": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "pb_gpf_grid_set": (C.c_int, [C.c_void_p, _dp, C.c_double, C.POINTER(C.c_int), C.c_void_p, C.c_double, C.c_double]),
    "pb_gpf_grid_loglik": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pb_flow_set_camera": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "pb_update_optical_flow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pb_step_legodo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int]),
    "pb_step_legodo_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _dp]),
    "pb_step_legodo_correct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_run_legodo": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.POINTER(C.c_float)]),
    "pb_replay_legodo_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp,
                                         C.POINTER(C.c_float)]),
    "pb_replay_legodo_checkpointed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int,
                                                C.POINTER(C.c_float)]),
    "pb_snapshot": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_compose_delta": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_set_process_noise_block": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pb_window_nll": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_int]),
    "pb_legodo_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_int64, C.c_int]),
    "pb_legodo_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pb_legodo_update_after_predict": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pb_legodo_set_contact_mode": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int]),
    "pb_legodo_set_control_contacts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pb_legodo_set_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_float)]),
    "pb_legodo_update_joints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "pb_legodo_set_param_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pb_legodo_set_zero_initial_velocity": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_legodo_set_message_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_legodo_set_measurement_mode": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]),
    "pb_step_legodo_joints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "pb_step_legodo_feet": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _dp, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                      C.c_double, C.c_void_p, C.c_void_p]),
    "pb_calib_copy_checksum": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "pb_legodo_fk": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pb_joint_filter_init": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]),
    "pb_joint_filter": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "pb_legodo_get": (C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]),
    "pb_yawlock_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "pb_yawlock_set_standing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pb_yawlock_set_gyro": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pb_yawlock_update_joints": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "pb_step_yawlock_joints": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "pb_yawlock_get": (C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]),
    "pb_score_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "pb_score_ground_truth": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "pb_score_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_score_last": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), _dp]),
    "pb_score_best": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp]),
    "pb_imu_notch_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "pb_imu_notch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_history_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_state_save": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_set_output_slot": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_set_pred_slot": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_head_slot": (C.c_int, [C.c_void_p]),
    "pb_snapshot_from_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "pb_host_alloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "pb_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pb_state_restore": (C.c_int, [C.c_void_p, C.c_int]),
    "pb_smooth_step": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    "pb_smooth_step_masked": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int]),
    "pb_slot_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "pb_get_head": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "pb_get_filter_state": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "pb_summary": (C.c_int, [C.c_void_p, _dp]),
    "pb_mask_count": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "pb_state_checksum": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "pb_calib_copy": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "pb_set_utime": (C.c_int, [C.c_void_p, C.c_int64]),
    "pb_get_utime": (C.c_int64, [C.c_void_p]),
    "pb_version": (C.c_char_p, []),
}


def exported_names():
    return sorted(_SIGS)


def load():
    """dlopen the library and bind every symbol the header declares; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "pronto_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    try:  # share torch's HIP runtime when torch is present (same soname, libamdhip64.so.7)
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if not hasattr(lib, name) and os.environ.get("PRONTO_BATCH_LIB"):
            continue  # an older A/B build named by PRONTO_BATCH_LIB may lack the newest entry points (timing runs only)
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
