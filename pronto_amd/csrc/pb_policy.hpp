// pb_policy.hpp -- which kernel runs: every decision of a kernel, a grid shape or a cache policy the library takes, and the one reader of
// the environment switches behind them.  Host-only: no HIP header, no kernel header, nothing that launches; it compiles with plain
// g++ -std=c++17, and tests/cpp/policy_table.cpp (tests/test_kernel_policy.py) checks it on the CPU.  pb_create makes ONE Policy per
// context (make_policy: pure, from the state size, the batch, the state bytes and the switches); the launchers of the pb_*.hip units
// switch on what the functions below answer and decide nothing themselves.
#pragma once

#include <cstdlib>
#include <cstring>

#include "../../include/pronto_batch.h"

namespace pb {

// Memory hint of the state round trip in the step kernels (template parameter MH, rbis_tile_io.hpp MemHint), picked here from the
// state size: while the state fits the 256 MB memory-side cache, stores with sc1 (write through the XCD's L2) are
// a few % faster; far beyond it, non-temporal loads AND stores are; in between neither helps.
enum { MH_DEFAULT = 0, MH_STORE_SC1 = 1, MH_STREAM_NT = 2 };
// k_update_coop_rt, k_update_quad_rt and k_update_quad_list are built for two cache policies: non-temporal streaming falls back to
// the default one
constexpr int two_policy_hint(int mh) { return mh == MH_STORE_SC1 ? MH_STORE_SC1 : MH_DEFAULT; }

// doubles of one filter in the tiled layout, Slots<NS>::NSLOT of rbis_device.hpp (asserted in pronto_batch.hip): the components --
// state, quaternion, log-likelihood, packed covariance -- rounded up to whole 16-byte pairs
constexpr int state_slots(int ns) { return ns == 15 ? 140 : 258; }
constexpr long state_bytes(int ns, long batch) { return (batch + 63) / 64 * 64 * state_slots(ns) * 8; }

// ---- the environment, read once per context (a function-local static kept the FIRST call's value for the whole process) ----
struct Switches {
  int coop15 = -1, xcd = -1, blocked = -1;   // -1: unset, else 0 / 1
  bool half = false, replay_onelane = false, generic_update = false, quad21 = true;
  bool has_mem_hint = false, has_block_filters = false;
  int mem_hint = 0;          // as given, possibly out of range
  long block_filters = 0;
  bool smooth_pivot = false, smooth_reg = false, smooth_lane = false;
  int smooth_grid = 0;
};

inline int env_flag(const char *e) { return e ? (e[0] == '1') : -1; }

inline Switches read_switches()
{
  Switches s;
  // 15-state hot kernel: the two-wave cooperative mapping (2 waves/SIMD, reads and writes interleave) measured
  // 3-20 % faster up to 256k filters, the one-lane-per-filter k_step 3-5 % faster beyond (profiles/).
  // =0/1 forces one of them (A/B runs and tests).
  s.coop15 = env_flag(getenv("PRONTO_BATCH_COOP15"));
  // Below ~48k filters the two-wave kernel's 64-filter tiles leave workgroup slots empty (1 024 slots: 256 CUs x 4 workgroups of two
  // waves at two waves per SIMD; 32 768 filters = 512 tiles).  Two workgroups per tile, 32 filters each, fill them -- and change
  // nothing: 13.12 against 13.14 us at 32 768 filters, slower everywhere else (profiles/r05_half_tile.txt).  The step time is
  // ~5 us of one tile's dependent chain + bytes / 9.4 TB/s at every size; more workgroups do not shorten the chain.  Kept as an A/B
  // switch (=1), off by default.
  s.half = env_flag(getenv("PRONTO_BATCH_HALF")) == 1;
  // =1: pb_replay_legodo_fused on the first, one-lane-per-filter kernel (15 states only; A/B runs)
  s.replay_onelane = env_flag(getenv("PRONTO_BATCH_REPLAY_ONELANE")) == 1;
  // XCD-contiguous tile order: each of the 8 XCDs walks one contiguous range of tiles instead of every 8th tile.  With
  // the tiled layout it measured equal or faster for both state sizes at every batch size (n = 21 at 192k filters:
  // 162 -> 146 us).  =0/1 forces it either way for A/B runs.
  s.xcd = env_flag(getenv("PRONTO_BATCH_XCD"));
  // =1: every stand-alone update on the run-time-index kernel (A/B runs and tests)
  s.generic_update = env_flag(getenv("PRONTO_BATCH_GENERIC_UPDATE")) == 1;
  // =0: the 21-state step, stand-alone updates and replay on the two-wave kernel instead of the four-wave one (A/B)
  if (const char *q21 = getenv("PRONTO_BATCH_QUAD21")) s.quad21 = q21[0] != '0';
  // =0/1/2 forces the cache policy of the state round trip (make_policy)
  if (const char *h = getenv("PRONTO_BATCH_MEMHINT")) {
    s.has_mem_hint = true;
    s.mem_hint = h[0] - '0';
  }
  // =0 / 1 switches pb_run_legodo's cache-blocked order off / on for any size (make_policy)
  s.blocked = env_flag(getenv("PRONTO_BATCH_BLOCKED"));
  // =<n> names its block size
  if (const char *ef = getenv("PRONTO_BATCH_BLOCK_FILTERS")) {
    s.has_block_filters = true;
    s.block_filters = atol(ef);
  }
  // =1: Eigen's diagonal pivoting in the smoother's factorisation of P^- (the reference's .ldlt(); parity with the oracle at
  // 1e-15); default: no pivot search (P^- is SPD; rbis_smooth.hpp)
  s.smooth_pivot = env_flag(getenv("PRONTO_SMOOTH_PIVOT")) == 1;
  // =reg: the 16 / 32-lanes-per-filter smoother kernel of rounds 2-4 (rbis_smooth.hpp); default: one lane per filter, the dense work
  // split over role waves (rbis_smooth_lane.hpp).  15 states: k_smooth_wide (rbis_smooth_wide.hpp, pb_smooth_wide.hip: persistent
  // workgroups, one wave per SIMD with 512 registers, data movement by whole rows) unless =lane asks for k_smooth_lane (two tiles per
  // CU, 256 registers: the default until the second half of round 5, and still the kernel for 21 states)
  if (const char *sk = getenv("PRONTO_SMOOTH_KERNEL")) {
    s.smooth_reg = !strcmp(sk, "reg");
    s.smooth_lane = !strcmp(sk, "lane");
  }
  // =<n>: workgroups of the persistent k_smooth_wide, for experiments (default: one per CU)
  if (const char *sg = getenv("PRONTO_SMOOTH_GRID")) s.smooth_grid = atoi(sg);
  return s;
}

// ---- the step mapping ----
enum Mapping {
  MAP_LANE15,   // k_step<15>: one lane per filter
  MAP_COOP15,   // k_step_coop<15>: two waves per tile at two waves per SIMD (rbis_coop.hpp)
  MAP_COOP21,   // k_step_coop<21>: the two-wave kernel at one wave per SIMD (the QUAD21=0 A/B path)
  MAP_QUAD21,   // k_step_quad: 231 packed covariance entries do not fit one lane's registers; four cooperating waves per tile at two
                // waves per SIMD (rbis_quad.hpp): one launch, one state round trip
};
struct StepChoice {
  Mapping map;
  bool half;    // MAP_COOP15 with two workgroups per tile (the whole-batch launch only)
};
constexpr Mapping step_mapping(int ns, bool coop15, bool quad21)
{
  return ns == 15 ? (coop15 ? MAP_COOP15 : MAP_LANE15) : (quad21 ? MAP_QUAD21 : MAP_COOP21);
}
constexpr int mapping_states(Mapping m) { return m == MAP_LANE15 || m == MAP_COOP15 ? 15 : 21; }

struct Policy {
  StepChoice step = { MAP_COOP15, false };
  int mem_hint = MH_DEFAULT;   // MH_* cache policy of the state round trip
  bool xcd_remap = true;       // -> Consts::xcd_remap, which the kernels read
  bool generic_update = false, replay_onelane = false;
  // pb_run_legodo's cache-blocked order (filter range outer, time inner) for states beyond the memory-side cache: filters per block
  // (whole tiles; 0 = the whole batch per launch), and the kernel / cache policy that block size wants
  int run_block = 0, run_block_hint = MH_DEFAULT;
  Mapping run_block_map = MAP_COOP15;
  bool smooth_pivot = false, smooth_reg = false, smooth_lane = false;
  int smooth_grid = 0;
};

// batch: filters; bytes: the whole state array (state_bytes)
inline Policy make_policy(int ns, long batch, long bytes, const Switches &s)
{
  Policy p;
  const bool coop15 = s.coop15 >= 0 ? s.coop15 == 1 : batch <= 393216;
  p.step.map = step_mapping(ns, coop15, s.quad21);
  p.step.half = p.step.map == MAP_COOP15 && s.half;
  p.replay_onelane = s.replay_onelane;
  p.generic_update = s.generic_update;
  p.xcd_remap = s.xcd >= 0 ? s.xcd == 1 : true;
  // Cache policy of the state round trip, measured on both step kernels: a state that
  // fits the XCDs' L2s (< ~48 MB) wants the default policy (sc1 stores 7 % slower at 32k x 15 states); up to ~1.3x
  // the 256 MB memory-side cache sc1 stores are 1-4 % faster; beyond, non-temporal loads+stores are 7-15 % faster
  // (1M filters: 469 -> 417 us) and 10-40 % SLOWER if used on a cache-sized state.
  p.mem_hint = s.has_mem_hint ? s.mem_hint
                              : (bytes < (48L << 20)    ? MH_DEFAULT
                                 : bytes < (310L << 20) ? MH_STORE_SC1
                                 : bytes < (350L << 20) ? MH_DEFAULT   // (160k 21-state filters, 336 MB: 112.6 us against 124.8 with sc1 stores, 118.7 non-temporal)
                                                        : MH_STREAM_NT);
  if (p.mem_hint < 0 || p.mem_hint > 2) p.mem_hint = MH_DEFAULT;
  // Bulk replays of a state that does not fit the memory-side cache (pb_run_legodo): filter range outer, time inner, over blocks
  // of whole tiles whose state stays cache-resident from step to step -- the filters are independent and the streams are known
  // up front (the reference's own many-runs workload replays one log 8 000 times, state-estimator/python/param_sweep.py:39-52).
  // Same T = 1 accounting: every step still loads and stores every posterior once, the round trip just ends in the cache.
  // Block size: the largest that measured at the cache-resident rate (profiles/r05_batch_sweep.txt), the blocks made equal;
  // each block runs the kernel and the cache policy of ITS size.
  // (15 states: 224k filters = 257 MB of state per block measured best, 0.87 of the roofline at 512k / 1 M filters with 64-step
  // streams against 0.74 step by step; 21 states: 112k = 237 MB, 0.84 against 0.67 -- profiles/r05_batch_sweep.txt)
  long want = s.has_block_filters ? s.block_filters : (ns == 15 ? 229376 : 114688);
  want = (want + 63) / 64 * 64;
  const bool on = s.blocked >= 0 ? s.blocked == 1 : bytes > (256L << 20);
  if (on && want >= 64 && want < batch && (batch & 63) == 0) {
    const long nblocks = (batch + want - 1) / want;
    p.run_block = (int) (((batch + nblocks - 1) / nblocks + 63) / 64 * 64);
    const long blk_bytes = (long) p.run_block * state_slots(ns) * 8;
    p.run_block_hint = s.has_mem_hint ? p.mem_hint : (blk_bytes < (48L << 20) ? MH_DEFAULT : MH_STORE_SC1);
    p.run_block_map = step_mapping(ns, s.coop15 >= 0 ? s.coop15 == 1 : true, s.quad21);
  }
  p.smooth_pivot = s.smooth_pivot;
  p.smooth_reg = s.smooth_reg;
  p.smooth_lane = s.smooth_lane;
  p.smooth_grid = s.smooth_grid;
  return p;
}

// pb_hot_kernel: the step kernel of a mapping as rocprofv3 prints it
inline const char *step_kernel_name(Mapping map, int mem_hint)
{
  static const char *const names[4][3] = { { "k_step<15,true,0>", "k_step<15,true,1>", "k_step<15,true,2>" },
                                           { "k_step_coop<15,true,0>", "k_step_coop<15,true,1>", "k_step_coop<15,true,2>" },
                                           { "k_step_coop<21,true,0>", "k_step_coop<21,true,1>", "k_step_coop<21,true,2>" },
                                           { "k_step_quad<true,0>", "k_step_quad<true,1>", "k_step_quad<true,2>" } };
  return names[map][mem_hint];
}

// Is there a pair kernel (IMU step + leg odometry + its update in one launch, pb_step_leg.hip / pb_legpar.hip)?  On the two-wave
// 15-state mapping (the default up to 393 216 filters) and the four-wave 21-state mapping.  Mode lin_rate (0) or lin_rot_rate (1) with
// leg_estimate's world constraint switched on needs the stand-alone kernel (mode 2, pos_and_lin_rate, tracks it inside the pair kernel).
constexpr bool pair_kernel_exists(Mapping map, bool world_constraint, int mode)
{
  return (map == MAP_COOP15 || map == MAP_QUAD21) && !(world_constraint && mode != 2);
}

// the fused step that also keeps its prediction in one launch (pb_step_pred.hip): every mapping but the one-lane one
constexpr bool pred_kernel_exists(Mapping map) { return map != MAP_LANE15; }

// the time-fused replay kernel (rbis_replay_kernels.hpp)
enum ReplayKernel {
  REPLAY_LANE15,   // k_replay_fused<15>: the first, one-lane-per-filter version; it has no write-through
  REPLAY_COOP15,   // k_replay_coop<15>
  REPLAY_COOP21,   // k_replay_coop<21>
  REPLAY_QUAD21,   // k_replay_quad<1>: four waves per tile, register budget of ONE wave per SIMD: 3.3e9 steps/s at 64k filters, T = 32; cut
                   // for two waves per SIMD it carries 452 B of scratch and measured 2.4e9; the two-wave kernel 1.7e9
};
constexpr ReplayKernel replay_kernel(const Policy &p, bool write_through)
{
  return mapping_states(p.step.map) == 15 ? (p.replay_onelane && !write_through ? REPLAY_LANE15 : REPLAY_COOP15)
                                          : (p.step.map == MAP_QUAD21 ? REPLAY_QUAD21 : REPLAY_COOP21);
}

// the RTS smoother step
enum SmoothKernel { SMOOTH_WIDE15, SMOOTH_LANE, SMOOTH_REG, SMOOTH_REG_PIVOT };
constexpr SmoothKernel smooth_kernel(const Policy &p)
{
  return p.smooth_pivot ? SMOOTH_REG_PIVOT : p.smooth_reg ? SMOOTH_REG : (mapping_states(p.step.map) == 15 && !p.smooth_lane) ? SMOOTH_WIDE15 : SMOOTH_LANE;
}
// workgroups of the persistent k_smooth_wide: one per CU walks the tiles
constexpr int smooth_wide_grid(const Policy &p, int ntiles, int n_cu)
{
  const int nwg = p.smooth_grid > 0 ? p.smooth_grid : n_cu;
  return ntiles < nwg ? ntiles : nwg;
}

// ---- the stand-alone indexed (+ orientation) update ----
enum UpdateFamily {
  UPD_CT_COOP,      // k_step_coop<NS,false,.,CORR>: a handler's list on the two-role mapping (one coalesced round trip, no column gather)
  UPD_CT_QUAD,      // k_update_quad<CORR>: the same on the four-wave mapping
  UPD_LANE_LIST,    // k_update_lane<15,6,IdxVelOmega>: a list that reaches the pass-through states, one lane per filter in registers
  UPD_QUAD_LIST,    // k_update_quad_list<.,3,4,5,0,1,2>: the same list for 21 states
  UPD_LANE_RT,      // k_update_lane_rt<15,M,ORIENT>: run-time index list, the whole 15-state filter in one lane's registers (m <= 4)
  UPD_COOP_RT,      // k_update_coop_rt<M>: m = 5, 6, where the one-lane kernel spills: two waves per tile
  UPD_QUAD_RT,      // k_update_quad_rt<M>: run-time index list, 21 states
  UPD_WIDE,         // k_update_wide<NS,M,ORIENT>: 7 ... 9 rows (pb_update_indexed_wide), one lane per filter, the measured columns in LDS
};
// the index lists the handlers produce; the rows up to CorrGpfZ in the order of the CORR types of rbis_coop.hpp
enum UpdateList { LIST_VEL, LIST_POS, LIST_POS_VEL, LIST_POS_ORIENT, LIST_POS_YAW, LIST_VEL_YAW, LIST_YAW, LIST_GPF_YAW_POS, LIST_GPF_CHI_POS,
                  LIST_GPF_Z, LIST_VEL_OMEGA, N_UPDATE_LISTS, LIST_NONE = -1 };
enum OrientRule { ORIENT_ANY, ORIENT_REQUIRED, ORIENT_FORBIDDEN };
struct UpdateListRow {
  int m, idx[6];
  OrientRule orient;   // of an orientation measurement beside the indexed one
  int ns;              // state-size restriction of the compile-time kernel (0: none)
};
inline constexpr UpdateListRow kUpdateLists[N_UPDATE_LISTS] = {
  { 3, { 3, 4, 5 }, ORIENT_ANY, 0 },
  { 3, { 9, 10, 11 }, ORIENT_ANY, 0 },
  { 6, { 9, 10, 11, 3, 4, 5 }, ORIENT_ANY, 0 },
  { 6, { 9, 10, 11, 6, 7, 8 }, ORIENT_REQUIRED, 0 },
  { 4, { 9, 10, 11, 8 }, ORIENT_REQUIRED, 0 },
  { 4, { 3, 4, 5, 8 }, ORIENT_REQUIRED, 0 },
  { 1, { 8 }, ORIENT_REQUIRED, 0 },
  { 4, { 8, 9, 10, 11 }, ORIENT_FORBIDDEN, 0 },        // GPF pos_yaw
  { 6, { 6, 7, 8, 9, 10, 11 }, ORIENT_FORBIDDEN, 0 },  // GPF pos_chi
  { 1, { 11 }, ORIENT_FORBIDDEN, 0 },                  // GPF z_only
  { 6, { 3, 4, 5, 0, 1, 2 }, ORIENT_FORBIDDEN, 15 },   // LegOdoCommon lin_rot_rate (rbis_legodo_common.cpp:66-67)
};
inline int update_list(int ns, int m, const int *idx, bool orient)
{
  for (int l = 0; l < N_UPDATE_LISTS; l++) {
    const UpdateListRow &r = kUpdateLists[l];
    if (r.m != m || memcmp(r.idx, idx, sizeof(int) * m) != 0) continue;
    if ((r.orient == ORIENT_REQUIRED && !orient) || (r.orient == ORIENT_FORBIDDEN && orient) || (r.ns && r.ns != ns)) continue;
    return l;
  }
  return LIST_NONE;
}
struct UpdateChoice {
  UpdateFamily family;
  int list;         // UpdateList of the first two families (which CORR), LIST_NONE otherwise
  bool host_args;   // z, the R diagonal and the measured quaternion travel as kernel arguments: nothing is staged
};
// map / generic_update: the context's; rkind: enum pb_rkind; all_broadcast: every input is a PB_HOST_BROADCAST value (one measurement
// for every filter, R among them); masked: a per-filter mask came with it.
// Never answers a (family, list) without an instantiated kernel: the two-role 21-state mapping has no six-row variants (they spill),
// and what has no compile-time kernel goes to the run-time-index family of its state size.
inline UpdateChoice update_choice(Mapping map, bool generic_update, int m, const int *idx, bool orient, int rkind, bool all_broadcast, bool masked)
{
  const int ns = mapping_states(map);
  const int list = generic_update ? LIST_NONE : update_list(ns, m, idx, orient);
  UpdateChoice u = { ns == 15 ? (m <= 4 ? UPD_LANE_RT : UPD_COOP_RT) : UPD_QUAD_RT, LIST_NONE, false };
  if (list == LIST_VEL_OMEGA) u.family = UPD_LANE_LIST;
  else if (list != LIST_NONE && ns == 15) u = { UPD_CT_COOP, list, false };
  else if (list != LIST_NONE && map == MAP_QUAD21) u = { UPD_CT_QUAD, list, false };
  else if (list != LIST_NONE && m <= 4) u = { UPD_CT_COOP, list, false };
  // (kept as it was: on 21 states lin_rot_rate's list takes its list kernel on either mapping, with or without an orientation
  // measurement beside it)
  else if (!generic_update && ns == 21 && m == 6 && memcmp(idx, kUpdateLists[LIST_VEL_OMEGA].idx, sizeof(int) * 6) == 0) u.family = UPD_QUAD_LIST;
  // (kept as it was: the argument form is not offered under a mask, although the kernels that take it honour one)
  u.host_args = all_broadcast && rkind == PB_R_DIAG_BROADCAST && !masked && u.family <= UPD_LANE_LIST;
  return u;
}

// pb_update_indexed_wide (up to PB_UPDATE_WIDE_MAX_ROWS rows): up to six rows go wherever update_choice sends them; seven to nine run
// k_update_wide (rbis_update_wide.hpp), whose inputs are always device blocks -- it has no argument form.
inline UpdateChoice wide_update_choice(Mapping map, bool generic_update, int m, const int *idx, bool orient, int rkind, bool all_broadcast, bool masked)
{
  if (m <= 6) return update_choice(map, generic_update, m, idx, orient, rkind, all_broadcast, masked);
  return { UPD_WIDE, LIST_NONE, false };
}

// pb_step_legodo_correct's correction (enum pb_corr) on the handlers' lists
constexpr UpdateList correction_list(int corr_kind) { return corr_kind == PB_CORR_POS_ORIENT ? LIST_POS_ORIENT : LIST_POS_YAW; }
// The stand-alone correction behind the 21-state fused step (pbk_step_correct).
// (kept as it was: it does not look at generic_update -- the switch reaches pb_update_indexed* and the smoothed replays only)
inline UpdateChoice correction_choice(Mapping map, int corr_kind, bool all_broadcast, bool masked)
{
  const UpdateListRow &r = kUpdateLists[correction_list(corr_kind)];
  return update_choice(map, false, r.m, r.idx, true, all_broadcast ? PB_R_DIAG_BROADCAST : PB_R_DIAG, all_broadcast, masked);
}
// May pb_step_legodo_correct pass one robot's correction as kernel arguments?  15 states: the fused kernel takes them; 21 states:
// where the stand-alone correction has the argument form (the two-wave mapping has no six-row kernel that does: its correction
// falls back to the run-time-index update, which needs the replicated blocks staged)
inline bool correction_as_args(Mapping map, int corr_kind)
{
  return mapping_states(map) == 15 || correction_choice(map, corr_kind, true, false).host_args;
}

}  // namespace pb
