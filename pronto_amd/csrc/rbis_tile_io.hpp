// rbis_tile_io.hpp -- how the gfx950 kernels of the batched RBIS EKF reach a tile of the state, and the argument structs they take.
// No kernels here: every kernel header (rbis_step_kernels.hpp, rbis_update_kernels.hpp, rbis_replay_kernels.hpp, rbis_util_kernels.hpp,
// rbis_quad_rt.hpp, rbis_legstep.hpp, rbis_smooth_wide.hpp, rbis_frontend.hpp), pb_yawlock.hip and pb_ctx.hpp include it.
//
// Data layout in HBM (Slots<NS> in rbis_device.hpp): the state array is cut into tiles of 64 filters; a tile is NROW rows
// of 64 x 16 bytes, row r holding the component pair (slot 2r, slot 2r+1) of each of its filters.  One lane owns one
// filter and moves 16 bytes per access, so every global access of a wave is one fully coalesced 1 KiB row and the whole
// round trip of a wave stays inside one contiguous tile (70 KiB for n=15, 129 KiB for n=21).
//
// Addressing: ONE 128-bit buffer descriptor per tile (64-bit tile base in SGPRs, so a context is not limited to 4 GiB),
// the row offset as an immediate / SGPR and ONE per-lane byte offset (lane * 16) shared by every access:
// `buffer_load/store_dwordx4 v, v_off, s[rsrc], s_off offen`.  No per-access 64-bit VGPR address is materialised.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pb_policy.hpp"
#include "rbis_device.hpp"

// workgroup size of the one-lane hot kernel = one tile
#define PB_STEP_BLOCK 64

namespace pb {

typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// 128-bit buffer descriptor over [p, p+bytes): out-of-range lanes read 0 / drop their stores (hardware check)
__device__ __forceinline__ rsrc_t mkbuf(const void *p, unsigned bytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, bytes, 0x00020000);
}
// buffer_load_dwordx2 v, v_off, s[rsrc], s_off offen : voff = per-lane byte offset, soff = uniform offset
// AUX = cache-policy bits of the instruction (gfx940+: 1 = sc0, 2 = nt, 16 = sc1)
template <int AUX = 0>
__device__ __forceinline__ double ldg(rsrc_t r, unsigned soff, unsigned voff)
{
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ void stg(rsrc_t r, unsigned soff, unsigned voff, double v)
{
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, voff, soff, AUX);
}
// 16 bytes per lane
template <int AUX = 0>
__device__ __forceinline__ d2_t ldg2(rsrc_t r, unsigned soff, unsigned voff)
{
  return __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX));
}
// HAZARD (found on MI355X, ROCm 7.2): a buffer store of more than 64 bits reads its data VGPRs over several cycles; a VALU
// instruction that overwrites one of them in the very next slot can reach the register file first, and the LAST four lanes
// of every 16 then store the new value (observed: `buffer_store_dwordx4 v[130:133] ... s48 offen` directly followed by
// `v_mul_f64 v[130:131], ...` corrupted lanes 12-15, 28-31, 44-47, 60-63 of that row, once per ~1000 launches).  LLVM's
// hazard recognizer inserts the wait state only when soffset is NOT an SGPR (GCNHazardRecognizer::createsVALUHazard);
// here soffset is always an SGPR, so the wait states are placed by hand: the volatile asm keeps its place behind the store
// (side-effect order) and takes the data registers as INPUTS, so they stay untouched until the nop has issued.
template <int AUX = 0>
__device__ __forceinline__ void stg2(rsrc_t r, unsigned soff, unsigned voff, d2_t v)
{
  const v4u d = __builtin_bit_cast(v4u, v);
  __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, soff, AUX);
  asm volatile("s_nop 1" ::"v"(d));
}

// Memory hint of the state round trip in the step kernels (template parameter MH): the MH_* constants and the host's pick from the
// state size are pb_policy.hpp's; here, the cache-policy bits of the loads (LA) and stores (SA) each stands for.
template <int MH> struct MemHint {
  static constexpr int LA = (MH == MH_STREAM_NT) ? 2 : 0;
  static constexpr int SA = (MH == MH_STORE_SC1) ? 16 : (MH == MH_STREAM_NT) ? 2 : 0;
};

// Workgroups are dealt round-robin to the 8 XCDs.  With k.xcd_remap each XCD walks one contiguous range of tiles
// (bijective for any grid size) instead of every 8th tile (host picks).
__device__ __forceinline__ unsigned xcd_workgroup(const Consts &k)
{
  unsigned wg = blockIdx.x;
  if (k.xcd_remap) {
    const unsigned nq = gridDim.x >> 3, nr = gridDim.x & 7u, xcd = blockIdx.x & 7u, rank = blockIdx.x >> 3;
    wg = (xcd < nr ? xcd * (nq + 1u) : nr * (nq + 1u) + (xcd - nr) * nq) + rank;
  }
  return wg;
}

// One lane's window on its tile: component-addressed reads and writes on top of 16-byte row accesses.
//   ld(comp)      value of a canonical component (Lay<NS> numbering); the row is loaded on first use and cached
//   need<R0,R1>() issue the loads of rows [R0, R1) now (before any store that could alias them)
//   st(comp, v)   posterior value of a component; a row is stored the moment both its halves are known
// Every index is a compile-time constant once the callers' loops are unrolled, so `loaded[]` / `have[]` fold away and
// the caches are plain registers (cdna_hip_programming.md rule 20); the kernels' resource usage shows 0 bytes of scratch.
template <int NS, int LA, int SA, bool TWO_ROLE = false>
struct TileIO {
  using S = Slots<NS>;
  rsrc_t rs, ro;
  unsigned vo;  // lane * 16
  d2_t cache[S::NROW];
  bool loaded[S::NROW];
  double outv[S::NSLOT];
  bool have[S::NSLOT];
  __device__ __forceinline__ TileIO(const double *st, double *sto, unsigned tile, unsigned lane)
  {
    rs = mkbuf(reinterpret_cast<const char *>(st) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
    ro = mkbuf(reinterpret_cast<char *>(sto) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
    vo = lane * 16u;
#pragma unroll
    for (int r = 0; r < S::NROW; r++) loaded[r] = false;
#pragma unroll
    for (int s = 0; s < S::NSLOT; s++) {
      have[s] = S::T.comp_of[s] < 0;  // a padding slot is always "known" (0)
      outv[s] = 0.0;
    }
  }
  __device__ __forceinline__ void fetch(int r)
  {
    if (!loaded[r]) {
      cache[r] = ldg2<LA>(rs, (unsigned) r * 1024u, vo);
      loaded[r] = true;
    }
  }
  template <int R0, int R1>
  __device__ __forceinline__ void need()
  {
#pragma unroll
    for (int r = R0; r < R1; r++) fetch(r);
  }
  __device__ __forceinline__ double ld(int comp)
  {
    const int s = S::T.slot_of[comp];
    fetch(s >> 1);
    return (s & 1) ? cache[s >> 1].y : cache[s >> 1].x;
  }
  __device__ __forceinline__ void st(int comp, double v)
  {
    const int s = S::T.slot_of[comp];
    if (TWO_ROLE && S::T.split2[s >> 1]) {  // the other half of this row is the other role's: store 8 bytes
      stg<SA>(ro, (unsigned) (s >> 1) * 1024u + (unsigned) (s & 1) * 8u, vo, v);
      return;
    }
    outv[s] = v;
    have[s] = true;
    if (have[s ^ 1]) {
      const d2_t o = { outv[s & ~1], outv[s | 1] };
      stg2<SA>(ro, (unsigned) (s >> 1) * 1024u, vo, o);
    }
  }
  // one component at a RUN-TIME slot (wave-uniform): an 8-byte access into the row
  __device__ __forceinline__ double ld_slot_rt(int slot) const
  {
    return ldg(rs, (unsigned) (slot >> 1) * 1024u + (unsigned) (slot & 1) * 8u, vo);
  }
};

// slot of a component known only at run time (wave-uniform: a scalar table read)
template <int NS>
__device__ __forceinline__ int slot_rt(int comp)
{
  return Slots<NS>::T.slot_of[comp];
}
__device__ __forceinline__ int pk_rt(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ---- argument structs and compile-time index lists of the kernels ----
struct IdxVel {
  static constexpr Idx<3> value = { { 3, 4, 5 } };
};

template <int M>
struct IdxArg {
  int v[M];
};
template <int M>
struct DiagArg {
  double v[M];
};

// inputs of the fused second update (CORR != NoCorr): z2 [M][B], R2 diagonal ([M][B], or broadcast values in rb2 when
// r2 == nullptr), quaternion measurement [4][B] (ORIENT), mask2 [B] (0 = the handler returned NULL for this filter)
struct CorrArgs {
  const double *z2 = nullptr, *r2 = nullptr, *qm2 = nullptr;
  const uint8_t *mask2 = nullptr;
  double rb2[6] = { 0, 0, 0, 0, 0, 0 };
  // zbc: ONE measurement for every filter (PB_HOST_BROADCAST): z and the quaternion travel as kernel arguments too
  double zb2[6] = { 0, 0, 0, 0, 0, 0 }, qb2[4] = { 1, 0, 0, 0 };
  int zbc = 0;
  // rfull: a FULL per-filter R, [m*m][B] column-major (pronto::indexed_measurement_t's R_effective); r2 / rb2 are unused then
  const double *rfull = nullptr;
};
// LegOdoCommon's lin_rot_rate list (rbis_legodo_common.cpp:66-67): velocity AND angular velocity -- the angular-velocity
// rows are pass-through states of the other role, so the two-role kernels do not take it (k_update_lane, rbis_update_kernels.hpp, does).
struct IdxVelOmega {
  static constexpr Idx<6> value = { { 3, 4, 5, 0, 1, 2 } };
};

// Write-through of the replay kernels (rbis_replay_kernels.hpp; pb_replay_legodo_checkpointed): every step's posterior is ALSO stored into its checkpoint slot -- the forward
// pass of the delayed-measurement history and of the smoother keeps every posterior (mav_state_est.cpp:50-70,98-189) -- while the
// state stays in the roles' registers: per step one slot is written and nothing is read, where the per-step path reads the
// previous slot and writes the next (268 MB per step through a 256 MB cache for 64k 21-state filters).
struct SlotOut {
  double *base = nullptr;       // first checkpoint slot to write (NULL: no write-through)
  size_t stride = 0;            // doubles per slot
};

// PB_HOST_BROADCAST inputs: dst [rows][B] <- one value per row (k_fill_rows, rbis_util_kernels.hpp; pronto_batch.hip stage_in)
struct RowVals {
  static constexpr int MAX = 81;  // the largest block of one call: a full 9 x 9 measurement covariance (pb_update_indexed_wide)
  double v[MAX];
};

// IMU front end (InsHandler::doFilter, sensor_handlers.cpp:154-162 + iir_notch.cpp:34-61): cascade of three 2nd-order
// IIR notches per accelerometer axis, one filter per lane, n_packets consecutive packets per call (a KVH batch message
// carries ~3 new 1 kHz packets; all are filtered, the newest filtered one feeds the predict).  State per filter:
// [axis][stage]{x0,x1,y0,y1} = 36 doubles in nst[36][stride].  Bytes: 24 B in per packet + 576 B state per call + 24 B out.
struct NotchCoef {
  double b[3][3], a[3][3];  // [stage][tap]
};
// (the cascade kernel itself is k_notch_counts, rbis_frontend.hpp: one lane per (filter, axis), an optional per-filter packet count)

}  // namespace pb
