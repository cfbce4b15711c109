// rbis_legpar.hpp -- where the odometry kernels (rbis_legstep.hpp, rbis_legodo_kernels.hpp) take the tunables of the leg odometry
// from: the eleven state_estimator.legodo.* scalars a parameter sweep varies.  Two sources with one interface, a template parameter
// of the kernel bodies:
//   LegParArgs  the kernel arguments (LegPar, LegMeasPar, LegStepArgs::r2 / r2_uncertain): one value for every filter;
//   LegParRows  a per-filter block [LPR_ROWS][stride] in the .cfg's units (pb_legodo_set_param_block), one coalesced 8-byte load per
//               lane and row, requested where the value is used and only for the rows the instantiation can use -- the odometry wave
//               of the pair kernels is the register-critical part (rbis_legstep.hpp, EARLY).
// The flags and modes (standing, filter_contact_events, use_controller_input, the measurement mode, the world constraint) stay kernel
// arguments, wave-uniform, with either source.
#pragma once

#include "rbis_tile_io.hpp"
#include "rbis_legodo.hpp"

namespace pb {

// rows of the block: PB_LEGPAR_* of include/pronto_batch.h (held equal in pb_legodo.hip)
enum { LPR_R_VXYZ = 0, LPR_R_VXYZ_UNCERTAIN, LPR_R_VANG, LPR_R_VANG_UNCERTAIN, LPR_R_XYZ, LPR_SCHMITT_LOW, LPR_SCHMITT_HIGH,
       LPR_SCHMITT_LOW_DELAY, LPR_SCHMITT_HIGH_DELAY, LPR_TOTAL_FORCE, LPR_STANDING_SCHMITT_LEVEL, LPR_ROWS };

#if defined(__HIPCC__)
struct LegParArgs {
  __device__ __forceinline__ const LegPar &contact_par(const LegPar &par, unsigned) const { return par; }
  __device__ __forceinline__ const LegMeasPar &meas_par(const LegMeasPar &mp, unsigned) const { return mp; }
  template <int SIX>
  __device__ __forceinline__ const LegStepArgs &noises(const LegStepArgs &la, unsigned) const { return la; }
};

struct LegParRows {
  const double *blk;  // [LPR_ROWS][stride]: lanes past the batch read in bounds
  long stride;

  // bo: the lane's byte offset in a row (filter index * 8)
  __device__ __forceinline__ double row(int r, unsigned bo) const
  {
    const unsigned S8 = (unsigned) stride * 8u;
    return ldg(mkbuf(blk, (unsigned) LPR_ROWS * S8), (unsigned) r * S8, bo);
  }
  // a standard deviation of the .cfg, squared where it is used like the scalars' bot_sq (rbis_legodo_common.cpp:38-44)
  __device__ __forceinline__ double sq(int r, unsigned bo) const
  {
    const double v = row(r, bo);
    return v * v;
  }
  // what leg_contacts reads: the Schmitt rows (FootContactAlt) or the two of the "standing" mode (wave-uniform), through `float` like
  // pb_legodo_init / pb_legodo_set_contact_mode
  __device__ __forceinline__ LegPar contact_par(const LegPar &par, unsigned bo) const
  {
    LegPar p = par;
    if (par.standing) {
      p.total_force = (float) row(LPR_TOTAL_FORCE, bo);
      p.standing_schmitt_level = (float) row(LPR_STANDING_SCHMITT_LEVEL, bo);
    } else {
      p.alt.low = (double) (float) row(LPR_SCHMITT_LOW, bo);
      p.alt.high = (double) (float) row(LPR_SCHMITT_HIGH, bo);
      p.alt.low_delay = (int64_t) row(LPR_SCHMITT_LOW_DELAY, bo);
      p.alt.high_delay = (int64_t) row(LPR_SCHMITT_HIGH_DELAY, bo);
    }
    return p;
  }
  // the variances measurement mode MODE reads (leg_measurement, leg_measurement6)
  template <int MODE>
  __device__ __forceinline__ void fill(LegMeasPar &mp, unsigned bo) const
  {
    mp.r_v2 = sq(LPR_R_VXYZ, bo);
    mp.r_v2_uncertain = sq(LPR_R_VXYZ_UNCERTAIN, bo);
    if constexpr (MODE == 1) {
      mp.r_a2 = sq(LPR_R_VANG, bo);
      mp.r_a2_uncertain = sq(LPR_R_VANG_UNCERTAIN, bo);
    }
    if constexpr (MODE == 2) mp.r_xyz2 = sq(LPR_R_XYZ, bo);
  }
  __device__ __forceinline__ LegMeasPar meas_par(const LegMeasPar &mp, unsigned bo) const
  {
    LegMeasPar o = mp;
    if (mp.mode == 1) fill<1>(o, bo);   // (wave-uniform)
    else if (mp.mode == 2) fill<2>(o, bo);
    else fill<0>(o, bo);
    return o;
  }
  template <int SIX>
  __device__ __forceinline__ LegStepArgs noises(const LegStepArgs &la, unsigned bo) const
  {
    LegStepArgs o = la;
    fill<SIX>(o.mp, bo);
    o.r2 = o.mp.r_v2;
    o.r2_uncertain = o.mp.r_v2_uncertain;
    return o;
  }
};
#endif

}  // namespace pb
