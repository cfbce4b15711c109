// pb_smooth.hip -- launcher of the RTS smoother kernel smooth_kernel (pb_policy.hpp) names (rbis_smooth.hpp, rbis_smooth_lane.hpp); see pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_smooth.hpp"
#include "rbis_smooth_lane.hpp"

int pbk_smooth_step(pb_ctx *c, const double *np_, const double *ns_, const double *cu, double *out, double dt)
{
  const SmoothKernel kernel = smooth_kernel(c->policy);
  if (!c->smooth_attr) {  // more than the default 64 KB of dynamic LDS per workgroup
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_lane<15>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) SmoothLaneCfg<15>::LDS_BYTES));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_lane<21>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) SmoothLaneCfg<21>::LDS_BYTES));
    const int l15 = (int) (sizeof(double) * SmoothRegCfg<15>::LDS_DOUBLES), l21 = (int) (sizeof(double) * SmoothRegCfg<21>::LDS_DOUBLES);
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_reg<15, true>), hipFuncAttributeMaxDynamicSharedMemorySize, l15));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_reg<21, true>), hipFuncAttributeMaxDynamicSharedMemorySize, l21));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_reg<15, false>), hipFuncAttributeMaxDynamicSharedMemorySize, l15));
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_smooth_reg<21, false>), hipFuncAttributeMaxDynamicSharedMemorySize, l21));
    c->smooth_attr = true;
  }
  if (kernel == SMOOTH_WIDE15) return pbk_smooth_wide(c, np_, ns_, cu, out, dt);
  const bool pivot = kernel == SMOOTH_REG_PIVOT;   // (below: SMOOTH_LANE, or k_smooth_reg with / without the pivot search)
  if (kernel == SMOOTH_LANE) {
    const dim3 grid((unsigned) ((c->B + 63) / 64));
    if (c->ns == 15) k_smooth_lane<15><<<grid, SmoothLaneCfg<15>::THREADS, SmoothLaneCfg<15>::LDS_BYTES, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
    else k_smooth_lane<21><<<grid, SmoothLaneCfg<21>::THREADS, SmoothLaneCfg<21>::LDS_BYTES, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
  } else if (c->ns == 15) {
    using S = SmoothRegCfg<15>;
    const dim3 grid((unsigned) ((c->B + S::F - 1) / S::F));
    const size_t ldsb = sizeof(double) * S::LDS_DOUBLES;
    if (pivot) k_smooth_reg<15, true><<<grid, S::THREADS, ldsb, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
    else k_smooth_reg<15, false><<<grid, S::THREADS, ldsb, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
  } else {
    using S = SmoothRegCfg<21>;
    const dim3 grid((unsigned) ((c->B + S::F - 1) / S::F));
    const size_t ldsb = sizeof(double) * S::LDS_DOUBLES;
    if (pivot) k_smooth_reg<21, true><<<grid, S::THREADS, ldsb, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
    else k_smooth_reg<21, false><<<grid, S::THREADS, ldsb, c->stream>>>(np_, ns_, cu, out, c->B, dt, c->k);
  }
  LAUNCHCHK(c);
#ifdef SML_TIMELINE  // attribution build: print the stamps of launch 60 (n = 15) and 310 (n = 21) of scripts/smooth_rate.py
  {
    static int calls = 0;
    if (++calls == 60 || calls == 310) {
      unsigned long long h[8][16];
      (void) hipStreamSynchronize(c->stream);
      (void) hipMemcpyFromSymbol(h, HIP_SYMBOL(sml_tl), sizeof(h));
      const int nr = c->ns == 15 ? SmoothLaneCfg<15>::NR : SmoothLaneCfg<21>::NR;
      for (int w = 0; w < nr; w++) {
        const double t0 = (double) h[0][0];
        fprintf(stderr, "timeline n=%d tile %d role %d [k cycles from role 0's start] first factor barrier %.1f, last %.1f, rhs done %.1f, subst done %.1f, "
                        "D staged %.1f, first chunk barrier %.1f, end %.1f; in the chunks: publish phases %.1f, final+M phases %.1f\n", c->ns, SML_TIMELINE, w,
                (h[w][1] - t0) / 1e3, (h[w][2] - t0) / 1e3, (h[w][3] - t0) / 1e3, (h[w][4] - t0) / 1e3, (h[w][5] - t0) / 1e3, (h[w][6] - t0) / 1e3,
                (h[w][7] - t0) / 1e3, h[w][8] / 1e3, h[w][9] / 1e3);

      }
    }
  }
#endif
  return PB_OK;
}
