// pb_update_wide.hip -- pb_update_indexed_wide and the launcher of k_update_wide<NS, M, ORIENT, MH> (rbis_update_wide.hpp): indexed
// (+ orientation) updates of seven to nine rows, one lane per filter, the measured columns in LDS.  Up to six rows go down
// pbk_update_common, the path of pb_update_indexed / pb_update_indexed_orient.  Built for two cache policies, like pb_update.hip's
// k_update_coop_rt: non-temporal streaming falls back to the default one.  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_update_wide.hpp"

template <int NS, int M, bool ORIENT>
static void launch_wide(pb_ctx *c, double *out, const int *idx, const UpdateIn &in)
{
  const WideTab<NS, M> tab = make_wide_tab<NS, M>(idx);
  DiagArg<M> da;
  for (int i = 0; i < M; i++) da.v[i] = in.r_bcast ? in.r_bcast[i] : 0.0;
  if (two_policy_hint(c->policy.mem_hint) == MH_STORE_SC1)
    k_update_wide<NS, M, ORIENT, MH_STORE_SC1><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, tab, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
  else
    k_update_wide<NS, M, ORIENT, MH_DEFAULT><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, tab, in.z, in.R(), in.rkind(), da, in.qm, in.mask, c->k);
}

template <int NS>
static int launch_wide_ns(pb_ctx *c, double *out, int m, const int *idx, const UpdateIn &in)
{
#define WIDE_CASE(M)                                          \
  case M:                                                     \
    if (in.qm) launch_wide<NS, M, true>(c, out, idx, in);     \
    else launch_wide<NS, M, false>(c, out, idx, in);          \
    break;
  switch (m) {
    WIDE_CASE(7) WIDE_CASE(8) WIDE_CASE(9)
    default: return fail(c, PB_ERR_STATE, "update: the wide kernel takes m = %d..%d (got %d)", WIDE_MIN_ROWS, WIDE_MAX_ROWS, m);
  }
#undef WIDE_CASE
  return PB_OK;
}

// family UPD_WIDE of pbk_update (pb_update_ct.hip); honours pb_set_output_slot like every update
int pbk_update_wide(pb_ctx *c, int m, const int *idx, const UpdateIn &in)
{
  double *out = update_target(c);
  if (int rc = c->ns == 15 ? launch_wide_ns<15>(c, out, m, idx, in) : launch_wide_ns<21>(c, out, m, idx, in)) return rc;
  LAUNCHCHK(c);
  update_done(c, out);
  return PB_OK;
}

static_assert(PB_UPDATE_WIDE_MAX_ROWS == WIDE_MAX_ROWS && PB_UPDATE_WIDE_MAX_ROWS * PB_UPDATE_WIDE_MAX_ROWS <= RowVals::MAX,
              "a broadcast full R of the widest update must fit one stage_in block");

extern "C" int pb_update_indexed_wide(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int r_kind,
                                      const double *quat_meas, const uint8_t *mask, int mem)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  const bool orient = quat_meas != nullptr;
  if (m < 1 || m > PB_UPDATE_WIDE_MAX_ROWS) return fail(c, PB_ERR_ARG, "update: m must be 1..%d (got %d)", PB_UPDATE_WIDE_MAX_ROWS, m);
  if (m < WIDE_MIN_ROWS) return pbk_update_common(c, m, idx, z, R, r_kind, quat_meas, orient, mask, mem);
  if (!idx || !z || !R) return fail(c, PB_ERR_ARG, "update: NULL input");
  if (int rc = pbk_check_indices(c, m, idx)) return rc;
  const size_t B = (size_t) c->B;
  // (every input block goes through one 32-bit-ranged buffer descriptor)
  if ((unsigned long long) B * (unsigned) (m * m) * 8ull >= (1ull << 32))
    return fail(c, PB_ERR_ARG, "update: batch %d too large for a %d x %d measurement covariance per filter", c->B, m, m);
  size_t rbytes;
  if (mem == PB_HOST_BROADCAST && r_kind == PB_R_DIAG) r_kind = PB_R_DIAG_BROADCAST;  // the same thing, without a fill
  if (r_kind == PB_R_DIAG_BROADCAST) rbytes = 0;
  else if (r_kind == PB_R_DIAG) rbytes = sizeof(double) * m * B;
  else if (r_kind == PB_R_FULL) rbytes = sizeof(double) * m * m * B;
  else return fail(c, PB_ERR_ARG, "update: bad r_kind %d", r_kind);
  const UpdateChoice u = wide_update_choice(c->policy.step.map, c->policy.generic_update, m, idx, orient, r_kind, mem == PB_HOST_BROADCAST, mask != nullptr);
  UpdateIn in;
  if (r_kind == PB_R_DIAG_BROADCAST) in.r_bcast = R;
  Part p[4] = { { z, sizeof(double) * m * B, 0 }, { in.r_bcast ? nullptr : R, rbytes, 0 },
                { orient ? quat_meas : nullptr, sizeof(double) * 4 * B, 0 }, { mask, B, 0 } };
  if (int rc = stage_in(c, mem, p, 4)) return rc;
  in.z = (const double *) p[0].dev;
  (r_kind == PB_R_FULL ? in.r_full : in.r_diag) = (const double *) p[1].dev;
  in.qm = (const double *) p[2].dev;
  in.mask = (const uint8_t *) p[3].dev;
  return pbk_update(c, u, m, idx, in);
}
