// pb_step.hip -- launchers of the step kernels (k_step, k_step_coop, k_step_quad) and of the replay kernels; see pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_step_kernels.hpp"
#include "rbis_replay_kernels.hpp"

// The ONE launch of the step kernel of a mapping (pb_policy.hpp): from `st` into `out`, a grid that covers nb filters (the inputs stay
// blocks [rows][B] of the whole batch: the kernels take B as the row stride).  step.half: two workgroups per tile -- the whole-batch
// 15-state cooperative launch only.
template <bool UPDATE, int MH>
static void launch_step_kernel(pb_ctx *c, const double *st, double *out, int nb, StepChoice step, const double *imu, const double *lo,
                               const uint8_t *mask, const double q[4], const StepBcast &bc, const Consts &k)
{
  const int B = c->B;
  switch (step.map) {
  case MAP_COOP15: {
    Consts kk = k;
    kk.half_tiles = step.half ? 1 : 0;   // (this launch only: every other kernel that takes c->k keeps whole tiles)
    k_step_coop<15, UPDATE, MH><<<nblk(nb) * (step.half ? 2 : 1), 128, 0, c->stream>>>(st, out, B, imu, lo, mask, q[0], q[1], q[2], q[3], kk, CorrArgs(), bc);
    break;
  }
  case MAP_LANE15:
    k_step<15, UPDATE, MH><<<(nb + PB_STEP_BLOCK - 1) / PB_STEP_BLOCK, PB_STEP_BLOCK, 0, c->stream>>>(st, out, B, imu, lo, mask, q[0], q[1], q[2], q[3], k, bc);
    break;
  case MAP_QUAD21:
    k_step_quad<UPDATE, MH><<<nblk(nb), 256, 0, c->stream>>>(st, out, B, imu, lo, mask, q[0], q[1], q[2], q[3], k, bc);
    break;
  case MAP_COOP21:
    k_step_coop<21, UPDATE, MH><<<nblk(nb), 128, 0, c->stream>>>(st, out, B, imu, lo, mask, q[0], q[1], q[2], q[3], k, CorrArgs(), bc);
    break;
  }
}

template <bool UPDATE>
static int launch_step(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], const StepBcast &bcast)
{
  double *out = update_target(c);
  int rc = PB_OK;
  StepBcast bc = bcast;
  imu = pbk_idle_prepare(c, imu, bc, &rc);
  if (rc) return rc;
  with_mem_hint(c->policy.mem_hint, [&](auto mh) {
    launch_step_kernel<UPDATE, decltype(mh)::value>(c, c->st, out, c->B, c->policy.step, imu, lo, mask, q, bc, c->k);
  });
  LAUNCHCHK(c);
  if ((rc = pbk_idle_restore(c, out, nullptr, q))) return rc;
  update_done(c, out);
  return PB_OK;
}

// The fused step on the filters [b0, b0 + nb) only -- b0 and the batch multiples of 64 (whole tiles), the posterior in place, the inputs
// still blocks [rows][B] of the WHOLE batch (the block is addressed by shifting every pointer, the per-filter process noise included:
// the kernels count filters from 0, so an unshifted block would give every range the noise of filters 0..nb-1).
// map / mem_hint are the caller's: a block that fits the memory-side cache wants the kernel and the cache policy of ITS size.
int pbk_step_range(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], long b0, int nb, Mapping map, int mem_hint)
{
  if (c->st != c->st_base || c->out_slot >= 0 || (c->B & 63) || (b0 & 63) || (nb & 63) || b0 + nb > c->B)
    return fail(c, PB_ERR_STATE, "pbk_step_range: whole tiles of a head that lives in the context's own array");
  const size_t tile_doubles = c->state_doubles / (size_t) (c->stride / 64);
  double *st = c->st + (size_t) (b0 / 64) * tile_doubles;
  const uint8_t *mask_b = mask ? mask + b0 : nullptr;
  Consts kk = c->k;   // (this launch only)
  if (kk.qblk) kk.qblk += b0;
  with_mem_hint(mem_hint, [&](auto mh) {
    launch_step_kernel<true, decltype(mh)::value>(c, st, st, nb, StepChoice{ map, false }, imu + b0, lo + b0, mask_b, q, StepBcast(), kk);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

// The fused step with a predicted slot pending (pb_set_pred_slot, consumed here): one launch that writes both posteriors where a kernel
// for it exists (k_step_coop_pred), otherwise the predict alone into the slot -- the head stays where it is -- and the fused step
// behind it.  Either way the filtered posterior is the fused step's, bit for bit, and the slot holds what pb_predict would leave.
static int step_pred(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], const StepBcast &bcast)
{
  double *pred = slot_ptr(c, c->pred_slot);
  const int ps = c->pred_slot;
  c->pred_slot = -1;
  int rc = PB_OK;
  StepBcast bc = bcast;
  imu = pbk_idle_prepare(c, imu, bc, &rc);   // (once: both launches of the fall-back read the same prepared block)
  if (rc) return rc;
  double *out = update_target(c);
  if (pbk_step_pred_kernel(c, out, pred, imu, lo, mask, q, bc) == PB_OK) {
    LAUNCHCHK(c);
    if ((rc = pbk_idle_restore(c, out, pred, q))) return rc;
    update_done(c, out);
    return PB_OK;
  }
  double *head = c->st;
  const int os = c->out_slot;
  c->out_slot = ps;
  rc = launch_step<false>(c, imu, nullptr, nullptr, q, bc);
  c->st = head;
  c->out_slot = os;
  if (rc) return rc;
  return launch_step<true>(c, imu, lo, mask, q, bc);
}

int pbk_step(pb_ctx *c, bool update, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
             const StepBcast *bcast)
{
  const StepBcast bc = bcast ? *bcast : StepBcast();
  if (update && c->pred_slot >= 0) return step_pred(c, imu, lo, mask, q, bc);
  return update ? launch_step<true>(c, imu, lo, mask, q, bc) : launch_step<false>(c, imu, nullptr, nullptr, q, bc);
}

int pbk_step_leg(pb_ctx *c, const double *imu, const StepBcast *bcast, const double q[4], const LegIn &lin, int64_t utime, const LegMeasPar &mp,
                 double *lo_out, uint8_t *mask_out)
{
  if (!pair_kernel_exists(c->policy.step.map, c->leg_par.world_constraint != 0, mp.mode)) return -1;
  StepBcast bc = bcast ? *bcast : StepBcast();
  LegStepArgs la{ c->legd, c->legi, c->stride, utime, mp.r_v2, mp.r_v2_uncertain, lo_out, mask_out, mp };
  double *out = update_target(c);
  int rc = PB_OK;
  imu = pbk_idle_prepare(c, imu, bc, &rc);
  if (rc) return rc;
  if (c->leg_blk_on) {  // per-filter noises and contact thresholds (pb_legodo_set_param_block): the sibling kernels
    if (c->ns == 15) pbk_legpar15(c, out, imu, q, bc, lin, la);
    else pbk_legpar21(c, out, imu, q, bc, lin, la);
  } else if (c->ns == 15) pbk_step_leg15(c, out, imu, q, bc, lin, la);
  else pbk_step_leg21(c, out, imu, q, bc, lin, la);
  LAUNCHCHK(c);
  if ((rc = pbk_idle_restore(c, out, nullptr, q))) return rc;
  update_done(c, out);
  return PB_OK;
}

int pbk_replay_fused(pb_ctx *c, int T, const double *imu, const double *lo, const uint8_t *mask, const double q[4], int slot0)
{
  SlotOut so;
  if (slot0 >= 0) {
    so.base = slot_ptr(c, slot0);
    so.stride = c->state_doubles;
  }
  switch (replay_kernel(c->policy, slot0 >= 0)) {
  case REPLAY_LANE15: k_replay_fused<15><<<nblk(c->B), 64, 0, c->stream>>>(c->st, c->B, T, imu, lo, mask, q[0], q[1], q[2], q[3], c->k); break;
  case REPLAY_COOP15: k_replay_coop<15><<<nblk(c->B), 128, 0, c->stream>>>(c->st, c->B, T, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, so); break;
  case REPLAY_QUAD21: k_replay_quad<1><<<nblk(c->B), 256, 0, c->stream>>>(c->st, c->B, T, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, so); break;
  case REPLAY_COOP21: k_replay_coop<21><<<nblk(c->B), 128, 0, c->stream>>>(c->st, c->B, T, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, so); break;
  default: return fail(c, PB_ERR_STATE, "pbk_replay_fused: no kernel");
  }
  LAUNCHCHK(c);
  return PB_OK;
}

// predict + leg-odometry update + one more (orientation) update in ONE state round trip on the cooperative kernel
template <int NS, int MH, class CORR>
static void launch_corr(pb_ctx *c, double *out, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                        const CorrArgs &ca, const StepBcast &bc)
{
  k_step_coop<NS, true, MH, CORR><<<nblk(c->B), 128, 0, c->stream>>>(c->st, out, c->B, imu, lo, mask, q[0], q[1], q[2], q[3], c->k, ca, bc);
}
int pbk_step_correct(pb_ctx *c, int corr_kind, const double *imu, const double *lo, const uint8_t *mask, const double q[4],
                     const double *z2, const double *r2, const double *rb2, const double *qm2, const uint8_t *mask2,
                     const StepBcast *bcast, const double *zb, const double *qb)
{
  if (c->ns == 21) {
    // 21 states: role C's 15 x 15 sub-matrix already fills the register file (256 VGPR + 242 AGPR for the plain step); a
    // second update stage in the same kernel spills 550-690 bytes per lane and measured SLOWER than two launches.  Same
    // arithmetic as two launches: the fused step, then the correction alone on the cooperative update kernel.  A pending predicted
    // slot is the first launch's (k_step_quad_pred / k_step_coop_pred<21>); the correction lands in the output slot.
    int rc = pbk_step(c, true, imu, lo, mask, q, bcast);
    if (rc) return rc;
    const UpdateListRow &l = kUpdateLists[correction_list(corr_kind)];
    const int slot = pb_head_slot(c);  // a checkpointed step: the correction lands in the same slot
    if (slot >= 0) c->out_slot = slot;
    const UpdateChoice u = correction_choice(c->policy.step.map, corr_kind, zb != nullptr, mask2 != nullptr);
    if (zb && !u.host_args) return fail(c, PB_ERR_ARG, "pb_step_legodo_correct: no kernel takes this correction as arguments; stage the blocks");
    UpdateIn in;
    in.z = z2; in.r_diag = r2; in.r_bcast = rb2; in.qm = qm2; in.mask = mask2; in.z_host = zb; in.q_host = qb;
    return pbk_update(c, u, l.m, l.idx, in);
  }
  CorrArgs ca;
  ca.z2 = z2; ca.r2 = r2; ca.qm2 = qm2; ca.mask2 = mask2;
  const int m2 = (corr_kind == PB_CORR_POS_ORIENT) ? 6 : 4;
  if (rb2)
    for (int i = 0; i < m2; i++) ca.rb2[i] = rb2[i];
  if (zb) {  // one correction for every filter: kernel arguments
    ca.zbc = 1;
    for (int i = 0; i < m2; i++) ca.zb2[i] = zb[i];
    for (int i = 0; i < 4; i++) ca.qb2[i] = qb[i];
  }
  StepBcast bc = bcast ? *bcast : StepBcast();
  // a predicted slot pending (pb_set_pred_slot, consumed here): the kernel that also stores the INS posterior (pb_step_corr_pred.hip)
  double *pred = c->pred_slot >= 0 ? slot_ptr(c, c->pred_slot) : nullptr;
  c->pred_slot = -1;
  double *out = update_target(c);
  int rc = PB_OK;
  imu = pbk_idle_prepare(c, imu, bc, &rc);
  if (rc) return rc;
  if (pred) {
    if (pbk_step_corr_pred_kernel(c, corr_kind, out, pred, imu, lo, mask, q, ca, bc)) return fail(c, PB_ERR_STATE, "pb_step_legodo_correct: no kernel keeps the prediction here");
  } else {
    with_mem_hint(c->policy.mem_hint, [&](auto mh) {
      if (corr_kind == PB_CORR_POS_ORIENT) launch_corr<15, decltype(mh)::value, CorrPosOrient>(c, out, imu, lo, mask, q, ca, bc);
      else launch_corr<15, decltype(mh)::value, CorrPosYaw>(c, out, imu, lo, mask, q, ca, bc);
    });
  }
  LAUNCHCHK(c);
  if ((rc = pbk_idle_restore(c, out, pred, q))) return rc;
  update_done(c, out);
  return PB_OK;
}
