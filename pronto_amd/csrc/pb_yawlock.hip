// pb_yawlock.hip -- the yaw-lock handler (rbis_yawlock.hpp): the kernels, their launchers and the pb_yawlock_* / pb_step_yawlock_joints
// entry points of the C ABI.  See pb_ctx.hpp.
//   k_yawlock_form      one lane per filter: the handler's state machine, the measurement block and the two masks
//   k_step_yawlock      the same, and the m <= 2 update applied in the same launch
//
// k_step_yawlock keeps one lane per filter (as k_update_lane_rt) for 15 AND 21 states.  A yaw-lock update measures one or
// two FIXED states, so the lane needs the one or two measured covariance columns (n doubles each), not the covariance: it
// reads them with 8-byte loads, forms the gain and the posterior state, and then streams the tile's rows through -- load
// 16 bytes, P_ij -= W_i D^-1 W_j, store 16 bytes -- CHUNK rows at a time.  Live registers: W (2 n doubles), x, q and one
// chunk, so 21 states fit one lane without the column gather through LDS of the two- / four-wave tiles, and no LDS is used.
// A filter without an update this message -- all of them on the period - 1 of period messages between corrections in mode
// yaw -- leaves after the small read (head pose, bias, yaw-lock state: no covariance traffic).  The exit is per lane: in a
// mixed wave the idle lanes are masked off for the rest of the kernel and the active ones still move whole 16-byte
// elements of their rows, so divergence costs an idle lane nothing and an active lane nothing extra.
#include "pb_ctx.hpp"
#include "rbis_yawlock.hpp"

namespace {

template <int NS>
__device__ __forceinline__ void yaw_head(const double *st, long b, Pose &head, double &bias_z)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
#pragma unroll
  for (int i = 0; i < 3; i++) head.t[i] = st[S::eidx(L::OFF_VEC + 9 + i, b)];
#pragma unroll
  for (int i = 0; i < 4; i++) head.q[i] = st[S::eidx(L::OFF_QUAT + i, b)];
  bias_z = 0.0;
  if constexpr (NS == 21) bias_z = st[S::eidx(L::OFF_VEC + 17, b)];
}

// the state machine of one filter: loads its yaw-lock state, forms the measurement, stores the state and the optional outputs
template <int NS>
__device__ __forceinline__ void yaw_lane(const double *st, long b, int B, long stride, const YawPar &par, const YawIn &yin,
                                         const LegIn &lin, const LegChain *__restrict__ chain, int64_t utime, double *__restrict__ yd,
                                         int64_t *__restrict__ yi, double *__restrict__ z_out, double *__restrict__ quat_out,
                                         uint8_t *__restrict__ mask_out, double (&z)[2], double (&q)[4], bool (&mask)[2])
{
  z[0] = z[1] = 0.0;
  q[0] = 1.0; q[1] = q[2] = q[3] = 0.0;
  mask[0] = mask[1] = false;
  if (lin.valid == nullptr || lin.valid[b] != 0) {  // a filter without a message keeps its state, its counter included
    Pose head;
    double bias_z;
    yaw_head<NS>(st, b, head, bias_z);
    const bool standing = yin.standing ? yin.standing[b] != 0 : yin.standing_all != 0;
    const double gyro_z = yin.gyro_z ? yin.gyro_z[b] : yin.gyro_z_all;
    const int64_t ut = lin.utimes ? lin.utimes[b] : utime;
    YawState s;
    yaw_load(s, yd, yi, stride, b);
    yaw_form(s, par, standing, gyro_z, head, bias_z, ut, [&](Pose &bl, Pose &br) { yaw_feet(lin, chain, b, B, bl, br); }, z, q, mask);
    yaw_store(s, yd, yi, stride, b, s.outcome == YO_CAPTURE);
  }
  if (z_out) {
    z_out[b] = z[0];
    z_out[(long) B + b] = z[1];
  }
  if (quat_out) {
#pragma unroll
    for (int i = 0; i < 4; i++) quat_out[(long) i * B + b] = q[i];
  }
  if (mask_out) {
    mask_out[b] = mask[0];
    mask_out[(long) B + b] = mask[1];
  }
}

template <int NS>
__global__ __launch_bounds__(64) void k_yawlock_form(const double *__restrict__ st, int B, long stride, YawPar par, YawIn yin, LegIn lin,
                                                     const LegChain *__restrict__ chain, int64_t utime, double *__restrict__ yd,
                                                     int64_t *__restrict__ yi, double *__restrict__ z_out, double *__restrict__ quat_out,
                                                     uint8_t *__restrict__ mask_out)
{
  const long b = (long) blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double z[2], q[4];
  bool mask[2];
  yaw_lane<NS>(st, b, B, stride, par, yin, lin, chain, utime, yd, yi, z_out, quat_out, mask_out, z, q, mask);
}

// the index list of a mode's row set: yawbias {17}, yaw {8}, yawbias_yaw {17, 8} (rbis_yawlock_update.cpp:75-99)
template <int MODE> struct YawIdx {
  static constexpr int M = (MODE == YL_YAWBIAS_YAW) ? 2 : 1;
  static constexpr Idx<2> value = { { MODE == YL_YAW ? 8 : 17, 8 } };
};

constexpr int YAW_CHUNK = 16;  // rows in flight per lane while the covariance streams through (64 VGPRs)

// RBISIndexedMeasurement / RBISIndexedPlusOrientationMeasurement::updateFilter for the row set of MODE on the filter of this
// lane.  The arithmetic is measurement_update_cols' (rbis_device.hpp), term for term: the same residual, LDL^T, W = P[:, idx]
// L^-T, dx = W D^-1 y through add_delta, and P_ij = fma(-(W_ik / d_k), W_jk, P_ij) in the same order of k.  In mode
// yawbias_yaw a lane whose correction is not valid applies the bias row alone: row 1 of the pair is switched off (W[:, 1] = 0,
// resid = 0, S_11 = 1, S_10 = 0), which leaves exactly the m = 1 update (d_1 = 1: det and the quadratic form unchanged, every
// fma with W[:, 1] adds -0 * x).
template <int NS, int MODE, int MH>
__device__ __forceinline__ void yaw_apply(const double *st, double *sto, unsigned tile, unsigned lane, const YawPar &par, const double (&z)[2],
                                          const double (&qm)[4], bool orient, const Consts &k)
{
  using L = Lay<NS>;
  using S = Slots<NS>;
  using I = YawIdx<MODE>;
  constexpr int M = I::M;
  constexpr Idx<2> idx = I::value;
  constexpr int LA = MemHint<MH>::LA, SA = MemHint<MH>::SA;
  const rsrc_t rs = mkbuf(reinterpret_cast<const char *>(st) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const rsrc_t ro = mkbuf(reinterpret_cast<char *>(sto) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const unsigned vo = lane * 16u;
  auto ld1 = [&](int comp) {
    const int sl = S::T.slot_of[comp];
    return ldg<LA>(rs, (unsigned) (sl >> 1) * 1024u + (unsigned) (sl & 1) * 8u, vo);
  };
  // the small part of the state and the measured columns (every load of this lane's rows that a store below could alias
  // is issued before the first store: the lane is the only reader and writer of its 16-byte elements)
  double x[NS], q[4], ll, W[NS][M];
#pragma unroll
  for (int i = 0; i < NS; i++) x[i] = ld1(L::OFF_VEC + i);
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = ld1(L::OFF_QUAT + i);
  ll = ld1(L::OFF_LL);
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int kk = 0; kk < M; kk++) W[i][kk] = ld1(L::OFF_P + pk(i, idx.v[kk]));
  double resid[M], Sm[M * (M + 1) / 2];
  double dq[3] = { 0.0, 0.0, 0.0 };
  if (MODE != YL_YAWBIAS) subtract_quats(qm, q, dq);  // rbis.cpp:199
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    resid[kk] = (idx.v[kk] == 8) ? dq[2] : z[kk] - x[idx.v[kk]];  // rbis.cpp:202-209
#pragma unroll
    for (int j = 0; j < kk; j++) Sm[pk(kk, j)] = W[idx.v[kk]][j];
    Sm[pk(kk, kk)] = W[idx.v[kk]][kk] + (idx.v[kk] == 8 ? par.r_yaw : par.r_bias);
  }
  if constexpr (MODE == YL_YAWBIAS_YAW) {
    if (!orient) {  // the bias row alone (rbis_yawlock_update.cpp:212-224)
#pragma unroll
      for (int i = 0; i < NS; i++) W[i][1] = 0.0;
      resid[1] = 0.0;
      Sm[pk(1, 0)] = 0.0;
      Sm[pk(1, 1)] = 1.0;
    }
  }
  double d[M];
  ldlt<M>(Sm, d);
  double y[M], id[M], quad = 0.0, det = 1.0;
#pragma unroll
  for (int kk = 0; kk < M; kk++) {
    double s = resid[kk];
#pragma unroll
    for (int j = 0; j < kk; j++) s -= Sm[pk(kk, j)] * y[j];
    y[kk] = s;
    id[kk] = 1.0 / d[kk];
    det *= d[kk];
    quad += s * s * id[kk];
  }
  ll += -log(det) - quad;  // rbis.cpp:142
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int kk = 0; kk < M; kk++) {
      double s = W[i][kk];
#pragma unroll
      for (int j = 0; j < kk; j++) s -= W[i][j] * Sm[pk(kk, j)];
      W[i][kk] = s;
    }
  double dx[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) {
    double s = 0.0;
#pragma unroll
    for (int kk = 0; kk < M; kk++) s = (kk == 0) ? W[i][0] * (y[0] * id[0]) : fma(W[i][kk], y[kk] * id[kk], s);
    dx[i] = s;
  }
  add_delta<NS>(x, q, dx, k.chi_tol);
  // the posterior value of a slot from its prior value
  auto post = [&](auto SL, double prior) {
    constexpr int comp = S::T.comp_of[decltype(SL)::value];
    if constexpr (comp < 0) return 0.0;  // padding
    else if constexpr (comp >= L::OFF_P) {
      constexpr int i = pk_row(comp - L::OFF_P), j = pk_col(comp - L::OFF_P);
      double acc = prior;
#pragma unroll
      for (int kk = 0; kk < M; kk++) acc = fma(-(W[i][kk] * id[kk]), W[j][kk], acc);
      return acc;
    } else if constexpr (comp == L::OFF_LL) return ll;
    else if constexpr (comp >= L::OFF_QUAT) return q[comp - L::OFF_QUAT];
    else return x[comp - L::OFF_VEC];
  };
  constexpr int NCH = (S::NROW + YAW_CHUNK - 1) / YAW_CHUNK;
  static_for<NCH>([&](auto CH) {
    constexpr int r0 = decltype(CH)::value * YAW_CHUNK, r1 = (r0 + YAW_CHUNK < S::NROW) ? r0 + YAW_CHUNK : S::NROW;
    d2_t buf[YAW_CHUNK];
    static_for<r1 - r0>([&](auto R) { buf[decltype(R)::value] = ldg2<LA>(rs, (unsigned) (r0 + decltype(R)::value) * 1024u, vo); });
    static_for<r1 - r0>([&](auto R) {
      constexpr int r = r0 + decltype(R)::value;
      const d2_t o = { post(std::integral_constant<int, 2 * r>{}, buf[decltype(R)::value].x),
                       post(std::integral_constant<int, 2 * r + 1>{}, buf[decltype(R)::value].y) };
      stg2<SA>(ro, (unsigned) r * 1024u, vo, o);
    });
  });
}

// a filter that gets no update while the posterior goes to another array than the head's (pb_set_output_slot, or a head that
// is a checkpoint slot): its state moves over unchanged
template <int NS, int MH>
__device__ __forceinline__ void yaw_copy(const double *st, double *sto, unsigned tile, unsigned lane)
{
  using S = Slots<NS>;
  const rsrc_t rs = mkbuf(reinterpret_cast<const char *>(st) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const rsrc_t ro = mkbuf(reinterpret_cast<char *>(sto) + (size_t) tile * S::TILE_BYTES, S::TILE_BYTES);
  const unsigned vo = lane * 16u;
  for (int r = 0; r < S::NROW; r++) stg2<MemHint<MH>::SA>(ro, (unsigned) r * 1024u, vo, ldg2<MemHint<MH>::LA>(rs, (unsigned) r * 1024u, vo));
}

template <int NS, int MODE, int MH>
__global__ __launch_bounds__(64) void k_step_yawlock(const double *st, double *sto, int B, long stride, YawPar par, YawIn yin, LegIn lin,
                                                     const LegChain *__restrict__ chain, int64_t utime, double *__restrict__ yd,
                                                     int64_t *__restrict__ yi, double *__restrict__ z_out, double *__restrict__ quat_out,
                                                     uint8_t *__restrict__ mask_out, Consts k)
{
  const unsigned tile = blockIdx.x, lane = threadIdx.x;
  const long b = (long) tile * 64 + lane;
  if (b >= B) return;
  double z[2], q[4];
  bool mask[2];
  yaw_lane<NS>(st, b, B, stride, par, yin, lin, chain, utime, yd, yi, z_out, quat_out, mask_out, z, q, mask);
  if (!mask[0] && !mask[1]) {
    if (st != sto) yaw_copy<NS, MH>(st, sto, tile, lane);
    return;
  }
  yaw_apply<NS, MODE, MH>(st, sto, tile, lane, par, z, q, mask[0], k);
}

template <int NS, int MODE>
void launch_step(pb_ctx *c, double *out, const YawIn &yin, const LegIn &lin, int64_t utime, double *z_out, double *quat_out, uint8_t *mask_out)
{
  with_mem_hint(c->policy.mem_hint, [&](auto mh) {
    k_step_yawlock<NS, MODE, decltype(mh)::value><<<nblk(c->B), 64, 0, c->stream>>>(c->st, out, c->B, c->stride, c->yaw_par, yin, lin, c->leg_chain,
                                                                                  utime, c->yawd, c->yawi, z_out, quat_out, mask_out, c->k);
  });
}

__global__ void k_yawlock_reset(double *yd, int64_t *yi, long stride, int B)
{
  const long b = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  YawState s;
  yaw_reset(s);
  yaw_store(s, yd, yi, stride, b);
}

__global__ void k_yawlock_get(const double *yd, const int64_t *yi, long stride, long b, double *poses, int64_t *info)
{
  YawState s;
  yaw_load(s, yd, yi, stride, b);
  for (int i = 0; i < 3; i++) { poses[i] = s.world_to_l.t[i]; poses[7 + i] = s.world_to_r.t[i]; }
  for (int i = 0; i < 4; i++) { poses[3 + i] = s.world_to_l.q[i]; poses[10 + i] = s.world_to_r.q[i]; }
  info[0] = s.counter; info[1] = s.lock_init; info[2] = s.disable_until; info[3] = (int64_t) s.outcome | (s.slips << 8);
}

}  // namespace

// ---- launchers.  form: state machine + measurement block + masks; step: the same and the update applied in the one kernel (honours
// pb_set_output_slot).  z_out [2][B], quat_out [4][B], mask_out [2][B] device or NULL (step) ----
static int pbk_yawlock_reset(pb_ctx *c)
{
  k_yawlock_reset<<<nblk(c->B), 64, 0, c->stream>>>(c->yawd, c->yawi, c->stride, c->B);
  LAUNCHCHK(c);
  return PB_OK;
}

static int pbk_yawlock_get(pb_ctx *c, int filter, double *poses_dev, int64_t *info_dev)
{
  k_yawlock_get<<<1, 1, 0, c->stream>>>(c->yawd, c->yawi, c->stride, filter, poses_dev, info_dev);
  LAUNCHCHK(c);
  return PB_OK;
}

static int pbk_yawlock_form(pb_ctx *c, const YawIn &yin, const LegIn &lin, int64_t utime, double *z_out, double *quat_out, uint8_t *mask_out)
{
  with_ns(c->ns, [&](auto NS) {
    k_yawlock_form<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(c->st, c->B, c->stride, c->yaw_par, yin, lin, c->leg_chain, utime, c->yawd,
                                                                           c->yawi, z_out, quat_out, mask_out);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

static int pbk_step_yawlock(pb_ctx *c, const YawIn &yin, const LegIn &lin, int64_t utime, double *z_out, double *quat_out, uint8_t *mask_out)
{
  double *out = update_target(c);
  if (c->ns == 15) launch_step<15, YL_YAW>(c, out, yin, lin, utime, z_out, quat_out, mask_out);
  else if (c->yaw_par.mode == YL_YAWBIAS) launch_step<21, YL_YAWBIAS>(c, out, yin, lin, utime, z_out, quat_out, mask_out);
  else if (c->yaw_par.mode == YL_YAW) launch_step<21, YL_YAW>(c, out, yin, lin, utime, z_out, quat_out, mask_out);
  else launch_step<21, YL_YAWBIAS_YAW>(c, out, yin, lin, utime, z_out, quat_out, mask_out);
  LAUNCHCHK(c);
  update_done(c, out);
  return PB_OK;
}

// ---- the entry points of the C ABI ----
extern "C" int pb_yawlock_init(pb_ctx *c, int mode, int correction_period, int yaw_slip_detect, double yaw_slip_threshold_degrees,
                               double yaw_slip_disable_period_s, double r_yaw_bias_deg, double r_yaw_deg)
{
  if (!c) return PB_ERR_ARG;
  // (the argument checks come before anything that needs the device)
  if (mode < YL_YAWBIAS || mode > YL_YAWBIAS_YAW) return fail(c, PB_ERR_ARG, "pb_yawlock_init: mode must be 0 (yawbias), 1 (yaw) or 2 (yawbias_yaw)");
  if (mode != YL_YAW && c->ns != 21) return fail(c, PB_ERR_ARG, "pb_yawlock_init: mode %d measures the gyro bias (state 17), this context has %d states", mode, c->ns);
  if (correction_period < 1) return fail(c, PB_ERR_ARG, "pb_yawlock_init: correction_period must be >= 1");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = dev_alloc(c, c->yawd, NYD * (size_t) c->stride)) return rc;
  if (int rc = dev_alloc(c, c->yawi, NYI * (size_t) c->stride)) return rc;
  YawPar &p = c->yaw_par;
  p.mode = mode;
  p.period = correction_period;
  p.slip_detect = yaw_slip_detect != 0;
  p.slip_threshold_deg = yaw_slip_threshold_degrees;
  p.slip_disable_s = yaw_slip_disable_period_s;
  const double rb = r_yaw_bias_deg * M_PI / 180.0, ry = r_yaw_deg * M_PI / 180.0;  // bot_to_radians, bot_sq (rbis_yawlock_update.cpp:80,88)
  p.r_bias = rb * rb;
  p.r_yaw = ry * ry;
  c->yaw_standing_dev = c->yaw_gyro_dev = false;
  c->yaw_standing_all = 0;
  c->yaw_gyro_all = 0.0;
  return pbk_yawlock_reset(c);
}

// What a handler keeps per filter between messages (pb_yawlock_set_standing / _set_gyro): [B] values in a device array of the
// context's own, allocated once -- or ONE value for every filter (PB_HOST_BROADCAST), which the caller has stored already.
template <class T>
static int keep_per_filter(pb_ctx *c, const char *who, T *&dev, bool &dev_on, const T *src, int mem)
{
  if (mem == PB_HOST_BROADCAST) {
    dev_on = false;
    return PB_OK;
  }
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "%s: bad mem", who);
  if (int rc = dev_alloc(c, dev, (size_t) c->stride)) return rc;
  HIPCHK(c, hipMemcpyAsync(dev, src, sizeof(T) * (size_t) c->B, mem == PB_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
  if (mem == PB_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's array is free again
  dev_on = true;
  return PB_OK;
}

extern "C" int pb_yawlock_set_standing(pb_ctx *c, const uint8_t *standing, int mem)
{
  CALL(c, 0);
  if (!c->yawd) return fail(c, PB_ERR_STATE, "pb_yawlock_set_standing before pb_yawlock_init");
  if (!standing) return fail(c, PB_ERR_ARG, "pb_yawlock_set_standing: NULL input");
  if (mem == PB_HOST_BROADCAST) c->yaw_standing_all = standing[0] != 0;
  return keep_per_filter(c, "pb_yawlock_set_standing", c->yaw_standing, c->yaw_standing_dev, standing, mem);
}

extern "C" int pb_yawlock_set_gyro(pb_ctx *c, const double *body_gyro_z, int mem)
{
  CALL(c, 0);
  if (!c->yawd) return fail(c, PB_ERR_STATE, "pb_yawlock_set_gyro before pb_yawlock_init");
  if (!body_gyro_z) return fail(c, PB_ERR_ARG, "pb_yawlock_set_gyro: NULL input");
  if (mem == PB_HOST_BROADCAST) c->yaw_gyro_all = body_gyro_z[0];
  return keep_per_filter(c, "pb_yawlock_set_gyro", c->yaw_gyro, c->yaw_gyro_dev, body_gyro_z, mem);
}

static int yawlock_impl(pb_ctx *c, const char *who, bool apply, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows,
                        const float *joint_position, int mem, double *z_out, double *quat_out, uint8_t *mask_out)
{
  if (!c->yawd) return fail(c, PB_ERR_STATE, "%s before pb_yawlock_init", who);
  LegIn lin;
  int rc = leg_in_joints(c, who, n_rows, joint_position, nullptr, nullptr, mem, lin);
  if (rc) return rc;
  lin.utimes = utimes;
  lin.valid = valid;
  YawIn yin;
  yin.standing = c->yaw_standing_dev ? c->yaw_standing : nullptr;
  yin.gyro_z = c->yaw_gyro_dev ? c->yaw_gyro : nullptr;
  yin.standing_all = c->yaw_standing_all;
  yin.gyro_z_all = c->yaw_gyro_all;
  return apply ? pbk_step_yawlock(c, yin, lin, utime, z_out, quat_out, mask_out) : pbk_yawlock_form(c, yin, lin, utime, z_out, quat_out, mask_out);
}

extern "C" int pb_yawlock_update_joints(pb_ctx *c, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows,
                                        const float *joint_position, int mem, double *z_out, double *quat_out, uint8_t *mask_out)
{
  CALL(c, NEEDS_STATE);
  return yawlock_impl(c, "pb_yawlock_update_joints", false, utime, utimes, valid, n_rows, joint_position, mem, z_out, quat_out, mask_out);
}

extern "C" int pb_step_yawlock_joints(pb_ctx *c, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows,
                                      const float *joint_position, int mem, double *z_out, double *quat_out, uint8_t *mask_out)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  return yawlock_impl(c, "pb_step_yawlock_joints", true, utime, utimes, valid, n_rows, joint_position, mem, z_out, quat_out, mask_out);
}

extern "C" int pb_yawlock_get(pb_ctx *c, int filter, double poses[14], int64_t info[4])
{
  CALL(c, 0);
  if (!c->yawd) return fail(c, PB_ERR_STATE, "pb_yawlock_get before pb_yawlock_init");
  if (filter < 0 || filter >= c->B || !poses || !info) return fail(c, PB_ERR_ARG, "pb_yawlock_get: bad argument");
  return get_small(c, poses, 14, info, [&](double *dp, int64_t *di) { return pbk_yawlock_get(c, filter, dp, di); });
}
