// pb_frontend.hip -- the IMU front end in front of the filters (rbis_frontend.hpp): the kernels, their launches and the entry points of
// the C ABI -- the per-filter IMU validity mask of a batched message (pb_set_imu_valid, pbk_idle_prepare), the notch cascade
// (pb_imu_notch*) and the body-frame conversion (pb_ins_body_*).  See pb_ctx.hpp.
#include "pb_ctx.hpp"
#include "rbis_frontend.hpp"

// ---- filters without an IMU message in a batched message (independent log segments) ----
extern "C" int pb_set_imu_valid(pb_ctx *c, const uint8_t *valid_dev)
{
  if (!c) return PB_ERR_ARG;
  c->imu_valid_next = valid_dev;
  return PB_OK;
}
// The call that takes the mask (CALL: IMU_STEP) holds it in imu_valid_cur; the launchers of the step kernels (pb_step.hip) pass their
// IMU block through pbk_idle_prepare right in front of their ONE launch (rbis_frontend.hpp, k_imu_idle_prepare).  A broadcast sample
// (bc.on bit 0: no block, the seven values are kernel arguments) is expanded into the prepared block and the bit cleared in the
// caller's copy of bc, so that the step reads that block like any other.
const double *pbk_idle_prepare(pb_ctx *c, const double *imu_dev, StepBcast &bc, int *rc_out)
{
  *rc_out = PB_OK;
  const uint8_t *valid = c->imu_valid_cur;
  const bool one = (bc.on & 1) != 0;
  if (!valid || (!imu_dev && !one)) return imu_dev;
  c->imu_valid_cur = nullptr;   // (one step launch per call)
  if ((*rc_out = dev_alloc(c, c->imu_keep, (7 + 12) * (size_t) c->stride))) return imu_dev;
  ImuSample s;
  for (int i = 0; i < 7; i++) s.v[i] = bc.imu[i];
  with_ns(c->ns, [&](auto NS) {
    k_imu_idle_prepare<decltype(NS)::value><<<(c->B + 255) / 256, 256, 0, c->stream>>>(c->st, valid, one ? nullptr : imu_dev, s, c->imu_keep,
                                                                                       c->imu_keep + 7 * (size_t) c->B, c->B);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *rc_out = fail(c, PB_ERR_HIP, "k_imu_idle_prepare: %s", hipGetErrorString(e));
    return imu_dev;
  }
  bc.on &= ~1;
  c->imu_idle_cur = valid;
  return c->imu_keep;
}

int pbk_idle_restore(pb_ctx *c, double *out, double *pred, const double q[4])
{
  if (!c->imu_idle_cur) return PB_OK;
  with_ns(c->ns, [&](auto NS) {
    k_imu_idle_restore<decltype(NS)::value><<<(c->B + 255) / 256, 256, 0, c->stream>>>(out, pred, c->imu_idle_cur, c->imu_keep + 7 * (size_t) c->B,
                                                                                       q[0], q[1], c->k.qblk, c->B);
  });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_imu_notch_init(pb_ctx *c, double notch_freq, double fs)
{
  CALL(c, 0);
  if (!(notch_freq > 0) || !(fs > 0) || notch_freq * 4 >= fs / 2)
    return fail(c, PB_ERR_ARG, "pb_imu_notch_init: need 0 < 4*notch_freq < fs/2 (got %g, %g)", notch_freq, fs);
  if (int rc = dev_alloc(c, c->notch, 36 * (size_t) c->stride)) return rc;
  HIPCHK(c, hipMemsetAsync(c->notch, 0, sizeof(double) * 36 * c->stride, c->stream));
  for (int i = 0; i < 3; i++) {
    // IIRNotch::IIRNotch + secondOrderNotch (iir_notch.cpp:3-32), notch_freq * 2^i (sensor_handlers.cpp:33-41)
    double Wo = (notch_freq * pow(2, i)) / (fs / 2);
    double BW = Wo;
    const double Ab = fabs(10 * log10(.5));
    BW = BW * M_PI;
    Wo = Wo * M_PI;
    const double Gb = pow(10, -Ab / 20.);
    const double beta = (sqrt(1.0 - Gb * Gb) / Gb) * tan(BW / 2.0);
    const double gain = 1 / (1 + beta);
    c->notch_coef.b[i][0] = gain * 1.0;
    c->notch_coef.b[i][1] = gain * (-2.0 * cos(Wo));
    c->notch_coef.b[i][2] = gain * 1;
    c->notch_coef.a[i][0] = 1.0;
    c->notch_coef.a[i][1] = -2 * gain * cos(Wo);
    c->notch_coef.a[i][2] = 2 * gain - 1;
  }
  c->notch_ready = true;
  return PB_OK;
}

static int imu_notch_impl(pb_ctx *c, const char *who, int n_packets, const int32_t *counts, const double *accel_packets, double *accel_out, int mem)
{
  if (!c->notch_ready) return fail(c, PB_ERR_STATE, "%s before pb_imu_notch_init", who);
  if (n_packets < 0 || (n_packets > 0 && (!accel_packets || !accel_out))) return fail(c, PB_ERR_ARG, "%s: bad argument", who);
  if (n_packets == 0) return PB_OK;
  const size_t B = (size_t) c->B;
  const size_t pk_bytes = sizeof(double) * 3 * B * n_packets, pk_pad = (pk_bytes + 255) / 256 * 256;
  const size_t cn_bytes = counts ? sizeof(int32_t) * B : 0, cn_pad = (cn_bytes + 255) / 256 * 256;
  const double *d_in = accel_packets;
  const int32_t *d_counts = counts;
  double *d_out = accel_out;
  if (mem == PB_HOST) {
    int rc = stage_reserve(c, pk_pad + cn_pad + sizeof(double) * 3 * B);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage, accel_packets, pk_bytes, hipMemcpyHostToDevice, c->stream));
    d_in = (const double *) c->stage;
    if (counts) {
      HIPCHK(c, hipMemcpyAsync((char *) c->stage + pk_pad, counts, cn_bytes, hipMemcpyHostToDevice, c->stream));
      d_counts = (const int32_t *) ((char *) c->stage + pk_pad);
    }
    d_out = (double *) ((char *) c->stage + pk_pad + cn_pad);
    if (counts) HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(double) * 3 * B, c->stream));   // (filters without a packet: a defined 0 comes back)
  } else if (mem != PB_DEVICE) {
    return fail(c, PB_ERR_ARG, "mem must be PB_HOST or PB_DEVICE");
  }
  k_notch_counts<<<dim3((unsigned) nblk(c->B), 3u), 64, 0, c->stream>>>(c->notch, c->stride, c->B, n_packets, d_counts, d_in, d_out, c->notch_coef);
  LAUNCHCHK(c);
  if (mem == PB_HOST) {
    HIPCHK(c, hipMemcpyAsync(accel_out, d_out, sizeof(double) * 3 * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return PB_OK;
}

extern "C" int pb_imu_notch(pb_ctx *c, int n_packets, const double *accel_packets, double *accel_out, int mem)
{
  CALL(c, 0);
  return imu_notch_impl(c, "pb_imu_notch", n_packets, nullptr, accel_packets, accel_out, mem);
}

extern "C" int pb_imu_notch_counts(pb_ctx *c, int max_packets, const int32_t *counts, const double *accel_packets, double *accel_out, int mem)
{
  CALL(c, 0);
  if (!counts) return fail(c, PB_ERR_ARG, "pb_imu_notch_counts: NULL counts");
  return imu_notch_impl(c, "pb_imu_notch_counts", max_packets, counts, accel_packets, accel_out, mem);
}

extern "C" int pb_ins_body_reset(pb_ctx *c)
{
  CALL(c, 0);
  if (int rc = dev_alloc(c, c->ins_last, 6 * (size_t) c->stride)) return rc;
  if (int rc = dev_alloc(c, c->ins_prev_ut, (size_t) c->stride)) return rc;
  HIPCHK(c, hipMemsetAsync(c->ins_last, 0, sizeof(double) * 6 * (size_t) c->stride, c->stream));
  HIPCHK(c, hipMemsetAsync(c->ins_prev_ut, 0, sizeof(int64_t) * (size_t) c->stride, c->stream));
  return PB_OK;
}

extern "C" int pb_ins_body_block(pb_ctx *c, const double *gyro, const double *accel, const double *raw_dt, const int64_t *utimes, int64_t utime,
                                 const uint8_t *valid, const double rot_quat[4], const double trans_vec[3], double dt_default, int dt_from_utimes,
                                 int mem, double *imu_block_out, uint8_t *valid_out)
{
  CALL(c, 0);
  if (!gyro || !accel || !rot_quat || !imu_block_out) return fail(c, PB_ERR_ARG, "pb_ins_body_block: NULL argument");
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_ins_body_block: mem must be PB_HOST or PB_DEVICE");
  if (!c->ins_last) {
    int rc = pb_ins_body_reset(c);
    if (rc) return rc;
  }
  const size_t B = (size_t) c->B;
  Part p[5] = { { gyro, sizeof(double) * 3 * B, 0 }, { accel, sizeof(double) * 3 * B, 0 }, { raw_dt, raw_dt ? sizeof(double) * B : 0, 0 },
                { utimes, utimes ? sizeof(int64_t) * B : 0, 0 }, { valid, valid ? B : 0, 0 } };
  int rc = stage_in(c, mem, p, 5);
  if (rc) return rc;
  InsFrame f;
  for (int i = 0; i < 4; i++) f.rot[i] = rot_quat[i];
  for (int i = 0; i < 3; i++) f.trans[i] = trans_vec ? trans_vec[i] : 0.0;
  f.translate = trans_vec != nullptr;
  f.dt_from_utimes = dt_from_utimes ? 1 : 0;
  f.dt_default = dt_default;
  k_ins_body<<<(unsigned) ((c->B + 255) / 256), 256, 0, c->stream>>>(c->B, c->stride, (const double *) p[0].dev, (const double *) p[1].dev,
                                                                      (const double *) p[2].dev, (const int64_t *) p[3].dev, utime,
                                                                      (const uint8_t *) p[4].dev, f, c->ins_last, c->ins_prev_ut, imu_block_out, valid_out);
  LAUNCHCHK(c);
  return PB_OK;
}
