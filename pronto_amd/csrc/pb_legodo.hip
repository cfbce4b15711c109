// pb_legodo.hip -- stand-alone leg odometry, forward kinematics and the joint-position filters in front of them (rbis_legodo.hpp,
// rbis_jointfilt.hpp): the kernels (rbis_legodo_kernels.hpp, rbis_jointfilt_kernels.hpp), their launches and the pb_legodo_* /
// pb_joint_filter* / pb_step_legodo_joints / _feet entry points of the C ABI.  See pb_ctx.hpp.
#include <cmath>

#include "pb_ctx.hpp"
#include "rbis_legodo_kernels.hpp"
#include "rbis_jointfilt_kernels.hpp"

extern "C" int pb_legodo_init(pb_ctx *c, double lt, double ht, int64_t low_delay, int64_t high_delay, int filter_contact_events)
{
  CALL(c, 0);
  if (!(ht >= lt) || low_delay < 0 || high_delay < 0) return fail(c, PB_ERR_ARG, "pb_legodo_init: need high >= low threshold, delays >= 0");
  if (low_delay > 2000000000LL || high_delay > 2000000000LL) return fail(c, PB_ERR_ARG, "pb_legodo_init: delays must be below 2e9 us");
  if (int rc = dev_alloc(c, c->legd, (size_t) (NLD + NLD_WC) * c->stride)) return rc;
  if (int rc = dev_alloc(c, c->legi, (size_t) NLI * c->stride)) return rc;
  // the thresholds pass through `float` variables in the reference (leg_estimate.cpp:103-104, FootContactAlt.cpp:5)
  // a (re-)initialised context starts like leg_estimate's constructor: FootContactAlt, no controller input, no world
  // constraint, controller contact counts -1 (leg_estimate.cpp:93-142, rbis_legodo_update.cpp:100-101)
  c->leg_par = LegPar{};
  c->leg_meas = LegMeasPar{};
  c->leg_nc_h[0] = c->leg_nc_h[1] = -1;
  c->leg_nc_dev = false;
  c->leg_blk_on = false;   // (the buffer stays the context's)
  c->leg_par.alt = SchmittPar{ (double) (float) lt, (double) (float) ht, low_delay, high_delay };
  c->leg_par.filter_contact_events = filter_contact_events ? 1 : 0;
  k_legodo_reset<<<nblk(c->B), 64, 0, c->stream>>>(c->legd, c->legi, c->stride, c->B, -1);
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_legodo_set_contact_mode(pb_ctx *c, int standing, double total_force, double standing_schmitt_level,
                                          int use_controller_input)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_contact_mode before pb_legodo_init");
  c->leg_par.standing = standing ? 1 : 0;
  c->leg_par.total_force = (float) total_force;                        // float members (FootContact.h:24-28)
  c->leg_par.standing_schmitt_level = (float) standing_schmitt_level;
  c->leg_par.use_controller_input = use_controller_input ? 1 : 0;
  return PB_OK;
}

extern "C" int pb_legodo_set_message_times(pb_ctx *c, const int64_t *utimes, const uint8_t *valid, int mem)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_message_times before pb_legodo_init");
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_legodo_set_message_times: mem must be PB_HOST or PB_DEVICE");
  c->leg_ut_on = c->leg_valid_on = false;
  c->leg_ut_ext = nullptr;
  c->leg_valid_ext = nullptr;
  if (mem == PB_DEVICE) {   // read in place by the consuming launch (no copy): the arrays stay the caller's until that launch has run
    c->leg_ut_ext = utimes;
    c->leg_valid_ext = valid;
    c->leg_ut_on = utimes != nullptr;
    c->leg_valid_on = valid != nullptr;
    return PB_OK;
  }
  if (utimes) {
    if (int rc = dev_alloc(c, c->leg_ut, (size_t) c->stride)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->leg_ut, utimes, sizeof(int64_t) * (size_t) c->B, hipMemcpyHostToDevice, c->stream));
    c->leg_ut_on = true;
  }
  if (valid) {
    if (int rc = dev_alloc(c, c->leg_valid, (size_t) c->stride)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->leg_valid, valid, (size_t) c->B, hipMemcpyHostToDevice, c->stream));
    c->leg_valid_on = true;
  }
  if (utimes || valid) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays are free again
  return PB_OK;
}
extern "C" int pb_legodo_set_measurement_mode(pb_ctx *c, int mode, double r_xyz, double r_vang, double r_vang_uncertain)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_measurement_mode before pb_legodo_init");
  if (mode < 0 || mode > 2) return fail(c, PB_ERR_ARG, "pb_legodo_set_measurement_mode: mode 0 (lin_rate), 1 (lin_rot_rate) or 2 (pos_and_lin_rate)");
  c->leg_meas = LegMeasPar{};
  c->leg_meas.mode = mode;
  c->leg_meas.r_xyz2 = r_xyz * r_xyz;                    // bot_sq (rbis_legodo_common.cpp:38-44)
  c->leg_meas.r_a2 = r_vang * r_vang;
  c->leg_meas.r_a2_uncertain = r_vang_uncertain * r_vang_uncertain;
  if (mode == 2) c->leg_par.world_constraint = 1;        // the position it measures is leg_estimate's world constraint
  return PB_OK;
}

static_assert((int) LPR_ROWS == (int) PB_LEGPAR_ROWS && (int) LPR_R_VXYZ == (int) PB_LEGPAR_R_VXYZ && (int) LPR_R_XYZ == (int) PB_LEGPAR_R_XYZ &&
                  (int) LPR_SCHMITT_LOW == (int) PB_LEGPAR_SCHMITT_LOW && (int) LPR_SCHMITT_HIGH_DELAY == (int) PB_LEGPAR_SCHMITT_HIGH_DELAY &&
                  (int) LPR_STANDING_SCHMITT_LEVEL == (int) PB_LEGPAR_STANDING_SCHMITT_LEVEL,
              "rbis_legpar.hpp's rows are the header's");

extern "C" int pb_legodo_set_param_block(pb_ctx *c, const double *block, int mem)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_param_block before pb_legodo_init");
  if (!block) {  // back to the scalars
    c->leg_blk_on = false;
    return PB_OK;
  }
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_legodo_set_param_block: mem must be PB_HOST or PB_DEVICE");
  const size_t B = (size_t) c->B;
  if (mem == PB_HOST) {
    static const char *const name[PB_LEGPAR_ROWS] = { "r_vxyz", "r_vxyz_uncertain", "r_vang", "r_vang_uncertain", "r_xyz", "schmitt_low_threshold",
                                                      "schmitt_high_threshold", "schmitt_low_delay", "schmitt_high_delay", "total_force",
                                                      "standing_schmitt_level" };
    for (size_t b = 0; b < B; b++) {
      auto at = [&](int row) { return block[(size_t) row * B + b]; };
      int bad = -1;
      for (int row = 0; row < PB_LEGPAR_ROWS && bad < 0; row++) {
        const double v = at(row);
        const bool noise = row <= PB_LEGPAR_R_XYZ, delay = row == PB_LEGPAR_SCHMITT_LOW_DELAY || row == PB_LEGPAR_SCHMITT_HIGH_DELAY;
        if (noise && !(std::isfinite(v) && v >= 0)) bad = row;
        if (delay && !(v >= 0 && v <= 2e9 && v == std::floor(v))) bad = row;
        if (row == PB_LEGPAR_SCHMITT_HIGH && !(v >= at(PB_LEGPAR_SCHMITT_LOW))) bad = row;
      }
      if (bad >= 0)
        return fail(c, PB_ERR_ARG, "pb_legodo_set_param_block: filter %zu, row %d (%s) = %g: noises finite and >= 0, high >= low threshold, "
                    "delays whole numbers in [0, 2e9] us", b, bad, name[bad], at(bad));
    }
  }
  // rows `stride` apart like legd: the lanes past the batch of a tile read in bounds (zeros)
  const bool fresh = c->leg_blk == nullptr;
  if (int rc = dev_alloc(c, c->leg_blk, (size_t) PB_LEGPAR_ROWS * c->stride)) return rc;
  if (fresh) HIPCHK(c, hipMemsetAsync(c->leg_blk, 0, sizeof(double) * PB_LEGPAR_ROWS * (size_t) c->stride, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(c->leg_blk, sizeof(double) * (size_t) c->stride, block, sizeof(double) * B, sizeof(double) * B, PB_LEGPAR_ROWS,
                             mem == PB_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's array is free again
  c->leg_blk_on = true;
  return PB_OK;
}

extern "C" int pb_legodo_set_zero_initial_velocity(pb_ctx *c, int ticks)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_zero_initial_velocity before pb_legodo_init");
  if (ticks > 65535) return fail(c, PB_ERR_ARG, "pb_legodo_set_zero_initial_velocity: at most 65535 ticks (16-bit per-robot counter)");
  k_legodo_reset<<<nblk(c->B), 64, 0, c->stream>>>(c->legd, c->legi, c->stride, c->B, ticks < 0 ? 0 : ticks);
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_legodo_set_control_contacts(pb_ctx *c, const int32_t *n_contacts, int mem)
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_set_control_contacts before pb_legodo_init");
  if (!n_contacts) return fail(c, PB_ERR_ARG, "pb_legodo_set_control_contacts: NULL input");
  if (mem == PB_HOST_BROADCAST) {
    c->leg_nc_h[0] = n_contacts[0];
    c->leg_nc_h[1] = n_contacts[1];
    c->leg_nc_dev = false;
    return PB_OK;
  }
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "mem must be PB_HOST, PB_DEVICE or PB_HOST_BROADCAST");
  if (int rc = dev_alloc(c, c->leg_nc, 2 * (size_t) c->B)) return rc;
  // kept by the context until the next call, like the handler keeps the last CONTROLLER_FOOT_CONTACT message
  HIPCHK(c, hipMemcpyAsync(c->leg_nc, n_contacts, sizeof(int32_t) * 2 * (size_t) c->B,
                           mem == PB_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
  if (mem == PB_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));
  c->leg_nc_dev = true;
  return PB_OK;
}

extern "C" int pb_legodo_set_chain(pb_ctx *c, int n_left, int n_right, const int *joint_type, const int *joint_row,
                                   const double *origin_xyz_rpy, const double *axis, const float *adjustment_gain)
{
  CALL(c, 0);
  if (n_left < 1 || n_right < 1 || n_left > LEG_MAXJ || n_right > LEG_MAXJ)
    return fail(c, PB_ERR_ARG, "pb_legodo_set_chain: 1..%d joints per leg", LEG_MAXJ);
  if (!joint_type || !joint_row || !origin_xyz_rpy || !axis) return fail(c, PB_ERR_ARG, "pb_legodo_set_chain: NULL input");
  LegChain ch;
  memset(&ch, 0, sizeof ch);
  ch.n[0] = n_left;
  ch.n[1] = n_right;
  int max_row = -1;
  for (int side = 0, k = 0; side < 2; side++) {
    for (int j = 0; j < ch.n[side]; j++, k++) {
      const int ty = joint_type[k];
      if (ty != LJ_FIXED && ty != LJ_REVOLUTE && ty != LJ_PRISMATIC) return fail(c, PB_ERR_ARG, "pb_legodo_set_chain: joint %d: bad type %d", k, ty);
      if (ty != LJ_FIXED && joint_row[k] < 0) return fail(c, PB_ERR_ARG, "pb_legodo_set_chain: joint %d: negative row", k);
      if (ty != LJ_FIXED && joint_row[k] > max_row) max_row = joint_row[k];
      if (!leg_chain_entry(ch, side, j, ty, joint_row[k], origin_xyz_rpy + 6 * k, axis + 3 * k, adjustment_gain ? adjustment_gain[k] : 0.0f))
        return fail(c, PB_ERR_ARG, "pb_legodo_set_chain: joint %d: zero axis", k);
    }
  }
  if (int rc = dev_alloc(c, c->leg_chain, 1)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // kernels in flight may still read the old table
  HIPCHK(c, hipMemcpy(c->leg_chain, &ch, sizeof ch, hipMemcpyHostToDevice));
  c->leg_chain_h = ch;
  c->leg_chain_rows = max_row + 1;
  c->jf_ready = false;  // the filters' row list came from the old chain
  return PB_OK;
}

// ---- joint-position filters in front of the kinematics (leg_estimate.cpp:411-428) ----------------------------------
extern "C" int pb_joint_filter_init(pb_ctx *c, int mode, double process_noise_pos, double process_noise_vel, double observation_noise)
{
  CALL(c, 0);
  if (mode != JF_LOWPASS && mode != JF_KALMAN) return fail(c, PB_ERR_ARG, "pb_joint_filter_init: mode must be 1 (lowpass) or 2 (kalman)");
  if (!c->leg_chain) return fail(c, PB_ERR_STATE, "pb_joint_filter_init before pb_legodo_set_chain");
  JfPar par;
  memset(&par, 0, sizeof par);
  par.mode = mode;
  const LegChain &ch = c->leg_chain_h;
  for (int side = 0; side < 2; side++) {
    for (int j = 0; j < ch.n[side]; j++) {
      if ((ch.code[side][j] & LC_TYPE) == LJ_FIXED) continue;
      const int row = ch.row[side][j];
      bool seen = false;
      for (int f = 0; f < par.nf; f++) seen = seen || par.row[f] == row;
      if (!seen && row < JF_NUM_FILT_JOINTS) par.row[par.nf++] = row;  // leg_estimate.cpp:415,419: i < NUM_FILT_JOINTS
      if (ch.gain[side][j] != 0.0f) {
        bool have = false;
        for (int a = 0; a < par.nadj; a++) have = have || par.adj_row[a] == row;
        if (!have) { par.adj_row[par.nadj] = row; par.adj_gain[par.nadj++] = ch.gain[side][j]; }
      }
    }
  }
  jf_lowpass_coeffs(par.coef);
  par.pn_pos = (float) process_noise_pos;   // float members (simple_kalman_filter.hpp:39-40)
  par.pn_vel = (float) process_noise_vel;
  par.r = (float) observation_noise;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void) dev_release(c, c->jf_ring);
  (void) dev_release(c, c->jf_kst);
  c->jf_ring_h.clear();
  c->jf_kst_h.clear();
  c->jf_par = par;
  c->jf_first = true;
  c->jf_input = -1;
  c->jf_head = 0;
  c->jf_tlast = 0;
  c->jf_ready = true;
  return PB_OK;
}

extern "C" int pb_joint_filter(pb_ctx *c, int64_t utime, int n_rows, const float *joint_position, const float *joint_velocity,
                               const float *joint_effort, int mem, float *joint_position_out)
{
  CALL(c, 0);
  if (!c->jf_ready) return fail(c, PB_ERR_STATE, "pb_joint_filter before pb_joint_filter_init (or the chain changed since)");
  if (!joint_position || !joint_position_out) return fail(c, PB_ERR_ARG, "pb_joint_filter: NULL input");
  if (n_rows < c->leg_chain_rows) return fail(c, PB_ERR_ARG, "pb_joint_filter: the chain reads joint row %d, the block has %d rows", c->leg_chain_rows - 1, n_rows);
  JfPar &par = c->jf_par;
  if (par.mode == JF_KALMAN && !joint_velocity) return fail(c, PB_ERR_ARG, "pb_joint_filter: the Kalman filter starts from joint_velocity");
  const int input = (mem == PB_HOST_BROADCAST) ? 1 : 0;
  if (c->jf_input >= 0 && c->jf_input != input)
    return fail(c, PB_ERR_STATE, "pb_joint_filter: per-robot and one-robot messages cannot be mixed (pb_joint_filter_init starts over)");
  const double t = (double) utime * 1E-6;  // leg_estimate.cpp:422
  const double dt = t - c->jf_tlast;
  const int first = c->jf_first ? 1 : 0;
  const size_t B = (size_t) c->B, nf = (size_t) par.nf;
  auto adjusted = [&](const float *pos, const float *eff, int row, size_t at) {
    float g = 0.0f;
    for (int a = 0; a < par.nadj; a++) g = (par.adj_row[a] == row) ? par.adj_gain[a] : g;
    return eff ? torque_adjust(pos[at], eff[at], g) : pos[at];
  };
  if (input == 1) {
    // one robot's joints for every filter of the batch: a per-MESSAGE computation, done once on the host with the functions
    // the kernel runs per robot; the output is a host array the caller passes on as PB_HOST_BROADCAST
    if (c->jf_input < 0) {
      c->jf_ring_h.assign(JF_TAPS * nf, 0.0f);
      c->jf_kst_h.assign(JF_KSTATE * nf, 0.0);
    }
    for (int row = 0; row < n_rows; row++) joint_position_out[row] = adjusted(joint_position, joint_effort, row, (size_t) row);
    for (size_t f = 0; f < nf; f++) {
      const int row = par.row[f];
      const float x = joint_position_out[row];
      if (par.mode == JF_LOWPASS) {
        float *ring = c->jf_ring_h.data();
        if (first) for (int s = 0; s < JF_TAPS; s++) ring[s * nf + f] = x;
        else ring[c->jf_head * nf + f] = x;
        const int head = c->jf_head;
        joint_position_out[row] = jf_lowpass(par.coef, [&](int i) { return first ? x : ring[((head + 1 + i) % JF_TAPS) * nf + f]; });
      } else {
        double s[JF_KSTATE];
        if (first) {
          s[0] = (double) x; s[1] = (double) joint_velocity[row];
          s[2] = 1.0; s[3] = 0.0; s[4] = 0.0; s[5] = 1.0;
        } else {
          for (int i = 0; i < JF_KSTATE; i++) s[i] = c->jf_kst_h[i * nf + f];
          joint_position_out[row] = jf_kalman(s, dt, x, par.pn_pos, par.pn_vel, par.r);
        }
        for (int i = 0; i < JF_KSTATE; i++) c->jf_kst_h[i * nf + f] = s[i];
      }
    }
  } else {
    if (par.mode == JF_LOWPASS)
      if (int rc = dev_alloc(c, c->jf_ring, JF_TAPS * (nf ? nf : 1) * B)) return rc;
    if (par.mode == JF_KALMAN)
      if (int rc = dev_alloc(c, c->jf_kst, JF_KSTATE * (nf ? nf : 1) * B)) return rc;
    const size_t blk = sizeof(float) * (size_t) n_rows * B;
    Part p[3] = { { joint_position, blk, 0 }, { joint_velocity, joint_velocity ? blk : 0, 0 }, { joint_effort, joint_effort ? blk : 0, 0 } };
    int rc = stage_in(c, mem, p, 3);
    if (rc) return rc;
    // four robots per lane (16-byte accesses) where the batch and every block's address allow it
    const bool v4 = c->B % 4 == 0 && ((uintptr_t) p[0].dev | (uintptr_t) p[1].dev | (uintptr_t) p[2].dev | (uintptr_t) joint_position_out) % 16 == 0;
    // (64k robots, 12 chain rows, one box: low-pass 11.7 / 12.8 / 9.9 us for 1 / 2 / 4 robots per lane, Kalman 15.4 / 14.6 / 16.0 us)
    const int V = !v4 ? 1 : par.mode == JF_KALMAN ? 2 : 4;
    auto launch = [&](auto v) {
      constexpr int W = decltype(v)::value;
      k_joint_filter<W><<<dim3((unsigned) ((c->B / W + 255) / 256), (unsigned) n_rows), 256, 0, c->stream>>>(
          par, c->B, (const float *) p[0].dev, (const float *) p[1].dev, (const float *) p[2].dev, joint_position_out, c->jf_ring, c->jf_kst,
          c->jf_head, first, dt);
    };
    if (V == 4) launch(std::integral_constant<int, 4>());
    else if (V == 2) launch(std::integral_constant<int, 2>());
    else launch(std::integral_constant<int, 1>());
    LAUNCHCHK(c);
  }
  c->jf_input = input;
  if (!first && par.mode == JF_LOWPASS) c->jf_head = (c->jf_head + 1) % JF_TAPS;
  c->jf_first = false;
  c->jf_tlast = t;
  return PB_OK;
}

// the joint-state inputs of one message as the kernels take them (LegIn kind 1); forces may be NULL (forward kinematics only)
int leg_in_joints(pb_ctx *c, const char *who, int n_rows, const float *jpos, const float *jeff, const float *forces, int mem, LegIn &in)
{
  if (!c->leg_chain) return fail(c, PB_ERR_STATE, "%s before pb_legodo_set_chain", who);
  if (!jpos) return fail(c, PB_ERR_ARG, "%s: NULL input", who);
  if (n_rows < c->leg_chain_rows) return fail(c, PB_ERR_ARG, "%s: the chain reads joint row %d, the block has %d rows", who, c->leg_chain_rows - 1, n_rows);
  in.kind = 1;
  if (mem == PB_HOST_BROADCAST) {
    // ONE robot's joint state for every filter of the batch: its two body-to-foot transforms are a per-MESSAGE quantity, the
    // same for all filters, so they are formed once, here, with the very leg_fk the kernels run per filter for per-filter
    // joint blocks (rbis_legodo.hpp), and travel as 14 kernel arguments -- not recomputed 65 536 times on the device.
    const LegChain &ch = c->leg_chain_h;
    Pose feet[2];
    for (int side = 0; side < 2; side++) {
      double ang[LEG_MAXJ];
      leg_angles(ch, side, [&](int j) {
        const int r = ch.row[side][j];  // (0 for the slots the chain does not use: leg_fk skips them)
        return (double) (jeff ? torque_adjust(jpos[r], jeff[r], ch.gain[side][j]) : jpos[r]);
      }, ang);
      leg_fk(ch, side, ang, [&](int j, int f) { return ch.rec[side][j][f]; }, feet[side]);
    }
    for (int side = 0; side < 2; side++) {
      for (int i = 0; i < 3; i++) in.v[7 * side + i] = feet[side].t[i];
      for (int i = 0; i < 4; i++) in.v[7 * side + 3 + i] = feet[side].q[i];
    }
    if (forces) { in.v[14] = forces[0]; in.v[15] = forces[1]; }
    in.kind = 0;
    in.bcast = 1;
    return PB_OK;
  }
  const size_t blk = sizeof(float) * (size_t) n_rows * c->B;
  Part p[3] = { { jpos, blk, 0 }, { jeff, jeff ? blk : 0, 0 }, { forces, forces ? sizeof(float) * 2 * (size_t) c->B : 0, 0 } };
  int rc = stage_in(c, mem, p, 3);
  if (rc) return rc;
  in.jpos = (const float *) p[0].dev;
  in.jeff = (const float *) p[1].dev;
  in.jforces = (const float *) p[2].dev;
  return PB_OK;
}

// the foot-pose inputs of one message (LegIn kind 0): one robot's poses for every filter travel as kernel arguments, no device block
static int leg_in_feet(pb_ctx *c, const double *feet, const double *forces, int mem, LegIn &in)
{
  if (mem == PB_HOST_BROADCAST) {
    memcpy(in.v, feet, sizeof(double) * 14);
    in.v[14] = forces[0];
    in.v[15] = forces[1];
    in.bcast = 1;
    return PB_OK;
  }
  Part p[2] = { { feet, sizeof(double) * 14 * c->B, 0 }, { forces, sizeof(double) * 2 * c->B, 0 } };
  int rc = stage_in(c, mem, p, 2);
  if (rc) return rc;
  in.feet = (const double *) p[0].dev;
  in.forces = (const double *) p[1].dev;
  return PB_OK;
}

// what the context adds to the inputs of an odometry launch: the controller's contact counts, the call's message times, and the
// measurement mode with the two noises of this call
static LegMeasPar leg_complete(pb_ctx *c, LegIn &in, const LegMsgTimes &mt, double r_vxyz, double r_vxyz_uncertain)
{
  if (c->leg_nc_dev) in.ncontacts = c->leg_nc;
  in.nc[0] = c->leg_nc_h[0];
  in.nc[1] = c->leg_nc_h[1];
  in.utimes = mt.utimes;
  in.valid = mt.valid;
  LegMeasPar mp = c->leg_meas;
  mp.r_v2 = r_vxyz * r_vxyz;                            // bot_sq (rbis_legodo_common.cpp:40-43)
  mp.r_v2_uncertain = r_vxyz_uncertain * r_vxyz_uncertain;
  return mp;
}

// the IMU block of a call (imu_in) for the odometry kernel, which runs the IMU step ahead of itself
static LegAhead leg_ahead(const StepBcast &bc, const double *d_imu)
{
  LegAhead ah;
  ah.on = 1;
  ah.bcast = bc.on & 1;
  memcpy(ah.v, bc.imu, sizeof(ah.v));
  ah.imu = d_imu;
  return ah;
}

// the odometry kernel.  split: two waves per 64 robots, one leg's forward kinematics each (per-filter joint blocks)
static int legodo_kernel(pb_ctx *c, bool split, const LegIn &in, const LegAhead &ah, int64_t utime, int zero_delta, const LegMeasPar &mp,
                         double *delta_out, double *status_out, double *lo_out, uint8_t *mask_out, double *pos_out, uint8_t *pos_ok_out)
{
#define LEGODO_ARGS c->st, c->legd, c->legi, c->stride, c->B, utime, c->leg_par, in, c->leg_chain, ah, zero_delta, mp, delta_out, status_out, lo_out, mask_out, pos_out, pos_ok_out, c->k
  const LegParRows rows{ c->leg_blk, c->stride };
  with_ns(c->ns, [&](auto NS) {
    if (c->leg_blk_on) {  // per-filter noises and contact thresholds (pb_legodo_set_param_block): the sibling kernel
      if (split) k_odo_legpar<decltype(NS)::value, true><<<nblk(c->B), 128, 0, c->stream>>>(LEGODO_ARGS, rows);
      else k_odo_legpar<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(LEGODO_ARGS, rows);
    } else if (split) k_legodo<decltype(NS)::value, true><<<nblk(c->B), 128, 0, c->stream>>>(LEGODO_ARGS);
    else k_legodo<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(LEGODO_ARGS);
  });
#undef LEGODO_ARGS
  LAUNCHCHK(c);
  return PB_OK;
}

static int legodo_launch(pb_ctx *c, LegIn &in, const LegMsgTimes &mt, const double *imu_block, int imu_mem, int64_t utime, int zero_delta, double r_vxyz,
                         double r_vxyz_uncertain, double *delta_out, double *status_out, double *lo_out, uint8_t *mask_out,
                         double *pos_out = nullptr, uint8_t *pos_ok_out = nullptr)
{
  LegAhead ah;
  if (imu_block) {
    StepBcast bc;
    Part p[1];
    if (int rc = imu_in(c, imu_block, imu_mem, bc, p)) return rc;
    ah = leg_ahead(bc, (const double *) p[0].dev);
  }
  const LegMeasPar mp = leg_complete(c, in, mt, r_vxyz, r_vxyz_uncertain);
  // the world constraint (the transition foot's world position) is tracked from the first call that asks for the position
  if (pos_out != nullptr) c->leg_par.world_constraint = 1;
  return legodo_kernel(c, in.kind == 1, in, ah, utime, zero_delta, mp, delta_out, status_out, lo_out, mask_out, pos_out, pos_ok_out);
}

static int legodo_update_impl(pb_ctx *c, const LegMsgTimes &mt, const double *imu_block, int imu_mem, bool ahead, int64_t utime, const double *feet,
                              const double *forces, int mem, int zero_delta, double r_vxyz, double r_vxyz_uncertain,
                              double *delta_out, double *status_out, double *lo_out, uint8_t *mask_out)
{
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_update before pb_legodo_init");
  if (!feet || !forces || (ahead && !imu_block)) return fail(c, PB_ERR_ARG, "pb_legodo_update: NULL input");
  if (ahead && imu_mem == PB_HOST && mem == PB_HOST)
    return fail(c, PB_ERR_ARG, "pb_legodo_update_after_predict: the IMU block and the foot blocks cannot both be PB_HOST");
  LegIn in;
  if (int rc = leg_in_feet(c, feet, forces, mem, in)) return rc;
  return legodo_launch(c, in, mt, ahead ? imu_block : nullptr, imu_mem, utime, zero_delta, r_vxyz, r_vxyz_uncertain, delta_out, status_out,
                       lo_out, mask_out);
}

extern "C" int pb_legodo_update(pb_ctx *c, int64_t utime, const double *feet, const double *forces, int mem, int zero_delta,
                                double r_vxyz, double r_vxyz_uncertain, double *delta_out, double *status_out, double *lo_out,
                                uint8_t *mask_out)
{
  CALL(c, LEG_TIMES | NEEDS_STATE);
  return legodo_update_impl(c, call.times, nullptr, PB_DEVICE, false, utime, feet, forces, mem, zero_delta, r_vxyz, r_vxyz_uncertain, delta_out,
                            status_out, lo_out, mask_out);
}

extern "C" int pb_legodo_update_after_predict(pb_ctx *c, const double *imu_block, int imu_mem, int64_t utime, const double *feet,
                                              const double *forces, int mem, int zero_delta, double r_vxyz, double r_vxyz_uncertain,
                                              double *delta_out, double *status_out, double *lo_out, uint8_t *mask_out)
{
  CALL(c, LEG_TIMES | NEEDS_STATE);
  return legodo_update_impl(c, call.times, imu_block, imu_mem, true, utime, feet, forces, mem, zero_delta, r_vxyz, r_vxyz_uncertain, delta_out,
                            status_out, lo_out, mask_out);
}

extern "C" int pb_legodo_update_joints(pb_ctx *c, const double *imu_block, int imu_mem, int64_t utime, int n_rows,
                                       const float *joint_position, const float *joint_effort, const float *forces, int mem,
                                       int zero_delta, double r_vxyz, double r_vxyz_uncertain, double *delta_out, double *status_out,
                                       double *lo_out, uint8_t *mask_out, double *position_out, uint8_t *position_status_out)
{
  CALL(c, LEG_TIMES | NEEDS_STATE);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_update_joints before pb_legodo_init");
  if (!forces) return fail(c, PB_ERR_ARG, "pb_legodo_update_joints: NULL input");
  if (imu_block && imu_mem == PB_HOST && mem == PB_HOST)
    return fail(c, PB_ERR_ARG, "pb_legodo_update_joints: the IMU block and the joint blocks cannot both be PB_HOST");
  LegIn in;
  int rc = leg_in_joints(c, "pb_legodo_update_joints", n_rows, joint_position, joint_effort, forces, mem, in);
  if (rc) return rc;
  return legodo_launch(c, in, call.times, imu_block, imu_mem, utime, zero_delta, r_vxyz, r_vxyz_uncertain, delta_out, status_out, lo_out, mask_out,
                       position_out, position_status_out);
}

// IMU step + leg odometry + its update (LegOdoCommon's mode, pb_legodo_set_measurement_mode) for one message pair: one kernel where
// the context has it (pbk_step_leg), else the odometry kernel slaved to the state after the IMU step followed by the fused step
// (lin_rate: two launches) or by the process step and the indexed update(s) (the six-row modes); same results to rounding
static int step_leg_impl(pb_ctx *c, LegIn &in, const LegMsgTimes &mt, const double *imu_block, int imu_mem, const double q[4], int64_t utime, double r_vxyz,
                         double r_vxyz_uncertain, double *lo_out, uint8_t *mask_out)
{
  StepBcast bc;
  Part pi[1];
  if (int rc = imu_in(c, imu_block, imu_mem, bc, pi)) return rc;
  const double *d_imu = (const double *) pi[0].dev;
  const LegMeasPar mp = leg_complete(c, in, mt, r_vxyz, r_vxyz_uncertain);
  if (mp.mode == 2) c->leg_par.world_constraint = 1;    // the measured position IS leg_estimate's world constraint, tracked from here on
  int rc = pbk_step_leg(c, d_imu, &bc, q, in, utime, mp, lo_out, mask_out);
  if (rc >= 0) return rc;
  const int rows = mp.mode == 0 ? 6 : 12;
  if (lo_out == nullptr) {  // the measurement has to pass through memory between the kernels
    const size_t B = (size_t) c->B;   // [12][B] doubles and [2][B] mask bytes behind them
    if ((rc = dev_alloc(c, c->leg_lo, 12 * B + (2 * B + 7) / 8))) return rc;
    lo_out = c->leg_lo;
    mask_out = (uint8_t *) (c->leg_lo + (size_t) rows * c->B);
  }
  // (one wave per 64 robots here, also for per-filter joint blocks)
  rc = legodo_kernel(c, false, in, leg_ahead(bc, d_imu), utime, 0, mp, nullptr, nullptr, lo_out, mask_out, nullptr, nullptr);
  if (rc) return rc;
  if (mp.mode == 0) return pbk_step(c, true, d_imu, lo_out, mask_out, q, &bc);
  rc = pbk_step(c, false, d_imu, nullptr, nullptr, q, &bc);
  if (rc) return rc;
  static const int idx_lr[6] = { 3, 4, 5, 0, 1, 2 }, idx_pv[6] = { 9, 10, 11, 3, 4, 5 }, idx_v[3] = { 3, 4, 5 };
  const size_t B = (size_t) c->B;
  const int slot = pb_head_slot(c);  // a checkpointed step: the update(s) land in the same slot
  if (slot >= 0) c->out_slot = slot;
  rc = pbk_update_common(c, 6, mp.mode == 1 ? idx_lr : idx_pv, lo_out, lo_out + 6 * B, PB_R_DIAG, nullptr, false, mask_out, PB_DEVICE);
  if (rc || mp.mode == 1) return rc;
  const int slot2 = pb_head_slot(c);
  if (slot2 >= 0) c->out_slot = slot2;
  return pbk_update_common(c, 3, idx_v, lo_out + 3 * B, lo_out + 9 * B, PB_R_DIAG, nullptr, false, mask_out + B, PB_DEVICE);
}

extern "C" int pb_step_legodo_joints(pb_ctx *c, const double *imu_block, int imu_mem, const double q[4], int64_t utime, int n_rows,
                                     const float *joint_position, const float *joint_effort, const float *forces, int mem,
                                     double r_vxyz, double r_vxyz_uncertain, double *lo_block_out, uint8_t *mask_out)
{
  CALL(c, IMU_STEP | LEG_TIMES | PRED_REFUSE | NEEDS_STATE);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_step_legodo_joints before pb_legodo_init");
  if (!imu_block || !q || !forces || (lo_block_out && !mask_out)) return fail(c, PB_ERR_ARG, "pb_step_legodo_joints: NULL input");
  if (imu_mem == PB_HOST && mem == PB_HOST)
    return fail(c, PB_ERR_ARG, "pb_step_legodo_joints: the IMU block and the joint blocks cannot both be PB_HOST");
  LegIn in;
  int rc = leg_in_joints(c, "pb_step_legodo_joints", n_rows, joint_position, joint_effort, forces, mem, in);
  if (rc) return rc;
  return step_leg_impl(c, in, call.times, imu_block, imu_mem, q, utime, r_vxyz, r_vxyz_uncertain, lo_block_out, mask_out);
}

extern "C" int pb_step_legodo_feet(pb_ctx *c, const double *imu_block, int imu_mem, const double q[4], int64_t utime, const double *feet,
                                   const double *forces, int mem, double r_vxyz, double r_vxyz_uncertain, double *lo_block_out,
                                   uint8_t *mask_out)
{
  CALL(c, IMU_STEP | LEG_TIMES | PRED_REFUSE | NEEDS_STATE);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_step_legodo_feet before pb_legodo_init");
  if (!imu_block || !q || !feet || !forces || (lo_block_out && !mask_out)) return fail(c, PB_ERR_ARG, "pb_step_legodo_feet: NULL input");
  if (imu_mem == PB_HOST && mem == PB_HOST)
    return fail(c, PB_ERR_ARG, "pb_step_legodo_feet: the IMU block and the foot blocks cannot both be PB_HOST");
  LegIn in;
  if (int rc = leg_in_feet(c, feet, forces, mem, in)) return rc;
  return step_leg_impl(c, in, call.times, imu_block, imu_mem, q, utime, r_vxyz, r_vxyz_uncertain, lo_block_out, mask_out);
}

extern "C" int pb_legodo_fk(pb_ctx *c, int n_rows, const float *joint_position, const float *joint_effort, int mem, double *feet_out)
{
  CALL(c, 0);
  if (!feet_out) return fail(c, PB_ERR_ARG, "pb_legodo_fk: NULL output");
  LegIn in;
  int rc = leg_in_joints(c, "pb_legodo_fk", n_rows, joint_position, joint_effort, nullptr, mem, in);
  if (rc) return rc;
  k_leg_fk<<<nblk(c->B), 64, 0, c->stream>>>(in, c->leg_chain, c->B, feet_out);
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_legodo_get(pb_ctx *c, int filter, double odom_to_body[7], int64_t info[4])
{
  CALL(c, 0);
  if (!c->legd) return fail(c, PB_ERR_STATE, "pb_legodo_get before pb_legodo_init");
  if (filter < 0 || filter >= c->B || !odom_to_body || !info) return fail(c, PB_ERR_ARG, "pb_legodo_get: bad argument");
  return get_small(c, odom_to_body, 7, info, [&](double *dp, int64_t *di) -> int {
    k_legodo_get<<<1, 1, 0, c->stream>>>(c->legd, c->legi, c->stride, filter, dp, di);
    LAUNCHCHK(c);
    return PB_OK;
  });
}
