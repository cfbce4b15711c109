// abi_recorder.cpp -- a recording stand-in for the C ABI functions (include/pronto_batch.h) that the estimator core and the
// update objects of pronto_amd/csrc/mav_state_est.hpp, and the sensor handlers of mav_state_est_batch.hpp, call.  No HIP, no device: every call appends ONE line to stdout -- the
// function's name, every scalar argument, index lists in full -- so that a trace is the list of decisions the estimator took.
// Pointer arguments are logged by kind, never as an address:
//     NULL | host:<FNV-1a of exactly the bytes the real call would read> | dev#<ordinal of its pb_malloc>+<byte offset> | out
// ("out" = a host buffer the call fills).  The recorder models only what the estimator reads back: pb_head_slot (follows
// pb_set_output_slot / every update / pb_state_restore / pb_reset as the library does), pb_batch, pb_n_states, pb_mask_count (an
// answer the driver sets), pb_get_head and the other host outputs a handler reads (pb_imu_notch / _counts with PB_HOST, pb_joint_filter
// for a broadcast message, pb_score_get / _last / _best): a deterministic pattern.  rec_fail_call() makes the k-th call of a named function
// return PB_ERR_HIP, which is how tests/cpp/estimator_trace.cpp reaches the error paths.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/pronto_batch.h"
#include "abi_recorder.h"

struct pb_ctx {
  int n, B, nhist = 0;
  int out_slot = -1, pred_slot = -1, head_slot = -1;
  int gets = 0, fills = 0;
};

namespace {
struct DevBlock { const char *base; size_t bytes; int ordinal; };
// (a block nobody pb_free'd shows in the trace as a missing pb_free line; its stand-in memory goes back at exit, so that a sanitized build
// can record such a trace)
struct DevBlocks : std::vector<DevBlock> {
  ~DevBlocks() { for (const DevBlock &d : *this) free((void *) d.base); }
} g_blocks;
int g_ordinal = 0, g_mask_count = 1;
std::map<std::string, int> g_fail_in;   // function -> calls left until the failing one
std::string g_error = "no error";

std::string host(const void *p, size_t bytes)
{
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < bytes; i++) h = (h ^ ((const unsigned char *) p)[i]) * 1099511628211ULL;
  char b[40];
  snprintf(b, sizeof b, "host:%016" PRIx64, h);
  return b;
}
// a pointer that is host or device memory by `mem`; a pb_malloc'ed block is recognised whatever `mem` says
std::string ptr(const void *p, int mem, size_t host_bytes)
{
  if (p == nullptr) return "NULL";
  for (const DevBlock &d : g_blocks)
    if ((const char *) p >= d.base && (const char *) p < d.base + d.bytes) {
      char b[48];
      snprintf(b, sizeof b, "dev#%d+%zu", d.ordinal, (size_t) ((const char *) p - d.base));
      return b;
    }
  return mem == PB_DEVICE ? std::string("dev:foreign") : host(p, host_bytes);
}
std::string dbl(const pb_ctx *c, const double *p, int mem, int rows) { return ptr(p, mem, sizeof(double) * rows * (mem == PB_HOST_BROADCAST ? 1 : c->B)); }
std::string msk(const pb_ctx *c, const uint8_t *p, int mem) { return ptr(p, mem, (size_t) c->B); }
// R of an indexed update: the broadcast diagonal is host double[m] wherever the measurement lives
std::string cov(const pb_ctx *c, const double *R, int r_kind, int m, int mem)
{
  if (r_kind == PB_R_DIAG_BROADCAST) return ptr(R, PB_HOST_BROADCAST, sizeof(double) * m);
  return dbl(c, R, mem, r_kind == PB_R_FULL ? m * m : m);
}
std::string list(const int *idx, int m)
{
  std::string s = "[";
  for (int i = 0; i < m; i++) s += (i ? "," : "") + std::to_string(idx[i]);
  return s + "]";
}
const char *out(const void *p) { return p ? "out" : "NULL"; }
std::string flt(const pb_ctx *c, const float *p, int mem, int rows) { return ptr(p, mem, sizeof(float) * rows * (mem == PB_HOST_BROADCAST ? 1 : c->B)); }
// an output that is a pb_malloc'ed block (logged as such) or a host buffer the call fills
std::string dst(const void *p) { return p == nullptr ? "NULL" : ptr(p, PB_DEVICE, 0) == "dev:foreign" ? "out" : ptr(p, PB_DEVICE, 0); }
// the pattern of a filled host output: differs from call to call and from entry to entry
template <class T> void pattern(pb_ctx *c, T *o, size_t k, const int32_t *only_where = nullptr, size_t B = 1)
{
  const double base = 0.5 * ++c->fills;
  for (size_t i = 0; o && i < k; i++)
    if (only_where == nullptr || only_where[i % B] > 0) o[i] = (T) (base + 0.03125 * (double) i);
}

// logs the line; returns PB_ERR_HIP when this call is the one rec_fail_call() named
int call(const char *fn, const char *fmt, ...)
{
  printf("%s", fn);
  va_list ap;
  va_start(ap, fmt);
  vprintf(fmt, ap);
  va_end(ap);
  auto it = g_fail_in.find(fn);
  if (it != g_fail_in.end() && --it->second == 0) {
    g_fail_in.erase(it);
    g_error = std::string("injected failure in ") + fn;
    printf(" -> PB_ERR_HIP\n");
    return PB_ERR_HIP;
  }
  printf("\n");
  return PB_OK;
}
// what every update does to the slots: the posterior lands in the pending output slot (else the context's own array)
int updated(pb_ctx *c, int rc)
{
  c->pred_slot = -1;
  if (rc == PB_OK) c->head_slot = c->out_slot;
  c->out_slot = -1;
  return rc;
}
}  // namespace

void rec_fail_call(const char *fn, int kth) { g_fail_in[fn] = kth; }
void rec_set_mask_count(int count) { g_mask_count = count; }
std::string rec_ptr(const void *p, int mem, size_t host_bytes) { return ptr(p, mem, host_bytes); }

#define S(x) (x).c_str()

extern "C" {
int pb_create(pb_ctx **o, int n_states, int batch, int device, int n_snapshots)
{
  const int rc = call("pb_create", " n=%d B=%d device=%d snapshots=%d", n_states, batch, device, n_snapshots);
  if (rc != PB_OK) return rc;
  *o = new pb_ctx;
  (*o)->n = n_states;
  (*o)->B = batch;
  return PB_OK;
}
int pb_destroy(pb_ctx *c)
{
  call("pb_destroy", "");
  delete c;
  return PB_OK;
}
const char *pb_last_error(const pb_ctx *)
{
  call("pb_last_error", "");
  return g_error.c_str();
}
int pb_n_states(const pb_ctx *c) { call("pb_n_states", " -> %d", c->n); return c->n; }
int pb_batch(const pb_ctx *c) { call("pb_batch", " -> %d", c->B); return c->B; }
int pb_malloc(pb_ctx *, uint64_t bytes, void **dev_ptr)
{
  const int rc = call("pb_malloc", " bytes=%" PRIu64 " -> dev#%d", bytes, g_ordinal);
  if (rc != PB_OK) return rc;
  *dev_ptr = calloc(1, bytes ? bytes : 1);
  g_blocks.push_back({ (const char *) *dev_ptr, (size_t) bytes, g_ordinal++ });
  return PB_OK;
}
int pb_free(pb_ctx *, void *p)
{
  const int rc = call("pb_free", " %s", S(ptr(p, PB_DEVICE, 0)));
  for (size_t i = 0; i < g_blocks.size(); i++)
    if (g_blocks[i].base == (const char *) p) {
      g_blocks.erase(g_blocks.begin() + i);
      free(p);
      break;
    }
  return rc;
}
int pb_set_utime(pb_ctx *, int64_t utime) { return call("pb_set_utime", " utime=%" PRId64, utime); }
int pb_set_imu_valid(pb_ctx *, const uint8_t *valid_dev) { return call("pb_set_imu_valid", " valid=%s", S(ptr(valid_dev, PB_DEVICE, 0))); }
int pb_mask_count(pb_ctx *, const uint8_t *mask_dev, int *count_out)
{
  const int rc = call("pb_mask_count", " mask=%s -> %d", S(ptr(mask_dev, PB_DEVICE, 0)), g_mask_count);
  if (rc == PB_OK) *count_out = g_mask_count;
  return rc;
}

int pb_reset(pb_ctx *c, const double *vec, const double *quat, const double *P, int broadcast, int mem)
{
  const int m = broadcast ? PB_HOST_BROADCAST : mem;
  const int rc = call("pb_reset", " vec=%s quat=%s cov=%s broadcast=%d mem=%d", S(dbl(c, vec, m, c->n)), S(dbl(c, quat, m, 4)),
                      S(dbl(c, P, m, c->n * c->n)), broadcast, mem);
  c->out_slot = -1;
  return updated(c, rc);
}
int pb_get_head(pb_ctx *c, int first, int count, double *vec, double *quat, double *P, double *ll, int mem)
{
  const int rc = call("pb_get_head", " first=%d count=%d vec=%s quat=%s cov=%s ll=%s mem=%d", first, count, out(vec), out(quat), out(P), out(ll), mem);
  if (rc != PB_OK) return rc;
  const double base = ++c->gets;   // a pattern that differs from call to call and from entry to entry
  for (int i = 0; vec && i < c->n * count; i++) vec[i] = base + 0.25 * i;
  for (int i = 0; quat && i < 4 * count; i++) quat[i] = base + 0.125 * i;
  for (int i = 0; P && i < c->n * c->n * count; i++) P[i] = base + 0.0625 * i;
  for (int i = 0; ll && i < count; i++) ll[i] = -base - i;
  return PB_OK;
}
int pb_set_head(pb_ctx *c, const double *vec, const double *quat, const double *P, const double *ll, int mem)
{
  return updated(c, call("pb_set_head", " vec=%s quat=%s cov=%s ll=%s mem=%d", S(dbl(c, vec, mem, c->n)), S(dbl(c, quat, mem, 4)),
                         S(dbl(c, P, mem, c->n * c->n)), S(dbl(c, ll, mem, 1)), mem));
}
int pb_predict(pb_ctx *c, const double *imu, const double q[4], int mem)
{
  return updated(c, call("pb_predict", " imu=%s q=%s mem=%d", S(dbl(c, imu, mem, 7)), S(host(q, 4 * sizeof(double))), mem));
}
int pb_update_indexed(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int r_kind, const uint8_t *mask, int mem)
{
  return updated(c, call("pb_update_indexed", " m=%d idx=%s z=%s R=%s r_kind=%d mask=%s mem=%d", m, S(list(idx, m)), S(dbl(c, z, mem, m)),
                         S(cov(c, R, r_kind, m, mem)), r_kind, S(msk(c, mask, mem)), mem));
}
int pb_update_indexed_orient(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int r_kind, const double *quat,
                             const uint8_t *mask, int mem)
{
  return updated(c, call("pb_update_indexed_orient", " m=%d idx=%s z=%s R=%s r_kind=%d quat=%s mask=%s mem=%d", m, S(list(idx, m)),
                         S(dbl(c, z, mem, m)), S(cov(c, R, r_kind, m, mem)), r_kind, S(dbl(c, quat, mem, 4)), S(msk(c, mask, mem)), mem));
}
int pb_step_legodo(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], int mem)
{
  return updated(c, call("pb_step_legodo", " imu=%s lo=%s mask=%s q=%s mem=%d", S(dbl(c, imu, mem, 7)), S(dbl(c, lo, mem, 6)),
                         S(msk(c, mask, mem)), S(host(q, 4 * sizeof(double))), mem));
}
int pb_step_legodo_split(pb_ctx *c, const double *imu, int imu_mem, const double *lo, const uint8_t *mask, int lo_mem, const double q[4])
{
  return updated(c, call("pb_step_legodo_split", " imu=%s imu_mem=%d lo=%s mask=%s lo_mem=%d q=%s", S(dbl(c, imu, imu_mem, 7)), imu_mem,
                         S(dbl(c, lo, lo_mem, 6)), S(msk(c, mask, lo_mem)), lo_mem, S(host(q, 4 * sizeof(double)))));
}
int pb_step_legodo_correct(pb_ctx *c, const double *imu, const double *lo, const uint8_t *mask, const double q[4], int mem, int kind,
                           const double *z2, const double *R2, int r_kind2, const double *quat2, const uint8_t *mask2, int mem2)
{
  const int m2 = kind == PB_CORR_POS_ORIENT ? 6 : 4;
  return updated(c, call("pb_step_legodo_correct", " imu=%s lo=%s mask=%s q=%s mem=%d kind=%d z2=%s R2=%s r_kind2=%d quat2=%s mask2=%s mem2=%d",
                         S(dbl(c, imu, mem, 7)), S(dbl(c, lo, mem, 6)), S(msk(c, mask, mem)), S(host(q, 4 * sizeof(double))), mem, kind,
                         S(dbl(c, z2, mem2, m2)), S(cov(c, R2, r_kind2, m2, mem2)), r_kind2, S(dbl(c, quat2, mem2, 4)), S(msk(c, mask2, mem2)), mem2));
}
int pb_yawlock_set_standing(pb_ctx *c, const uint8_t *standing, int mem)
{
  return call("pb_yawlock_set_standing", " standing=%s mem=%d", S(ptr(standing, mem, mem == PB_HOST_BROADCAST ? 1 : (size_t) c->B)), mem);
}
int pb_yawlock_set_gyro(pb_ctx *c, const double *gz, int mem) { return call("pb_yawlock_set_gyro", " gyro_z=%s mem=%d", S(dbl(c, gz, mem, 1)), mem); }
int pb_step_yawlock_joints(pb_ctx *c, int64_t utime, const int64_t *utimes, const uint8_t *valid, int n_rows, const float *joints, int mem,
                           double *z_out, double *quat_out, uint8_t *mask_out)
{
  const size_t cols = mem == PB_HOST_BROADCAST ? 1 : (size_t) c->B;
  return updated(c, call("pb_step_yawlock_joints", " utime=%" PRId64 " utimes=%s valid=%s n_rows=%d joints=%s mem=%d z_out=%s quat_out=%s mask_out=%s",
                         utime, S(ptr(utimes, mem, sizeof(int64_t) * c->B)), S(msk(c, valid, mem)), n_rows, S(ptr(joints, mem, sizeof(float) * n_rows * cols)),
                         mem, S(ptr(z_out, PB_DEVICE, 0)), S(ptr(quat_out, PB_DEVICE, 0)), S(ptr(mask_out, PB_DEVICE, 0))));
}

int pb_history_reserve(pb_ctx *c, int n_slots)
{
  const int rc = call("pb_history_reserve", " slots=%d", n_slots);
  if (rc == PB_OK) c->nhist = n_slots;
  return rc;
}
int pb_set_output_slot(pb_ctx *c, int slot)
{
  const int rc = call("pb_set_output_slot", " slot=%d", slot);
  if (rc == PB_OK) c->out_slot = slot;
  return rc;
}
int pb_set_pred_slot(pb_ctx *c, int slot)
{
  const int rc = call("pb_set_pred_slot", " slot=%d", slot);
  if (rc == PB_OK) c->pred_slot = slot;
  return rc;
}
int pb_head_slot(const pb_ctx *c) { call("pb_head_slot", " -> %d", c->head_slot); return c->head_slot; }
int pb_state_save(pb_ctx *, int slot) { return call("pb_state_save", " slot=%d", slot); }
int pb_state_restore(pb_ctx *c, int slot)
{
  const int rc = call("pb_state_restore", " slot=%d", slot);
  if (rc == PB_OK) c->head_slot = c->out_slot = -1;
  return rc;
}
int pb_snapshot(pb_ctx *, int slot) { return call("pb_snapshot", " slot=%d", slot); }
int pb_snapshot_from_slot(pb_ctx *, int slot, int checkpoint_slot) { return call("pb_snapshot_from_slot", " slot=%d checkpoint=%d", slot, checkpoint_slot); }
int pb_smooth_step(pb_ctx *, int next_pred, int next, int cur, int o, double dt)
{
  return call("pb_smooth_step", " next_pred=%d next=%d cur=%d out=%d dt=%.17g", next_pred, next, cur, o, dt);
}
int pb_smooth_step_masked(pb_ctx *c, int next_pred, int next, int cur, int o, double dt, const uint8_t *step, int mem)
{
  return call("pb_smooth_step_masked", " next_pred=%d next=%d cur=%d out=%d dt=%.17g step=%s mem=%d", next_pred, next, cur, o, dt, S(msk(c, step, mem)), mem);
}
// ---- what the sensor handlers (mav_state_est_batch.hpp) call ----
int pb_memcpy_h2d(pb_ctx *, void *d, const void *src, uint64_t bytes)
{
  return call("pb_memcpy_h2d", " dst=%s src=%s bytes=%" PRIu64, S(dst(d)), S(ptr(src, PB_HOST, (size_t) bytes)), bytes);
}
int pb_compose_delta(pb_ctx *c, int slot, const double *t, const double *q, double *z_out, double *quat_out, int mem)
{
  return call("pb_compose_delta", " slot=%d t=%s q=%s z_out=%s quat_out=%s mem=%d", slot, S(dbl(c, t, mem, 3)), S(dbl(c, q, mem, 4)), S(dst(z_out)),
              S(dst(quat_out)), mem);
}
int pb_imu_notch_init(pb_ctx *, double f, double fs) { return call("pb_imu_notch_init", " notch_freq=%.17g fs=%.17g", f, fs); }
int pb_imu_notch(pb_ctx *c, int n_packets, const double *acc, double *o, int mem)
{
  const int rc = call("pb_imu_notch", " n_packets=%d accel=%s out=%s mem=%d", n_packets, S(dbl(c, acc, mem, 3 * n_packets)), S(dst(o)), mem);
  if (rc == PB_OK && mem == PB_HOST) pattern(c, o, (size_t) 3 * c->B);
  return rc;
}
int pb_imu_notch_counts(pb_ctx *c, int max_packets, const int32_t *counts, const double *acc, double *o, int mem)
{
  const int rc = call("pb_imu_notch_counts", " max_packets=%d counts=%s accel=%s out=%s mem=%d", max_packets, S(ptr(counts, mem, sizeof(int32_t) * c->B)),
                      S(dbl(c, acc, mem, 3 * max_packets)), S(dst(o)), mem);
  if (rc == PB_OK && mem == PB_HOST) pattern(c, o, (size_t) 3 * c->B, counts, (size_t) c->B);   // a filter without a new packet is not written
  return rc;
}
int pb_ins_body_block(pb_ctx *c, const double *gyro, const double *accel, const double *raw_dt, const int64_t *utimes, int64_t utime, const uint8_t *valid,
                      const double rot_quat[4], const double trans_vec[3], double dt_default, int dt_from_utimes, int mem, double *o, uint8_t *valid_out)
{
  return call("pb_ins_body_block", " gyro=%s accel=%s raw_dt=%s utimes=%s utime=%" PRId64 " valid=%s rot=%s trans=%s dt=%.17g dt_from_utimes=%d mem=%d out=%s valid_out=%s",
              S(dbl(c, gyro, mem, 3)), S(dbl(c, accel, mem, 3)), S(dbl(c, raw_dt, mem, 1)), S(ptr(utimes, mem, sizeof(int64_t) * c->B)), utime, S(msk(c, valid, mem)),
              S(host(rot_quat, 4 * sizeof(double))), trans_vec ? S(host(trans_vec, 3 * sizeof(double))) : "NULL", dt_default, dt_from_utimes, mem, S(dst(o)),
              S(dst(valid_out)));
}
int pb_legodo_init(pb_ctx *, double lt, double ht, int64_t ld, int64_t hd, int fce)
{
  return call("pb_legodo_init", " low=%.17g high=%.17g low_delay=%" PRId64 " high_delay=%" PRId64 " filter_contact_events=%d", lt, ht, ld, hd, fce);
}
int pb_legodo_set_contact_mode(pb_ctx *, int standing, double total_force, double level, int ctrl)
{
  return call("pb_legodo_set_contact_mode", " standing=%d total_force=%.17g level=%.17g use_controller_input=%d", standing, total_force, level, ctrl);
}
int pb_legodo_set_zero_initial_velocity(pb_ctx *, int ticks) { return call("pb_legodo_set_zero_initial_velocity", " ticks=%d", ticks); }
int pb_legodo_set_measurement_mode(pb_ctx *, int mode, double r_xyz, double r_vang, double r_vang_u)
{
  return call("pb_legodo_set_measurement_mode", " mode=%d r_xyz=%.17g r_vang=%.17g r_vang_uncertain=%.17g", mode, r_xyz, r_vang, r_vang_u);
}
int pb_legodo_set_param_block(pb_ctx *c, const double *block, int mem) { return call("pb_legodo_set_param_block", " block=%s mem=%d", S(dbl(c, block, mem, PB_LEGPAR_ROWS)), mem); }
int pb_legodo_set_control_contacts(pb_ctx *c, const int32_t *n, int mem)
{
  return call("pb_legodo_set_control_contacts", " n_contacts=%s mem=%d", S(ptr(n, mem, sizeof(int32_t) * 2 * (mem == PB_HOST_BROADCAST ? 1 : c->B))), mem);
}
int pb_legodo_set_message_times(pb_ctx *c, const int64_t *utimes, const uint8_t *valid, int mem)
{
  return call("pb_legodo_set_message_times", " utimes=%s valid=%s mem=%d", S(ptr(utimes, mem, sizeof(int64_t) * c->B)), S(msk(c, valid, mem)), mem);
}
int pb_legodo_set_chain(pb_ctx *, int n_left, int n_right, const int *type, const int *row, const double *org, const double *axis, const float *gain)
{
  const int k = n_left + n_right;
  return call("pb_legodo_set_chain", " n_left=%d n_right=%d type=%s row=%s origin=%s axis=%s gain=%s", n_left, n_right, S(list(type, k)), S(list(row, k)),
              S(host(org, sizeof(double) * 6 * k)), S(host(axis, sizeof(double) * 3 * k)), gain ? S(host(gain, sizeof(float) * k)) : "NULL");
}
int pb_legodo_update(pb_ctx *c, int64_t utime, const double *feet, const double *forces, int mem, int zero_delta, double r, double ru, double *o_delta,
                     double *o_status, double *lo, uint8_t *mask)
{
  return call("pb_legodo_update", " utime=%" PRId64 " feet=%s forces=%s mem=%d zero_delta=%d r=%.17g ru=%.17g delta_out=%s status_out=%s lo_out=%s mask_out=%s", utime,
              S(dbl(c, feet, mem, 14)), S(dbl(c, forces, mem, 2)), mem, zero_delta, r, ru, S(dst(o_delta)), S(dst(o_status)), S(dst(lo)), S(dst(mask)));
}
int pb_legodo_update_after_predict(pb_ctx *c, const double *imu, int imu_mem, int64_t utime, const double *feet, const double *forces, int mem, int zero_delta,
                                   double r, double ru, double *o_delta, double *o_status, double *lo, uint8_t *mask)
{
  return call("pb_legodo_update_after_predict", " imu=%s imu_mem=%d utime=%" PRId64 " feet=%s forces=%s mem=%d zero_delta=%d r=%.17g ru=%.17g delta_out=%s status_out=%s lo_out=%s mask_out=%s",
              S(dbl(c, imu, imu_mem, 7)), imu_mem, utime, S(dbl(c, feet, mem, 14)), S(dbl(c, forces, mem, 2)), mem, zero_delta, r, ru, S(dst(o_delta)), S(dst(o_status)),
              S(dst(lo)), S(dst(mask)));
}
int pb_legodo_update_joints(pb_ctx *c, const double *imu, int imu_mem, int64_t utime, int n_rows, const float *jp, const float *je, const float *forces, int mem,
                            int zero_delta, double r, double ru, double *o_delta, double *o_status, double *lo, uint8_t *mask, double *o_pos, uint8_t *o_pos_ok)
{
  return call("pb_legodo_update_joints", " imu=%s imu_mem=%d utime=%" PRId64 " n_rows=%d position=%s effort=%s forces=%s mem=%d zero_delta=%d r=%.17g ru=%.17g delta_out=%s status_out=%s lo_out=%s mask_out=%s position_out=%s position_status_out=%s",
              S(dbl(c, imu, imu_mem, 7)), imu_mem, utime, n_rows, S(flt(c, jp, mem, n_rows)), S(flt(c, je, mem, n_rows)), S(flt(c, forces, mem, 2)), mem, zero_delta, r, ru,
              S(dst(o_delta)), S(dst(o_status)), S(dst(lo)), S(dst(mask)), S(dst(o_pos)), S(dst(o_pos_ok)));
}
int pb_step_legodo_joints(pb_ctx *c, const double *imu, int imu_mem, const double q[4], int64_t utime, int n_rows, const float *jp, const float *je,
                          const float *forces, int mem, double r, double ru, double *lo, uint8_t *mask)
{
  return updated(c, call("pb_step_legodo_joints", " imu=%s imu_mem=%d q=%s utime=%" PRId64 " n_rows=%d position=%s effort=%s forces=%s mem=%d r=%.17g ru=%.17g lo_out=%s mask_out=%s",
                         S(dbl(c, imu, imu_mem, 7)), imu_mem, S(host(q, 4 * sizeof(double))), utime, n_rows, S(flt(c, jp, mem, n_rows)), S(flt(c, je, mem, n_rows)),
                         S(flt(c, forces, mem, 2)), mem, r, ru, S(dst(lo)), S(dst(mask))));
}
int pb_step_legodo_feet(pb_ctx *c, const double *imu, int imu_mem, const double q[4], int64_t utime, const double *feet, const double *forces, int mem, double r,
                        double ru, double *lo, uint8_t *mask)
{
  return updated(c, call("pb_step_legodo_feet", " imu=%s imu_mem=%d q=%s utime=%" PRId64 " feet=%s forces=%s mem=%d r=%.17g ru=%.17g lo_out=%s mask_out=%s", S(dbl(c, imu, imu_mem, 7)),
                         imu_mem, S(host(q, 4 * sizeof(double))), utime, S(dbl(c, feet, mem, 14)), S(dbl(c, forces, mem, 2)), mem, r, ru, S(dst(lo)), S(dst(mask))));
}
int pb_joint_filter_init(pb_ctx *, int mode, double pp, double pv, double on)
{
  return call("pb_joint_filter_init", " mode=%d process_noise_pos=%.17g process_noise_vel=%.17g observation_noise=%.17g", mode, pp, pv, on);
}
int pb_joint_filter(pb_ctx *c, int64_t utime, int n_rows, const float *jp, const float *jv, const float *je, int mem, float *o)
{
  const int rc = call("pb_joint_filter", " utime=%" PRId64 " n_rows=%d position=%s velocity=%s effort=%s mem=%d out=%s", utime, n_rows, S(flt(c, jp, mem, n_rows)),
                      S(flt(c, jv, mem, n_rows)), S(flt(c, je, mem, n_rows)), mem, S(dst(o)));
  if (rc == PB_OK && mem == PB_HOST_BROADCAST) pattern(c, o, (size_t) n_rows);   // (per-filter messages are filtered into a device block)
  return rc;
}
int pb_yawlock_init(pb_ctx *, int mode, int period, int slip, double thr, double disable, double r_bias, double r_yaw)
{
  return call("pb_yawlock_init", " mode=%d correction_period=%d yaw_slip_detect=%d threshold=%.17g disable_period=%.17g r_yaw_bias=%.17g r_yaw=%.17g", mode, period, slip, thr,
              disable, r_bias, r_yaw);
}
int pb_score_init(pb_ctx *, double t, double d) { return call("pb_score_init", " time_threshold=%.17g distance_threshold=%.17g", t, d); }
int pb_score_ground_truth(pb_ctx *c, int64_t utime, const int64_t *utimes, const double *pose7, const uint8_t *valid, int slot, int flags, int mem)
{
  return call("pb_score_ground_truth", " utime=%" PRId64 " utimes=%s pose7=%s valid=%s slot=%d flags=%d mem=%d", utime, S(ptr(utimes, mem, sizeof(int64_t) * c->B)),
              S(dbl(c, pose7, mem, 7)), S(msk(c, valid, mem)), slot, flags, mem);
}
int pb_score_get(pb_ctx *c, int first, int count, double *rows_out, int64_t *counts_out, int mem)
{
  const int rc = call("pb_score_get", " first=%d count=%d rows=%s counts=%s mem=%d", first, count, S(dst(rows_out)), S(dst(counts_out)), mem);
  if (rc == PB_OK && mem == PB_HOST) {
    pattern(c, rows_out, (size_t) PB_SCORE_ROWS * count);
    pattern(c, counts_out, (size_t) PB_SCORE_COUNTS * count);
  }
  return rc;
}
// no window yet for the first question, then a window that closes with every second one
int pb_score_last(pb_ctx *c, int filter, int64_t *utime, double o[10])
{
  const int rc = call("pb_score_last", " filter=%d utime=out out=out", filter);
  if (rc != PB_OK) return rc;
  c->gets++;
  *utime = c->gets < 2 ? -2 : 1000 * (int64_t) (c->gets / 2);
  pattern(c, o, 10);
  return PB_OK;
}
int pb_score_best(pb_ctx *c, int metric, int *filter_out, double *value_out)
{
  const int rc = call("pb_score_best", " metric=%d filter=out value=%s", metric, out(value_out));
  if (rc != PB_OK) return rc;
  *filter_out = metric % c->B;
  pattern(c, value_out, value_out ? 1 : 0);
  return PB_OK;
}
}  // extern "C"
