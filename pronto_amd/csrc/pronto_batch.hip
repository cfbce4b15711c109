// pronto_batch.hip -- host side of the C ABI declared in include/pronto_batch.h: the context and its streams, staging, the step and
// update entry points, read-back and diagnostics.  The kernels launched from here are the utility ones (rbis_util_kernels.hpp, included
// by this file only); the step / update / smoother kernels are launched from the pb_*.hip units, and the handler families -- leg
// odometry and joint filters, yaw lock, IMU front end, scorer, checkpoint slots and smoothing -- have their entry points beside their
// kernels (pb_legodo.hip, pb_yawlock.hip, pb_frontend.hip, pb_score.hip, pb_history.hip; pb_ctx.hpp).
// The per-filter arithmetic is rbis_device.hpp.
// There is no CPU path here: without a gfx950 device pb_create fails with PB_ERR_NO_DEVICE.
#include <algorithm>
#include <new>

#include "pb_ctx.hpp"
#include "rbis_util_kernels.hpp"

#define PB_VERSION_STR "pronto_batch 0.3 gfx950"

extern "C" const char *pb_version(void) { return PB_VERSION_STR; }

extern "C" const char *pb_last_error(const pb_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

extern "C" int pb_create(pb_ctx **out, int n_states, int batch, int device, int n_snapshots)
{
  if (!out) return fail(nullptr, PB_ERR_ARG, "pb_create: out is NULL");
  *out = nullptr;
  if (n_states != 15 && n_states != 21) return fail(nullptr, PB_ERR_ARG, "pb_create: n_states must be 15 or 21");
  if (batch <= 0 || n_snapshots < 0) return fail(nullptr, PB_ERR_ARG, "pb_create: bad batch / n_snapshots");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, PB_ERR_NO_DEVICE, "pb_create: no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, PB_ERR_ARG, "pb_create: device %d out of range", device);
  hipDeviceProp_t prop;
  HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, PB_ERR_NO_DEVICE, "pb_create: device %d is %s; kernels are built for gfx950 only", device,
                prop.gcnArchName);
  pb_ctx *c = new (std::nothrow) pb_ctx();
  if (!c) return fail(nullptr, PB_ERR_ARG, "pb_create: out of host memory");
  c->ns = n_states;
  c->B = batch;
  c->dev = device;
  c->nsnap = n_snapshots;
  c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->stride = ((long) batch + 63) / 64 * 64;
  c->nc = (n_states == 15) ? Lay<15>::NC : Lay<21>::NC;
  c->state_doubles = (size_t) c->stride * (size_t) ((n_states == 15) ? Slots<15>::NSLOT : Slots<21>::NSLOT);
  static_assert(Slots<15>::NSLOT == state_slots(15) && Slots<21>::NSLOT == state_slots(21), "pb_policy.hpp: state_slots");
  // which kernels, grids and cache policies this context runs: decided once, here, from the switches as they are NOW (pb_policy.hpp)
  c->policy = make_policy(n_states, batch, (long) c->state_doubles * 8, read_switches());
  c->k.xcd_remap = c->policy.xcd_remap ? 1 : 0;
  // The kernels address the STATE through one buffer descriptor per 64-filter tile (64-bit tile base), so its size is
  // bounded by HBM only; the per-message INPUT blocks ([rows][B], at most 36 rows; pb_update_indexed_wide checks its up to 81 itself)
  // go through one 32-bit-ranged descriptor each, which bounds the batch of one context at 2^32 / (36 * 8) filters.
  if ((unsigned long long) batch * 36ull * 8ull >= (1ull << 32)) {
    delete c;
    return fail(nullptr, PB_ERR_ARG, "pb_create: batch %d too large for one context (input blocks must stay below 4 GiB; "
                "split the batch over several contexts)", batch);
  }
#define CRCHK(call) CRCHK_AS(#call, call)
#define CRCHK_AS(what, call)                                                                        \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      fail(nullptr, PB_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e_));                       \
      pb_destroy(c);                                                                                \
      return PB_ERR_HIP;                                                                            \
    }                                                                                               \
  } while (0)
  CRCHK(hipSetDevice(device));
  CRCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  CRCHK_AS("hipMalloc (state)", dev_alloc_hip(c, c->st_base, c->state_doubles));
  c->st = c->st_base;
  CRCHK(hipMemsetAsync(c->st, 0, sizeof(double) * c->state_doubles, c->stream));
  if (n_snapshots > 0) {
    CRCHK_AS("hipMalloc (snapshots)", dev_alloc_hip(c, c->snaps, (size_t) 7 * c->stride * n_snapshots));
    CRCHK(hipMemsetAsync(c->snaps, 0, sizeof(double) * 7 * c->stride * n_snapshots, c->stream));
  }
  CRCHK_AS("hipMalloc (small staging)", dev_alloc_hip(c, c->d_small, 1024));
  CRCHK(hipEventCreate(&c->ev0));
  CRCHK(hipEventCreate(&c->ev1));
  CRCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  CRCHK(hipEventCreateWithFlags(&c->ev_consumed[0], hipEventDisableTiming));
  CRCHK(hipEventCreateWithFlags(&c->ev_consumed[1], hipEventDisableTiming));
  CRCHK(hipEventCreateWithFlags(&c->ev_copied, hipEventDisableTiming));
  CRCHK(hipStreamSynchronize(c->stream));
#undef CRCHK_AS
#undef CRCHK
  *out = c;
  return PB_OK;
}

extern "C" int pb_destroy(pb_ctx *c)
{
  if (!c) return PB_OK;
  (void) hipSetDevice(c->dev);
  if (c->stream) (void) hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void) hipStreamSynchronize(c->copy_stream);
  for (void *p : c->owned) (void) hipFree(p);
  for (int i = 0; i < c->n_fences; i++)
    if (c->fence[i]) (void) hipEventDestroy(c->fence[i]);
  if (c->ev_upload) (void) hipEventDestroy(c->ev_upload);
  for (int i = 0; i < 2; i++)
    if (c->ev_consumed[i]) (void) hipEventDestroy(c->ev_consumed[i]);
  if (c->ev_copied) (void) hipEventDestroy(c->ev_copied);
  if (c->copy_stream) (void) hipStreamDestroy(c->copy_stream);
  if (c->ev0) (void) hipEventDestroy(c->ev0);
  if (c->ev1) (void) hipEventDestroy(c->ev1);
  if (c->own_stream) (void) hipStreamDestroy(c->own_stream);
  delete c;
  return PB_OK;
}

extern "C" int pb_set_stream(pb_ctx *c, void *s)
{
  if (!c) return PB_ERR_ARG;
  if ((hipStream_t) s != c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));  // staging buffers in flight belong to the old stream
  c->stream = (hipStream_t) s;  // literal handle: NULL is the (legacy) null stream, which is torch's default stream
  return PB_OK;
}

extern "C" int pb_use_own_stream(pb_ctx *c)
{
  if (!c) return PB_ERR_ARG;
  if (c->stream != c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = c->own_stream;
  return PB_OK;
}

extern "C" int pb_set_constants(pb_ctx *c, double g, double chi_tol)
{
  if (!c) return PB_ERR_ARG;
  if (!(g > 0) || !(chi_tol >= 0)) return fail(c, PB_ERR_ARG, "pb_set_constants: g must be > 0 and chi_tol >= 0");
  c->k.g = g;
  c->k.chi_tol = chi_tol;
  return PB_OK;
}

extern "C" int pb_sync(pb_ctx *c)
{
  if (!c) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

extern "C" int pb_run_block(const pb_ctx *c) { return c ? c->policy.run_block : 0; }

extern "C" const char *pb_hot_kernel(const pb_ctx *c)
{
  if (!c) return "";
  return step_kernel_name(c->policy.step.map, c->policy.mem_hint);
}
extern "C" int pb_batch(const pb_ctx *c) { return c ? c->B : -1; }
extern "C" int pb_n_states(const pb_ctx *c) { return c ? c->ns : -1; }

extern "C" int pb_malloc(pb_ctx *c, uint64_t bytes, void **p)
{
  if (!c || !p) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipMalloc(p, bytes));
  return PB_OK;
}
extern "C" int pb_free(pb_ctx *c, void *p)
{
  if (!c) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipFree(p));
  return PB_OK;
}
extern "C" int pb_memcpy_h2d(pb_ctx *c, void *d, const void *h, uint64_t bytes)
{
  if (!c || (!d && bytes) || (!h && bytes)) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}
extern "C" int pb_memcpy_d2h(pb_ctx *c, void *h, const void *d, uint64_t bytes)
{
  if (!c || (!d && bytes) || (!h && bytes)) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

extern "C" int pb_host_alloc(pb_ctx *c, uint64_t bytes, void **host_ptr)
{
  if (!c || !host_ptr) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipHostMalloc(host_ptr, bytes ? (size_t) bytes : 8, hipHostMallocDefault));
  return PB_OK;
}

extern "C" int pb_host_free(pb_ctx *c, void *host_ptr)
{
  if (!c) return PB_ERR_ARG;
  if (host_ptr) HIPCHK(c, hipHostFree(host_ptr));
  return PB_OK;
}

// ---- chunked uploads: a block of pre-staged inputs goes to HBM on the copy stream while the kernels of the previous block run ----
extern "C" int pb_fence_create(pb_ctx *c, int *fence_out)
{
  if (!c || !fence_out) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  if (c->n_fences >= PB_MAX_FENCES) return fail(c, PB_ERR_STATE, "pb_fence_create: at most %d fences per context", PB_MAX_FENCES);
  HIPCHK(c, hipEventCreateWithFlags(&c->fence[c->n_fences], hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->fence[c->n_fences], c->stream));   // (a fence that was never recorded would not be waitable)
  *fence_out = c->n_fences++;
  return PB_OK;
}
extern "C" int pb_fence_record(pb_ctx *c, int fence)
{
  if (!c) return PB_ERR_ARG;
  if (fence < 0 || fence >= c->n_fences) return fail(c, PB_ERR_ARG, "pb_fence_record: no fence %d", fence);
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipEventRecord(c->fence[fence], c->stream));
  return PB_OK;
}
extern "C" int pb_fence_wait(pb_ctx *c, int fence)
{
  if (!c) return PB_ERR_ARG;
  if (fence < 0 || fence >= c->n_fences) return fail(c, PB_ERR_ARG, "pb_fence_wait: no fence %d", fence);
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipEventSynchronize(c->fence[fence]));
  return PB_OK;
}
extern "C" int pb_upload_async(pb_ctx *c, void *d, const void *h, uint64_t bytes, int after_fence)
{
  if (!c || (!d && bytes) || (!h && bytes)) return PB_ERR_ARG;
  if (after_fence >= c->n_fences) return fail(c, PB_ERR_ARG, "pb_upload_async: no fence %d", after_fence);
  HIPCHK(c, hipSetDevice(c->dev));
  if (after_fence >= 0) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->fence[after_fence], 0));
  if (bytes) HIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->copy_stream));
  return PB_OK;
}
extern "C" int pb_upload_join(pb_ctx *c)
{
  if (!c) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->ev_upload) HIPCHK(c, hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->ev_upload, c->copy_stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_upload, 0));
  return PB_OK;
}
extern "C" int pb_upload_sync(pb_ctx *c)
{
  if (!c) return PB_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->copy_stream));
  return PB_OK;
}

// staging area for PB_HOST inputs/outputs: a device buffer the host blocks are copied into
int stage_reserve(pb_ctx *c, size_t bytes)
{
  if (bytes <= c->stage_bytes) return PB_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stage_bytes = 0;
  HIPCHK(c, dev_release(c, c->stage));
  if (int rc = dev_alloc(c, c->stage, bytes)) return rc;
  c->stage_bytes = bytes;
  return PB_OK;
}

// the input resolver (Part, pb_ctx.hpp)
int stage_in(pb_ctx *c, int mem, Part *parts, int n)
{
  if (mem == PB_DEVICE) {
    for (int i = 0; i < n; i++) parts[i].dev = parts[i].src;
    return PB_OK;
  }
  if (mem != PB_HOST && mem != PB_HOST_BROADCAST) return fail(c, PB_ERR_ARG, "mem must be PB_HOST, PB_DEVICE or PB_HOST_BROADCAST");
  size_t tot = 0;
  for (int i = 0; i < n; i++) tot += (parts[i].bytes + 255) / 256 * 256;
  int rc = (mem == PB_HOST_BROADCAST) ? stage_reserve(c, tot) : PB_OK;
  if (rc) return rc;
  void *in_buf = nullptr;
  bool copied = false;
  if (mem == PB_HOST) {
    // Double-buffered H2D staging on the copy stream.  Everything enqueued on the main stream so far includes the
    // consumer of the buffer used by the previous call; the buffer used now was consumed two calls ago.
    const int prev = c->in_idx, cur = prev ^ 1;
    HIPCHK(c, hipEventRecord(c->ev_consumed[prev], c->stream));
    c->in_idx = cur;
    if (tot > c->in_stage_bytes[cur]) {
      HIPCHK(c, hipEventSynchronize(c->ev_consumed[cur]));
      c->in_stage_bytes[cur] = 0;
      HIPCHK(c, dev_release(c, c->in_stage[cur]));
      if (int rc = dev_alloc(c, c->in_stage[cur], tot)) return rc;
      c->in_stage_bytes[cur] = tot;
    }
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_consumed[cur], 0));
    in_buf = c->in_stage[cur];
  }
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    if (parts[i].src && mem == PB_HOST_BROADCAST) {
      // One value per ROW, the same for every filter (one robot's message feeding a whole parameter sweep): the rows are
      // expanded on the device, nothing of batch size crosses PCIe.  A mask (bytes == B) cannot be broadcast.
      const size_t rows = parts[i].bytes / (sizeof(double) * (size_t) c->B);
      if (rows * sizeof(double) * (size_t) c->B != parts[i].bytes || rows == 0 || rows > (size_t) RowVals::MAX)
        return fail(c, PB_ERR_ARG, "PB_HOST_BROADCAST: only blocks of 1..%d double rows can be broadcast (pass mask = NULL)",
                    RowVals::MAX);
      RowVals v;
      memcpy(v.v, parts[i].src, rows * sizeof(double));
      k_fill_rows<<<nblk(c->B), 64, 0, c->stream>>>((double *) ((char *) c->stage + off), (int) rows, c->B, v);
      HIPCHK(c, hipGetLastError());
      parts[i].dev = (char *) c->stage + off;
    } else if (parts[i].src) {
      HIPCHK(c, hipMemcpyAsync((char *) in_buf + off, parts[i].src, parts[i].bytes, hipMemcpyHostToDevice, c->copy_stream));
      parts[i].dev = (char *) in_buf + off;
      copied = true;
    } else {
      parts[i].dev = nullptr;
    }
    off += (parts[i].bytes + 255) / 256 * 256;
  }
  if (copied) {
    // The caller may reuse its buffers as soon as this returns, so wait for the copy -- NOT for the main stream: the
    // kernels of the previous message keep running underneath.
    HIPCHK(c, hipEventRecord(c->ev_copied, c->copy_stream));
    HIPCHK(c, hipEventSynchronize(c->ev_copied));
  }
  return PB_OK;
}

// (the per-call contract -- CALL(c, flags) -- is in pb_ctx.hpp)

extern "C" int pb_reset(pb_ctx *c, const double *vec, const double *quat, const double *cov, int broadcast, int mem)
{
  CALL(c, 0);
  if (!vec || !quat || !cov) return fail(c, PB_ERR_ARG, "pb_reset: NULL input");
  c->st = c->st_base;  // a reset always lands in the context's own array (a checkpoint the head lived in stays intact)
  c->out_slot = -1;
  const int n = c->ns, B = c->B;
  if (broadcast) {
    if (mem != PB_HOST) return fail(c, PB_ERR_ARG, "pb_reset: broadcast inputs must be host memory");
    double comp[Lay<21>::NC];
    const int off_q = n, off_ll = n + 4, off_p = n + 5;
    for (int i = 0; i < n; i++) comp[i] = vec[i];
    for (int i = 0; i < 4; i++) comp[off_q + i] = quat[i];
    comp[off_ll] = 0.0;
    for (int i = 0; i < n; i++)
      for (int j = 0; j <= i; j++) comp[off_p + pk(i, j)] = cov[j * n + i];
    HIPCHK(c, hipMemcpyAsync(c->d_small, comp, sizeof(double) * c->nc, hipMemcpyHostToDevice, c->stream));
    with_ns(n, [&](auto NS) { k_reset_bcast<decltype(NS)::value><<<nblk(B), 64, 0, c->stream>>>(c->st, B, c->d_small); });
    LAUNCHCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));  // comp is a stack buffer
  } else {
    Part p[3] = { { vec, sizeof(double) * n * B, 0 }, { quat, sizeof(double) * 4 * B, 0 },
                  { cov, sizeof(double) * n * n * B, 0 } };
    int rc = stage_in(c, mem, p, 3);
    if (rc) return rc;
    with_ns(n, [&](auto NS) {
      k_reset<decltype(NS)::value><<<nblk(B), 64, 0, c->stream>>>(c->st, B, (const double *) p[0].dev, (const double *) p[1].dev, (const double *) p[2].dev);
    });
    LAUNCHCHK(c);
  }
  c->have_state = true;
  return PB_OK;
}

// The posterior of an update that was computed OUTSIDE the library (the shim's RBISHostUpdate: user code written against the
// reference's updateFilter(prior_state, prior_cov, prior_loglikelihood) contract, rbis_update_interface.hpp:14-35) becomes the head.
extern "C" int pb_set_head(pb_ctx *c, const double *vec, const double *quat, const double *cov, const double *loglik, int mem)
{
  CALL(c, NEEDS_STATE);
  if (!vec || !quat || !cov) return fail(c, PB_ERR_ARG, "pb_set_head: NULL input");
  if (mem != PB_HOST && mem != PB_DEVICE) return fail(c, PB_ERR_ARG, "pb_set_head: mem must be PB_HOST or PB_DEVICE");
  const int n = c->ns, B = c->B;
  Part p[4] = { { vec, sizeof(double) * n * B, 0 }, { quat, sizeof(double) * 4 * B, 0 }, { cov, sizeof(double) * n * n * B, 0 },
                { loglik, loglik ? sizeof(double) * B : 0, 0 } };
  int rc = stage_in(c, mem, p, 4);
  if (rc) return rc;
  double *target = update_target(c);   // like every update: in place, or into the checkpoint slot named by pb_set_output_slot
  with_ns(n, [&](auto NS) {
    k_reset<decltype(NS)::value><<<nblk(B), 64, 0, c->stream>>>(target, B, (const double *) p[0].dev, (const double *) p[1].dev, (const double *) p[2].dev,
                                                                (const double *) p[3].dev);
  });
  LAUNCHCHK(c);
  update_done(c, target);
  return PB_OK;
}

// The IMU block of a call, resolved.  PB_HOST_BROADCAST -- one message for every filter -- travels as kernel arguments (bc; p[0].dev
// stays NULL): no device block, no fill launch, no input traffic.  A block in any other space goes through stage_in as p[0], in the
// same call as the n - 1 parts the caller put behind it because they live in the same space (the double-buffered host staging must
// not be flipped twice before its consumer is enqueued).
int imu_in(pb_ctx *c, const double *imu_block, int imu_mem, StepBcast &bc, Part *p, int n)
{
  p[0] = Part{ imu_block, sizeof(double) * 7 * c->B, nullptr };
  if (imu_mem != PB_HOST_BROADCAST) return stage_in(c, imu_mem, p, n);
  memcpy(bc.imu, imu_block, sizeof(bc.imu));
  bc.on |= 1;
  return PB_OK;
}

// the frame of a timed entry point: device time between the two events (elapsed_ms NULL: not timed, no event)
int timed_begin(pb_ctx *c, const float *elapsed_ms)
{
  if (elapsed_ms) HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  return PB_OK;
}
int timed_end(pb_ctx *c, float *elapsed_ms)
{
  if (!elapsed_ms) return PB_OK;
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  HIPCHK(c, hipEventElapsedTime(elapsed_ms, c->ev0, c->ev1));
  return PB_OK;
}

extern "C" int pb_predict(pb_ctx *c, const double *imu_block, const double q[4], int mem)
{
  CALL(c, IMU_STEP | PRED_REFUSE | NEEDS_STATE);
  if (!imu_block || !q) return fail(c, PB_ERR_ARG, "pb_predict: NULL input");
  StepBcast bc;
  Part p[1];
  if (int rc = imu_in(c, imu_block, mem, bc, p)) return rc;
  return pbk_step(c, false, (const double *) p[0].dev, nullptr, nullptr, q, &bc);
}

// The fused step with its two input groups (the IMU block; the measurement and its mask) each in a space of its own.  At most one
// of the two goes through the double-buffered host staging (PB_HOST) -- in ONE call when both live there; a broadcast group
// travels as kernel arguments (a parameter sweep replaying one robot's log), a device group is read in place.
static int step_legodo_impl(pb_ctx *c, const char *who, const double *imu_block, int imu_mem, const double *lo_block, const uint8_t *mask,
                            int lo_mem, const double q[4])
{
  if (!imu_block || !lo_block || !q) return fail(c, PB_ERR_ARG, "%s: NULL input", who);
  const bool together = imu_mem == lo_mem;
  StepBcast bc;
  Part p[3] = { {}, { lo_block, sizeof(double) * 6 * c->B, nullptr }, { mask, (size_t) c->B, nullptr } };
  if (int rc = imu_in(c, imu_block, imu_mem, bc, p, together ? 3 : 1)) return rc;
  if (lo_mem == PB_HOST_BROADCAST) {
    if (mask) return fail(c, PB_ERR_ARG, "PB_HOST_BROADCAST: a mask cannot be broadcast (pass mask = NULL)");
    memcpy(bc.lo, lo_block, sizeof(bc.lo));
    bc.on |= 2;
  } else if (!together) {
    if (int rc = stage_in(c, lo_mem, p + 1, 2)) return rc;
  }
  return pbk_step(c, true, (const double *) p[0].dev, (const double *) p[1].dev, (const uint8_t *) p[2].dev, q, &bc);
}

extern "C" int pb_step_legodo(pb_ctx *c, const double *imu_block, const double *lo_block, const uint8_t *mask,
                              const double q[4], int mem)
{
  CALL(c, IMU_STEP | PRED_TAKE | NEEDS_STATE);
  return step_legodo_impl(c, "pb_step_legodo", imu_block, mem, lo_block, mask, mem, q);
}

extern "C" int pb_step_legodo_split(pb_ctx *c, const double *imu_block, int imu_mem, const double *lo_block,
                                    const uint8_t *mask, int lo_mem, const double q[4])
{
  CALL(c, IMU_STEP | PRED_TAKE | NEEDS_STATE);
  return step_legodo_impl(c, "pb_step_legodo_split", imu_block, imu_mem, lo_block, mask, lo_mem, q);
}

extern "C" int pb_step_legodo_correct(pb_ctx *c, const double *imu_block, const double *lo_block, const uint8_t *mask,
                                      const double q[4], int mem, int corr_kind, const double *z2, const double *R2,
                                      int r_kind2, const double *quat_meas2, const uint8_t *mask2, int mem2)
{
  CALL(c, IMU_STEP | PRED_TAKE | PRED_WITH_OUT | NEEDS_STATE);
  if (!imu_block || !lo_block || !q || !z2 || !R2 || !quat_meas2) return fail(c, PB_ERR_ARG, "pb_step_legodo_correct: NULL input");
  if (corr_kind != PB_CORR_POS_ORIENT && corr_kind != PB_CORR_POS_YAW) return fail(c, PB_ERR_ARG, "pb_step_legodo_correct: bad corr_kind %d", corr_kind);
  if (mem2 == PB_HOST_BROADCAST && r_kind2 == PB_R_DIAG) r_kind2 = PB_R_DIAG_BROADCAST;
  if (r_kind2 != PB_R_DIAG && r_kind2 != PB_R_DIAG_BROADCAST) return fail(c, PB_ERR_ARG, "pb_step_legodo_correct: R2 must be diagonal (PB_R_DIAG or PB_R_DIAG_BROADCAST)");
  const int m2 = (corr_kind == PB_CORR_POS_ORIENT) ? 6 : 4;
  const size_t B = (size_t) c->B;
  const bool rbc = r_kind2 == PB_R_DIAG_BROADCAST;
  const bool arg_kernel = correction_as_args(c->policy.step.map, corr_kind);
  Part p[7] = { { imu_block, sizeof(double) * 7 * B, 0 }, { lo_block, sizeof(double) * 6 * B, 0 }, { mask, B, 0 },
                { z2, sizeof(double) * m2 * B, 0 }, { rbc ? nullptr : R2, rbc ? 0 : sizeof(double) * m2 * B, 0 },
                { quat_meas2, sizeof(double) * 4 * B, 0 }, { mask2, B, 0 } };
  if (mem == PB_HOST_BROADCAST && mem2 == PB_HOST_BROADCAST && rbc && !mask && !mask2 && arg_kernel) {
    // one robot's three messages for every filter: everything travels as kernel arguments
    StepBcast bc;
    (void) imu_in(c, imu_block, mem, bc, p);
    memcpy(bc.lo, lo_block, sizeof(bc.lo));
    bc.on |= 2;
    return pbk_step_correct(c, corr_kind, nullptr, nullptr, nullptr, q, nullptr, nullptr, R2, nullptr, nullptr, &bc, z2, quat_meas2);
  }
  // one staging call when both groups live in the same space (the double-buffered host staging must not be flipped twice
  // before its consumer is enqueued); otherwise at most one of the two groups is PB_HOST
  int rc;
  if (mem == mem2) rc = stage_in(c, mem, p, 7);
  else {
    rc = stage_in(c, mem, p, 3);
    if (!rc) rc = stage_in(c, mem2, p + 3, 4);
  }
  if (rc) return rc;
  return pbk_step_correct(c, corr_kind, (const double *) p[0].dev, (const double *) p[1].dev, (const uint8_t *) p[2].dev, q,
                          (const double *) p[3].dev, (const double *) p[4].dev, rbc ? R2 : nullptr, (const double *) p[5].dev,
                          (const uint8_t *) p[6].dev);
}

extern "C" int pb_run_legodo(pb_ctx *c, int n_steps, const double *imu_stream, const double *lo_stream,
                             const uint8_t *mask_stream, const double q[4], float *elapsed_ms)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  if (n_steps < 0 || !imu_stream || !lo_stream || !q) return fail(c, PB_ERR_ARG, "pb_run_legodo: bad argument");
  const size_t B = (size_t) c->B;
  if (int rc = timed_begin(c, elapsed_ms)) return rc;
  const Policy &pol = c->policy;
  if (pol.run_block > 0 && n_steps > 1 && c->st == c->st_base && c->out_slot < 0) {
    // cache-blocked order (pb_create): every block of filters runs the whole stream before the next block starts
    for (long b0 = 0; b0 < (long) B; b0 += pol.run_block) {
      const int nb = (int) std::min<long>(pol.run_block, (long) B - b0);
      for (int s = 0; s < n_steps; s++) {
        int rc = pbk_step_range(c, imu_stream + (size_t) s * 7 * B, lo_stream + (size_t) s * 6 * B,
                                mask_stream ? mask_stream + (size_t) s * B : nullptr, q, b0, nb, pol.run_block_map, pol.run_block_hint);
        if (rc) return rc;
      }
    }
  } else {
    for (int s = 0; s < n_steps; s++) {
      int rc = pbk_step(c, true, imu_stream + (size_t) s * 7 * B, lo_stream + (size_t) s * 6 * B,
                        mask_stream ? mask_stream + (size_t) s * B : nullptr, q);
      if (rc) return rc;
    }
  }
  return timed_end(c, elapsed_ms);
}

// write_through: the posterior of step t also goes to checkpoint slot first_slot + t
static int replay_impl(pb_ctx *c, const char *who, int n_steps, int steps_per_launch, const double *imu_stream, const double *lo_stream,
                       const uint8_t *mask_stream, const double q[4], bool write_through, int first_slot, float *elapsed_ms)
{
  if (n_steps < 0 || steps_per_launch < 1 || !imu_stream || !lo_stream || !q) return fail(c, PB_ERR_ARG, "%s: bad argument", who);
  if (write_through && (first_slot < 0 || first_slot + n_steps > c->nhist))
    return fail(c, PB_ERR_ARG, "%s: slots %d..%d of %d (pb_history_reserve)", who, first_slot, first_slot + n_steps - 1, c->nhist);
  const size_t B = (size_t) c->B;
  // this kernel works in place, never on a checkpoint slot: the state rides in registers from the context's own array, the slots
  // only receive copies
  if (int rc = detach_head(c, true)) return rc;
  if (int rc = timed_begin(c, elapsed_ms)) return rc;
  for (int s = 0; s < n_steps; s += steps_per_launch) {
    const int T = (n_steps - s < steps_per_launch) ? n_steps - s : steps_per_launch;
    int rc = pbk_replay_fused(c, T, imu_stream + (size_t) s * 7 * B, lo_stream + (size_t) s * 6 * B,
                              mask_stream ? mask_stream + (size_t) s * B : nullptr, q, write_through ? first_slot + s : -1);
    if (rc) return rc;
  }
  return timed_end(c, elapsed_ms);
}

extern "C" int pb_replay_legodo_fused(pb_ctx *c, int n_steps, int steps_per_launch, const double *imu_stream,
                                      const double *lo_stream, const uint8_t *mask_stream, const double q[4],
                                      float *elapsed_ms)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  return replay_impl(c, "pb_replay_legodo_fused", n_steps, steps_per_launch, imu_stream, lo_stream, mask_stream, q, false, -1, elapsed_ms);
}

extern "C" int pb_replay_legodo_checkpointed(pb_ctx *c, int n_steps, int steps_per_launch, const double *imu_stream,
                                             const double *lo_stream, const uint8_t *mask_stream, const double q[4], int first_slot,
                                             float *elapsed_ms)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  return replay_impl(c, "pb_replay_legodo_checkpointed", n_steps, steps_per_launch, imu_stream, lo_stream, mask_stream, q, true, first_slot, elapsed_ms);
}

int pbk_check_indices(pb_ctx *c, int m, const int *idx)
{
  for (int i = 0; i < m; i++) {
    if (idx[i] < 0 || idx[i] >= c->ns) return fail(c, PB_ERR_ARG, "update: index %d out of range for n_states=%d", idx[i], c->ns);
    for (int j = 0; j < i; j++)
      if (idx[i] == idx[j]) return fail(c, PB_ERR_ARG, "update: duplicate index %d", idx[i]);
  }
  return PB_OK;
}

int pbk_update_common(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int rkind, const double *qm, bool orient,
                      const uint8_t *mask, int mem)
{
  if (m < 1 || m > 6) return fail(c, PB_ERR_ARG, "update: m must be 1..6 (got %d)", m);
  if (!idx || !z || !R) return fail(c, PB_ERR_ARG, "update: NULL input");
  if (orient && !qm) return fail(c, PB_ERR_ARG, "update: quat_meas is NULL");
  if (int rc = pbk_check_indices(c, m, idx)) return rc;
  const size_t B = (size_t) c->B;
  size_t rbytes;
  if (mem == PB_HOST_BROADCAST && rkind == PB_R_DIAG) rkind = PB_R_DIAG_BROADCAST;  // the same thing, without a fill
  if (rkind == PB_R_DIAG_BROADCAST) rbytes = 0;
  else if (rkind == PB_R_DIAG) rbytes = sizeof(double) * m * B;
  else if (rkind == PB_R_FULL) rbytes = sizeof(double) * m * m * B;
  else return fail(c, PB_ERR_ARG, "update: bad r_kind %d", rkind);
  const UpdateChoice u = update_choice(c->policy.step.map, c->policy.generic_update, m, idx, orient, rkind, mem == PB_HOST_BROADCAST, mask != nullptr);
  UpdateIn in;
  if (rkind == PB_R_DIAG_BROADCAST) in.r_bcast = R;
  if (u.host_args) {  // one measurement for every filter on a compile-time-index kernel: z, R and the quaternion are kernel arguments
    in.z_host = z;
    in.q_host = orient ? qm : nullptr;
    return pbk_update(c, u, m, idx, in);
  }
  Part p[4] = { { z, sizeof(double) * m * B, 0 }, { in.r_bcast ? nullptr : R, rbytes, 0 },
                { orient ? qm : nullptr, sizeof(double) * 4 * B, 0 }, { mask, B, 0 } };
  if (int rc = stage_in(c, mem, p, 4)) return rc;
  in.z = (const double *) p[0].dev;
  (rkind == PB_R_FULL ? in.r_full : in.r_diag) = (const double *) p[1].dev;
  in.qm = (const double *) p[2].dev;
  in.mask = (const uint8_t *) p[3].dev;
  return pbk_update(c, u, m, idx, in);
}

extern "C" int pb_update_indexed(pb_ctx *c, int m, const int *idx, const double *z, const double *R, int r_kind,
                                 const uint8_t *mask, int mem)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  return pbk_update_common(c, m, idx, z, R, r_kind, nullptr, false, mask, mem);
}

extern "C" int pb_update_indexed_orient(pb_ctx *c, int m, const int *idx, const double *z, const double *R,
                                        int r_kind, const double *quat_meas, const uint8_t *mask, int mem)
{
  CALL(c, PRED_REFUSE | NEEDS_STATE);
  return pbk_update_common(c, m, idx, z, R, r_kind, quat_meas, true, mask, mem);
}

extern "C" int pb_snapshot(pb_ctx *c, int slot)
{
  CALL(c, NEEDS_STATE);
  if (slot < 0 || slot >= c->nsnap) return fail(c, PB_ERR_STATE, "pb_snapshot: slot %d of %d", slot, c->nsnap);
  double *snap = c->snaps + (size_t) slot * 7 * c->stride;
  with_ns(c->ns, [&](auto NS) { k_snapshot<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(c->st, c->stride, c->B, snap); });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_snapshot_from_slot(pb_ctx *c, int slot, int checkpoint_slot)
{
  CALL(c, 0);
  if (slot < 0 || slot >= c->nsnap) return fail(c, PB_ERR_STATE, "pb_snapshot_from_slot: slot %d of %d", slot, c->nsnap);
  if (checkpoint_slot < 0 || checkpoint_slot >= c->nhist)
    return fail(c, PB_ERR_STATE, "pb_snapshot_from_slot: checkpoint slot %d of %d", checkpoint_slot, c->nhist);
  double *snap = c->snaps + (size_t) slot * 7 * c->stride;
  const double *src = slot_ptr(c, checkpoint_slot);
  with_ns(c->ns, [&](auto NS) { k_snapshot<decltype(NS)::value><<<nblk(c->B), 64, 0, c->stream>>>(src, c->stride, c->B, snap); });
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_compose_delta(pb_ctx *c, int slot, const double *t, const double *q, double *z_out,
                                double *quat_out, int mem)
{
  CALL(c, 0);
  if (slot < 0 || slot >= c->nsnap) return fail(c, PB_ERR_STATE, "pb_compose_delta: slot %d of %d", slot, c->nsnap);
  if (!t || !q || !z_out || !quat_out) return fail(c, PB_ERR_ARG, "pb_compose_delta: NULL argument");
  Part p[2] = { { t, sizeof(double) * 3 * c->B, 0 }, { q, sizeof(double) * 4 * c->B, 0 } };
  int rc = stage_in(c, mem, p, 2);
  if (rc) return rc;
  const double *snap = c->snaps + (size_t) slot * 7 * c->stride;
  k_compose<<<nblk(c->B), 64, 0, c->stream>>>(snap, c->stride, c->B, (const double *) p[0].dev, (const double *) p[1].dev, z_out, quat_out);
  LAUNCHCHK(c);
  return PB_OK;
}

static int get_state_impl(pb_ctx *c, const double *st, int first, int count, double *vec_out, double *quat_out, double *cov_out, double *ll_out, int mem);

extern "C" int pb_get_head(pb_ctx *c, int first, int count, double *vec_out, double *quat_out, double *cov_out,
                           double *ll_out, int mem)
{
  CALL(c, NEEDS_STATE);
  return get_state_impl(c, c->st, first, count, vec_out, quat_out, cov_out, ll_out, mem);
}

// the same read of a posterior that lives in a checkpoint slot (the head is not touched)
extern "C" int pb_get_slot(pb_ctx *c, int slot, int first, int count, double *vec_out, double *quat_out, double *cov_out, double *ll_out, int mem)
{
  CALL(c, 0);
  if (slot < 0 || slot >= c->nhist) return fail(c, PB_ERR_STATE, "pb_get_slot: checkpoint slot %d of %d", slot, c->nhist);
  return get_state_impl(c, slot_ptr(c, slot), first, count, vec_out, quat_out, cov_out, ll_out, mem);
}

static int get_state_impl(pb_ctx *c, const double *st, int first, int count, double *vec_out, double *quat_out, double *cov_out, double *ll_out, int mem)
{
  if (first < 0 || count < 0 || (long) first + count > c->B) return fail(c, PB_ERR_ARG, "pb_get_head: range [%d,+%d) outside batch %d", first, count, c->B);
  if (count == 0) return PB_OK;
  const int n = c->ns;
  double *dv = vec_out, *dq = quat_out, *dc = cov_out, *dl = ll_out;
  size_t o_v = 0, o_q = 0, o_c = 0, o_l = 0;
  if (mem == PB_HOST) {
    size_t tot = 0;
    o_v = tot; tot += vec_out ? sizeof(double) * n * count : 0;
    o_q = tot; tot += quat_out ? sizeof(double) * 4 * count : 0;
    o_c = tot; tot += cov_out ? sizeof(double) * n * n * count : 0;
    o_l = tot; tot += ll_out ? sizeof(double) * count : 0;
    int rc = stage_reserve(c, tot ? tot : 8);
    if (rc) return rc;
    char *s = (char *) c->stage;
    dv = vec_out ? (double *) (s + o_v) : nullptr;
    dq = quat_out ? (double *) (s + o_q) : nullptr;
    dc = cov_out ? (double *) (s + o_c) : nullptr;
    dl = ll_out ? (double *) (s + o_l) : nullptr;
  } else if (mem != PB_DEVICE) {
    return fail(c, PB_ERR_ARG, "mem must be PB_HOST or PB_DEVICE");
  }
  with_ns(n, [&](auto NS) { k_get_head<decltype(NS)::value><<<nblk(count), 64, 0, c->stream>>>(st, first, count, dv, dq, dc, dl); });
  LAUNCHCHK(c);
  if (mem == PB_HOST) {
    if (vec_out) HIPCHK(c, hipMemcpyAsync(vec_out, dv, sizeof(double) * n * count, hipMemcpyDeviceToHost, c->stream));
    if (quat_out) HIPCHK(c, hipMemcpyAsync(quat_out, dq, sizeof(double) * 4 * count, hipMemcpyDeviceToHost, c->stream));
    if (cov_out) HIPCHK(c, hipMemcpyAsync(cov_out, dc, sizeof(double) * n * n * count, hipMemcpyDeviceToHost, c->stream));
    if (ll_out) HIPCHK(c, hipMemcpyAsync(ll_out, dl, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return PB_OK;
}

extern "C" int pb_get_filter_state(pb_ctx *c, int filter, double quat[4], double state[21], double cov[441])
{
  if (!c || !quat || !state || !cov) return PB_ERR_ARG;
  const int n = c->ns;
  double v[21], P[441];
  int rc = pb_get_head(c, filter, 1, v, quat, P, nullptr, PB_HOST);
  if (rc) return rc;
  memset(state, 0, sizeof(double) * 21);
  memset(cov, 0, sizeof(double) * 441);
  for (int i = 0; i < n; i++) state[i] = v[i];
  for (int col = 0; col < n; col++)
    for (int r = 0; r < n; r++) cov[col * 21 + r] = P[col * n + r];
  return PB_OK;
}

// bit-level checksum of a whole state array: wrapping sum and xor of every 64-bit word after a position-dependent rotation,
// combined with integer atomics, hence independent of the order in which waves finish
static __global__ __launch_bounds__(256) void k_state_checksum(const uint64_t *__restrict__ w, size_t n, unsigned long long *__restrict__ out)
{
  unsigned long long sum = 0, x = 0;
  for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
    const uint64_t v = w[i];
    const unsigned r = (unsigned) (i % 63) + 1;
    sum += v * (2 * (uint64_t) (i % 1021) + 1);
    x ^= (v << r) | (v >> (64 - r));
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    x ^= __shfl_xor(x, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, sum);
    atomicXor(out + 1, x);
  }
}

extern "C" int pb_state_checksum(pb_ctx *c, int slot, uint64_t out[2])
{
  CALL(c, NEEDS_STATE);
  if (!out) return PB_ERR_ARG;
  if (slot >= c->nhist) return fail(c, PB_ERR_ARG, "pb_state_checksum: slot %d of %d", slot, c->nhist);
  const double *src = slot < 0 ? c->st : slot_ptr(c, slot);
  int rc = stage_reserve(c, 2 * sizeof(uint64_t));
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->stage, 0, 2 * sizeof(uint64_t), c->stream));
  k_state_checksum<<<2048, 256, 0, c->stream>>>((const uint64_t *) src, c->state_doubles, (unsigned long long *) c->stage);
  LAUNCHCHK(c);
  HIPCHK(c, hipMemcpyAsync(out, c->stage, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PB_OK;
}

extern "C" int pb_summary(pb_ctx *c, double out[4])
{
  CALL(c, NEEDS_STATE);
  if (!out) return PB_ERR_ARG;
  const int nb = nblk(c->B);
  int rc = stage_reserve(c, sizeof(double) * 4 * (size_t) nb);
  if (rc) return rc;
  double *part = (double *) c->stage;
  with_ns(c->ns, [&](auto NS) { k_summary<decltype(NS)::value><<<nb, 64, 0, c->stream>>>(c->st, c->B, part); });
  LAUNCHCHK(c);
  double *h = (double *) malloc(sizeof(double) * 4 * (size_t) nb);
  if (!h) return fail(c, PB_ERR_ARG, "pb_summary: out of host memory");
  hipError_t e = hipMemcpyAsync(h, part, sizeof(double) * 4 * (size_t) nb, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    free(h);
    return fail(c, PB_ERR_HIP, "pb_summary copy failed: %s", hipGetErrorString(e));
  }
  out[0] = out[1] = out[2] = out[3] = 0.0;
  for (int i = 0; i < nb; i++) {
    out[0] += h[4 * i];
    out[1] += h[4 * i + 1];
    if (h[4 * i + 2] > out[2]) out[2] = h[4 * i + 2];
    out[3] += h[4 * i + 3];
  }
  free(h);
  return PB_OK;
}

// number of filters a device-resident update mask [B] lets through (one wave-level popcount + atomic per 256 filters)
static __global__ __launch_bounds__(256) void k_mask_count(const uint8_t *__restrict__ mask, int B, unsigned *__restrict__ out)
{
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool on = b < B && mask[b] != 0;
  const unsigned n = (unsigned) __popcll(__ballot(on));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

extern "C" int pb_mask_count(pb_ctx *c, const uint8_t *mask_dev, int *count_out)
{
  CALL(c, 0);
  if (!mask_dev || !count_out) return fail(c, PB_ERR_ARG, "pb_mask_count: NULL argument");
  int rc = stage_reserve(c, sizeof(unsigned));
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->stage, 0, sizeof(unsigned), c->stream));
  k_mask_count<<<(c->B + 255) / 256, 256, 0, c->stream>>>(mask_dev, c->B, (unsigned *) c->stage);
  LAUNCHCHK(c);
  unsigned n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, c->stage, sizeof n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *count_out = (int) n;
  return PB_OK;
}

extern "C" int pb_set_process_noise_block(pb_ctx *c, const double *q_block_dev)
{
  if (!c) return PB_ERR_ARG;
  c->k.qblk = q_block_dev;  // [4][B] device memory, or NULL to go back to the scalar q of each call
  return PB_OK;
}

template <int NS>
static int launch_nll(pb_ctx *c, int m, const int *idx, const double *tv, const double *tq, double *out, double *err)
{
#define NLL_CASE(M)                                                                                         \
  case M: {                                                                                                 \
    IdxArg<M> ia;                                                                                           \
    for (int i = 0; i < M; i++) ia.v[i] = idx[i];                                                           \
    k_window_nll<NS, M><<<nblk(c->B), 64, 0, c->stream>>>(c->st, c->B, ia, tv, tq, out, err);    \
  } break;
  switch (m) {
    NLL_CASE(1) NLL_CASE(2) NLL_CASE(3) NLL_CASE(4) NLL_CASE(5) NLL_CASE(6) NLL_CASE(7) NLL_CASE(8) NLL_CASE(9)
    default: return fail(c, PB_ERR_ARG, "pb_window_nll: m must be 1..9");
  }
#undef NLL_CASE
  LAUNCHCHK(c);
  return PB_OK;
}

extern "C" int pb_window_nll(pb_ctx *c, int m, const int *idx, const double *truth_vec, const double *truth_quat,
                             double *out3, double *err_out, int mem)
{
  CALL(c, NEEDS_STATE);
  if (m < 1 || m > 9 || !idx || !truth_vec || !truth_quat || !out3) return fail(c, PB_ERR_ARG, "pb_window_nll: bad argument");
  for (int i = 0; i < m; i++) {
    if (idx[i] < 0 || idx[i] >= c->ns) return fail(c, PB_ERR_ARG, "pb_window_nll: index %d out of range", idx[i]);
    for (int j = 0; j < i; j++)
      if (idx[i] == idx[j]) return fail(c, PB_ERR_ARG, "pb_window_nll: duplicate index %d", idx[i]);
  }
  const size_t B = (size_t) c->B, n = (size_t) c->ns;
  const double *tv = truth_vec, *tq = truth_quat;
  double *d_out = out3, *d_err = err_out;
  if (mem == PB_HOST) {
    const size_t o1 = sizeof(double) * n * B, o2 = o1 + sizeof(double) * 4 * B, o3 = o2 + sizeof(double) * 3 * B;
    int rc = stage_reserve(c, o3 + sizeof(double) * n * B);
    if (rc) return rc;
    char *s = (char *) c->stage;
    HIPCHK(c, hipMemcpyAsync(s, truth_vec, o1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s + o1, truth_quat, sizeof(double) * 4 * B, hipMemcpyHostToDevice, c->stream));
    tv = (const double *) s;
    tq = (const double *) (s + o1);
    d_out = (double *) (s + o2);
    d_err = err_out ? (double *) (s + o3) : nullptr;
  } else if (mem != PB_DEVICE) {
    return fail(c, PB_ERR_ARG, "mem must be PB_HOST or PB_DEVICE");
  }
  int rc = (c->ns == 15) ? launch_nll<15>(c, m, idx, tv, tq, d_out, d_err) : launch_nll<21>(c, m, idx, tv, tq, d_out, d_err);
  if (rc) return rc;
  if (mem == PB_HOST) {
    HIPCHK(c, hipMemcpyAsync(out3, d_out, sizeof(double) * 3 * B, hipMemcpyDeviceToHost, c->stream));
    if (err_out) HIPCHK(c, hipMemcpyAsync(err_out, d_err, sizeof(double) * n * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return PB_OK;
}

static int calib_copy_impl(pb_ctx *c, int reps, float *elapsed_ms, uint64_t *checksum)
{
  if (reps < 1) return fail(c, PB_ERR_ARG, "pb_calib_copy: reps must be >= 1");
  double *dst = nullptr;
  const size_t bytes = sizeof(double) * c->state_doubles;
  if (checksum) {
    int rc = stage_reserve(c, 2 * sizeof(uint64_t));
    if (rc) return rc;
  }
  HIPCHK(c, hipMalloc((void **) &dst, bytes));
  hipError_t e = hipEventRecord(c->ev0, c->stream);
  for (int r = 0; r < reps && e == hipSuccess; r++) {
    k_calib_copy<<<nblk(c->B), 64, 0, c->stream>>>(c->st, dst, c->B, (int) (c->state_doubles / (size_t) c->stride / 2));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
  if (e == hipSuccess && checksum) {
    e = hipMemsetAsync(c->stage, 0, 2 * sizeof(uint64_t), c->stream);
    if (e == hipSuccess) {
      k_state_checksum<<<2048, 256, 0, c->stream>>>((const uint64_t *) dst, c->state_doubles, (unsigned long long *) c->stage);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(checksum, c->stage, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e == hipSuccess) e = hipEventSynchronize(c->ev1);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
  (void) hipFree(dst);
  if (e != hipSuccess) return fail(c, PB_ERR_HIP, "pb_calib_copy failed: %s", hipGetErrorString(e));
  if (elapsed_ms) *elapsed_ms = ms;
  return PB_OK;
}

extern "C" int pb_calib_copy(pb_ctx *c, int reps, float *elapsed_ms)
{
  CALL(c, 0);
  return calib_copy_impl(c, reps, elapsed_ms, nullptr);
}

extern "C" int pb_calib_copy_checksum(pb_ctx *c, int reps, uint64_t out[2])
{
  CALL(c, NEEDS_STATE);
  if (!out) return PB_ERR_ARG;
  return calib_copy_impl(c, reps, nullptr, out);
}

extern "C" int pb_set_utime(pb_ctx *c, int64_t utime)
{
  if (!c) return PB_ERR_ARG;
  c->utime = utime;
  return PB_OK;
}
extern "C" int64_t pb_get_utime(const pb_ctx *c) { return c ? c->utime : 0; }
