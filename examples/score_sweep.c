/* score_sweep.c -- a parameter sweep judged the way the reference judges an estimator: drift per distance travelled against
 * ground truth (motion_estimate/scripts/drift_per_distance.py), computed on the device next to the filters, in plain C.
 *
 * One synthetic robot walks a planar path (forward speed and yaw rate vary slowly); its IMU and leg-odometry streams carry a
 * known measurement noise, and its true pose is the ground truth (what Vicon gives the script on POSE_GROUND_TRUTH).  Every
 * filter of the batch replays the same streams with its own leg-odometry noise r_vxyz and IMU process noise, as
 * examples/param_sweep.c does.  After every 10 s segment the truth is scored as ONE broadcast message
 * (pb_score_ground_truth, PB_HOST_BROADCAST): no head is downloaded.  At the end pb_score_best names the candidate with the
 * smallest mean percent drift per distance travelled, printed next to the log-likelihood winner param_sweep.c picks.
 * Which of the two is "right" is not asserted: exit status 0 means the sweep ran and the winner is a filter of the batch.
 *
 * The script's window test is strict (utime - last.utime > threshold), so truth messages exactly 10 s apart would close a
 * window only every 20 s with its default threshold of 10.0: the threshold here is 9 s.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/score_sweep.c -Lpronto_amd/lib -lpronto_batch -lm -o score_sweep
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pronto_batch.h"

#define CHECK(call)                                                                     \
  do {                                                                                  \
    int rc_ = (call);                                                                   \
    if (rc_ != PB_OK) {                                                                 \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, pb_last_error(ctx));                \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

static uint64_t rng = 88172645463325252ULL;
static double urand(void)
{
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return ((rng >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand(void) { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }

int main(void)
{
  enum { NR = 16, NQ = 8, B = NR * NQ, SEG = 1000, NSEG = 8, N = 15 };
  const double g = 9.80665, dt = 1e-2, true_r = 0.1;  /* 100 Hz; true leg-odometry noise 0.1 m/s */
  pb_ctx *ctx = NULL;
  if (pb_create(&ctx, N, B, 0, 0) != PB_OK) {
    fprintf(stderr, "pb_create: %s\n", pb_last_error(NULL));
    return 2;
  }
  /* the robot: forward speed v (body x) and yaw rate w; truth = (x, y, yaw) */
  double x = 0, y = 0, yaw = 0, t = 0;
  double x0[N] = { 0 }, q0[4] = { 1, 0, 0, 0 }, P0[N * N] = { 0 };
  x0[3] = 0.5;
  for (int i = 3; i < 12; i++) P0[i * N + i] = (i < 6) ? 0.0225 : (i < 9 ? 0.0027 : 0.01);
  CHECK(pb_reset(ctx, x0, q0, P0, 1, PB_HOST));
  CHECK(pb_score_init(ctx, 9.0, 0.0));

  double *imu = malloc(sizeof(double) * (size_t) SEG * 7 * B), *lo = malloc(sizeof(double) * (size_t) SEG * 6 * B);
  double *qblk = malloc(sizeof(double) * 4 * B);
  for (int b = 0; b < B; b++) {
    const double qg = 0.5 * pow(1.3, b / NR) * M_PI / 180.0; /* candidate q_gyro (deg/s -> rad/s) */
    qblk[b] = qg * qg; qblk[B + b] = 0.01; qblk[2 * B + b] = 0; qblk[3 * B + b] = 0;
  }
  void *d_imu, *d_lo, *d_q;
  CHECK(pb_malloc(ctx, sizeof(double) * (size_t) SEG * 7 * B, &d_imu));
  CHECK(pb_malloc(ctx, sizeof(double) * (size_t) SEG * 6 * B, &d_lo));
  CHECK(pb_malloc(ctx, sizeof(double) * 4 * B, &d_q));
  CHECK(pb_memcpy_h2d(ctx, d_q, qblk, sizeof(double) * 4 * B));
  CHECK(pb_set_process_noise_block(ctx, d_q));

  const double q_unused[4] = { 0, 0, 0, 0 };
  float ms_total = 0;
  for (int s = 0; s <= NSEG; s++) {
    /* the ground-truth message at the segment boundary: one pose for every candidate */
    const double pose7[7] = { x, y, 0.0, cos(0.5 * yaw), 0.0, 0.0, sin(0.5 * yaw) };
    CHECK(pb_score_ground_truth(ctx, (int64_t) llround(t * 1e6), NULL, pose7, NULL, PB_SLOT_HEAD, PB_SCORE_DRIFT | PB_SCORE_ABS,
                                PB_HOST_BROADCAST));
    if (s == NSEG) break;
    for (int k = 0; k < SEG; k++) {
      const double v = 0.5 + 0.2 * sin(0.05 * t), vdot = 0.2 * 0.05 * cos(0.05 * t), w = 0.15 * sin(0.11 * t);
      /* planar motion with body velocity (v, 0, 0): body acceleration (vdot, w v, 0), specific force adds g along body z */
      const double gyro[3] = { 0.01 * nrand(), 0.01 * nrand(), w + 0.01 * nrand() };
      const double acc[3] = { vdot + 0.1 * nrand(), w * v + 0.1 * nrand(), g + 0.1 * nrand() };
      x += v * cos(yaw) * dt; y += v * sin(yaw) * dt; yaw += w * dt; t += dt;
      const double vn = 0.5 + 0.2 * sin(0.05 * t);
      const double z[3] = { vn + true_r * nrand(), true_r * nrand(), true_r * nrand() };
      for (int b = 0; b < B; b++) {
        const double r = 0.02 * pow(1.25, b % NR); /* candidate r_vxyz: 0.02 ... 0.57 */
        for (int i = 0; i < 3; i++) {
          imu[((size_t) k * 7 + i) * B + b] = gyro[i];
          imu[((size_t) k * 7 + 3 + i) * B + b] = acc[i];
          lo[((size_t) k * 6 + i) * B + b] = z[i];
          lo[((size_t) k * 6 + 3 + i) * B + b] = r * r;
        }
        imu[((size_t) k * 7 + 6) * B + b] = dt;
      }
    }
    float ms = 0;
    CHECK(pb_memcpy_h2d(ctx, d_imu, imu, sizeof(double) * (size_t) SEG * 7 * B));
    CHECK(pb_memcpy_h2d(ctx, d_lo, lo, sizeof(double) * (size_t) SEG * 6 * B));
    CHECK(pb_run_legodo(ctx, SEG, d_imu, d_lo, NULL, q_unused, &ms));
    ms_total += ms;
  }

  double ll[B];
  CHECK(pb_get_head(ctx, 0, B, NULL, NULL, NULL, ll, PB_HOST));
  int by_ll = 0;
  for (int b = 1; b < B; b++)
    if (ll[b] > ll[by_ll]) by_ll = b;
  int by_ddt = -1, by_ate = -1;
  double ddt = 0, ate = 0;
  CHECK(pb_score_best(ctx, PB_SCORE_MEAN_PDDT, &by_ddt, &ddt));
  CHECK(pb_score_best(ctx, PB_SCORE_ATE_RMSE, &by_ate, &ate));
  int64_t ut = 0;
  double em[10];
  const int ok = by_ddt >= 0 && by_ddt < B && by_ate >= 0 && by_ate < B;
  printf("%d candidates x %d steps in %.2f ms (%s)\n", B, SEG * NSEG, ms_total, pb_hot_kernel(ctx));
  printf("  best log-likelihood     : filter %3d  r_vxyz = %.3f  q_gyro index %d  (ll %.1f)\n", by_ll, 0.02 * pow(1.25, by_ll % NR), by_ll / NR, ll[by_ll]);
  if (ok) {
    CHECK(pb_score_last(ctx, by_ddt, &ut, em));
    printf("  best mean %%DDT          : filter %3d  r_vxyz = %.3f  q_gyro index %d  (%.3f %% drift per distance travelled)\n", by_ddt,
           0.02 * pow(1.25, by_ddt % NR), by_ddt / NR, ddt);
    printf("    its last window (utime %lld): %.3f m drift in %.2f m travelled, yaw error %.3f deg, time_elapsed %.1f s (the script's sign)\n",
           (long long) ut, em[3], em[7], em[6], em[9]);
    printf("  best absolute error     : filter %3d  r_vxyz = %.3f  q_gyro index %d  (rmse %.3f m); true r_vxyz %.3f\n", by_ate,
           0.02 * pow(1.25, by_ate % NR), by_ate / NR, ate, true_r);
  }
  printf(ok ? "PASS\n" : "FAIL\n");
  pb_free(ctx, d_imu); pb_free(ctx, d_lo); pb_free(ctx, d_q);
  pb_destroy(ctx);
  free(imu); free(lo); free(qblk);
  return ok ? 0 : 1;
}
