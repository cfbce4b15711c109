/* leg_noise_sweep.c -- a parameter sweep over the MEASUREMENT side of the leg odometry, in plain C on the C ABI: what the reference
 * does with one process per `-O key=value` override (state-estimator/python/param_sweep.py:39-52) as one batch.  ONE robot's IMU +
 * joint-state log (PB_HOST_BROADCAST) drives every filter; each filter has its own leg-odometry noise r_vxyz (with r_vxyz_uncertain
 * twice that) and its own schmitt_high_threshold of the contact detector (pb_legodo_set_param_block), a 16 x 16 grid.  The pelvis
 * pose the gait was made for is scored as ground truth on the device (pb_score_ground_truth, one broadcast message every 0.1 s) and
 * pb_score_best names the candidate with the smallest absolute trajectory error.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/leg_noise_sweep.c -Lpronto_amd/lib -lpronto_batch -lm -o leg_noise_sweep
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

static uint64_t rng = 0x1234567887654321ULL;
static double urand(void)
{
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return ((rng >> 11) + 0.5) / 9007199254740992.0;
}
static double nrand(void) { return sqrt(-2 * log(urand())) * cos(2 * M_PI * urand()); }
static double ramp(double x) { return x < 0 ? 0 : (x > 0.05 ? 1.0 : x / 0.05); }

int main(void)
{
  enum { NR = 16, NH = 16, B = NR * NH, T = 1500, N = 15, NJ = 12, EVERY = 50 };
  pb_ctx *ctx = NULL;
  if (pb_create(&ctx, N, B, 0, 0) != PB_OK) {
    fprintf(stderr, "pb_create: %s\n", pb_last_error(NULL));
    return 2;
  }
  double x0[N] = { 0 }, q0[4] = { 1, 0, 0, 0 }, P0[N * N] = { 0 };
  x0[11] = 0.86; /* pelvis height */
  for (int i = 3; i < 12; i++) P0[i * N + i] = (i < 6) ? 0.0225 : (i < 9 ? 0.0027 : 0.25);
  CHECK(pb_reset(ctx, x0, q0, P0, 1, PB_HOST));

  /* leg_estimate's parameters (leg_estimate.cpp:93-121) and the two kinematic chains: hip yaw / roll / pitch, knee, ankle pitch /
   * roll per leg (test values; pb_legodo_set_chain takes what kdl_parser reads out of the URDF: <origin xyz rpy>, <axis>) */
  CHECK(pb_legodo_init(ctx, 475.0, 525.0, 7000, 7000, 1));
  int type[2 * 6], row[2 * 6];
  double org[2 * 6 * 6] = { 0 }, axis[2 * 6 * 3] = { 0 };
  float gain[2 * 6];
  const double xyz[6][3] = { { 0, 0.089, 0 }, { 0, 0, 0 }, { 0.05, 0.0225, -0.066 }, { -0.05, 0, -0.374 }, { 0, 0, -0.422 }, { 0, 0, 0 } };
  const int ax[6] = { 2, 0, 1, 1, 1, 0 };
  for (int side = 0; side < 2; side++)
    for (int j = 0; j < 6; j++) {
      const int k = 6 * side + j;
      type[k] = 1; /* revolute */
      row[k] = k;  /* row of the joint-position block */
      for (int i = 0; i < 3; i++) org[6 * k + i] = xyz[j][i];
      if (side) org[6 * k + 1] = -org[6 * k + 1];
      axis[3 * k + ax[j]] = 1.0;
      gain[k] = (j == 3) ? 10000.0f : 0.0f; /* torque adjustment on the knees (rbis_legodo_update.cpp:29-53) */
    }
  CHECK(pb_legodo_set_chain(ctx, 6, 6, type, row, org, axis, gain));
  CHECK(pb_joint_filter_init(ctx, 1 /* lowpass */, 0.01, 5e-4, 5e-4)); /* state_estimator.legodo.filter_joint_positions */

  /* the candidates: r_vxyz (rows of the grid) x schmitt_high_threshold (columns); every other row holds one value */
  double *blk = malloc(sizeof(double) * PB_LEGPAR_ROWS * B);
  for (int b = 0; b < B; b++) {
    const double r = 5.0 * pow(1.15, b / NH), high = 480.0 + 25.0 * (b % NH);
    blk[PB_LEGPAR_R_VXYZ * B + b] = r;
    blk[PB_LEGPAR_R_VXYZ_UNCERTAIN * B + b] = 2.0 * r;
    blk[PB_LEGPAR_R_VANG * B + b] = blk[PB_LEGPAR_R_VANG_UNCERTAIN * B + b] = blk[PB_LEGPAR_R_XYZ * B + b] = 0.0;  /* (lin_rate reads none) */
    blk[PB_LEGPAR_SCHMITT_LOW * B + b] = 475.0;
    blk[PB_LEGPAR_SCHMITT_HIGH * B + b] = high;
    blk[PB_LEGPAR_SCHMITT_LOW_DELAY * B + b] = blk[PB_LEGPAR_SCHMITT_HIGH_DELAY * B + b] = 7000.0;
    blk[PB_LEGPAR_TOTAL_FORCE * B + b] = blk[PB_LEGPAR_STANDING_SCHMITT_LEVEL * B + b] = 0.0;  /* (the "standing" contact mode's) */
  }
  CHECK(pb_legodo_set_param_block(ctx, blk, PB_HOST));   /* copied: the array is free again */
  CHECK(pb_score_init(ctx, 0.5, 0.0));

  /* one robot walks: 500 Hz IMU + joint-state pairs */
  const double g = 9.80665, dt = 0.002, period = 1.1, swing = 0.25;
  const double speed = 0.3, qg = 0.3 * M_PI / 180.0, q[4] = { qg * qg, 0.04 * 0.04, 0, 0 };
  for (int k = 0; k < T; k++) {
    const int64_t utime = 1000000 + (int64_t) (k + 1) * 2000;
    const double t = (k + 1) * dt;
    double ph = t / period;
    ph -= floor(ph);
    double wl = ramp(ph) * ramp(0.6 - ph), wr = ramp(ph - 0.5) * ramp(1.1 - ph) + (ph < 0.1 ? ramp(0.1 - ph) : 0.0);
    if (t < 0.4) wl = wr = 1.0;
    const double sw = sin(2 * M_PI * ph);
    float jp[NJ], jv[NJ] = { 0 }, je[NJ], jf[NJ], ff[2] = { (float) fabs(900 * wl + 5 * nrand()), (float) fabs(900 * wr + 5 * nrand()) };
    for (int side = 0; side < 2; side++) {
      const double sgn = side ? -1.0 : 1.0, lift = fmax(0.0, -sgn * sw);
      float *p = jp + 6 * side;
      p[0] = (float) (0.05 * sgn * sw);
      p[1] = (float) (0.03 * sgn + 0.02 * sw);
      p[2] = (float) (-0.35 - sgn * swing * sw - 0.2 * lift);
      p[3] = (float) (0.7 + 0.5 * lift);
      p[4] = (float) (-0.35 + sgn * swing * sw * 0.5 - 0.3 * lift);
      p[5] = (float) (-0.03 * sgn - 0.02 * sw);
    }
    for (int j = 0; j < NJ; j++) { jp[j] += (float) (0.002 * nrand()); je[j] = (float) (40 * nrand()); }
    const double imu[7] = { 0.01 * nrand(), 0.01 * nrand(), 0.01 * nrand(), 0.2 * nrand(), 0.2 * nrand(), g + 0.2 * nrand(), dt };
    /* torque adjustment + joint filters (one robot: on the host, output [NJ]), then IMU step + odometry + update: one kernel */
    CHECK(pb_joint_filter(ctx, utime, NJ, jp, jv, je, PB_HOST_BROADCAST, jf));
    /* (the two noise arguments are ignored while a parameter block is set) */
    CHECK(pb_step_legodo_joints(ctx, imu, PB_HOST_BROADCAST, q, utime, NJ, jf, NULL, ff, PB_HOST_BROADCAST, 0.0, 0.0, NULL, NULL));
    if ((k + 1) % EVERY == 0) {  /* the ground truth: the pelvis walks forward at the gait's nominal speed, upright */
      const double pose7[7] = { speed * (t - 0.4 > 0 ? t - 0.4 : 0.0), 0.0, 0.86, 1.0, 0.0, 0.0, 0.0 };
      CHECK(pb_score_ground_truth(ctx, utime, NULL, pose7, NULL, PB_SLOT_HEAD, PB_SCORE_DRIFT | PB_SCORE_ABS, PB_HOST_BROADCAST));
    }
  }
  double sum[4], *vec = malloc(sizeof(double) * N * B), *rows = malloc(sizeof(double) * PB_SCORE_ROWS * B), *score = malloc(sizeof(double) * B);
  int64_t *counts = malloc(sizeof(int64_t) * PB_SCORE_COUNTS * B);
  CHECK(pb_summary(ctx, sum));
  CHECK(pb_get_head(ctx, 0, B, vec, NULL, NULL, NULL, PB_HOST));
  CHECK(pb_score_get(ctx, 0, B, rows, counts, PB_HOST));
  int best = -1, finite = sum[3] == 0;
  double best_rmse = 0;
  CHECK(pb_score_best(ctx, PB_SCORE_ATE_RMSE, &best, &best_rmse));
  for (int i = 0; i < N * B; i++) finite = finite && isfinite(vec[i]);
  for (int b = 0; b < B; b++) score[b] = sqrt(rows[PB_SCORE_ABS_SUM_SQ * B + b] / (double) counts[PB_SCORE_ABS_N * B + b]);
  /* the score must depend on both swept parameters: not constant along either axis of the grid */
  int varies_r = 0, varies_h = 0;
  for (int b = 0; b < B; b++) {
    varies_r = varies_r || score[b] != score[b % NH];          /* against the first row, same column */
    varies_h = varies_h || score[b] != score[(b / NH) * NH];   /* against the first column, same row */
  }
  const int ok = finite && best >= 0 && best < B && varies_r && varies_h;
  if (best >= 0 && best < B)
    printf("%d candidates x %d message pairs (%s): smallest absolute trajectory error %.4f m (worst %s) at r_vxyz = %.2f m/s, "
           "schmitt_high_threshold = %.0f N (filter %d)\n", B, T, pb_hot_kernel(ctx), best_rmse, finite ? "finite" : "NOT finite",
           5.0 * pow(1.15, best / NH), 480.0 + 25.0 * (best % NH), best);
  printf(ok ? "PASS\n" : "FAIL\n");
  pb_destroy(ctx);
  free(blk); free(vec); free(rows); free(score); free(counts);
  return ok ? 0 : 1;
}
