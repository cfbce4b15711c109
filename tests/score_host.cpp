// score_host.cpp -- g++ build of the per-lane functions of the ground-truth scorer (pronto_amd/csrc/rbis_score.hpp), test-only:
// the code the kernel k_score_gt runs per filter, driven here for B filters in a host loop (tests/test_score_host.py).
#include <stdint.h>

#include "../pronto_amd/csrc/rbis_score.hpp"

using namespace pb;

extern "C" {

void sh_rows(int *n_rows, int *n_counts)
{
  *n_rows = PB_SCORE_ROWS;
  *n_counts = PB_SCORE_COUNTS;
}

void sh_reset(double *d, int64_t *iw, int B)
{
  for (long b = 0; b < B; b++) score_reset(d, iw, B, b);
}

// one ground-truth message for B filters: pose7 / est7 [7][B] (pos[3], quat[4]); utimes, valid [B] or NULL; closed [B] out
void sh_message(double *d, int64_t *iw, int B, double time_threshold_s, double distance_threshold, int flags, int64_t utime,
                const int64_t *utimes, const double *pose7, const uint8_t *valid, const double *est7, uint8_t *closed)
{
  ScorePar par;
  par.time_threshold_s = time_threshold_s;
  par.distance_threshold = distance_threshold;
  for (long b = 0; b < B; b++) {
    closed[b] = 0;
    if (valid && valid[b] == 0) continue;
    double p[3], q[4], ep[3], eq[4];
    for (int i = 0; i < 3; i++) { p[i] = pose7[(long) i * B + b]; ep[i] = est7[(long) i * B + b]; }
    for (int i = 0; i < 4; i++) { q[i] = pose7[(long) (3 + i) * B + b]; eq[i] = est7[(long) (3 + i) * B + b]; }
    closed[b] = (uint8_t) score_message(d, iw, B, b, par, flags, utimes ? utimes[b] : utime, p, q, ep, eq);
  }
}

void sh_metric(const double *d, const int64_t *iw, int B, int metric, double *value, uint8_t *has)
{
  for (long b = 0; b < B; b++) {
    value[b] = 0.0;
    has[b] = score_metric(d, iw, B, b, metric, value[b]) ? 1 : 0;
  }
}

// the pose algebra on its own: a, b, ab = 7 doubles each (pos[3], quat[4])
void sh_transform_relative(const double *a, const double *b, double *ab)
{
  ScorePose A, Bp, AB;
  for (int i = 0; i < 3; i++) { A.t[i] = a[i]; Bp.t[i] = b[i]; }
  for (int i = 0; i < 4; i++) { A.q[i] = a[3 + i]; Bp.q[i] = b[3 + i]; }
  score_transform_relative(A, Bp, AB);
  for (int i = 0; i < 3; i++) ab[i] = AB.t[i];
  for (int i = 0; i < 4; i++) ab[3 + i] = AB.q[i];
}

double sh_wrap_deg(double a) { return score_wrap_deg(a); }
}
