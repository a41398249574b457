// The truncated-normal terms that vlnce_waypoint_eval (waypoint_dist.hip) and vlnce_waypoint_act
// (waypoint_act.hip) share, so that the log-probability a rollout stores and the one
// evaluate_actions later computes for the same element are ONE arithmetic.  fp64 throughout.
#pragma once
#include "common.h"

constexpr int WP_THREADS = 64;
constexpr int WP_MAX_P = 63;
constexpr int WP_MAX_K = 32;

constexpr double WP_SQRT_2PI = 2.50662827463100050242;
constexpr double WP_INV_SQRT_2PI = 0.398942280401432677940;
constexpr double WP_INV_SQRT2 = 0.707106781186547524401;
constexpr double WP_HALF_LOG_2PIE = 1.41893853320467274178;   // log(2 pi e) / 2

// N(loc, s^2) on [lo, hi] (models/utils.py:24-152): the standardised window [a, b], its mass under
// the parent normal, the densities at its ends, and the two edge terms of the moments
struct WpTruncated {
  double s, a, b, mass, pa, pb;
  double e1;   // (pdf(a) - pdf(b)) / mass
  double e2;   // (a pdf(a) - b pdf(b)) / mass
};

__device__ inline WpTruncated wp_truncated_terms(double loc, double var, double lo, double hi) {
  WpTruncated t;
  t.s = sqrt(var);
  t.a = (lo - loc) / t.s;
  t.b = (hi - loc) / t.s;
  t.mass = 0.5 * (erf(t.b * WP_INV_SQRT2) - erf(t.a * WP_INV_SQRT2));
  t.pa = exp(-0.5 * t.a * t.a) * WP_INV_SQRT_2PI;
  t.pb = exp(-0.5 * t.b * t.b) * WP_INV_SQRT_2PI;
  t.e1 = (t.pa - t.pb) / t.mass;
  t.e2 = (t.a * t.pa - t.b * t.pb) / t.mass;
  return t;
}

// log p(v), and z = (v - loc) / s
__device__ inline double wp_truncated_logp(const WpTruncated& t, double loc, double v, double* z_out) {
  const double z = (v - loc) / t.s;
  *z_out = z;
  return -0.5 * z * z - log(WP_SQRT_2PI * t.s * t.mass);
}

inline bool wp_kind_ok(int kind, int K) {
  if (kind == VLNCE_WP_DISCRETE) return K >= 1 && K <= WP_MAX_K;
  return kind == VLNCE_WP_ABSENT || kind == VLNCE_WP_CONTINUOUS;
}
