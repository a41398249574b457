// The distribution arithmetic of WaypointPolicy.evaluate_actions (waypoint_policy.py:258-347 over
// TruncatedNormal / CustomFixedCategorical, models/utils.py:24-152, 269-289) on the device: the
// composite log-probability and the three entropies of a stored action in ONE launch, their
// gradients in ONE more.  One thread per row, the whole row in fp64, one rounding to fp32 at each
// store, no floating-point atomics: two runs give the same bits.
//
// saved [S][B] (row b of plane s at s * B + b), the partial derivatives the backward multiplies
// with the incoming gradients, gate * weight folded in:
//   planes 0 .. P            d logp_pano / d logits[b, i]
//   planes P+1 .. 2P+1       d H_pano    / d logits[b, i]
//   then per part (offset, distance):
//     continuous (4 planes)  d logp / d loc, d logp / d variance, d H / d loc, d H / d variance
//     discrete (2 K planes)  d logp / d first[b, h, j] (K planes), d H / d first[b, h, j] (K planes);
//                            the H planes WITHOUT gate * weight: a discrete part's entropy output is
//                            the reference's [B, B] broadcast E[i][j] = gate_i weight H_j, whose
//                            backward sums column j over the rows' gates
#include <stdint.h>

#include <limits>

#include "waypoint_math.h"

namespace {

__host__ __device__ inline int wp_saved_planes(int kind, int K) {
  return kind == VLNCE_WP_CONTINUOUS ? 4 : kind == VLNCE_WP_DISCRETE ? 2 * K : 0;
}

// logp of class `c` and the entropy of the categorical over z[0 .. n) (stride 1), and their
// gradients times `w` / `wh` into the saved planes dlp / dh (plane j at j * B).  `ok` false (the class is
// out of range): nothing is read through c.  A class of probability 0 contributes 0 to the entropy
// and gets a zero entropy gradient (torch clamps log p at the smallest float before p * log p).
__device__ inline void wp_categorical(const float* __restrict__ z, int n, long c, bool ok, double w,
                                      double wh, double* logp, double* ent,
                                      float* __restrict__ dlp, float* __restrict__ dh, long B) {
  float zmax = z[0];
  for (int i = 1; i < n; ++i) zmax = fmaxf(zmax, z[i]);
  double se = 0.0;
  for (int i = 0; i < n; ++i) se += exp((double)z[i] - (double)zmax);
  const double lse = (double)zmax + log(se);
  double h = 0.0;
  for (int i = 0; i < n; ++i) {
    const double lp = (double)z[i] - lse, p = exp(lp);
    if (p > 0.0 || p != p) h -= p * lp;
  }
  *logp = ok ? (double)z[c] - lse : std::numeric_limits<double>::quiet_NaN();
  *ent = h;
  for (int i = 0; i < n; ++i) {
    const double lp = (double)z[i] - lse, p = exp(lp);
    dlp[(long)i * B] = (float)(w * ((ok && i == c ? 1.0 : 0.0) - p));
    dh[(long)i * B] = (float)(wh * ((p > 0.0 || p != p) ? -p * (lp + h) : 0.0));
  }
}

// the truncated normal of models/utils.py:24-152 on [lo, hi]: log p(v), the entropy, and their
// derivatives with respect to loc and to the VARIANCE (scale = sqrt(variance))
__device__ inline void wp_truncated_normal(double loc, double var, double v, double lo, double hi,
                                           double* logp, double* ent, double d[4]) {
  const WpTruncated t = wp_truncated_terms(loc, var, lo, hi);
  const double s = t.s, a = t.a, b = t.b, mass = t.mass, pa = t.pa, pb = t.pb, e1 = t.e1, e2 = t.e2;
  double z;
  *logp = wp_truncated_logp(t, loc, v, &z);
  *ent = WP_HALF_LOG_2PIE + log(s * mass) + 0.5 * e2;
  // d a / d loc = d b / d loc = -1 / s; d a / d s = -a / s, d b / d s = -b / s;
  // d mass / d loc = (pa - pb) / s; d mass / d s = (a pa - b pb) / s; d (x pdf(x)) / d x = pdf(x) (1 - x^2)
  const double qa = pa * (1.0 - a * a), qb = pb * (1.0 - b * b);
  const double dlp_loc = (z - e1) / s;
  const double dlp_s = (z * z - 1.0 - e2) / s;
  const double dh_loc = (e1 + 0.5 * (-(qa - qb) / mass - e2 * e1)) / s;
  const double dh_s = (1.0 + e2 + 0.5 * (-(a * qa - b * qb) / mass - e2 * e2)) / s;
  const double half_inv_s = 0.5 / s;   // d s / d variance
  d[0] = dlp_loc;
  d[1] = dlp_s * half_inv_s;
  d[2] = dh_loc;
  d[3] = dh_s * half_inv_s;
}

// gate * weight of row i, from its panorama choice alone (0 for a choice outside [0, P])
__device__ inline double wp_row_weight(const long* __restrict__ pano, long i, int P, float weight,
                                       bool* ok) {
  const long c = pano[i];
  *ok = c >= 0 && c <= P;
  return *ok && c != P ? (double)weight : 0.0;
}

// one component of row b at heading h: adds its flags, returns gate * weight * logp and the entropy
// (continuous: times gate * weight; discrete: the row's own H, see the [B, B] output) in fp64
__device__ inline void wp_part_fwd(const vlnce_wp_part& part, int shift, long b, int h, bool h_ok,
                                   double gate, int P, long B, float* __restrict__ saved,
                                   int* flags, double* logp, double* ent) {
  *logp = 0.0;
  *ent = 0.0;
  if (part.kind == VLNCE_WP_ABSENT) return;
  const double w = gate * (double)part.weight;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (part.kind == VLNCE_WP_CONTINUOUS) {
    const float v = static_cast<const float*>(part.element)[b];
    double lp = nan, e = nan, d[4] = {nan, nan, nan, nan};
    if (!(v >= part.lo && v <= part.hi)) *flags |= VLNCE_WP_FLAG_ELEMENT << shift;
    if (h_ok) {
      const float loc = part.first[b * P + h], var = part.second[b * P + h];
      if (!(loc >= part.lo && loc <= part.hi)) *flags |= VLNCE_WP_FLAG_LOC << shift;
      if (!(sqrtf(var) >= 0.f)) *flags |= VLNCE_WP_FLAG_VARIANCE << shift;
      wp_truncated_normal((double)loc, (double)var, (double)v, (double)part.lo, (double)part.hi, &lp,
                          &e, d);
    }
    *logp = w * lp;
    *ent = w * e;
    for (int k = 0; k < 4; ++k) saved[(long)k * B] = (float)(w * d[k]);
    return;
  }
  const int K = part.K;
  const long c = static_cast<const long*>(part.element)[b];
  const bool c_ok = c >= 0 && c < K;
  if (!c_ok) *flags |= VLNCE_WP_FLAG_CLASS << shift;
  if (h_ok) {
    double lp, e;
    wp_categorical(part.first + (b * P + h) * K, K, c, c_ok, w, 1.0, &lp, &e, saved,
                   saved + (long)K * B, B);
    *logp = w * lp;
    *ent = e;
  } else {
    *logp = nan;
    *ent = nan;
  }
}

__global__ __launch_bounds__(WP_THREADS) void waypoint_eval_kernel(
    const float* __restrict__ logits, const long* __restrict__ pano, vlnce_wp_part offset,
    vlnce_wp_part distance, int B_, int P, float* __restrict__ out, float* __restrict__ saved,
    int* __restrict__ flags) {
  const long B = B_;
  const long b = (long)blockIdx.x * WP_THREADS + threadIdx.x;
  if (b >= B) return;
  const long c = pano[b];
  const bool c_ok = c >= 0 && c <= P;
  const int h = c_ok ? (int)(c % P) : 0;
  const double gate = c_ok && c != P ? 1.0 : 0.0;
  int fl = c_ok ? 0 : VLNCE_WP_FLAG_PANO;

  double lp_pano, h_pano, lp_o, h_o, lp_d, h_d;
  float* sv = saved + b;
  wp_categorical(logits + b * (P + 1), P + 1, c, c_ok, 1.0, 1.0, &lp_pano, &h_pano, sv,
                 sv + (long)(P + 1) * B, B);
  sv += 2L * (P + 1) * B;
  wp_part_fwd(offset, VLNCE_WP_FLAG_SHIFT_OFFSET, b, h, c_ok, gate, P, B, sv, &fl, &lp_o, &h_o);
  sv += (long)wp_saved_planes(offset.kind, offset.K) * B;
  wp_part_fwd(distance, VLNCE_WP_FLAG_SHIFT_DISTANCE, b, h, c_ok, gate, P, B, sv, &fl, &lp_d, &h_d);

  const float nan = std::numeric_limits<float>::quiet_NaN();
  flags[b] = fl;
  out[b] = fl ? nan : (float)(lp_pano + lp_d + lp_o);   // the reference adds distance, then offset
  out[B + b] = fl ? nan : (float)h_pano;
  float* e_out = out + 2 * B;
  const vlnce_wp_part* parts[2] = {&offset, &distance};
  const double ents[2] = {h_o, h_d};
  for (int k = 0; k < 2; ++k) {
    if (parts[k]->kind != VLNCE_WP_DISCRETE) {
      e_out[b] = fl ? nan : (float)ents[k];
      e_out += B;
      continue;
    }
    for (long i = 0; i < B; ++i) {   // column b of E[i][b] = gate_i weight H_b
      bool ok;
      const double wi = wp_row_weight(pano, i, P, parts[k]->weight, &ok);
      e_out[i * B + b] = (fl || !ok) ? nan : (float)(wi * ents[k]);
    }
    e_out += B * B;
  }
}

// dense gradient of one component for row b: the chosen heading gets saved * g, the rest zero; a
// flagged row is NaN throughout
__device__ inline void wp_part_bwd(const vlnce_wp_part_grad& part, long b, int h, bool flagged,
                                   double g_logp, const float* __restrict__ g, int P, long B,
                                   const long* __restrict__ pano, const float* __restrict__ saved) {
  if (part.kind == VLNCE_WP_ABSENT) return;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  double g_ent = 0.0;
  if (g && part.kind == VLNCE_WP_CONTINUOUS) g_ent = (double)g[b];
  if (g && part.kind == VLNCE_WP_DISCRETE)
    for (long i = 0; i < B; ++i) {   // column b of the [B, B] gradient, rows in order
      bool ok;
      const double wi = wp_row_weight(pano, i, P, part.weight, &ok);
      if (ok) g_ent += wi * (double)g[i * B + b];
    }
  if (part.kind == VLNCE_WP_CONTINUOUS) {
    const float dloc = (float)((double)saved[0] * g_logp + (double)saved[2 * B] * g_ent);
    const float dvar = (float)((double)saved[B] * g_logp + (double)saved[3 * B] * g_ent);
    for (int i = 0; i < P; ++i) {
      part.d_first[b * P + i] = flagged ? nan : i == h ? dloc : 0.f;
      part.d_second[b * P + i] = flagged ? nan : i == h ? dvar : 0.f;
    }
    return;
  }
  const int K = part.K;
  float* row = part.d_first + b * P * K;
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < K; ++j) {
      float v = 0.f;
      if (flagged) v = nan;
      else if (i == h)
        v = (float)((double)saved[(long)j * B] * g_logp + (double)saved[(long)(K + j) * B] * g_ent);
      row[i * K + j] = v;
    }
}

__global__ __launch_bounds__(WP_THREADS) void waypoint_eval_bwd_kernel(
    const float* __restrict__ g_logp, const float* __restrict__ g_ent_pano,
    const float* __restrict__ g_ent_offset, const float* __restrict__ g_ent_distance,
    const long* __restrict__ pano, const float* __restrict__ saved, const int* __restrict__ flags,
    vlnce_wp_part_grad offset, vlnce_wp_part_grad distance, int B_, int P,
    float* __restrict__ d_logits) {
  const long B = B_;
  const long b = (long)blockIdx.x * WP_THREADS + threadIdx.x;
  if (b >= B) return;
  const bool flagged = flags[b] != 0;
  const long c = pano[b];
  const int h = (c >= 0 && c <= P) ? (int)(c % P) : 0;
  const double gl = g_logp ? (double)g_logp[b] : 0.0;
  const double gp = g_ent_pano ? (double)g_ent_pano[b] : 0.0;
  const float nan = std::numeric_limits<float>::quiet_NaN();

  const float* sv = saved + b;
  for (int i = 0; i <= P; ++i) {
    const double v = (double)sv[(long)i * B] * gl + (double)sv[(long)(P + 1 + i) * B] * gp;
    d_logits[b * (P + 1) + i] = flagged ? nan : (float)v;
  }
  sv += 2L * (P + 1) * B;
  wp_part_bwd(offset, b, h, flagged, gl, g_ent_offset, P, B, pano, sv);
  sv += (long)wp_saved_planes(offset.kind, offset.K) * B;
  wp_part_bwd(distance, b, h, flagged, gl, g_ent_distance, P, B, pano, sv);
}

}  // namespace

extern "C" int vlnce_waypoint_eval_supported(int B, int P, int K_offset, int K_distance) {
  return B >= 1 && P >= 1 && P <= WP_MAX_P && K_offset >= 0 && K_offset <= WP_MAX_K &&
         K_distance >= 0 && K_distance <= WP_MAX_K;
}

extern "C" int vlnce_waypoint_eval(const float* logits, const int64_t* pano,
                                   const vlnce_wp_part* offset, const vlnce_wp_part* distance, int B,
                                   int P, float* out, long out_floats, float* saved,
                                   long saved_floats, int32_t* flags, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(logits && pano && offset && distance && out && saved && flags,
                  "waypoint_eval: null argument");
  const vlnce_wp_part* parts[2] = {offset, distance};
  for (const vlnce_wp_part* p : parts) {
    VLNCE_CHECK_ARG(wp_kind_ok(p->kind, p->K),
                    "waypoint_eval: part of kind %d with K = %d (kinds 0..2, 1 <= K <= %d)", p->kind,
                    p->K, WP_MAX_K);
    VLNCE_CHECK_ARG(p->kind == VLNCE_WP_ABSENT || (p->first && p->element),
                    "waypoint_eval: null first / element of a present part");
    VLNCE_CHECK_ARG(p->kind != VLNCE_WP_CONTINUOUS || p->second,
                    "waypoint_eval: null second of a continuous part");
  }
  const int Ko = offset->kind == VLNCE_WP_DISCRETE ? offset->K : 0;
  const int Kd = distance->kind == VLNCE_WP_DISCRETE ? distance->K : 0;
  VLNCE_CHECK_ARG(vlnce_waypoint_eval_supported(B, P, Ko, Kd),
                  "waypoint_eval: B = %d, P = %d, K = %d / %d outside B >= 1, 1 <= P <= %d, K <= %d", B,
                  P, Ko, Kd, WP_MAX_P, WP_MAX_K);
  const long S = 2L * (P + 1) + wp_saved_planes(offset->kind, offset->K) +
                 wp_saved_planes(distance->kind, distance->K);
  VLNCE_CHECK_ARG(saved_floats >= S * (long)B, "waypoint_eval: saved holds %ld floats, %ld needed",
                  saved_floats, S * (long)B);
  const long O = (long)B * (2 + (Ko ? B : 1) + (Kd ? B : 1));
  VLNCE_CHECK_ARG(out_floats >= O, "waypoint_eval: out holds %ld floats, %ld needed", out_floats, O);
  hipLaunchKernelGGL(waypoint_eval_kernel, dim3((B + WP_THREADS - 1) / WP_THREADS), dim3(WP_THREADS),
                     0, reinterpret_cast<hipStream_t>(stream), logits,
                     reinterpret_cast<const long*>(pano), *offset, *distance, B, P, out, saved, flags);
  VLNCE_CHECK_LAUNCH("waypoint_eval");
  return 0;
}

extern "C" int vlnce_waypoint_eval_bwd(const float* g_logp, const float* g_ent_pano,
                                       const float* g_ent_offset, const float* g_ent_distance,
                                       const int64_t* pano, const float* saved, const int32_t* flags,
                                       const vlnce_wp_part_grad* offset,
                                       const vlnce_wp_part_grad* distance, int B, int P,
                                       float* d_logits, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(pano && saved && flags && offset && distance && d_logits,
                  "waypoint_eval_bwd: null argument");
  const vlnce_wp_part_grad* parts[2] = {offset, distance};
  for (const vlnce_wp_part_grad* p : parts) {
    VLNCE_CHECK_ARG(wp_kind_ok(p->kind, p->K),
                    "waypoint_eval_bwd: part of kind %d with K = %d (kinds 0..2, 1 <= K <= %d)",
                    p->kind, p->K, WP_MAX_K);
    VLNCE_CHECK_ARG(p->kind == VLNCE_WP_ABSENT || p->d_first,
                    "waypoint_eval_bwd: null d_first of a present part");
    VLNCE_CHECK_ARG(p->kind != VLNCE_WP_CONTINUOUS || p->d_second,
                    "waypoint_eval_bwd: null d_second of a continuous part");
  }
  const int Ko = offset->kind == VLNCE_WP_DISCRETE ? offset->K : 0;
  const int Kd = distance->kind == VLNCE_WP_DISCRETE ? distance->K : 0;
  VLNCE_CHECK_ARG(vlnce_waypoint_eval_supported(B, P, Ko, Kd),
                  "waypoint_eval_bwd: B = %d, P = %d, K = %d / %d outside B >= 1, 1 <= P <= %d, K <= %d",
                  B, P, Ko, Kd, WP_MAX_P, WP_MAX_K);
  hipLaunchKernelGGL(waypoint_eval_bwd_kernel, dim3((B + WP_THREADS - 1) / WP_THREADS),
                     dim3(WP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g_logp, g_ent_pano,
                     g_ent_offset, g_ent_distance, reinterpret_cast<const long*>(pano), saved, flags,
                     *offset, *distance, B, P, d_logits);
  VLNCE_CHECK_LAUNCH("waypoint_eval_bwd");
  return 0;
}
