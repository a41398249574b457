// The rollout step of the Waypoint DD-PPO trainer on the device (ABI 154).
//   vlnce_waypoint_act           what WaypointPolicy.act does behind the net (waypoint_policy.py:129-247
//                                over TruncatedNormal / CustomFixedCategorical, models/utils.py:24-152,
//                                269-289): the panorama choice, the two sub-actions, their metric values,
//                                modes and variances, the composite log-probability, the normalised
//                                logits and one packed host row per environment, in ONE launch.  One thread
//                                per row, the whole row in fp64, one rounding to fp32 at each store, no
//                                atomics.  The randomness is an INPUT (u [B, 3] uniforms): the launch is a
//                                pure function of its arguments.
//   vlnce_waypoint_history_pick  the trainer's pick of the chosen panorama frame of every sensor
//                                (ddppo_waypoint_trainer.py:190-200) as one launch over a table of fields;
//                                the choice is read on the device.  Plain vector loads and stores.
#include <stdint.h>

#include <limits>

#include "waypoint_math.h"

namespace {

// z - max z and log sum exp of z[0 .. n), the arithmetic of wp_categorical in waypoint_dist.hip
__device__ inline double wp_lse(const float* __restrict__ z, int n, float* zmax_out, double* se_out) {
  float zmax = z[0];
  for (int i = 1; i < n; ++i) zmax = fmaxf(zmax, z[i]);
  double se = 0.0;
  for (int i = 0; i < n; ++i) se += exp((double)z[i] - (double)zmax);
  *zmax_out = zmax;
  *se_out = se;
  return (double)zmax + log(se);
}

__device__ inline int wp_argmax(const float* __restrict__ z, int n) {   // the first maximum
  int c = 0;
  for (int i = 1; i < n; ++i)
    if (z[i] > z[c]) c = i;
  return c;
}

// the first k with sum_{j <= k} p_j > u * S, p_j = exp(z_j - zmax) added up in index order (the order
// of S itself); the last class of non-zero probability when rounding leaves none
__device__ inline int wp_draw_class(const float* __restrict__ z, int n, float zmax, double se, float u) {
  const double t = (double)u * se;
  double cum = 0.0;
  int c = -1, last = 0;
  for (int i = 0; i < n; ++i) {
    const double p = exp((double)z[i] - (double)zmax);
    if (p > 0.0) last = i;
    cum += p;
    if (c < 0 && cum > t) c = i;
  }
  return c < 0 ? last : c;
}

struct ActPartResult {
  double logp;      // of the stored-before-substitution element
  float metric;     // what the simulator gets
  float logged;     // the stored element in metres / radians
  float variance;
};

// one component of row b at heading h: draws, scores, stores element / mode / variance (NaN when
// `flags` ends up non-zero is the caller's: it overwrites), adds the part's flags
__device__ inline ActPartResult wp_act_part(const vlnce_wp_part& part, const vlnce_wp_act_part& out,
                                            int shift, long b, int h, int P, bool deterministic, float u,
                                            int* flags, float* elem_f, long* elem_i, float* mode_f,
                                            long* mode_i) {
  ActPartResult r;
  r.logp = 0.0;
  r.metric = out.off_metric;
  r.logged = out.off_element;
  r.variance = 0.f;
  *elem_f = *mode_f = 0.f;
  *elem_i = *mode_i = 0;
  if (part.kind == VLNCE_WP_ABSENT) return r;
  const bool on = part.weight != 0.f;
  if (part.kind == VLNCE_WP_CONTINUOUS) {
    const float loc = part.first[b * P + h], var = part.second[b * P + h];
    if (!(loc >= part.lo && loc <= part.hi)) *flags |= VLNCE_WP_FLAG_LOC << shift;
    if (!(sqrtf(var) >= 0.f)) *flags |= VLNCE_WP_FLAG_VARIANCE << shift;
    const WpTruncated t = wp_truncated_terms((double)loc, (double)var, (double)part.lo, (double)part.hi);
    double x = (double)loc;
    if (!deterministic) {
      const double fa = 0.5 * erfc(-t.a * WP_INV_SQRT2), fb = 0.5 * erfc(-t.b * WP_INV_SQRT2);
      x = (double)loc + t.s * normcdfinv(fa + (double)u * (fb - fa));
    }
    const float v = fminf(fmaxf((float)x, part.lo), part.hi);
    double z;
    r.logp = wp_truncated_logp(t, (double)loc, (double)v, &z);
    *mode_f = loc;
    if (on) {
      *elem_f = v;
      r.metric = r.logged = v;
      r.variance = (float)(t.s * t.s * (1.0 + t.e2 - t.e1 * t.e1));
    } else {
      *elem_f = out.off_element;
    }
    return r;
  }
  const int K = part.K;
  const float* z = part.first + (b * P + h) * K;
  float zmax;
  double se;
  const double lse = wp_lse(z, K, &zmax, &se);
  const int mode = wp_argmax(z, K);
  const int k = deterministic ? mode : wp_draw_class(z, K, zmax, se, u);
  r.logp = (double)z[k] - lse;
  *mode_i = mode;
  const double step = (out.bin_hi - out.bin_lo) / (double)(K - 1);
  if (on) {
    *elem_i = k;
    r.metric = r.logged = (float)(out.bin_lo + (double)k * step);
    r.variance = std::numeric_limits<float>::quiet_NaN();   // Categorical.variance
  } else {
    r.logged = (float)out.bin_lo;   // class 0 is what is stored
  }
  return r;
}

__device__ inline void wp_act_store(const vlnce_wp_part& part, const vlnce_wp_act_part& out, long b,
                                    bool flagged, float elem_f, long elem_i, float mode_f, long mode_i,
                                    float variance) {
  if (part.kind == VLNCE_WP_ABSENT) return;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  if (part.kind == VLNCE_WP_CONTINUOUS) {
    static_cast<float*>(out.element)[b] = flagged ? nan : elem_f;
    static_cast<float*>(out.mode)[b] = flagged ? nan : mode_f;
  } else {
    static_cast<long*>(out.element)[b] = flagged ? 0 : elem_i;
    static_cast<long*>(out.mode)[b] = flagged ? 0 : mode_i;
  }
  out.variance[b] = flagged ? nan : variance;
}

__global__ __launch_bounds__(WP_THREADS) void waypoint_act_kernel(
    const float* __restrict__ logits, vlnce_wp_part offset, vlnce_wp_part distance,
    vlnce_wp_act_part offset_out, vlnce_wp_act_part distance_out, int deterministic,
    const float* __restrict__ u, int B_, int P, long* __restrict__ pano, float* __restrict__ log_prob,
    float* __restrict__ norm_logits, float* __restrict__ host_rows, int* __restrict__ flags) {
  const long B = B_;
  const long b = (long)blockIdx.x * WP_THREADS + threadIdx.x;
  if (b >= B) return;
  const int n = P + 1;
  const float* z = logits + b * n;
  int fl = 0;
  for (int i = 0; i < n; ++i)
    if (!(fabsf(z[i]) <= std::numeric_limits<float>::max())) fl |= VLNCE_WP_FLAG_PANO;
  const bool det = deterministic != 0;
  const float u0 = det ? 0.f : u[b * 3], u1 = det ? 0.f : u[b * 3 + 1], u2 = det ? 0.f : u[b * 3 + 2];

  float zmax;
  double se;
  const double lse = wp_lse(z, n, &zmax, &se);
  const int c = fl ? P : det ? wp_argmax(z, n) : wp_draw_class(z, n, zmax, se, u0);
  const int h = c % P;
  const double gate = c != P ? 1.0 : 0.0;

  float oe_f, om_f, de_f, dm_f;
  long oe_i, om_i, de_i, dm_i;
  const ActPartResult o = wp_act_part(offset, offset_out, VLNCE_WP_FLAG_SHIFT_OFFSET, b, h, P, det, u1, &fl,
                                      &oe_f, &oe_i, &om_f, &om_i);
  const ActPartResult d = wp_act_part(distance, distance_out, VLNCE_WP_FLAG_SHIFT_DISTANCE, b, h, P, det,
                                      u2, &fl, &de_f, &de_i, &dm_f, &dm_i);
  const bool flagged = fl != 0;
  const float nan = std::numeric_limits<float>::quiet_NaN();

  double lp = (double)z[c] - lse;   // the reference adds distance, then offset
  if (distance.kind != VLNCE_WP_ABSENT && distance.weight != 0.f) lp += gate * (double)distance.weight * d.logp;
  if (offset.kind != VLNCE_WP_ABSENT && offset.weight != 0.f) lp += gate * (double)offset.weight * o.logp;

  const double two_pi = 6.28318530717958647692;
  double theta = fmod((double)h * (two_pi / (double)P) + (double)o.metric, two_pi);
  if (theta < 0.0) theta += two_pi;

  pano[b] = flagged ? P : c;
  flags[b] = fl;
  log_prob[b] = flagged ? nan : (float)lp;
  for (int i = 0; i < n; ++i) norm_logits[b * n + i] = flagged ? nan : (float)((double)z[i] - lse);
  wp_act_store(offset, offset_out, b, flagged, oe_f, oe_i, om_f, om_i, o.variance);
  wp_act_store(distance, distance_out, b, flagged, de_f, de_i, dm_f, dm_i, d.variance);
  float* row = host_rows + b * 8;
  row[0] = (flagged || c == P) ? 1.f : 0.f;
  row[1] = flagged ? nan : d.metric;
  row[2] = flagged ? nan : (float)theta;
  row[3] = flagged ? nan : d.logged;
  row[4] = flagged ? nan : o.logged;
  row[5] = flagged ? nan : d.variance;
  row[6] = flagged ? nan : o.variance;
  row[7] = (float)fl;
}

// ---- history pick
constexpr int HP_CHUNK = VLNCE_ROLLOUT_CHUNK;   // elements of a row per workgroup
constexpr int HP_THREADS = 256;

struct PickFieldArg {
  const unsigned char* src;
  unsigned char* dst;
  long E, src_stride;
  long first_block;     // of this field in the launch's grid
  int chunks_per_row;
  short elem_bytes;     // 1 | 4
  short vec;            // 16-byte accesses
};

struct PickArg {
  PickFieldArg f[VLNCE_WP_HISTORY_MAX_FIELDS];
  int n_fields, B, P;
};

template <typename T>
__device__ __forceinline__ void pick_chunk(const PickFieldArg& a, long local, const long* __restrict__ pano,
                                           int P) {
  const long b = local / a.chunks_per_row;
  const long off = (local - b * a.chunks_per_row) * HP_CHUNK;
  const long left = a.E - off;
  const int n = left < HP_CHUNK ? (int)left : HP_CHUNK;
  const long p = pano[b];
  const bool take = p >= 0 && p < P;   // (uniform over the block)
  const T* s = reinterpret_cast<const T*>(a.src) + b * a.src_stride + (take ? p : 0) * a.E + off;
  T* d = reinterpret_cast<T*>(a.dst) + b * a.E + off;
  const int tid = (int)threadIdx.x;
  if (a.vec) {   // E * sizeof(T) is a multiple of 16, and so is every chunk's length in bytes
    const int nv = n * (int)sizeof(T) / 16;
    const uint4* sv = reinterpret_cast<const uint4*>(s);
    uint4* dv = reinterpret_cast<uint4*>(d);
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < nv; i += HP_THREADS) dv[i] = take ? sv[i] : zero;
    return;
  }
  for (int i = tid; i < n; i += HP_THREADS) d[i] = take ? s[i] : (T)0;
}

__global__ __launch_bounds__(HP_THREADS) void waypoint_history_pick_kernel(PickArg arg,
                                                                           const long* __restrict__ pano) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_WP_HISTORY_MAX_FIELDS; ++k)
    if (k < arg.n_fields && (long)blockIdx.x >= arg.f[k].first_block) s = k;
  const PickFieldArg& a = arg.f[s];
  const long local = (long)blockIdx.x - a.first_block;
  if (a.elem_bytes == 4) pick_chunk<unsigned int>(a, local, pano, arg.P);   // (uniform over the block)
  else pick_chunk<unsigned char>(a, local, pano, arg.P);
}

}  // namespace

extern "C" int vlnce_waypoint_act_supported(int B, int P, int K_offset, int K_distance) {
  return vlnce_waypoint_eval_supported(B, P, K_offset, K_distance);
}

extern "C" int vlnce_waypoint_act(const float* logits, const vlnce_wp_part* offset,
                                  const vlnce_wp_part* distance, const vlnce_wp_act_part* offset_out,
                                  const vlnce_wp_act_part* distance_out, int deterministic, const float* u,
                                  int B, int P, int64_t* pano, float* log_prob, float* norm_logits,
                                  float* host_rows, int32_t* flags, vlnce_stream_t stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  VLNCE_CHECK_ARG(logits && offset && distance && offset_out && distance_out && pano && log_prob &&
                      norm_logits && host_rows && flags,
                  "waypoint_act: null argument");
  VLNCE_CHECK_ARG(deterministic || u, "waypoint_act: null noise for a sampled action");
  const vlnce_wp_part* parts[2] = {offset, distance};
  const vlnce_wp_act_part* outs[2] = {offset_out, distance_out};
  for (int k = 0; k < 2; ++k) {
    const vlnce_wp_part* p = parts[k];
    VLNCE_CHECK_ARG(wp_kind_ok(p->kind, p->K),
                    "waypoint_act: part of kind %d with K = %d (kinds 0..2, 1 <= K <= %d)", p->kind, p->K,
                    WP_MAX_K);
    if (p->kind == VLNCE_WP_ABSENT) continue;
    VLNCE_CHECK_ARG(p->first, "waypoint_act: null first of a present part");
    VLNCE_CHECK_ARG(p->kind != VLNCE_WP_CONTINUOUS || p->second,
                    "waypoint_act: null second of a continuous part");
    VLNCE_CHECK_ARG(outs[k]->element && outs[k]->mode && outs[k]->variance,
                    "waypoint_act: null output of a present part");
  }
  const int Ko = offset->kind == VLNCE_WP_DISCRETE ? offset->K : 0;
  const int Kd = distance->kind == VLNCE_WP_DISCRETE ? distance->K : 0;
  VLNCE_CHECK_ARG(vlnce_waypoint_act_supported(B, P, Ko, Kd),
                  "waypoint_act: B = %d, P = %d, K = %d / %d outside B >= 1, 1 <= P <= %d, K <= %d", B, P,
                  Ko, Kd, WP_MAX_P, WP_MAX_K);
  hipLaunchKernelGGL(waypoint_act_kernel, dim3((B + WP_THREADS - 1) / WP_THREADS), dim3(WP_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, *offset, *distance, *offset_out,
                     *distance_out, deterministic, u, B, P, reinterpret_cast<long*>(pano), log_prob,
                     norm_logits, host_rows, flags);
  VLNCE_CHECK_LAUNCH("waypoint_act");
  return 0;
}

extern "C" int vlnce_waypoint_history_pick(const vlnce_wp_history_field* fields, int n_fields,
                                           const int64_t* pano, int B, int P, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(fields && pano && B > 0 && P > 0, "waypoint_history_pick: bad argument");
  VLNCE_CHECK_ARG(n_fields > 0 && n_fields <= VLNCE_WP_HISTORY_MAX_FIELDS,
                  "waypoint_history_pick: %d fields (1..%d per call)", n_fields, VLNCE_WP_HISTORY_MAX_FIELDS);
  PickArg arg{};
  arg.n_fields = n_fields;
  arg.B = B;
  arg.P = P;
  long blocks = 0;
  for (int k = 0; k < n_fields; ++k) {
    const vlnce_wp_history_field& in = fields[k];
    PickFieldArg& a = arg.f[k];
    VLNCE_CHECK_ARG(in.dtype == VLNCE_TRAJ_F32 || in.dtype == VLNCE_TRAJ_U8,
                    "waypoint_history_pick: field %d: dtype %d (f32 or u8)", k, in.dtype);
    VLNCE_CHECK_ARG(in.src && in.dst && in.E > 0 && in.E < (1L << 40) && in.src_row_stride >= (long)P * in.E,
                    "waypoint_history_pick: field %d: bad geometry", k);
    const int eb = in.dtype == VLNCE_TRAJ_F32 ? 4 : 1;
    const uintptr_t sp = reinterpret_cast<uintptr_t>(in.src), dp = reinterpret_cast<uintptr_t>(in.dst);
    VLNCE_CHECK_ARG(sp % eb == 0 && dp % eb == 0, "waypoint_history_pick: field %d: misaligned pointer", k);
    a.src = static_cast<const unsigned char*>(in.src);
    a.dst = static_cast<unsigned char*>(in.dst);
    a.E = in.E;
    a.src_stride = in.src_row_stride;
    a.elem_bytes = (short)eb;
    a.vec = sp % 16 == 0 && dp % 16 == 0 && (in.src_row_stride * eb) % 16 == 0 && (in.E * eb) % 16 == 0;
    a.chunks_per_row = (int)((in.E + HP_CHUNK - 1) / HP_CHUNK);
    a.first_block = blocks;
    blocks += (long)a.chunks_per_row * B;
    VLNCE_CHECK_ARG(blocks < (1L << 31), "waypoint_history_pick: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(waypoint_history_pick_kernel, dim3((unsigned)blocks), dim3(HP_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), arg, reinterpret_cast<const long*>(pano));
  VLNCE_CHECK_LAUNCH("waypoint_history_pick");
  return 0;
}
