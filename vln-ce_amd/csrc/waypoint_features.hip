// The trunk-feature cache of the Waypoint DD-PPO loop (ABI 155).  Both visual encoders of the Waypoint
// trainer are frozen and run in eval mode in both phases (models/encoders/resnet_encoders.py:46,142;
// ddppo_waypoint_trainer.py:496,526-530), so a trunk's output is a fixed function of ONE frame: the
// rollout stores it beside the frame, and neither the history frame nor a minibatch update goes
// through a trunk again.  What is left is moving rows of fp32 features:
//   vlnce_waypoint_feature_pick  the chosen panorama slot's features as the next step's history
//                                (the feature-side twin of vlnce_waypoint_history_pick; a STOP row
//                                gets trunk(zero frame), not zeros)
//   vlnce_waypoint_feature_rows  [B, P + 1, F]: the P panorama rows and the history row times its
//                                not-done mask (waypoint_predictors.py:330-341 on cached features)
// The recipe of rollout.hip: the field table travels in the launch's arguments, a row is dealt out in
// VLNCE_ROLLOUT_CHUNK pieces, one workgroup each, 16 bytes per lane where the field's alignment allows.
// Plain vector loads and stores only; no copy, no allocation, no synchronisation.
#include "common.h"

namespace {

constexpr int CHUNK = VLNCE_ROLLOUT_CHUNK;   // elements of a row per workgroup
constexpr int THREADS = 256;

struct PickFieldArg {
  const float* src;
  const float* zero;
  float* dst;
  long F, src_stride;
  long first_block;     // of this field in the launch's grid
  int chunks_per_row;
  int vec;              // 16-byte accesses
};

struct PickArg {
  PickFieldArg f[VLNCE_WP_FEATURE_MAX_FIELDS];
  int n_fields, B, P;
};

struct RowsFieldArg {
  const float* pano;
  const float* hist;
  const float* zero;
  float* out;
  long F, pano_stride, hist_stride;
  long first_block;
  int chunks_per_row;
  int vec;
};

struct RowsArg {
  RowsFieldArg f[VLNCE_WP_FEATURE_MAX_FIELDS];
  int n_fields, B, P;
  int mask_u8;          // masks: uint8 [B], else fp32 [B]
};

// n <= CHUNK floats from s to d by the whole workgroup; vec: s, d 16-byte aligned and n % 4 == 0
__device__ __forceinline__ void copy_chunk(const float* __restrict__ s, float* __restrict__ d, int n,
                                           bool vec) {
  const int tid = (int)threadIdx.x;
  if (vec) {
    constexpr int VPT = CHUNK / 4 / THREADS;   // 16-byte accesses per thread in a whole chunk
    static_assert(VPT == 4 && VPT * 4 * THREADS == CHUNK, "chunk geometry");
    const uint4* sv = reinterpret_cast<const uint4*>(s);
    uint4* dv = reinterpret_cast<uint4*>(d);
    if (n == CHUNK) {   // a whole chunk: four loads in flight before their stores
      const uint4 v0 = sv[tid], v1 = sv[tid + THREADS], v2 = sv[tid + 2 * THREADS],
                  v3 = sv[tid + 3 * THREADS];
      dv[tid] = v0;
      dv[tid + THREADS] = v1;
      dv[tid + 2 * THREADS] = v2;
      dv[tid + 3 * THREADS] = v3;
      return;
    }
    const int nv = n / 4;
    for (int i = tid; i < nv; i += THREADS) dv[i] = sv[i];
    return;
  }
  for (int i = tid; i < n; i += THREADS) d[i] = s[i];
}

__global__ __launch_bounds__(THREADS) void waypoint_feature_pick_kernel(PickArg arg,
                                                                        const long* __restrict__ pano) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_WP_FEATURE_MAX_FIELDS; ++k)
    if (k < arg.n_fields && (long)blockIdx.x >= arg.f[k].first_block) s = k;
  const PickFieldArg& a = arg.f[s];
  const long local = (long)blockIdx.x - a.first_block;
  const long b = local / a.chunks_per_row;
  const long off = (local - b * a.chunks_per_row) * CHUNK;
  const long left = a.F - off;
  const long p = pano[b];
  const bool take = p >= 0 && p < arg.P;   // (uniform over the block)
  const float* src = take ? a.src + b * a.src_stride + p * a.F : a.zero;
  copy_chunk(src + off, a.dst + b * a.F + off, left < CHUNK ? (int)left : CHUNK, a.vec != 0);
}

__global__ __launch_bounds__(THREADS) void waypoint_feature_rows_kernel(RowsArg arg,
                                                                        const void* __restrict__ masks) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_WP_FEATURE_MAX_FIELDS; ++k)
    if (k < arg.n_fields && (long)blockIdx.x >= arg.f[k].first_block) s = k;
  const RowsFieldArg& a = arg.f[s];
  const long local = (long)blockIdx.x - a.first_block;
  const long q = local / a.chunks_per_row;           // output row b * (P + 1) + j
  const long off = (local - q * a.chunks_per_row) * CHUNK;
  const long left = a.F - off;
  const long b = q / (arg.P + 1);
  const long j = q - b * (arg.P + 1);
  const float* src;                                  // (uniform over the block)
  if (j < arg.P) {
    src = a.pano + b * a.pano_stride + j * a.F;
  } else {
    const bool going = arg.mask_u8 ? static_cast<const unsigned char*>(masks)[b] != 0
                                   : static_cast<const float*>(masks)[b] != 0.0f;
    src = going ? a.hist + b * a.hist_stride : a.zero;
  }
  copy_chunk(src + off, a.out + q * a.F + off, left < CHUNK ? (int)left : CHUNK, a.vec != 0);
}

inline bool aligned(const void* p, unsigned n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

extern "C" int vlnce_waypoint_feature_pick(const vlnce_wp_feature_pick_field* fields, int n_fields,
                                           const int64_t* pano, int B, int P, vlnce_stream_t stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  static_assert(sizeof(PickArg) <= 4096, "launch arguments");
  VLNCE_CHECK_ARG(fields && pano && B > 0 && P > 0, "waypoint_feature_pick: bad argument");
  VLNCE_CHECK_ARG(n_fields > 0 && n_fields <= VLNCE_WP_FEATURE_MAX_FIELDS,
                  "waypoint_feature_pick: %d fields (1..%d per call)", n_fields,
                  VLNCE_WP_FEATURE_MAX_FIELDS);
  PickArg arg{};
  arg.n_fields = n_fields;
  arg.B = B;
  arg.P = P;
  long blocks = 0;
  for (int k = 0; k < n_fields; ++k) {
    const vlnce_wp_feature_pick_field& in = fields[k];
    PickFieldArg& a = arg.f[k];
    VLNCE_CHECK_ARG(in.src && in.zero && in.dst, "waypoint_feature_pick: field %d: null pointer", k);
    VLNCE_CHECK_ARG(in.F > 0 && in.F < (1L << 40), "waypoint_feature_pick: field %d: F = %ld", k, in.F);
    VLNCE_CHECK_ARG(in.src_row_stride >= (long)P * in.F,
                    "waypoint_feature_pick: field %d: row stride %ld for rows of %ld elements", k,
                    in.src_row_stride, (long)P * in.F);
    VLNCE_CHECK_ARG(aligned(in.src, 4) && aligned(in.zero, 4) && aligned(in.dst, 4),
                    "waypoint_feature_pick: field %d: misaligned pointer", k);
    a.src = in.src;
    a.zero = in.zero;
    a.dst = in.dst;
    a.F = in.F;
    a.src_stride = in.src_row_stride;
    a.vec = aligned(in.src, 16) && aligned(in.zero, 16) && aligned(in.dst, 16) &&
            (in.src_row_stride * 4) % 16 == 0 && (in.F * 4) % 16 == 0;
    a.chunks_per_row = (int)((in.F + CHUNK - 1) / CHUNK);
    a.first_block = blocks;
    blocks += (long)a.chunks_per_row * B;
    VLNCE_CHECK_ARG(blocks < (1L << 31), "waypoint_feature_pick: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(waypoint_feature_pick_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), arg, reinterpret_cast<const long*>(pano));
  VLNCE_CHECK_LAUNCH("waypoint_feature_pick");
  return 0;
}

extern "C" int vlnce_waypoint_feature_rows(const vlnce_wp_feature_rows_field* fields, int n_fields,
                                           const void* masks, int mask_dtype, int B, int P,
                                           vlnce_stream_t stream) {
  static_assert(sizeof(RowsArg) <= 4096, "launch arguments");
  VLNCE_CHECK_ARG(fields && masks && B > 0 && P > 0, "waypoint_feature_rows: bad argument");
  VLNCE_CHECK_ARG(mask_dtype == VLNCE_TRAJ_U8 || mask_dtype == VLNCE_TRAJ_F32,
                  "waypoint_feature_rows: masks of dtype %d (u8 or f32)", mask_dtype);
  VLNCE_CHECK_ARG(mask_dtype == VLNCE_TRAJ_U8 || aligned(masks, 4),
                  "waypoint_feature_rows: misaligned masks");
  VLNCE_CHECK_ARG(n_fields > 0 && n_fields <= VLNCE_WP_FEATURE_MAX_FIELDS,
                  "waypoint_feature_rows: %d fields (1..%d per call)", n_fields,
                  VLNCE_WP_FEATURE_MAX_FIELDS);
  RowsArg arg{};
  arg.n_fields = n_fields;
  arg.B = B;
  arg.P = P;
  arg.mask_u8 = mask_dtype == VLNCE_TRAJ_U8;
  long blocks = 0;
  for (int k = 0; k < n_fields; ++k) {
    const vlnce_wp_feature_rows_field& in = fields[k];
    RowsFieldArg& a = arg.f[k];
    VLNCE_CHECK_ARG(in.pano && in.hist && in.zero && in.out,
                    "waypoint_feature_rows: field %d: null pointer", k);
    VLNCE_CHECK_ARG(in.F > 0 && in.F < (1L << 40), "waypoint_feature_rows: field %d: F = %ld", k, in.F);
    VLNCE_CHECK_ARG(in.pano_row_stride >= (long)P * in.F && in.hist_row_stride >= in.F,
                    "waypoint_feature_rows: field %d: row strides %ld / %ld for rows of %ld / %ld elements",
                    k, in.pano_row_stride, in.hist_row_stride, (long)P * in.F, in.F);
    VLNCE_CHECK_ARG(aligned(in.pano, 4) && aligned(in.hist, 4) && aligned(in.zero, 4) && aligned(in.out, 4),
                    "waypoint_feature_rows: field %d: misaligned pointer", k);
    a.pano = in.pano;
    a.hist = in.hist;
    a.zero = in.zero;
    a.out = in.out;
    a.F = in.F;
    a.pano_stride = in.pano_row_stride;
    a.hist_stride = in.hist_row_stride;
    a.vec = aligned(in.pano, 16) && aligned(in.hist, 16) && aligned(in.zero, 16) && aligned(in.out, 16) &&
            (in.pano_row_stride * 4) % 16 == 0 && (in.hist_row_stride * 4) % 16 == 0 &&
            (in.F * 4) % 16 == 0;
    a.chunks_per_row = (int)((in.F + CHUNK - 1) / CHUNK);
    a.first_block = blocks;
    blocks += (long)a.chunks_per_row * B * (P + 1);
    VLNCE_CHECK_ARG(blocks < (1L << 31), "waypoint_feature_rows: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(waypoint_feature_rows_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), arg, masks);
  VLNCE_CHECK_LAUNCH("waypoint_feature_rows");
  return 0;
}
