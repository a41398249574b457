// The optimizer step of both reference trainers (torch.optim.Adam, base_il_trainer.py:69-77 and
// ddppo_waypoint_trainer.py:441, with WDDPPO's clip_grad_norm_ in front) over a LIST of fp32
// tensors in two launches: grad_sumsq_kernel (only when clipping) leaves ADAM_PARTIALS fp64
// partial sums of squares, adam_step_kernel re-reduces them in one fixed order in every
// workgroup and applies torch's Adam to its chunk.  No atomics, no grid-wide or host
// synchronisation; each element is evaluated in fp64 and rounded once per store, and element i
// of a chunk belongs to thread (i / 4) % 256 on both access paths: two runs give the same bits.
//
// The stable half of the tensor list is a device table of int64 words (built by the host once per
// parameter set): n_tensors x {p, m, v, numel}, then one word per chunk, tensor << 32 | chunk
// index inside the tensor.  The half that changes every step (the gradient pointers, new under
// zero_grad(set_to_none=True), and the per-tensor bias corrections) travels BY VALUE in the
// kernel arguments: nothing is staged in memory that a later step could overwrite.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = 4096;        // elements per workgroup: 4 x float4 per thread and array
constexpr int ADAM_MAX_TENSORS = 128;   // 24 B each by value: 3 KB of the 4 KB a launch may carry
constexpr int ADAM_PARTIALS = 512;      // == the grid of grad_sumsq_kernel, 2 per thread to re-reduce
static_assert(ADAM_PARTIALS == 2 * ADAM_THREADS, "adam_step_kernel reads two partials per thread");
static_assert(ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "whole float4 rounds per chunk");

struct AdamStepArgs {
  const float* g[ADAM_MAX_TENSORS];       // NULL: the tensor is skipped (grad is None)
  double step_size[ADAM_MAX_TENSORS];     // lr / (1 - b1^t)
  double inv_bc2_sqrt[ADAM_MAX_TENSORS];  // 1 / sqrt(1 - b2^t)
};
struct AdamGradArgs {
  const float* g[ADAM_MAX_TENSORS];
};

// the same tree every time: xor shuffles inside a wave, then the four wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double* red /* [4] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// up to 4 consecutive floats: one 16-byte access when the workgroup's chunk allows it (vec is
// wave-uniform) and the group is whole, else element by element
__device__ __forceinline__ f32x4 load4(const float* p, int cnt, bool vec) {
  if (vec && cnt == 4) return *reinterpret_cast<const f32x4*>(p);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < cnt; ++j) r[j] = p[j];
  return r;
}
__device__ __forceinline__ void store4(float* p, f32x4 x, int cnt, bool vec) {
  if (vec && cnt == 4) {
    *reinterpret_cast<f32x4*>(p) = x;
    return;
  }
  for (int j = 0; j < cnt; ++j) p[j] = x[j];
}

// workgroup w takes chunks w, w + ADAM_PARTIALS, ...: partials[w] = (accumulate ? partials[w] : 0)
// + its sum, so a list split over several launches still leaves ADAM_PARTIALS values
__global__ __launch_bounds__(ADAM_THREADS) void grad_sumsq_kernel(
    const long* __restrict__ table, int n_tensors, long n_chunks, AdamGradArgs a,
    double* __restrict__ partials, int accumulate) {
  __shared__ double red[4];
  const long* chunks = table + 4L * n_tensors;
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long c = blockIdx.x; c < n_chunks; c += ADAM_PARTIALS) {
    const long word = chunks[c];
    const int t = (int)(word >> 32);
    if (t < 0 || t >= n_tensors) continue;
    const float* g = a.g[t];
    if (!g) continue;
    const long numel = table[4L * t + 3];
    const long off = (word & 0xffffffffL) * ADAM_CHUNK;
    if (off >= numel) continue;
    const int n = (int)(numel - off < ADAM_CHUNK ? numel - off : ADAM_CHUNK);
    g += off;
    const bool vec = aligned16(g);
#pragma unroll 4
    for (int i = tid * 4; i < n; i += ADAM_THREADS * 4) {
      const int cnt = n - i < 4 ? n - i : 4;
      const f32x4 x = load4(g + i, cnt, vec);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];   // (padding lanes are 0)
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) partials[blockIdx.x] = (accumulate ? partials[blockIdx.x] : 0.0) + s;
}

// one workgroup per chunk
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(
    const long* __restrict__ table, int n_tensors, AdamStepArgs a,
    const double* __restrict__ partials, double max_norm, double b1, double b2, double eps,
    double weight_decay, float* __restrict__ norm_out) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double coef = 1.0;
  if (partials) {   // uniform over the launch
    const double total = block_sum(partials[tid] + partials[tid + ADAM_THREADS], red);
    const double norm = sqrt(total);
    const double c = max_norm / (norm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;   // NaN stays NaN, as torch.clamp(max=1) leaves it
    if (blockIdx.x == 0 && tid == 0 && norm_out) norm_out[0] = (float)norm;
  }
  const long word = table[4L * n_tensors + blockIdx.x];
  const int t = (int)(word >> 32);
  if (t < 0 || t >= n_tensors) return;
  const float* g = a.g[t];
  if (!g) return;
  const long numel = table[4L * t + 3];
  const long off = (word & 0xffffffffL) * ADAM_CHUNK;
  if (off >= numel) return;
  const int n = (int)(numel - off < ADAM_CHUNK ? numel - off : ADAM_CHUNK);
  float* p = reinterpret_cast<float*>(table[4L * t + 0]) + off;
  float* m = reinterpret_cast<float*>(table[4L * t + 1]) + off;
  float* v = reinterpret_cast<float*>(table[4L * t + 2]) + off;
  g += off;
  const bool vec = aligned16(p) && aligned16(m) && aligned16(v) && aligned16(g);
  const double step_size = a.step_size[t], inv_bc2_sqrt = a.inv_bc2_sqrt[t];
  const double one_b1 = 1.0 - b1, one_b2 = 1.0 - b2;
#pragma unroll 2
  for (int i = tid * 4; i < n; i += ADAM_THREADS * 4) {
    const int cnt = n - i < 4 ? n - i : 4;
    const f32x4 g4 = load4(g + i, cnt, vec);
    f32x4 p4 = load4(p + i, cnt, vec);
    f32x4 m4 = load4(m + i, cnt, vec);
    f32x4 v4 = load4(v + i, cnt, vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double pj = (double)p4[j];
      double gj = coef * (double)g4[j];
      if (weight_decay != 0.0) gj += weight_decay * pj;
      const double mj = (double)m4[j] + (gj - (double)m4[j]) * one_b1;
      const double vj = b2 * (double)v4[j] + one_b2 * gj * gj;
      const double denom = sqrt(vj) * inv_bc2_sqrt + eps;
      p4[j] = (float)(pj - step_size * mj / denom);
      m4[j] = (float)mj;
      v4[j] = (float)vj;
    }
    store4(p + i, p4, cnt, vec);
    store4(m + i, m4, cnt, vec);
    store4(v + i, v4, cnt, vec);
  }
}

int check_list(const char* what, const int64_t* table, int n_tensors, long n_chunks) {
  VLNCE_CHECK_ARG(table, "%s: null table", what);
  VLNCE_CHECK_ARG(n_tensors >= 1 && n_tensors <= ADAM_MAX_TENSORS,
                  "%s: %d tensors outside 1..%d per launch (split the list)", what, n_tensors,
                  ADAM_MAX_TENSORS);
  VLNCE_CHECK_ARG(n_chunks >= 0 && n_chunks <= 0x7fffffffL, "%s: %ld chunks outside 0..2^31-1", what,
                  n_chunks);
  return 0;
}

}  // namespace

extern "C" int vlnce_adam_max_tensors(void) { return ADAM_MAX_TENSORS; }
extern "C" int vlnce_adam_chunk(void) { return ADAM_CHUNK; }

extern "C" int vlnce_adam_supported(int n_tensors, long n_chunks) {
  return n_tensors >= 1 && n_tensors <= ADAM_MAX_TENSORS && n_chunks >= 0 && n_chunks <= 0x7fffffffL;
}

extern "C" int vlnce_grad_sumsq(const int64_t* table, int n_tensors, long n_chunks,
                                const float* const* grads, double* partials, int accumulate,
                                vlnce_stream_t stream) {
  if (check_list("grad_sumsq", table, n_tensors, n_chunks)) return 1;
  VLNCE_CHECK_ARG(grads && partials, "grad_sumsq: null grads or partials");
  AdamGradArgs a;
  for (int t = 0; t < ADAM_MAX_TENSORS; ++t) a.g[t] = t < n_tensors ? grads[t] : nullptr;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(ADAM_PARTIALS), dim3(ADAM_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long*>(table),
                     n_tensors, n_chunks, a, partials, accumulate);
  VLNCE_CHECK_LAUNCH("grad_sumsq");
  return 0;
}

extern "C" int vlnce_adam_step(const int64_t* table, int n_tensors, long n_chunks,
                               const float* const* grads, const double* step_size,
                               const double* inv_bc2_sqrt, const double* partials, double max_norm,
                               double beta1, double beta2, double eps, double weight_decay,
                               float* norm_out, vlnce_stream_t stream) {
  if (check_list("adam_step", table, n_tensors, n_chunks)) return 1;
  VLNCE_CHECK_ARG(grads && step_size && inv_bc2_sqrt, "adam_step: null grads or bias corrections");
  if (n_chunks == 0) return 0;
  AdamStepArgs a;
  for (int t = 0; t < ADAM_MAX_TENSORS; ++t) {
    const bool in = t < n_tensors;
    a.g[t] = in ? grads[t] : nullptr;
    a.step_size[t] = in ? step_size[t] : 0.0;
    a.inv_bc2_sqrt[t] = in ? inv_bc2_sqrt[t] : 0.0;
  }
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(ADAM_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long*>(table),
                     n_tensors, a, partials, max_norm, beta1, beta2, eps, weight_decay, norm_out);
  VLNCE_CHECK_LAUNCH("adam_step");
  return 0;
}
