// The imitation-learning objective of BaseVLNCETrainer._update_agent (base_il_trainer.py:134-180)
// on the device: the inflection-weighted cross entropy with its per-episode normalisation and
// the progress monitor's [R, E] mean squared error (aux_losses.py:24-32 over the broadcast of
// cma_policy.py:296-307), each as ONE launch of one workgroup that also produces the gradient.
// fp64 accumulators, a fixed reduction order, no floating-point atomics: two runs give the same
// bits.
#include <stdint.h>

#include <limits>

#include "common.h"

namespace {

constexpr int IL_THREADS = 256;
constexpr int IL_MAX_N = 1024;   // column sums live in LDS
constexpr int IL_MAX_A = 16;     // the action head's own bound

// sum of one value per thread over the workgroup, the same tree every time: xor shuffles inside a
// wave, then the four wave sums in wave order.  Every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* red /* [4] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// rows are time-major, r = t * N + n.  The T steps of a column are dealt to K = max(1, 256 / N)
// threads (thread k of column n takes t = k, k + K, ...), whose partial sums are added in k order;
// with N >= 256 a thread walks whole columns n = tid, tid + 256, ...
__global__ __launch_bounds__(IL_THREADS) void il_loss_kernel(
    const float* __restrict__ logits, const long* __restrict__ targets,
    const float* __restrict__ weights, const float* __restrict__ aux, float inv_scalar, int T, int N,
    int A, float* __restrict__ stats, float* __restrict__ dlogits) {
  __shared__ double colw[IL_MAX_N];    // sum_t w[t, n]
  __shared__ double colce[IL_MAX_N];   // sum_t w[t, n] * ce[t, n]
  __shared__ double part[IL_THREADS];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int K = N >= IL_THREADS ? 1 : IL_THREADS / N;
  const int slots = K * N;   // <= 256 when K > 1, N (<= 1024) when K == 1

  for (int s = tid; s < slots; s += IL_THREADS) {
    const int n = s % N, k = s / N;
    double acc = 0.0;
    for (int t = k; t < T; t += K) acc += (double)weights[(long)t * N + n];
    if (K == 1) colw[n] = acc;
    else part[s] = acc;
  }
  __syncthreads();
  if (K > 1 && tid < N) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += part[k * N + tid];
    colw[tid] = acc;
  }
  __syncthreads();

  const double scale = (double)inv_scalar / (double)N;
  for (int s = tid; s < slots; s += IL_THREADS) {
    const int n = s % N, k = s / N;
    const double wsum = colw[n];
    double acc = 0.0;
    for (int t = k; t < T; t += K) {
      const long r = (long)t * N + n;
      const float* z = logits + r * A;
      float* dz = dlogits + r * A;
      const long tgt = targets[r];
      const double w = (double)weights[r];
      float zmax = z[0];
      for (int a = 1; a < A; ++a) zmax = fmaxf(zmax, z[a]);
      double se = 0.0;
      for (int a = 0; a < A; ++a) se += exp((double)z[a] - (double)zmax);
      const double lse = (double)zmax + log(se);
      const bool in_range = tgt >= 0 && tgt < A;   // outside: NaN for the row, nothing read
      const double ce = in_range ? lse - (double)z[in_range ? tgt : 0]
                                 : std::numeric_limits<double>::quiet_NaN();
      acc += w * ce;   // a product, as torch: a padded row (w = 0) is multiplied, not skipped
      const double g = w / wsum * scale;
      for (int a = 0; a < A; ++a) {
        const double p = exp((double)z[a] - lse);
        dz[a] = in_range ? (float)((p - (a == tgt ? 1.0 : 0.0)) * g)
                         : std::numeric_limits<float>::quiet_NaN();
      }
    }
    if (K == 1) colce[n] = acc;
    else part[s] = acc;
  }
  __syncthreads();
  if (K > 1 && tid < N) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += part[k * N + tid];
    colce[tid] = acc;
  }
  __syncthreads();

  double v = 0.0;
  for (int n = tid; n < N; n += IL_THREADS) v += colce[n] / colw[n];   // 0 / 0 as torch divides it
  const double action = block_sum(v, red) / (double)N;
  if (tid == 0) {
    const double x = aux ? (double)aux[0] : 0.0;
    stats[0] = (float)((action + x) * (double)inv_scalar);
    stats[1] = (float)action;
    stats[2] = (float)x;
  }
}

// sum_i (e - t_i)^2 = R d^2 - 2 d S1 + S2 with d = e - mu, S1 = sum_i (t_i - mu), S2 = sum_i
// (t_i - mu)^2 around the targets' mean mu: the closed form of the column sum without its
// cancellation (both leading terms are non-negative, S1 is rounding noise).
__global__ __launch_bounds__(IL_THREADS) void pair_mse_kernel(
    const float* __restrict__ estimate, const float* __restrict__ target,
    const uint8_t* __restrict__ mask, int E, int R, float* __restrict__ value,
    float* __restrict__ d_estimate) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double a = 0.0, c = 0.0;
  for (int i = tid; i < R; i += IL_THREADS) a += (double)target[i];
  for (int j = tid; j < E; j += IL_THREADS) c += mask[j] ? 1.0 : 0.0;
  const double mu = block_sum(a, red) / (double)R;
  const double count = block_sum(c, red);
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < R; i += IL_THREADS) {
    const double u = (double)target[i] - mu;
    s1 += u;
    s2 += u * u;
  }
  const double S1 = block_sum(s1, red), S2 = block_sum(s2, red);
  const double inv = 1.0 / ((double)R * count);   // no selected column: 0 / 0, the mean of nothing
  double acc = 0.0;
  for (int j = tid; j < E; j += IL_THREADS) {
    const double d = (double)estimate[j] - mu;
    const bool m = mask[j] != 0;
    if (m) acc += (double)R * d * d - 2.0 * d * S1 + S2;
    d_estimate[j] = m ? (float)(2.0 * ((double)R * d - S1) * inv) : 0.f;
  }
  const double total = block_sum(acc, red);
  if (tid == 0) value[0] = (float)(total * inv);
}

}  // namespace

extern "C" int vlnce_il_loss_supported(int T, int N, int A) {
  return T > 0 && N > 0 && N <= IL_MAX_N && A > 0 && A <= IL_MAX_A;
}

extern "C" int vlnce_il_loss(const float* logits, const int64_t* targets, const float* weights,
                             const float* aux, float inv_scalar, int T, int N, int A, float* stats,
                             float* dlogits, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(logits && targets && weights && stats && dlogits, "il_loss: null argument");
  VLNCE_CHECK_ARG(vlnce_il_loss_supported(T, N, A),
                  "il_loss: T = %d, N = %d, A = %d outside T >= 1, 1 <= N <= %d, 1 <= A <= %d", T, N,
                  A, IL_MAX_N, IL_MAX_A);
  hipLaunchKernelGGL(il_loss_kernel, dim3(1), dim3(IL_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), logits,
                     reinterpret_cast<const long*>(targets), weights, aux, inv_scalar, T, N, A, stats,
                     dlogits);
  VLNCE_CHECK_LAUNCH("il_loss");
  return 0;
}

extern "C" int vlnce_pair_mse(const float* estimate, const float* target, const uint8_t* mask, int E,
                              int R, float* value, float* d_estimate, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(estimate && target && mask && value && d_estimate, "pair_mse: null argument");
  VLNCE_CHECK_ARG(E > 0 && R > 0, "pair_mse: empty estimate or target");
  hipLaunchKernelGGL(pair_mse_kernel, dim3(1), dim3(IL_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), estimate, target, mask, E, R, value,
                     d_estimate);
  VLNCE_CHECK_LAUNCH("pair_mse");
  return 0;
}
