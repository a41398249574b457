// DD-PPO rollout storage on the device.  The reference's
// ActionDictRolloutStorage (vlnce_baselines/common/rollout_storage.py) is host-paced: ~17 copy_
// launches per simulator step (insert, :85-111), ~11 per after_update (:113-125), and for every
// minibatch a Python loop over environments that slices every field and rebuilds the batch with ~25
// stack / view launches (recurrent_generator, :154-276); WDDPPO.get_advantages (ddppo_alg.py:30-35)
// adds a mean() / std() chain.  Here:
//   vlnce_rollout_copy     one launch moves one row block of EVERY field (insert, after_update)
//   vlnce_rollout_gather   one launch cuts one minibatch out of every arena, time-major
//   vlnce_ppo_advantages   one launch of one workgroup, fp64 statistics in a fixed order
// The field tables and the environment indices travel in the launch's argument struct (as TrajArg
// in traj.hip): a call makes no copy, no allocation and no synchronisation.  Pure data movement with
// plain vector loads and stores: 16 bytes per lane where a field's alignment allows, loads of a
// chunk issued before its stores.
#include "common.h"

namespace {

constexpr int CHUNK = VLNCE_ROLLOUT_CHUNK;   // elements of a row per workgroup
constexpr int PACKED_BELOW = 256;            // shorter rows: one thread per element, rows packed
constexpr int THREADS = 256;

// (src dtype, dst dtype) of vlnce_rollout_copy
enum { PAIR_F32 = 0, PAIR_I64, PAIR_U8, PAIR_I64_F32, PAIR_U8_F32, PAIR_F32_I64, PAIR_F32_U8, PAIR_NONE };

inline int pair_of(int s, int d) {
  if (s == VLNCE_TRAJ_F32 && d == VLNCE_TRAJ_F32) return PAIR_F32;
  if (s == VLNCE_TRAJ_I64 && d == VLNCE_TRAJ_I64) return PAIR_I64;
  if (s == VLNCE_TRAJ_U8 && d == VLNCE_TRAJ_U8) return PAIR_U8;
  if (s == VLNCE_TRAJ_I64 && d == VLNCE_TRAJ_F32) return PAIR_I64_F32;
  if (s == VLNCE_TRAJ_U8 && d == VLNCE_TRAJ_F32) return PAIR_U8_F32;
  if (s == VLNCE_TRAJ_F32 && d == VLNCE_TRAJ_I64) return PAIR_F32_I64;
  if (s == VLNCE_TRAJ_F32 && d == VLNCE_TRAJ_U8) return PAIR_F32_U8;
  return PAIR_NONE;
}

inline int dtype_bytes(int dtype) {
  return dtype == VLNCE_TRAJ_I64 ? 8 : dtype == VLNCE_TRAJ_F32 ? 4 : 1;
}

struct CopyFieldArg {
  const unsigned char* src;
  unsigned char* dst;
  long E, src_stride, dst_stride;
  long first_block;     // of this field in the launch's grid
  int chunks_per_row;   // 0: packed (E < PACKED_BELOW)
  short pair;
  short vec;            // 16-byte accesses
};

struct CopyArg {
  CopyFieldArg f[VLNCE_ROLLOUT_MAX_FIELDS];
  int n_fields, n_rows;
};

struct GatherFieldArg {
  const unsigned char* arena;
  unsigned char* out;
  long E, N, out_N;
  long first_block;
  int chunks_per_row;   // 0: packed
  short elem_bytes;
  short flags;          // bit 0: 16-byte accesses; bit 1: one time step only
};

struct GatherArg {
  GatherFieldArg f[VLNCE_ROLLOUT_MAX_FIELDS];
  int envs[VLNCE_ROLLOUT_MAX_ENVS];
  int n_fields, n_envs, T;
};

template <typename S, typename D>
struct same_type { static constexpr bool value = false; };
template <typename S>
struct same_type<S, S> { static constexpr bool value = true; };

// n <= CHUNK elements from s to d by the whole workgroup
template <typename S, typename D>
__device__ __forceinline__ void copy_chunk(const S* s, D* d, int n, bool vec) {
  const int tid = (int)threadIdx.x;
  if constexpr (same_type<S, D>::value) {
    if (vec) {
      constexpr int PER = 16 / (int)sizeof(S);                          // elements per access
      constexpr int VPT = CHUNK * (int)sizeof(S) / 16 / THREADS;        // accesses per thread
      static_assert(VPT >= 1 && VPT * 16 * THREADS == CHUNK * (int)sizeof(S), "chunk geometry");
      const int nv = n / PER;
      const uint4* sv = reinterpret_cast<const uint4*>(s);
      uint4* dv = reinterpret_cast<uint4*>(d);
      if (n == CHUNK && VPT % 4 == 0) {   // a whole chunk: four loads in flight before their stores
#pragma unroll
        for (int k = 0; k < VPT; k += 4) {
          const int i = tid + k * THREADS;
          const uint4 v0 = sv[i], v1 = sv[i + THREADS], v2 = sv[i + 2 * THREADS], v3 = sv[i + 3 * THREADS];
          dv[i] = v0;
          dv[i + THREADS] = v1;
          dv[i + 2 * THREADS] = v2;
          dv[i + 3 * THREADS] = v3;
        }
        return;
      }
      for (int i = tid; i < nv; i += THREADS) dv[i] = sv[i];
      for (int i = nv * PER + tid; i < n; i += THREADS) d[i] = s[i];   // the tail of a row
      return;
    }
  }
  for (int i = tid; i < n; i += THREADS) d[i] = (D)s[i];
}

template <typename S, typename D>
__device__ __forceinline__ void copy_field(const CopyFieldArg& a, long local, int n_rows) {
  const S* src = reinterpret_cast<const S*>(a.src);
  D* dst = reinterpret_cast<D*>(a.dst);
  if (a.chunks_per_row == 0) {
    const long item = local * THREADS + (long)threadIdx.x;
    if (item >= (long)n_rows * a.E) return;
    const long r = item / a.E, e = item - r * a.E;
    dst[r * a.dst_stride + e] = (D)src[r * a.src_stride + e];
    return;
  }
  const long r = local / a.chunks_per_row;
  const long off = (local - r * a.chunks_per_row) * CHUNK;
  const long left = a.E - off;
  copy_chunk<S, D>(src + r * a.src_stride + off, dst + r * a.dst_stride + off,
                   left < CHUNK ? (int)left : CHUNK, a.vec != 0);
}

__global__ __launch_bounds__(THREADS) void rollout_copy_kernel(CopyArg arg) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_ROLLOUT_MAX_FIELDS; ++k)
    if (k < arg.n_fields && (long)blockIdx.x >= arg.f[k].first_block) s = k;
  const CopyFieldArg& a = arg.f[s];
  const long local = (long)blockIdx.x - a.first_block;
  switch (a.pair) {   // (uniform over the block)
    case PAIR_F32: copy_field<float, float>(a, local, arg.n_rows); break;
    case PAIR_I64: copy_field<long, long>(a, local, arg.n_rows); break;
    case PAIR_U8: copy_field<unsigned char, unsigned char>(a, local, arg.n_rows); break;
    case PAIR_I64_F32: copy_field<long, float>(a, local, arg.n_rows); break;
    case PAIR_U8_F32: copy_field<unsigned char, float>(a, local, arg.n_rows); break;
    case PAIR_F32_I64: copy_field<float, long>(a, local, arg.n_rows); break;
    case PAIR_F32_U8: copy_field<float, unsigned char>(a, local, arg.n_rows); break;
    default: break;   // (the launcher admits nothing else)
  }
}

template <typename W>
__device__ __forceinline__ void gather_field(const GatherArg& arg, const GatherFieldArg& a,
                                             long local) {
  const W* arena = reinterpret_cast<const W*>(a.arena);
  W* out = reinterpret_cast<W*>(a.out);
  const int n_envs = arg.n_envs;
  const long rows = (long)((a.flags & 2) ? 1 : arg.T) * n_envs;   // row q = t * n_envs + j
  if (a.chunks_per_row == 0) {
    const long item = local * THREADS + (long)threadIdx.x;
    if (item >= rows * a.E) return;
    const long q = item / a.E, e = item - q * a.E;
    const long t = q / n_envs;
    const int j = (int)(q - t * n_envs);
    out[(t * a.out_N + j) * a.E + e] = arena[(t * a.N + arg.envs[j]) * a.E + e];
    return;
  }
  const long q = local / a.chunks_per_row;
  const long off = (local - q * a.chunks_per_row) * CHUNK;
  const long t = q / n_envs;
  const int j = (int)(q - t * n_envs);
  const long left = a.E - off;
  copy_chunk<W, W>(arena + (t * a.N + arg.envs[j]) * a.E + off, out + (t * a.out_N + j) * a.E + off,
                   left < CHUNK ? (int)left : CHUNK, (a.flags & 1) != 0);
}

__global__ __launch_bounds__(THREADS) void rollout_gather_kernel(GatherArg arg) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_ROLLOUT_MAX_FIELDS; ++k)
    if (k < arg.n_fields && (long)blockIdx.x >= arg.f[k].first_block) s = k;
  const GatherFieldArg& a = arg.f[s];
  const long local = (long)blockIdx.x - a.first_block;
  switch (a.elem_bytes) {   // (uniform over the block)
    case 1: gather_field<unsigned char>(arg, a, local); break;
    case 2: gather_field<unsigned short>(arg, a, local); break;
    case 4: gather_field<unsigned int>(arg, a, local); break;
    case 8: gather_field<unsigned long>(arg, a, local); break;
    default: break;
  }
}

// blocks a field of `rows` rows of E elements takes, and its chunks_per_row (0: packed)
inline long field_blocks(long E, long rows, int* chunks_per_row) {
  if (E < PACKED_BELOW) {
    *chunks_per_row = 0;
    return (rows * E + THREADS - 1) / THREADS;
  }
  const long c = (E + CHUNK - 1) / CHUNK;
  *chunks_per_row = (int)c;
  return c * rows;
}

constexpr int ADV_THREADS = 1024;

// the sum of v over the workgroup in ONE order: thread i adds slots i and i + o, o = 512 .. 1
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = (int)threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = ADV_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// every pass takes d = returns - value_preds again, in fp32 (one rounding, as torch's subtraction)
__global__ __launch_bounds__(ADV_THREADS) void ppo_advantages_kernel(const float* returns,
                                                                     const float* value_preds,
                                                                     float* adv, long n, int normalize,
                                                                     double eps) {
  __shared__ double red[ADV_THREADS];
  const int tid = (int)threadIdx.x;
  if (!normalize) {
    for (long i = tid; i < n; i += ADV_THREADS) adv[i] = returns[i] - value_preds[i];
    return;
  }
  double s = 0.0;
  for (long i = tid; i < n; i += ADV_THREADS) s += (double)(returns[i] - value_preds[i]);
  const double mean = block_sum(s, red) / (double)n;
  double q = 0.0;
  for (long i = tid; i < n; i += ADV_THREADS) {
    const double c = (double)(returns[i] - value_preds[i]) - mean;
    q += c * c;
  }
  const double sd = sqrt(block_sum(q, red) / (double)(n - 1));   // n == 1: 0 / 0, NaN as torch.std
  const double denom = sd + eps;
  for (long i = tid; i < n; i += ADV_THREADS)
    adv[i] = (float)(((double)(returns[i] - value_preds[i]) - mean) / denom);
}

}  // namespace

extern "C" int vlnce_rollout_copy_supported(int src_dtype, int dst_dtype) {
  return pair_of(src_dtype, dst_dtype) != PAIR_NONE;
}

extern "C" int vlnce_rollout_copy(const vlnce_rollout_field* fields, int n_fields, int n_rows,
                                  vlnce_stream_t stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  static_assert(sizeof(CopyArg) <= 4096, "launch arguments");
  VLNCE_CHECK_ARG(fields && n_rows > 0, "rollout_copy: bad argument");
  VLNCE_CHECK_ARG(n_fields > 0 && n_fields <= VLNCE_ROLLOUT_MAX_FIELDS,
                  "rollout_copy: %d fields (1..%d per call)", n_fields, VLNCE_ROLLOUT_MAX_FIELDS);
  CopyArg arg{};
  arg.n_fields = n_fields;
  arg.n_rows = n_rows;
  long blocks = 0;
  for (int k = 0; k < n_fields; ++k) {
    const vlnce_rollout_field& in = fields[k];
    CopyFieldArg& a = arg.f[k];
    const int pair = pair_of(in.src_dtype, in.dst_dtype);
    VLNCE_CHECK_ARG(pair != PAIR_NONE, "rollout_copy: field %d: dtype %d -> %d is not a supported pair",
                    k, in.src_dtype, in.dst_dtype);
    VLNCE_CHECK_ARG(in.src && in.dst && in.E > 0 && in.E < (1L << 40), "rollout_copy: field %d: bad geometry",
                    k);
    VLNCE_CHECK_ARG(n_rows == 1 || (in.src_row_stride >= 0 && in.dst_row_stride >= in.E),
                    "rollout_copy: field %d: row strides %ld -> %ld for rows of %ld elements", k,
                    in.src_row_stride, in.dst_row_stride, in.E);
    const int sb = dtype_bytes(in.src_dtype), db = dtype_bytes(in.dst_dtype);
    const uintptr_t sp = reinterpret_cast<uintptr_t>(in.src), dp = reinterpret_cast<uintptr_t>(in.dst);
    VLNCE_CHECK_ARG(sp % sb == 0 && dp % db == 0, "rollout_copy: field %d: misaligned pointer", k);
    a.src = static_cast<const unsigned char*>(in.src);
    a.dst = static_cast<unsigned char*>(in.dst);
    a.E = in.E;
    a.src_stride = n_rows == 1 ? 0 : in.src_row_stride;
    a.dst_stride = n_rows == 1 ? 0 : in.dst_row_stride;
    a.pair = (short)pair;
    a.vec = sb == db && sp % 16 == 0 && dp % 16 == 0 && (a.src_stride * sb) % 16 == 0 &&
            (a.dst_stride * db) % 16 == 0;
    a.first_block = blocks;
    blocks += field_blocks(in.E, n_rows, &a.chunks_per_row);
    VLNCE_CHECK_ARG(blocks < (1L << 31), "rollout_copy: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(rollout_copy_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), arg);
  VLNCE_CHECK_LAUNCH("rollout_copy");
  return 0;
}

extern "C" int vlnce_rollout_gather(const vlnce_rollout_gfield* fields, int n_fields, const int* envs,
                                    int n_envs, int T, vlnce_stream_t stream) {
  static_assert(sizeof(GatherArg) <= 4096, "launch arguments");
  VLNCE_CHECK_ARG(fields && envs && T > 0, "rollout_gather: bad argument");
  VLNCE_CHECK_ARG(n_fields > 0 && n_fields <= VLNCE_ROLLOUT_MAX_FIELDS,
                  "rollout_gather: %d fields (1..%d per call)", n_fields, VLNCE_ROLLOUT_MAX_FIELDS);
  VLNCE_CHECK_ARG(n_envs > 0 && n_envs <= VLNCE_ROLLOUT_MAX_ENVS,
                  "rollout_gather: %d environments (1..%d per call)", n_envs, VLNCE_ROLLOUT_MAX_ENVS);
  GatherArg arg{};
  arg.n_fields = n_fields;
  arg.n_envs = n_envs;
  arg.T = T;
  for (int j = 0; j < n_envs; ++j) arg.envs[j] = envs[j];
  long blocks = 0;
  for (int k = 0; k < n_fields; ++k) {
    const vlnce_rollout_gfield& in = fields[k];
    GatherFieldArg& a = arg.f[k];
    VLNCE_CHECK_ARG(in.arena && in.out && in.E > 0 && in.E < (1L << 40) && in.N > 0 && in.out_N >= n_envs,
                    "rollout_gather: field %d: bad geometry", k);
    VLNCE_CHECK_ARG(in.elem_bytes == 1 || in.elem_bytes == 2 || in.elem_bytes == 4 || in.elem_bytes == 8,
                    "rollout_gather: field %d: elements of %d bytes (1 | 2 | 4 | 8)", k, in.elem_bytes);
    for (int j = 0; j < n_envs; ++j)
      VLNCE_CHECK_ARG(envs[j] >= 0 && envs[j] < in.N,
                      "rollout_gather: field %d: environment %d outside the arena's %ld", k, envs[j], in.N);
    const uintptr_t ap = reinterpret_cast<uintptr_t>(in.arena), op = reinterpret_cast<uintptr_t>(in.out);
    VLNCE_CHECK_ARG(ap % in.elem_bytes == 0 && op % in.elem_bytes == 0,
                    "rollout_gather: field %d: misaligned pointer", k);
    a.arena = static_cast<const unsigned char*>(in.arena);
    a.out = static_cast<unsigned char*>(in.out);
    a.E = in.E;
    a.N = in.N;
    a.out_N = in.out_N;
    a.elem_bytes = (short)in.elem_bytes;
    const bool vec = ap % 16 == 0 && op % 16 == 0 && (in.E * in.elem_bytes) % 16 == 0;
    a.flags = (short)((vec ? 1 : 0) | (in.once ? 2 : 0));
    a.first_block = blocks;
    blocks += field_blocks(in.E, (long)(in.once ? 1 : T) * n_envs, &a.chunks_per_row);
    VLNCE_CHECK_ARG(blocks < (1L << 31), "rollout_gather: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(rollout_gather_kernel, dim3((unsigned)blocks), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), arg);
  VLNCE_CHECK_LAUNCH("rollout_gather");
  return 0;
}

extern "C" int vlnce_ppo_advantages(const float* returns, const float* value_preds, float* adv, int T,
                                    int N, int normalize, float eps, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(returns && value_preds && adv && T > 0 && N > 0, "ppo_advantages: bad argument");
  hipLaunchKernelGGL(ppo_advantages_kernel, dim3(1), dim3(ADV_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), returns, value_preds, adv, (long)T * N,
                     normalize, (double)eps);
  VLNCE_CHECK_LAUNCH("ppo_advantages");
  return 0;
}
