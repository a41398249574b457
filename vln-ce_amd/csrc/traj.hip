// DAgger rollout collection on the device (the WRITE half of the feature
// cache).  The reference's collection loop (dagger_trainer.py:248-467) leaves the device on every
// step: two forward hooks copy the trunk outputs to the host (o.cpu(), 8.9 MB of fp32 at 64
// environments), every environment's previous / expert / chosen action is read back with .item(),
// and a finished episode is re-stacked and narrowed to fp16 by numpy.  Here the per-step rows
// accumulate in arenas [num_envs][capacity][D] on the device, already in their storage dtype:
//   vlnce_traj_append        one launch appends one step of every sensor for every live environment
//   vlnce_dagger_mix_actions the beta mix, the skip rule and prev_actions.copy_ (:414-442), one launch
// Both are pure data movement; the sensor table and the row -> (slot, step) map travel in the
// launch's argument struct (as GatherArg in ingest.hip), so a call makes no copy, no allocation
// and no synchronisation.
#include "common.h"

namespace {

enum { PATH_ELEM = 0, PATH_VEC4 = 1, PATH_P16 = 2, PATH_P4 = 3 };

struct TrajSensorArg {
  const unsigned char* src;
  unsigned char* dst;
  long row_stride, c_stride, p_stride;
  int C, P;
  int src_dtype, dst_dtype;
  int path;
  int blocks_per_row;   // 256 work items (elements, 4-vectors or channels) per block
  int first_block;      // of this sensor in the launch's grid
};

struct TrajArg {
  TrajSensorArg s[VLNCE_TRAJ_MAX_SENSORS];
  int slot[VLNCE_TRAJ_MAX_ROWS];
  int step[VLNCE_TRAJ_MAX_ROWS];
  long capacity;
  int n_sensors;
};

// the reference's conversions: batch_obs casts every sensor to float (int64 tokens included),
// numpy's astype(float16) then rounds to nearest even, keeps subnormals, overflows to infinity --
// v_cvt_f16_f32 in the default modes
template <typename S, typename D>
__device__ __forceinline__ D convert(S v) {
  if constexpr (sizeof(D) == 2) return (_Float16)(float)v;
  else return (D)v;
}

template <typename T, int N>
struct alignas(sizeof(T) * N < 16 ? sizeof(T) * N : 16) Pack {
  T v[N];
};

// a lane owns channel c of one row: P loads, each coalesced along c across the wave (the trunks'
// NHWC view: c_stride 1), then its P outputs as one contiguous run of the NCHW row
template <typename S, typename D, int P>
__device__ __forceinline__ void row_transposed(const S* __restrict__ src, D* __restrict__ dst,
                                               long p_stride, int C, int c) {
  if (c >= C) return;
  const S* q = src + c;
  Pack<D, P> out;
#pragma unroll
  for (int p = 0; p < P; ++p) out.v[p] = convert<S, D>(q[p * p_stride]);
  *reinterpret_cast<Pack<D, P>*>(dst + (long)c * P) = out;
}

template <typename S, typename D>
__device__ __forceinline__ void append_rows(const TrajSensorArg& a, long src_row, long dst_row,
                                            int item) {
  const long Dn = (long)a.C * a.P;
  const S* src = reinterpret_cast<const S*>(a.src) + src_row * a.row_stride;
  D* dst = reinterpret_cast<D*>(a.dst) + dst_row * Dn;
  if (a.path == PATH_P16) {
    row_transposed<S, D, 16>(src, dst, a.p_stride, a.C, item);
  } else if (a.path == PATH_P4) {
    row_transposed<S, D, 4>(src, dst, a.p_stride, a.C, item);
  } else if (a.path == PATH_VEC4) {
    if (4L * item >= Dn) return;
    const Pack<S, 4> in = *reinterpret_cast<const Pack<S, 4>*>(src + 4L * item);
    Pack<D, 4> out;
#pragma unroll
    for (int k = 0; k < 4; ++k) out.v[k] = convert<S, D>(in.v[k]);
    *reinterpret_cast<Pack<D, 4>*>(dst + 4L * item) = out;
  } else {   // any strides, any alignment: one output element per lane
    if (item >= Dn) return;
    const int c = item / a.P, p = item - c * a.P;
    dst[item] = convert<S, D>(src[c * a.c_stride + p * a.p_stride]);
  }
}

__global__ __launch_bounds__(256) void traj_append_kernel(TrajArg arg) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < VLNCE_TRAJ_MAX_SENSORS; ++k)
    if (k < arg.n_sensors && (int)blockIdx.x >= arg.s[k].first_block) s = k;
  const TrajSensorArg& a = arg.s[s];
  const int local = (int)blockIdx.x - a.first_block;
  const int r = local / a.blocks_per_row;
  const int item = (local - r * a.blocks_per_row) * 256 + (int)threadIdx.x;
  const long dst_row = (long)arg.slot[r] * arg.capacity + arg.step[r];
  switch (a.src_dtype * 4 + a.dst_dtype) {   // (uniform over the block)
    case VLNCE_TRAJ_F32 * 4 + VLNCE_TRAJ_F16: append_rows<float, _Float16>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_F32 * 4 + VLNCE_TRAJ_F32: append_rows<float, float>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_F32 * 4 + VLNCE_TRAJ_I64: append_rows<float, long>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_I64 * 4 + VLNCE_TRAJ_F16: append_rows<long, _Float16>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_I64 * 4 + VLNCE_TRAJ_F32: append_rows<long, float>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_I64 * 4 + VLNCE_TRAJ_I64: append_rows<long, long>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_U8 * 4 + VLNCE_TRAJ_F16: append_rows<unsigned char, _Float16>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_U8 * 4 + VLNCE_TRAJ_F32: append_rows<unsigned char, float>(a, r, dst_row, item); break;
    case VLNCE_TRAJ_U8 * 4 + VLNCE_TRAJ_I64: append_rows<unsigned char, long>(a, r, dst_row, item); break;
    default: break;   // (the launcher admits nothing else)
  }
}

// no __restrict__: the caller may hand prev_actions in as `actions`
template <typename E>
__global__ __launch_bounds__(256) void dagger_mix_actions_kernel(const long* actions, const E* expert,
                                                                 const float* uniform, float beta,
                                                                 int n, long* prev_actions,
                                                                 long* stepped) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long e = (long)expert[i];
  long a = uniform[i] < beta ? e : actions[i];
  const bool skip = e == -1;
  if (skip) a = 0;
  prev_actions[i] = a;
  stepped[i] = a;
  stepped[n + i] = skip ? 1 : 0;
}

inline int elem_bytes(int dtype) {
  return dtype == VLNCE_TRAJ_I64 ? 8 : dtype == VLNCE_TRAJ_F32 ? 4 : dtype == VLNCE_TRAJ_F16 ? 2 : 1;
}

}  // namespace

extern "C" int vlnce_traj_append(const vlnce_traj_sensor* sensors, int n_sensors, const int* slots,
                                 const int* steps, int n_rows, long capacity,
                                 vlnce_stream_t stream) {
  static_assert(sizeof(long) == sizeof(int64_t), "LP64");
  static_assert(sizeof(TrajArg) <= 4096, "launch arguments");
  VLNCE_CHECK_ARG(sensors && slots && steps && capacity > 0, "traj_append: bad argument");
  VLNCE_CHECK_ARG(n_sensors > 0 && n_sensors <= VLNCE_TRAJ_MAX_SENSORS,
                  "traj_append: %d sensors (1..%d per call)", n_sensors, VLNCE_TRAJ_MAX_SENSORS);
  VLNCE_CHECK_ARG(n_rows > 0 && n_rows <= VLNCE_TRAJ_MAX_ROWS, "traj_append: %d rows (1..%d per call)",
                  n_rows, VLNCE_TRAJ_MAX_ROWS);
  TrajArg arg{};
  arg.capacity = capacity;
  arg.n_sensors = n_sensors;
  for (int r = 0; r < n_rows; ++r) {
    VLNCE_CHECK_ARG(slots[r] >= 0 && steps[r] >= 0 && steps[r] < capacity,
                    "traj_append: row %d -> (slot %d, step %d) outside the arena (capacity %ld)", r,
                    slots[r], steps[r], capacity);
    arg.slot[r] = slots[r];
    arg.step[r] = steps[r];
  }
  long blocks = 0;
  for (int k = 0; k < n_sensors; ++k) {
    const vlnce_traj_sensor& in = sensors[k];
    TrajSensorArg& a = arg.s[k];
    VLNCE_CHECK_ARG(in.src && in.dst && in.C > 0 && in.P > 0 && in.row_stride >= 0 &&
                        in.c_stride >= 0 && in.p_stride >= 0,
                    "traj_append: sensor %d: bad geometry", k);
    VLNCE_CHECK_ARG(in.src_dtype == VLNCE_TRAJ_F32 || in.src_dtype == VLNCE_TRAJ_I64 ||
                        in.src_dtype == VLNCE_TRAJ_U8,
                    "traj_append: sensor %d: source dtype %d (f32 | i64 | u8)", k, in.src_dtype);
    VLNCE_CHECK_ARG(in.dst_dtype == VLNCE_TRAJ_F16 || in.dst_dtype == VLNCE_TRAJ_F32 ||
                        in.dst_dtype == VLNCE_TRAJ_I64,
                    "traj_append: sensor %d: storage dtype %d (f16 | f32 | i64)", k, in.dst_dtype);
    const long Dn = (long)in.C * in.P;
    VLNCE_CHECK_ARG(Dn < (1L << 30), "traj_append: sensor %d: rows of %ld elements", k, Dn);
    const int sb = elem_bytes(in.src_dtype), db = elem_bytes(in.dst_dtype);
    const uintptr_t sp = reinterpret_cast<uintptr_t>(in.src), dp = reinterpret_cast<uintptr_t>(in.dst);
    VLNCE_CHECK_ARG(sp % sb == 0 && dp % db == 0, "traj_append: sensor %d: misaligned pointer", k);
    a.src = static_cast<const unsigned char*>(in.src);
    a.dst = static_cast<unsigned char*>(in.dst);
    a.row_stride = in.row_stride;
    a.c_stride = in.c_stride;
    a.p_stride = in.p_stride;
    a.C = in.C;
    a.P = in.P;
    a.src_dtype = in.src_dtype;
    a.dst_dtype = in.dst_dtype;
    long items = Dn;
    a.path = PATH_ELEM;
    if ((in.P == 16 || in.P == 4) && in.c_stride == 1 && dp % 16 == 0) {
      // a lane's P outputs start at (row * C + c) * P * db bytes: a multiple of its store width
      a.path = in.P == 16 ? PATH_P16 : PATH_P4;
      items = in.C;
    } else if (in.P == 1 && in.c_stride == 1 && Dn % 4 == 0 && in.row_stride % 4 == 0 &&
               sp % (4 * sb < 16 ? 4 * sb : 16) == 0 && dp % (4 * db < 16 ? 4 * db : 16) == 0) {
      a.path = PATH_VEC4;
      items = Dn / 4;
    }
    a.blocks_per_row = (int)((items + 255) / 256);
    a.first_block = (int)blocks;
    blocks += (long)a.blocks_per_row * n_rows;
    VLNCE_CHECK_ARG(blocks < (1L << 31), "traj_append: grid of %ld blocks", blocks);
  }
  hipLaunchKernelGGL(traj_append_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), arg);
  VLNCE_CHECK_LAUNCH("traj_append");
  return 0;
}

extern "C" int vlnce_dagger_mix_actions(const int64_t* actions, const void* expert, int expert_dtype,
                                        const float* uniform, float beta, int n,
                                        int64_t* prev_actions, int64_t* stepped,
                                        vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(actions && expert && uniform && prev_actions && stepped && n > 0,
                  "dagger_mix_actions: bad argument");
  VLNCE_CHECK_ARG(expert_dtype == VLNCE_TRAJ_F32 || expert_dtype == VLNCE_TRAJ_I64,
                  "dagger_mix_actions: expert dtype %d (f32 | i64)", expert_dtype);
  const dim3 g(ceil_div(n, 256)), blk(256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long* act = reinterpret_cast<const long*>(actions);
  long* prev = reinterpret_cast<long*>(prev_actions);
  long* out = reinterpret_cast<long*>(stepped);
  if (expert_dtype == VLNCE_TRAJ_F32)
    hipLaunchKernelGGL(dagger_mix_actions_kernel<float>, g, blk, 0, s, act,
                       static_cast<const float*>(expert), uniform, beta, n, prev, out);
  else
    hipLaunchKernelGGL(dagger_mix_actions_kernel<long>, g, blk, 0, s, act,
                       static_cast<const long*>(expert), uniform, beta, n, prev, out);
  VLNCE_CHECK_LAUNCH("dagger_mix_actions");
  return 0;
}
