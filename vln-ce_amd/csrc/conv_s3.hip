// conv_s3_kernel: stride-1 1x1 convolutions with SHORT K (64 or 128 input channels) and wide N
// (the 64->256 / 128->512 expansions of the bottlenecks: 268 / 134 MB of output per launch).
// These launches are bound by the HBM write of their output, and in conv_u3_kernel they reach
// 2.2-2.7 TB/s: a tile there is 2-4 K-chunks of MFMAs and a 128 KB store burst, and the loads of
// the next tile (B fragments of its second k-slab, raw A two chunks ahead) queue behind the burst
// in the wave's one in-order vmcnt, so a wave alternates between draining and computing
// (profiles/archive/r03_h_u3_phase_timers_short_k.txt).  Here nothing a tile needs is loaded less than
// a tile before its use, and a tile's stores are issued UNDER the next tile's MFMAs:
//   * the B fragments of the wave's 32 columns for ALL of K stay in registers for the whole
//     launch (K = 64: 48 VGPRs, K = 128: 96) -- a workgroup keeps its column tile;
//   * the raw A rows of tile t + 2 (K = 128: t + 1) are requested while tile t is transformed
//     (64-row tiles: one float4 per thread and chunk);
//   * TWO accumulator sets: while the MFMAs of tile t fill one, the 32 stores of tile t - 1 drain
//     the other, a few behind every k-slab (sched_group_barrier pins the interleave; the epilogue
//     activation is a select so the slab body stays one basic block).  Stores are fire-and-forget:
//     when the store queue is full the wave stalls at a store and the SIMD's other wave issues
//     its MFMAs, so per tile a CU needs max(stores, MFMAs) instead of their sum.  Round 3's
//     serial form (transform, barrier, MFMAs, then 32 stores at the CU's ~12 B/cycle = 54 % of
//     the launch) measured 90.4 / 75.0 us on 64->256 / 128->512 at num_envs 64; this form 71.4 /
//     72.1 us (profiles/r04_a_conv_s3_pipelined_epilogue.txt);
//   * the first two tiles are peeled: the compiler's s_waitcnt at a loop header is the minimum
//     over the paths into it, and entered from the preamble the wait for the raw rows would
//     drain the previous tile's stores on every trip.
// 8 waves (two per SIMD), wave w owns columns [32w, 32w + 32) of a 64 x 256 tile; one barrier
// per tile.  Arithmetic, patch rows, fragment layout and statistics are conv_u3_kernel's
// (conv_u3.hip).
// STORE = false is the statistics-only launch (vlnce_epilogue.stats_only): the same tiles, the same
// MFMA order and the same wave_bn_tile / wave_stats_block calls on the same accumulators, but no
// output: the stores(...) lambda, the second accumulator set and the store interleave are
// compiled out, and a tile's statistics are taken right behind its own MFMAs.  It is the first
// half of a block end that regenerates conv3's output instead of reading it back (DESIGN.md
// section 6): the BatchNorm statistics need a pass over conv3's INPUT, not a stored output.
#include "igemm_shared.h"

using namespace vlnce_detail;

namespace vlnce_detail {
namespace {

template <int NCC, int MATH, bool STORE>
__global__ __launch_bounds__(512) void conv_s3_kernel(IgemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Planes<MATH> PL;
  constexpr int P3_ROW = PL::ROW, NA = PL::NA, NP = PL::NP;
  constexpr int BM = 64, MT = 2, KS = NCC * 2;
  constexpr int CBUF = BM * P3_ROW;            // one chunk of a tile's patch
  constexpr int PBUF = NCC * CBUF;             // one tile's patch
  constexpr int SPS = 32 / KS;                 // stores of the previous tile behind each k-slab
  extern __shared__ __attribute__((aligned(16))) char xsm[];  // [2][PBUF] + prologue vectors

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int trow = tid >> 3;
  const int lk4 = (tid & 7) * 4;

  const int n0 = ((int)blockIdx.x % p.tiles_n) * 256;
  const int wg = (int)blockIdx.x / p.tiles_n, nwg = (int)gridDim.x / p.tiles_n;
  const int my_tiles = (p.tiles_m - wg + nwg - 1) / nwg;

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.A)), 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.Bfrag)), 0, (int)((long)p.N * p.K * 6),
      0x00020000);
  // (STORE = false: C is null and c_bytes 0 -- the descriptor is never used)
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.C), 0, STORE ? (int)p.c_bytes : 0, 0x00020000);
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();
  const bool relu_out = p.act == VLNCE_ACT_RELU;  // the launcher admits VLNCE_ACT_NONE / _RELU only

  bf16x8 bres[KS][3];
  {
    const int vb = (n0 / 32 + wave) * KS * 3072 + lane * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        bres[ks][q] = __builtin_bit_cast(
            bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, vb + q * 1024, ks * 3072, 0));
  }
  // prologue vectors always in LDS here: the second accumulator set takes their registers
  float* const vlds = reinterpret_cast<float*>(xsm + 2 * PBUF);  // [3][NCC * 32]
  if (tid < 8) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f}, one4 = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int c = 0; c < NCC; ++c) {
      f32x4 s_ = one4, t_ = zero4, c_ = zero4;
      if (p.in_scale != nullptr) {
        s_ = ldg4(p.in_scale + c * 32 + lk4);
        t_ = ldg4(p.in_shift + c * 32 + lk4);
        if (p.in_center) c_ = ldg4(p.in_center + c * 32 + lk4);
      }
      *reinterpret_cast<f32x4*>(vlds + c * 32 + lk4) = s_;
      *reinterpret_cast<f32x4*>(vlds + NCC * 32 + c * 32 + lk4) = t_;
      *reinterpret_cast<f32x4*>(vlds + 2 * NCC * 32 + c * 32 + lk4) = c_;
    }
  }
  __syncthreads();
  const int col = n0 + wave * 32 + l31;
  const float e_sc = (p.scale ? p.scale[col] : 1.f) * PL::POST;
  const float e_sh = p.shift ? p.shift[col] : 0.f;

  // raw A ring: two tiles ahead for K = 64; ONE for K = 128, where the second
  // accumulator set leaves no registers for it (with the stores spread over the MFMA phase the
  // request of tile t + 1 sits behind the stores of tile t - 2 only, a whole tile old)
  constexpr int RING = NCC > 2 ? 1 : 2;
  f32x4 raw[RING][NCC];
  auto load_raw = [&](f32x4 (&r)[NCC], int round) {
    const int m = (wg + round * nwg) * BM + trow;
    const int vo = (round < my_tiles && m < p.M) ? (m * p.lda + lk4) * 4 : BUF_OOB;
#pragma unroll
    for (int c = 0; c < NCC; ++c)
      r[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, c * 128, 0));
  };
#pragma unroll
  for (int k = 0; k < RING; ++k) load_raw(raw[k], k);
  constexpr int NACC = STORE ? 2 : 1;
  constexpr int B1 = NACC - 1;   // the accumulator set of the odd tiles
  f32x16 acc[NACC][MT];  // [tile parity][row block]
#pragma unroll
  for (int b = 0; b < NACC; ++b)
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][i][r] = 0.f;
  const int a_off = l31 * P3_ROW + half * 16;

  WaveBn<1> wbn;   // BatchNorm finished in this launch (p.bn): the wave's running column sums
  wave_bn_reset(wbn);
  // statistics of a finished tile (raw accumulators, 32-row blocks)
  auto stats = [&](const f32x16 (&a)[MT], int m0) {
    if (p.bn.acc != nullptr) {
      wave_bn_tile<MT, 1>(reinterpret_cast<const f32x16(&)[MT][1]>(a), wbn, p.bn.acc, n0 + wave * 32,
                          p.N, p.M - m0, half, l31, PL::POST);
    } else if (p.stat_partial != nullptr) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
        wave_stats_block<1>(reinterpret_cast<const f32x16(&)[1]>(a[i]), p.stat_partial,
                            m0 / 32 + i, p.M - (m0 + i * 32), n0 + wave * 32, p.N, half, l31, PL::POST);
    }
  };
  // stores [first, first + count) of the 32 of a finished tile; the registers are cleared behind
  auto stores = [&](f32x16 (&a)[MT], int m0, int first, int count) {
    const int rows_left = p.M - (m0 + 4 * half);
    const int e_voff = (int)((((long)(m0 + 4 * half)) * p.ldc + col) * 4);
#pragma unroll
    for (int k = first; k < first + count; ++k) {
      const int i = k >> 4, r2 = k & 15;
      const int rw = i * 32 + (r2 & 3) + 8 * (r2 >> 2);
      const float lin = a[i][r2] * e_sc + e_sh;
      const float v = relu_out ? (lin > 0.f ? lin : 0.f) : lin;  // (act is none or ReLU: selects, no branch)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc_c,
                                            rw < rows_left ? e_voff : BUF_OOB, rw * p.ldc * 4, 0);
      a[i][r2] = 0.f;
    }
  };

  // one tile: cur = accumulator set of this tile, prv = the set of the tile before it (its
  // statistics and stores are issued here, under this tile's MFMAs)
  auto tile = [&](int round, f32x4 (&r)[NCC], f32x16 (&cur)[MT], f32x16 (&prv)[MT]) {
    const int m0 = (wg + round * nwg) * BM;
    const int m0_prev = (wg + (round - 1) * nwg) * BM;
    const bool has_prev = round > 0;
    char* const pb = xsm + (round & 1) * PBUF;
    const bool row_ok = m0 + trow < p.M;
#pragma unroll
    for (int c = 0; c < NCC; ++c) {
      f32x4 v = r[c];
      const f32x4 s_ = *reinterpret_cast<const f32x4*>(vlds + c * 32 + lk4);
      const f32x4 t_ = *reinterpret_cast<const f32x4*>(vlds + NCC * 32 + c * 32 + lk4);
      const f32x4 c_ = *reinterpret_cast<const f32x4*>(vlds + 2 * NCC * 32 + c * 32 + lk4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = fmaxf(fmaf(v[e] - c_[e], s_[e], t_[e]), relu_floor);
        v[e] = row_ok ? v[e] : 0.f;
      }
      p3_split_store<MATH>(v, pb + c * CBUF + trow * P3_ROW + lk4 * 2);
    }
    load_raw(r, round + RING);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (STORE)
      if (has_prev) stats(prv, m0_prev);
#pragma unroll
    for (int c = 0; c < NCC; ++c)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 f[MT][NA];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int q = 0; q < NA; ++q)
            f[i][q] = *reinterpret_cast<const bf16x8*>(pb + c * CBUF + a_off + i * 32 * P3_ROW +
                                                       q * 64 + s2 * 32);
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
          for (int i = 0; i < MT; ++i)
            cur[i] = plane_mfma<MATH>(f[i][PL::PA[q]], bres[c * 2 + s2][PL::PB[q]], cur[i]);
        // the previous tile's next SPS stores ride behind this slab's 12 MFMAs (a tile whose
        // predecessor does not exist stores to the out-of-range offset: no branch in the body)
        if constexpr (STORE) {
          stores(prv, has_prev ? m0_prev : p.M, (c * 2 + s2) * SPS, SPS);
          // schedule of the slab: its 12 MFMAs with the SPS stores spread evenly between them
          // (K = 64: 2 MFMAs, store, 1 MFMA, store, four times; K = 128: 3 MFMAs, store, four times)
          if constexpr (MATH == MATH_F16X3) {
            // 6 MFMAs per slab: K = 64: MFMA, store, store, MFMA, store (x2, then 2 MFMAs + 2 stores);
            // K = 128: 3 MFMAs, 2 stores, twice
#pragma unroll
            for (int g = 0; g < 2; ++g) {
              if constexpr (SPS == 8) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
              } else {
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 2, 0);
              }
            }
          } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              if constexpr (SPS == 8) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);  // VMEM write
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
              } else {
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
              }
            }
          }
        }
      }
    if constexpr (!STORE) {   // nothing to hide the statistics under: taken here, registers cleared behind
      stats(cur, m0);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) cur[i][r2] = 0.f;
    }
  };
  // The first two tiles are peeled: the compiler's s_waitcnt at a loop header is the minimum
  // over the paths into it, and entered straight from the preamble the first wait for raw rows
  // would be vmcnt(3) on EVERY trip -- i.e. the stores of the tile before would be drained every
  // second tile (round 3's unpeeled form had exactly that: vmcnt(3) / vmcnt(35) alternated in its ISA).
  // Behind the peeled tiles both ways into the loop have a tile's 32 stores after the request.
  if (my_tiles <= 0) return;  // (cannot happen with launch_s3's grid; uniform per workgroup)
  tile(0, raw[0], acc[0], acc[B1]);
  if (1 < my_tiles) tile(1, raw[RING - 1], acc[B1], acc[0]);
  for (int round = 2; round < my_tiles; round += 2) {
    tile(round, raw[0], acc[0], acc[B1]);
    if (round + 1 < my_tiles) tile(round + 1, raw[RING - 1], acc[B1], acc[0]);
  }
  if constexpr (!STORE) {
    if (p.bn.acc != nullptr) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);
  } else {  // the last tile's epilogue has nothing left to hide under
    const int m0 = (wg + (my_tiles - 1) * nwg) * BM;
    if ((my_tiles - 1) & 1) {
      stats(acc[B1], m0);
      if (p.bn.acc != nullptr) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);  // in front of the stores
      stores(acc[B1], m0, 0, 32);
    } else {
      stats(acc[0], m0);
      if (p.bn.acc != nullptr) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);
      stores(acc[0], m0, 0, 32);
    }
  }
#endif
}

template <int NCC, int MATH, bool STORE>
int launch_s3(const IgemmParams& p, hipStream_t stream) {
  constexpr int smem_bytes = 2 * NCC * 64 * Planes<MATH>::ROW + 3 * NCC * 32 * 4;  // two tile patches + the prologue vectors
  auto kern = conv_s3_kernel<NCC, MATH, STORE>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes);
    if (e != hipSuccess) {
      vlnce_set_error("conv_s3: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return 2;
    }
    attr_set = true;
  }
  IgemmParams q = p;
  q.tiles_m = ceil_div(p.M, 64);
  q.tiles_n = p.N / 256;
  q.splitk = 1;
  const int cus = x3_cus();
  long grid = (long)q.tiles_m * q.tiles_n;
  if (grid > cus) grid = cus - cus % q.tiles_n;  // resident workgroups, a multiple of tiles_n
  if (const int cap = vlnce_opt(VLNCE_OPT_S3_WGS); cap > 0 && grid > cap)   // option "s3_wgs" (tests)
    grid = cap >= q.tiles_n ? cap - cap % q.tiles_n : q.tiles_n;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), smem_bytes, stream, q);
  VLNCE_CHECK_LAUNCH("conv_s3");
  return 0;
}

template <bool STORE>
int s3_launch_(const IgemmParams& p, hipStream_t stream) {
  if (p.math == MATH_F16X3)
    return p.Cin == 64 ? launch_s3<2, MATH_F16X3, STORE>(p, stream)
                       : launch_s3<4, MATH_F16X3, STORE>(p, stream);
  return p.Cin == 64 ? launch_s3<2, MATH_BF16X6, STORE>(p, stream)
                     : launch_s3<4, MATH_BF16X6, STORE>(p, stream);
}

}  // namespace

int s3_launch(const IgemmParams& p, hipStream_t stream) {   // Cin is 64 or 128 (the router's test)
  // the statistics-only instance has no output: a launch must say which one it means
  if (p.stats_only ? p.C != nullptr : p.C == nullptr) {
    vlnce_set_error("conv_s3: %s", p.stats_only ? "a statistics-only launch takes no output pointer"
                                                : "null output");
    return 1;
  }
  if (p.stats_only && p.bn.acc == nullptr && p.stat_partial == nullptr) {
    vlnce_set_error("conv_s3: a statistics-only launch needs bn or stat_partial");
    return 1;
  }
  note_conv_kernel(VLNCE_CONV_KERNEL(VLNCE_CONV_PATH_P3, p.math, VLNCE_CONV_KERNEL_S3,
                                     p.Cin == 64 ? 64 : 128, p.stats_only ? 1 : 0, 0));
  return p.stats_only ? s3_launch_<false>(p, stream) : s3_launch_<true>(p, stream);
}

}  // namespace vlnce_detail
