// conv_r3_kernel: the END of a ResNet-50 bottleneck of layers 1-2 in train mode, with conv3's raw
// output REGENERATED instead of read back (vlnce_prologue.regen):
//   raw3 = conv1x1(relu(bn2(raw2)), W3)                    K1 = 64 / 128 -> N1 = 4 K1   (first product)
//   y    = relu(bn3(raw3) + skip)  [skip: identity, or a raw downsample output with its own BatchNorm]
//   out  = conv1x1(y, Wnext)                               K2 = N1 -> N2 = 64 / 128 / 256 (second product)
// y goes to side_out (the next block's skip), out is stored raw and its BatchNorm column sums /
// tile moments are taken like in every other convolution here.  bn3's vectors come from a
// statistics-only launch of conv_s3_kernel over the same raw2 (conv_s3.hip, STORE = false) and the
// ordinary finalize launch: raw3 never exists in memory.  Per 64 rows that is 64 x (K1 + N1 + N1 + N2)
// floats moved instead of 64 x (K1 + 2 N1) + 64 x (2 N1 + N1 + N2) by conv_s3 + the dual block end.
//
// One workgroup (8 waves) per CU walks 64-row tiles a grid apart, as conv_s3_kernel does.  Per tile:
//   1. every thread transforms one float4 per 32-channel chunk of raw2 (bn2, ReLU, plane split) into
//      the LDS patch P1 -- conv_s3_kernel's code and patch format; the rows of the next tile are
//      requested here;
//   2. per 256-column pass over N1 (one for K1 = 64, two for K1 = 128) wave w owns columns
//      [32 w, 32 w + 32): the MFMA sequence per output element is conv_s3_kernel's (same
//      Planes<MATH>, same k-slab order, B fragments of W3 in registers), so the accumulators ARE the
//      values the statistics were taken from;
//   3. epilogue in registers, in the operation order of the dual loaders of conv_u3 / conv_x3:
//      identity skip  y = max(fma(raw3 - c3, s3, t3) + skip, 0)
//      skip with BN   y = max(fma(raw3 - c3, s3, fma(skip - c2, s2, t3 + t2)), 0)
//      with the skip loaded in the accumulator layout (128 B per row and half-wave);
//   4. y is split into planes and written to the LDS patch Y in the A-fragment row format: chunk w
//      of the pass = the wave's 32 columns.  Neighbouring lanes exchange one value (DPP quad_perm)
//      so that every lane writes whole 32-bit words {column 2i, 2i + 1} of one row;
//   5. second product over the pass's 256 values of K2 from Y against Wnext's B fragments out of
//      L2 (two or three k-slabs in flight), accumulated across the passes: wave w owns 32-column block w % (N2 / 32); N2 = 256: both
//      32-row blocks, N2 = 128: row block w / 4, N2 = 64: waves 0-3 only (12 % of the tile's
//      matrix-pipe time idles; the tile is bound by its 64 x (2 N1 + ...) floats);
//   6. y is stored to side_out and the finished 64 x N2 tile to C BEHIND the second product: a wave's
//      loads return in issue order behind its stores (one vmcnt), so the B fragments of step 5 must
//      not queue behind them; the first fragments and the skip of the next pass / tile are requested
//      in front of the stores for the same reason.
// Barriers per tile: one behind step 1, one behind step 4 of every pass, one between two passes
// (Y is reused).  No communication between workgroups.
//
// LDS per workgroup = P1 + Y + bn2's vectors = (K1 / 32 + 8) x 64 x ROW + 12 K1 bytes:
//   fp16 planes (ROW 144): K1 = 64  92 928 B,  K1 = 128 112 128 B
//   bf16 planes (ROW 208): K1 = 64 133 888 B,  K1 = 128 161 280 B      (a CU has 163 840 B)
#include "igemm_shared.h"

using namespace vlnce_detail;

namespace vlnce_detail {
namespace {

// lane l <-> lane l ^ 1 (DPP quad_perm [1, 0, 3, 2])
__device__ __forceinline__ float swap_odd_even(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

template <int NCC, int N2B, int SKIP, int MATH>
__global__ __launch_bounds__(512) void conv_r3_kernel(IgemmParams p, RegenParams g) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Planes<MATH> PL;
  constexpr int ROW = PL::ROW, NA = PL::NA, NP = PL::NP;
  constexpr int BM = 64, MT = 2;
  constexpr int KS1 = NCC * 2;              // k-slabs (16 values of K1) of the first product
  constexpr int NPASS = NCC / 2;            // 256-column passes over N1 = 128 NCC
  constexpr int KS2 = NCC * 8;              // k-slabs of the whole second product (K2 = N1)
  constexpr int CBUF = BM * ROW;            // one 32-channel chunk of a 64-row patch
  constexpr int P1 = NCC * CBUF;            // the first product's patch
  constexpr int YB = 8 * CBUF;              // y of one pass: 8 chunks
  constexpr int MT2 = N2B == 8 ? 2 : 1;     // 32-row blocks per wave in the second product
  constexpr int AHEAD = (NCC == 2 && MATH == MATH_F16X3) ? 3 : 2;   // k-slabs of Wnext's fragments in flight
  // K1 = 64: the next tile's first AHEAD slabs are requested in front of this tile's stores (step 6)
  // and stay in registers through its first product; K1 = 128 has no registers for that and
  // requests them at the top of the second product
  constexpr bool EARLY_B2 = NCC == 2;
  constexpr int AH1 = NCC == 2 ? 4 : 2;     // k-slabs of W3's fragments in registers
  // the instances that would otherwise spill keep the scheduler inside one k-slab at a time
  constexpr bool FENCE_SLABS = NCC == 4 || MATH == MATH_BF16X6;
  extern __shared__ __attribute__((aligned(16))) char xsm[];  // [P1][YB] + bn2's vectors

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int trow = tid >> 3;
  const int lk4 = (tid & 7) * 4;
  const int wg = (int)blockIdx.x, nwg = (int)gridDim.x;
  const int my_tiles = (p.tiles_m - wg + nwg - 1) / nwg;
  if (my_tiles <= 0) return;  // (cannot happen with launch_r3's grid; uniform per workgroup)

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(g.x)), 0, (int)g.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_b1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(g.w_frag)), 0, NCC * 128 * NCC * 32 * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_s = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.A2)), 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_y = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.side_out), 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_b2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.Bfrag)), 0, N2B * 32 * NCC * 128 * 6, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.C), 0, (int)p.c_bytes, 0x00020000);
  const float relu2 = g.relu ? 0.f : -__builtin_huge_valf();
  const float relu3 = p.in_relu ? 0.f : -__builtin_huge_valf();

  // W3's fragments of the wave's 32 columns of a pass.  K1 = 64: its four k-slabs stay in registers
  // for the launch.  K1 = 128 (two passes x eight slabs = 192 registers): two slabs in flight, each
  // fetched again from L2 for every tile.
  bf16x8 bres[AH1][3];
  auto load_b1 = [&](bf16x8 (&f)[3], int pass, int ks) {
    const int vb = (pass * 8 + wave) * KS1 * 3072 + lane * 16;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      f[q] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b1, vb + q * 1024, ks * 3072, 0));
  };
  auto preload_b1 = [&](int pass) {
#pragma unroll
    for (int k = 0; k < AH1; ++k) load_b1(bres[k], pass, k);
  };
  preload_b1(0);
  float* const vlds = reinterpret_cast<float*>(xsm + P1 + YB);  // bn2: [3][NCC * 32]
  if (tid < 8) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f}, one4 = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int c = 0; c < NCC; ++c) {
      f32x4 s_ = one4, t_ = zero4, c_ = zero4;
      if (g.scale != nullptr) {
        s_ = ldg4(g.scale + c * 32 + lk4);
        t_ = ldg4(g.shift + c * 32 + lk4);
        if (g.center) c_ = ldg4(g.center + c * 32 + lk4);
      }
      *reinterpret_cast<f32x4*>(vlds + c * 32 + lk4) = s_;
      *reinterpret_cast<f32x4*>(vlds + NCC * 32 + c * 32 + lk4) = t_;
      *reinterpret_cast<f32x4*>(vlds + 2 * NCC * 32 + c * 32 + lk4) = c_;
    }
  }
  __syncthreads();
  // bn3 (and the skip's BatchNorm) of the lane's column in each pass
  float s3[NPASS], t3[NPASS], c3[NPASS], s2[NPASS], c2[NPASS];
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps) {
    const int col = ps * 256 + wave * 32 + l31;
    s3[ps] = p.in_scale[col];
    t3[ps] = p.in_shift[col];
    c3[ps] = p.in_center ? p.in_center[col] : 0.f;
    s2[ps] = c2[ps] = 0.f;
    if constexpr (SKIP == 2) {
      s2[ps] = p.in2_scale[col];
      t3[ps] = t3[ps] + p.in2_shift[col];   // both shifts in one add (as the dual loaders)
      c2[ps] = p.in2_center ? p.in2_center[col] : 0.f;
    }
  }

  f32x4 raw[NCC];
  auto load_raw = [&](int round) {
    const int m = (wg + round * nwg) * BM + trow;
    const int vo = (round < my_tiles && m < p.M) ? (m * g.ldx + lk4) * 4 : BUF_OOB;
#pragma unroll
    for (int c = 0; c < NCC; ++c)
      raw[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, c * 128, 0));
  };
  // the skip of (tile, pass) in the accumulator layout: register r of block i = row
  // i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, column of the lane
  float sk[MT][16];
  auto load_skip = [&](int round, int pass) {
    const int m0 = (wg + round * nwg) * BM;
    const int rows_left = p.M - (m0 + 4 * half);
    const int voff = round < my_tiles
                         ? (int)((((long)(m0 + 4 * half)) * p.lda + pass * 256 + wave * 32 + l31) * 4)
                         : BUF_OOB;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rw = i * 32 + (r & 3) + 8 * (r >> 2);
        sk[i][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                 rsrc_s, rw < rows_left ? voff : BUF_OOB, rw * p.lda * 4, 0));
        if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (eight row selects alive at a time, not 32)
      }
  };
  load_raw(0);
  load_skip(0, 0);

  // the wave's share of the second product
  const bool active2 = N2B == 2 ? wave < 4 : true;
  const int cb = wave % N2B;                        // 32-column block of N2
  const int rb = N2B == 8 ? 0 : (wave / N2B) & 1;   // first 32-row block
  const int vb2 = cb * KS2 * 3072 + lane * 16;
  bf16x8 fb[AHEAD][3];
  auto load_b2 = [&](bf16x8 (&f)[3], int slab) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      f[q] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_b2, vb2 + q * 1024, slab * 3072, 0));
  };
  auto preload_b2 = [&](int ps) {
    if (active2) {
#pragma unroll
      for (int k = 0; k < AHEAD; ++k) load_b2(fb[k], ps * 16 + k);
    }
  };
  if constexpr (EARLY_B2) preload_b2(0);
  WaveBn<1> wbn;
  wave_bn_reset(wbn);
  const int a_off = l31 * ROW + half * 16;
  char* const ypatch = xsm + P1;
  const bool odd = (l31 & 1) != 0;

  for (int round = 0; round < my_tiles; ++round) {
    const int m0 = (wg + round * nwg) * BM;
    // ---- 1. raw2 -> bn2, ReLU, planes -> P1 (conv_s3_kernel's transform)
    {
      const bool row_ok = m0 + trow < p.M;
#pragma unroll
      for (int c = 0; c < NCC; ++c) {
        f32x4 v = raw[c];
        const f32x4 s_ = *reinterpret_cast<const f32x4*>(vlds + c * 32 + lk4);
        const f32x4 t_ = *reinterpret_cast<const f32x4*>(vlds + NCC * 32 + c * 32 + lk4);
        const f32x4 c_ = *reinterpret_cast<const f32x4*>(vlds + 2 * NCC * 32 + c * 32 + lk4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = fmaxf(fmaf(v[e] - c_[e], s_[e], t_[e]), relu2);
          v[e] = row_ok ? v[e] : 0.f;
        }
        p3_split_store<MATH>(v, xsm + c * CBUF + trow * ROW + lk4 * 2);
      }
      load_raw(round + 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    f32x16 acc2[MT2];
#pragma unroll
    for (int i = 0; i < MT2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[i][r] = 0.f;
    const int rows_left = p.M - (m0 + 4 * half);

#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      // ---- 2. first product: conv_s3_kernel's MFMA sequence
      f32x16 acc[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
      for (int c = 0; c < NCC; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          bf16x8 f[MT][NA];
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < NA; ++q)
              f[i][q] = *reinterpret_cast<const bf16x8*>(xsm + c * CBUF + a_off + i * 32 * ROW + q * 64 +
                                                         h * 32);
#pragma unroll
          for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int i = 0; i < MT; ++i)
              acc[i] = plane_mfma<MATH>(f[i][PL::PA[q]], bres[(c * 2 + h) % AH1][PL::PB[q]], acc[i]);
          if (c * 2 + h + AH1 < KS1) load_b1(bres[(c * 2 + h) % AH1], ps, c * 2 + h + AH1);
          if constexpr (FENCE_SLABS) __builtin_amdgcn_sched_barrier(0);
        }
      // (the phases are fenced for the instruction scheduler: left alone it hoists the LDS reads and
      // address arithmetic of later phases over earlier ones and runs out of registers)
      __builtin_amdgcn_sched_barrier(0);
      // ---- 3. + 4. y in registers, planes of y -> patch Y.  (y has registers of its own: written back
      // into the accumulator vectors element by element, the compiler stored element 0 of each block
      // to all its 16 rows of side_out -- the test of the block output against the old pair caught it.)
      float yv[MT][16];
      {
        char* const yb = ypatch + wave * CBUF + half * 4 * ROW + (l31 >> 1) * 4 + (odd ? ROW : 0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rw = i * 32 + (r & 3) + 8 * (r >> 2);
            const float raw3 = fmaf(acc[i][r], PL::POST, 0.f);   // what conv_s3_kernel stores
            float v;
            if constexpr (SKIP == 2)
              v = fmaxf(fmaf(raw3 - c3[ps], s3[ps], fmaf(sk[i][r] - c2[ps], s2[ps], t3[ps])), relu3);
            else
              v = fmaxf(fmaf(raw3 - c3[ps], s3[ps], t3[ps]) + sk[i][r], relu3);
            yv[i][r] = rw < rows_left ? v : 0.f;
          }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            // registers 2j / 2j + 1 = rows rw / rw + 1: the even lane takes row rw of columns
            // {l, l + 1}, the odd lane row rw + 1 of columns {l - 1, l}
            const int rw = i * 32 + ((2 * j) & 3) + 8 * ((2 * j) >> 2);
            const float v0 = yv[i][2 * j], v1 = yv[i][2 * j + 1];
            const float got = swap_odd_even(odd ? v0 : v1);
            unsigned w[NA];
            split_pair<MATH>(odd ? got : v0, odd ? v1 : got, w);
#pragma unroll
            for (int q = 0; q < NA; ++q) *reinterpret_cast<unsigned*>(yb + rw * ROW + q * 64) = w[q];
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
          }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // ---- 5. second product over this pass's 256 values of K2
      if constexpr (!EARLY_B2) preload_b2(ps);
      if (active2) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int sl = c * 2 + h;
            bf16x8 f[MT2][NA];
#pragma unroll
            for (int i = 0; i < MT2; ++i)
#pragma unroll
              for (int q = 0; q < NA; ++q)
                f[i][q] = *reinterpret_cast<const bf16x8*>(ypatch + c * CBUF + a_off +
                                                           (rb + i) * 32 * ROW + q * 64 + h * 32);
#pragma unroll
            for (int q = 0; q < NP; ++q)
#pragma unroll
              for (int i = 0; i < MT2; ++i)
                acc2[i] = plane_mfma<MATH>(f[i][PL::PA[q]], fb[sl % AHEAD][PL::PB[q]], acc2[i]);
            if (sl + AHEAD < 16) load_b2(fb[sl % AHEAD], ps * 16 + sl + AHEAD);
            if constexpr (FENCE_SLABS) __builtin_amdgcn_sched_barrier(0);
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- 6. what the next pass / tile needs first in front of this pass's stores, y -> side_out
      {
        const int y_voff = (int)((((long)(m0 + 4 * half)) * p.lda + ps * 256 + wave * 32 + l31) * 4);
        if constexpr (NPASS > 1) preload_b1((ps + 1) % NPASS);   // (the last pass: the next tile's first)
        if constexpr (EARLY_B2) preload_b2((ps + 1) % NPASS);
        if (ps + 1 < NPASS) load_skip(round, ps + 1);
        else load_skip(round + 1, 0);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rw = i * 32 + (r & 3) + 8 * (r >> 2);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv[i][r]), rsrc_y,
                                                  rw < rows_left ? y_voff : BUF_OOB, rw * p.lda * 4, 0);
            if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
          }
      }
      if (ps + 1 < NPASS) {   // Y is written again: every wave has read it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- the finished 64 x N2 tile: statistics of the raw sums, then the stores
    if (active2) {
      const int r0 = m0 + rb * 32;
      if (p.bn.acc != nullptr) {
        wave_bn_tile<MT2, 1>(reinterpret_cast<const f32x16(&)[MT2][1]>(acc2), wbn, p.bn.acc, cb * 32,
                             p.N, p.M - r0, half, l31, PL::POST);
      } else if (p.stat_partial != nullptr) {
#pragma unroll
        for (int i = 0; i < MT2; ++i)
          wave_stats_block<1>(reinterpret_cast<const f32x16(&)[1]>(acc2[i]), p.stat_partial,
                              r0 / 32 + i, p.M - (r0 + i * 32), cb * 32, p.N, half, l31, PL::POST);
      }
      const int rows_left2 = p.M - (r0 + 4 * half);
      const int e_voff = (int)((((long)(r0 + 4 * half)) * p.ldc + cb * 32 + l31) * 4);
#pragma unroll
      for (int i = 0; i < MT2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rw = i * 32 + (r & 3) + 8 * (r >> 2);
          const float v = fmaf(acc2[i][r], PL::POST, 0.f);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc_c,
                                                rw < rows_left2 ? e_voff : BUF_OOB, rw * p.ldc * 4, 0);
          if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
  }
  if (p.bn.acc != nullptr) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);
#endif
}

template <int NCC, int N2B, int SKIP, int MATH>
int launch_r3(const IgemmParams& p, const RegenParams& g, hipStream_t stream) {
  constexpr int smem_bytes = (NCC + 8) * 64 * Planes<MATH>::ROW + 3 * NCC * 32 * 4;
  if (smem_bytes > x3_lds_max()) {
    vlnce_set_error("conv_r3: %d bytes of LDS per workgroup, the device allows %d", smem_bytes, x3_lds_max());
    return 1;
  }
  auto kern = conv_r3_kernel<NCC, N2B, SKIP, MATH>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes);
    if (e != hipSuccess) {
      vlnce_set_error("conv_r3: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return 2;
    }
    attr_set = true;
  }
  IgemmParams q = p;
  q.tiles_m = ceil_div(p.M, 64);
  q.tiles_n = 1;
  q.splitk = 1;
  long grid = q.tiles_m;
  if (grid > x3_cus()) grid = x3_cus();
  if (const int cap = vlnce_opt(VLNCE_OPT_S3_WGS); cap > 0 && grid > cap) grid = cap;   // option "s3_wgs" (tests)
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), smem_bytes, stream, q, g);
  VLNCE_CHECK_LAUNCH("conv_r3");
  return 0;
}

template <int NCC, int N2B, int MATH>
int launch_r3_skip(const IgemmParams& p, const RegenParams& g, hipStream_t stream) {
  return p.in2_scale != nullptr ? launch_r3<NCC, N2B, 2, MATH>(p, g, stream)
                                : launch_r3<NCC, N2B, 1, MATH>(p, g, stream);
}

template <int MATH>
int r3_launch_(const IgemmParams& p, const RegenParams& g, hipStream_t stream) {
  if (g.K1 == 64 && p.N == 64) return launch_r3_skip<2, 2, MATH>(p, g, stream);
  if (g.K1 == 64 && p.N == 128) return launch_r3_skip<2, 4, MATH>(p, g, stream);
  if (g.K1 == 128 && p.N == 128) return launch_r3_skip<4, 4, MATH>(p, g, stream);
  if (g.K1 == 128 && p.N == 256) return launch_r3_skip<4, 8, MATH>(p, g, stream);
  vlnce_set_error("conv_r3: no instance for %d -> %d -> %d channels", g.K1, p.K, p.N);
  return 1;
}

}  // namespace

// The caller (vlnce_conv2d_fwd) has tested what the kernel assumes: a stride-1 1x1 launch with
// K = 4 K1, both weight images, bn3's vectors, the skip and side_out, 16-byte aligned operands
// below 2 GiB, and a raw output (statistics or nothing in the epilogue).
int r3_launch(const IgemmParams& p, const RegenParams& g, hipStream_t stream) {
  note_conv_kernel(VLNCE_CONV_KERNEL(VLNCE_CONV_PATH_P3, p.math, VLNCE_CONV_KERNEL_R3, g.K1, p.N / 32,
                                     p.in2_scale != nullptr ? 2 : 1));
  return p.math == MATH_F16X3 ? r3_launch_<MATH_F16X3>(p, g, stream)
                              : r3_launch_<MATH_BF16X6>(p, g, stream);
}

}  // namespace vlnce_detail
