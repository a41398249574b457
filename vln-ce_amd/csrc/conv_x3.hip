// conv_x3_kernel: the hot convolution path (channels-last, Cin % 32 == 0, [N,K] weights) -- the
// 1x1 / strided convolutions of the frozen trunks that the router in conv_p3.hip (conv_p3_kernel /
// conv_u3_kernel / conv_s3_kernel, a file each) does not take.  One launcher for the router in
// igemm.hip: x3_try_launch (igemm_shared.h).
//
// fp32 convolution on the bf16 matrix pipe.  gfx950 has no fp32-rate matrix instruction beyond
// v_mfma_f32_32x32x2_f32 (157 TF/s, = the vector rate); v_mfma_f32_32x32x16_bf16 is 16x faster.
// Every fp32 operand is split EXACTLY into three bf16 planes (round to nearest at each step),
//     x = x1 + x2 + x3   (8 + 8 + 8 mantissa bits, same exponent range as fp32),
// and a product a*b is the six plane products of order <= 2^-16,
//     a1 b1 + (a1 b2 + a2 b1) + (a2 b2 + a1 b3 + a3 b1),
// each exact in the fp32 accumulator; the dropped terms are <= 2^-26 relative.  Round 2 split by
// TRUNCATION (dropped terms 2^-24): measured against fp64 that was rms 3.4-5.0e-7 on the 3x3
// layers = 1.1-1.2x the fp32-MFMA kernel (igemm.hip) and 2-3x torch's own fp32 convolution (1.6-1.7e-7;
// profiles/archive/r02_o_conv_accuracy_*.txt) -- fp32-class, NOT equal to it as round 2's text claimed.
// With the round-to-nearest split: profiles/archive/r03_*_conv_accuracy*.txt.  Six
// bf16 MFMAs of 32 cycles replace eight fp32 MFMAs of 64 cycles per 32x32x16 block: 2.7x less
// matrix-pipe time.
//
// What the fp32-MFMA kernel taught (profiles/archive/r02_c_*): with every wave doing "load, transform,
// write LDS, barrier, read fragments, MFMA", the matrix pipe idles while the wave does anything
// else, and the co-resident workgroup runs in lock-step, so nothing covers it.  Here the roles
// are split.  A workgroup is 16 waves, four per SIMD, one workgroup per CU:
//   * waves 8-15, the PRODUCERS (two per SIMD: one wave alone issues one instruction per ~4
//     cycles, not enough for ~400 instructions per K-tile): buffer-load the A (im2col) and B
//     (weight) K-tiles into a register ring several tiles ahead, apply the operand prologue
//     (previous layer's BatchNorm + ReLU, the dual-input block end, zero padding after it),
//     split to bf16 planes and write them to LDS;
//   * waves 0-7, the MATRIX waves (two per SIMD, taking turns on the matrix pipe: while one
//     waits for LDS or a counter the other issues): ds_read_b128 fragments, MFMAs, and the
//     epilogue of their 64x32 sub-tile straight from the accumulator registers.
// The SIMD's matrix pipe (matrix wave) and its VALU / memory pipes (producer waves) run side by
// side by hardware arbitration, not by compiler scheduling.
// LDS: two stages of {A, B} x 3 planes x rows x 80 bytes (32 bf16 + 16 bytes pad: the
// ds_read_b128 fragment reads are conflict-free).  The hand-over is two LDS counters instead of
// s_barrier (measured: a barrier per K-tile costs the matrix pipe ~200 idle cycles of skew):
// per stage, `full` counts its writes (8 per K-tile), `empty` the matrix waves done reading it
// (8 per K-tile); whoever is ahead never waits.  The LDS unit executes one wave's operations in
// order, so "data writes, then counter add" needs no wait in between.
// A workgroup walks a strided list of output tiles; the K-tile stream (and the producers'
// register ring) runs across tile boundaries, so the prologue of a tile (addresses, first loads)
// and its epilogue are covered by the neighbours' MFMAs.
#include "igemm_shared.h"

namespace vlnce_detail {

namespace {

constexpr int X3_PITCH = 80;      // bytes per LDS row of one plane
constexpr int X3_PRODUCERS = 8;  // producer waves; the matrix waves are WM x WN = 8 (or 4)

template <int ROWS, int DUAL>
struct X3Staged {
  f32x4 a[ROWS];
  f32x4 a2[DUAL ? ROWS : 1];
  unsigned ok;
  int m0;
};

// x (4 consecutive k of one row) -> the three planes' 8-byte LDS words.  Round-to-nearest split
// (v_cvt_pk_bf16_f32): x = x1 + x2 + x3 exactly, |x2| <= 2^-9 |x|, |x3| <= 2^-18 |x|, so the three
// dropped cross terms are <= 2^-26 relative (truncation, rounds 2: 2^-24); same instruction count.
// (MATH_F16X3: two fp16 A planes, see Planes<> in igemm_shared.h)
template <int MATH>
__device__ __forceinline__ void x3_split_store(f32x4 x, char* row_ptr, int plane_bytes) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  constexpr int NA = Planes<MATH>::NA;
  unsigned w0[NA], w1[NA];
  split_pair<MATH>(x[0], x[1], w0);
  split_pair<MATH>(x[2], x[3], w1);
#pragma unroll
  for (int q = 0; q < NA; ++q) *reinterpret_cast<u32x2*>(row_ptr + q * plane_bytes) = u32x2{w0[q], w1[q]};
}

template <int BM, int BN, int WM, int WN, int DUAL, int MATH>
__global__ __launch_bounds__((WM * WN + X3_PRODUCERS) * 64) void conv_x3_kernel(IgemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Planes<MATH> PL;
  constexpr int NA = PL::NA;
  constexpr int X3_MATRIX = WM * WN;  // matrix waves (8: two per SIMD take turns on the pipe)
  constexpr int WTM = BM / WM, WTN = BN / WN, MT = WTM / 32, NT = WTN / 32;
  constexpr int A_PLANE = BM * X3_PITCH, B_PLANE = BN * X3_PITCH;
  constexpr int A_BYTES = NA * A_PLANE, B_BYTES = 3 * B_PLANE;
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int PR = X3_PRODUCERS * 64 / 8;          // rows per producer pass (8 float4 each)
  constexpr int A_ROWS = BM / PR;                    // producer passes over the A tile
  static_assert(MT >= 1 && NT >= 1 && A_ROWS >= 1 && BN <= X3_PRODUCERS * 16, "tile");

  extern __shared__ __attribute__((aligned(16))) char xsm[];
  // counters per STAGE: waves are at most one K-tile apart, so a single running count could be
  // reached by fast waves' next-K-tile adds while a slow wave's are missing; a stage's count
  // cannot (its next use waits for everybody's current one)
  int* const full = reinterpret_cast<int*>(xsm + 2 * STAGE_BYTES);  // [2]
  int* const empty = full + 2;                                       // [2]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int KT = p.K / BK;

  // ---- this workgroup's tiles: virtual block ids blockIdx.x + r * gridDim.x through the
  // XCD-aware map of igemm_kernel (gridDim.x is a multiple of 8 or the whole tile count)
  const int ntiles = p.tiles_m * p.tiles_n;
  const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int G_total = my_tiles * KT;  // K-tiles this workgroup streams
  auto tile_of = [&](int round, int& m0, int& n0) {
    const int v = blockIdx.x + round * gridDim.x;
    const int q = ntiles >> 3, r = ntiles & 7, xcd = v & 7, idx = v >> 3;
    const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int tm = tile / p.tiles_n;
    m0 = tm * BM;
    n0 = (tile - tm * p.tiles_n) * BN;
  };

  if (tid < 4) full[tid] = 0;
  __syncthreads();

  if (wave >= X3_MATRIX) {
    // ================================================================ producer waves
    const int ptid = tid - X3_MATRIX * 64;
    const int lrow = ptid >> 3;
    const int lk4 = (ptid & 7) * 4;
    const long bias = ((long)p.pad * p.W + p.pad) * p.lda * 4;  // keeps voffsets non-negative
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.A)) - bias, 0, (int)(p.a_bytes + bias),
        0x00020000);
    __amdgpu_buffer_rsrc_t rsrc_a2 = rsrc_a;
    if constexpr (DUAL)
      rsrc_a2 = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(reinterpret_cast<const char*>(p.A2)) - bias, 0,
          (int)(p.a_bytes + bias), 0x00020000);
    // B comes pre-split (vlnce_conv2d_split_weights): three planes of N*K bf16, row n = K
    // contiguous; thread -> (row ptid / 4, 16-byte chunk ptid % 4 of the K-tile's 64 bytes)
    const int plane_b = (int)(p.b_bytes >> 1);  // bytes of one plane
    const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.Bsplit)), 0, 3 * plane_b, 0x00020000);
    const int brow = ptid >> 2, bchunk = ptid & 3;
    const bool has_pro = p.in_scale != nullptr;
    const bool pad_matters = p.pad > 0;
    const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();  // max(x, -inf) = x
    const int HoWo = p.Ho * p.Wo;

    // ---- load cursor: the tile whose K-tiles are being fetched
    int a_voff[A_ROWS], b_voff;
    unsigned a_taps[A_ROWS];  // bit t: filter tap t of this output pixel reads inside the image
    int l_round = 0, l_m0 = 0, l_n0 = 0, l_kt = 0;
    int u_r = 0, u_q = 0, u_ci = 0, u_k = 0;  // wave-uniform (tap, channel, k) of the next fetch
    auto setup_tile = [&](int round) {
      int m0, n0;
      tile_of(round, m0, n0);
      l_m0 = m0;
      l_n0 = n0;
#pragma unroll
      for (int i = 0; i < A_ROWS; ++i) {
        const int m = m0 + i * PR + lrow;
        a_voff[i] = BUF_OOB;
        a_taps[i] = 0;
        if (m < p.M) {
          const int img = m / HoWo;
          const int rem = m - img * HoWo;
          const int ho = rem / p.Wo;
          const int wo = rem - ho * p.Wo;
          const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
          a_voff[i] =
              (int)((((long)(img * p.H + hi0 + p.pad) * p.W + wi0 + p.pad) * p.lda + lk4) * 4);
          unsigned mask = 0;
          for (int r = 0; r < p.KH; ++r)
            for (int q = 0; q < p.KW; ++q)
              if ((unsigned)(hi0 + r) < (unsigned)p.H && (unsigned)(wi0 + q) < (unsigned)p.W)
                mask |= 1u << (r * p.KW + q);
          a_taps[i] = mask;
        }
      }
      b_voff = (brow < BN && n0 + brow < p.N) ? ((n0 + brow) * p.ldb + bchunk * 8) * 2 : BUF_OOB;
      u_r = u_q = u_ci = u_k = 0;
    };

    // Register ring of NSET staged K-tiles: NSET-1 tiles of loads are in flight while one is
    // transformed and written to LDS (8 producer waves per CU: 1 K-tile each = 8 in flight).  Loads past the last K-tile are issued out of range (the
    // hardware returns zeros, no traffic).
    constexpr int NSET = 2;  // (3 measured 1-4 % slower: the registers it costs spill)
    typedef X3Staged<A_ROWS, DUAL> Staged;
    Staged st[NSET];
    u32x4 sb[NSET][3];
    // The prologue vectors of a K-tile (its 32 input channels) are not part of the ring: one copy,
    // fetched right after the previous K-tile was written (they are L1/L2 hits: every row of
    // every workgroup reads the same few KB), a K-tile time before they are used.
    f32x4 ps = {0.f, 0.f, 0.f, 0.f}, pt = ps, pc = ps, p2s = {1.f, 1.f, 1.f, 1.f}, pt2 = ps, p2c = ps;
    int s_ci = 0;  // first input channel of the K-tile to be written next
    auto load_vec = [&]() {
      if (has_pro) {
        ps = ldg4(p.in_scale + s_ci + lk4);
        pt = ldg4(p.in_shift + s_ci + lk4);
        if (p.in_center) pc = ldg4(p.in_center + s_ci + lk4);
        if constexpr (DUAL) {
          if (p.in2_scale != nullptr) {
            p2s = ldg4(p.in2_scale + s_ci + lk4);
            pt2 = pt + ldg4(p.in2_shift + s_ci + lk4);
            if (p.in2_center) p2c = ldg4(p.in2_center + s_ci + lk4);
          }
        }
      }
    };

    auto load = [&](Staged& s, u32x4 (&b)[3], bool live) {
      const int tap = u_r * p.KW + u_q;
      const int soff = ((u_r * p.W + u_q) * p.lda + u_ci) * 4;
      if constexpr (DUAL) s.m0 = l_n0 == 0 ? l_m0 : -1;  // side_out rows, or -1: not this tile's job
      s.ok = 0;
#pragma unroll
      for (int i = 0; i < A_ROWS; ++i) {
        const unsigned ok = live ? ((a_taps[i] >> tap) & 1u) : 0u;
        s.ok |= ok << i;
        s.a[i] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, ok ? a_voff[i] : BUF_OOB, soff, 0));
        if constexpr (DUAL)
          s.a2[i] = __builtin_bit_cast(
              f32x4,
              __builtin_amdgcn_raw_buffer_load_b128(rsrc_a2, ok ? a_voff[i] : BUF_OOB, soff, 0));
      }
#pragma unroll
      for (int q = 0; q < 3; ++q)
        b[q] = __builtin_amdgcn_raw_buffer_load_b128(
            rsrc_b, (live && b_voff != BUF_OOB) ? b_voff + q * plane_b : BUF_OOB, u_k * 2, 0);
      // advance the cursor by one K-tile; past the tile's last one, move to the next tile
      u_k += BK;
      u_ci += BK;
      if (u_ci >= p.Cin) {
        u_ci = 0;
        if (++u_q == p.KW) {
          u_q = 0;
          ++u_r;
        }
      }
      if (++l_kt == KT) {
        l_kt = 0;
        if (++l_round < my_tiles) setup_tile(l_round);
      }
    };

    auto stash = [&](const Staged& s, const u32x4 (&b)[3], char* stage) {
      char* arow = stage + lrow * X3_PITCH + lk4 * 2;
#pragma unroll
      for (int i = 0; i < A_ROWS; ++i) {
        f32x4 v = s.a[i];
        if (has_pro) {
          // (scalar fma / max per element: packed fp32 VALU beside MFMAs costs more issue time
          // than the two plain instructions it replaces -- MI355X_MICROARCH.md)
          if constexpr (DUAL) {
            if (p.in2_scale != nullptr) {  // downsample branch: its own BatchNorm (pt2 = pt + p2t)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                v[e] = fmaxf(fmaf(v[e] - pc[e], ps[e], fmaf(s.a2[i][e] - p2c[e], p2s[e], pt2[e])),
                             relu_floor);
            } else {  // identity skip: added as is
#pragma unroll
              for (int e = 0; e < 4; ++e)
                v[e] = fmaxf(fmaf(v[e] - pc[e], ps[e], pt[e]) + s.a2[i][e], relu_floor);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(v[e] - pc[e], ps[e], pt[e]), relu_floor);
          }
          // zero padding comes AFTER the transform (rows past M are never stored or counted)
          if (pad_matters && !((s.ok >> i) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
          if constexpr (DUAL) {
            // the materialised block output: written once, by the workgroups of n-tile 0
            // (1x1 convolution: every tile of one tile_m row has the same rows)
            if (p.side_out != nullptr && s.m0 >= 0 && ((s.ok >> i) & 1u))
              *reinterpret_cast<f32x4*>(p.side_out + (long)(s.m0 + i * PR + lrow) * p.lda + s_ci +
                                        lk4) = v;
          }
        }
        x3_split_store<MATH>(v, arow + i * PR * X3_PITCH, A_PLANE);
      }
      if (brow < BN) {
        char* bdst = stage + A_BYTES + brow * X3_PITCH + bchunk * 16;
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(bdst + q * B_PLANE) = b[q];
      }
    };

    // K-tile g of the stream goes to stage g & 1 once the matrix waves are done with K-tile
    // g - 2; iteration g: issue the loads of K-tile g + NSET - 1, write K-tile g
    DBG_T(long long d_pl = 0, d_pw = 0, d_pm = 0, d_ps = 0; const long long d_p0 = clock64();)
    setup_tile(0);
    load_vec();
#pragma unroll
    for (int j = 0; j < NSET - 1; ++j) load(st[j], sb[j], j < G_total);
    for (int g0 = 0; g0 < G_total; g0 += NSET) {
#pragma unroll
      for (int j = 0; j < NSET; ++j) {
        const int g = g0 + j;
        if (g < G_total) {
          DBG_T(const long long d_0 = clock64();)
          const int seen = x3_peek(empty + (g & 1));
          load(st[(j + NSET - 1) % NSET], sb[(j + NSET - 1) % NSET], g + NSET - 1 < G_total);
          DBG_T(const long long d_1 = clock64();)
          x3_wait(empty + (g & 1), seen, X3_MATRIX * (g >> 1));  // K-tile g-2 has been read
          DBG_T(const long long d_2 = clock64();
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSET - 1) * (A_ROWS * (1 + DUAL) + 3)) : "memory");
                const long long d_3 = clock64();)
          stash(st[j], sb[j], xsm + (g & 1) * STAGE_BYTES);
          if (lane == 0) x3_signal(full + (g & 1));  // (in LDS order behind this wave's stage writes)
          s_ci += BK;
          if (s_ci >= p.Cin) s_ci = 0;
          if (g + 1 < G_total) load_vec();
          DBG_T(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const long long d_4 = clock64();
                d_pl += d_1 - d_0; d_pw += d_2 - d_1; d_pm += d_3 - d_2; d_ps += d_4 - d_3;)
        }
      }
    }
#ifdef VLNCE_DBG_TIME
    if (blockIdx.x == 8 && (tid == X3_MATRIX * 64 || tid == X3_MATRIX * 64 + 448))
      printf("x3 producer wave %d: total %lld: issue loads %lld, wait for matrix waves %lld, wait for "
             "data %lld, transform+write %lld\n", wave, (long long)(clock64() - d_p0), d_pl, d_pw, d_pm, d_ps);
#endif
  } else {
    // ================================================================ matrix waves
    const int wm = wave / WN, wn = wave % WN;
    struct Frag {
      bf16x8 a[MT][NA];
      bf16x8 b[NT][3];
    };
    const char* abase = xsm + (wm * WTM + l31) * X3_PITCH + half * 16;
    const char* bbase = xsm + A_BYTES + (wn * WTN + l31) * X3_PITCH + half * 16;
    auto read = [&](Frag& f, int stage, int slab) {
      const int off = stage * STAGE_BYTES + slab * 32;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < NA; ++q)
          f.a[i][q] = *reinterpret_cast<const bf16x8*>(abase + off + q * A_PLANE + i * 32 * X3_PITCH);
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          f.b[j][q] = *reinterpret_cast<const bf16x8*>(bbase + off + q * B_PLANE + j * 32 * X3_PITCH);
    };
    f32x16 acc[MT][NT];
    auto mma = [&](const Frag& f) {
#pragma unroll
      for (int q = 0; q < PL::NP; ++q)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = plane_mfma<MATH>(f.a[i][PL::PA[q]], f.b[j][PL::PB[q]], acc[i][j]);
    };
    const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(p.C), 0, (int)p.c_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.residual ? p.residual : p.C)), 0,
        (int)p.c_bytes, 0x00020000);   // (ldr == ldc: the output's extent)

    DBG_T(const long long d_c0 = clock64(), d_w0 = wall_clock64(); long long d_wait = 0;)
    Frag fa, fb;
    WaveBn<NT> wbn;   // BatchNorm finished in this launch (p.bn): the wave's running column sums
    wave_bn_reset(wbn);
    // the SIMD's VALU issue port is shared with the producer waves: the MFMAs must win it the
    // moment the matrix pipe frees up, the producers take the slots in between
    __builtin_amdgcn_s_setprio(3);
    x3_wait(full, x3_peek(full), X3_PRODUCERS);  // K-tile 0 is written (stage 0's first)
    read(fa, 0, 0);
    int g = 0;
    DBG_T(const long long d_c1 = clock64();)
    for (int round = 0; round < my_tiles; ++round) {
      int m0, n0;
      tile_of(round, m0, n0);
      // epilogue vectors of this wave's columns (loaded now, used after the K loop)
      float e_sc[NT], e_sh[NT];
      int e_voff[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * WTN + j * 32 + l31;
        const bool ok = col < p.N;
        e_sc[j] = ((ok && p.scale) ? p.scale[col] : 1.f) * PL::POST;
        e_sh[j] = (ok && p.shift) ? p.shift[col] : 0.f;
        e_voff[j] = ok ? (int)((((long)(m0 + wm * WTM + 4 * half)) * p.ldc + col) * 4) : BUF_OOB;
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

      for (int t = 0; t < KT; ++t, ++g) {
        // (the scheduling fences keep the LDS reads of the NEXT slab in front of the current
        // slab's MFMAs; left alone the compiler sinks them behind and the pipe waits on LDS)
        const int seen = x3_peek(full + ((g + 1) & 1));
        read(fb, g & 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(fa);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 1 < G_total) {
          DBG_T(const long long d_a = clock64();)
          x3_wait(full + ((g + 1) & 1), seen, X3_PRODUCERS * (((g + 1) >> 1) + 1));  // K-tile g+1 is written
          DBG_T(d_wait += clock64() - d_a;)
          read(fa, (g + 1) & 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // this wave's reads of K-tile g are complete once fb has arrived (LDS returns in order)
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NA * MT + 3 * NT) : "memory");
        if (lane == 0) x3_signal(empty + (g & 1));
        __builtin_amdgcn_sched_barrier(0);
        mma(fb);
        __builtin_amdgcn_sched_barrier(0);
      }

      // -------------------------------------------------------------- statistics
      if (p.bn.acc != nullptr) {
        wave_bn_tile<MT, NT>(acc, wbn, p.bn.acc, n0 + wn * WTN, p.N, p.M - (m0 + wm * WTM), half, l31,
                             PL::POST);
        if (round == my_tiles - 1) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);  // in front of the stores
      } else if (p.stat_partial != nullptr) {
        const int tile_m = m0 / BM;
        if (p.stat_rows == 32 && MT > 1) {
          // one partial per 32x32 MFMA block row: exactly the 16 accumulator registers of a lane
#pragma unroll
          for (int i = 0; i < MT; ++i)
            wave_stats_block<NT>(acc[i], p.stat_partial, (m0 + wm * WTM) / 32 + i,
                                 p.M - (m0 + wm * WTM + i * 32), n0 + wn * WTN, p.N, half, l31,
                                 PL::POST);
        } else if (p.stat_rows > 0 && p.stat_rows < WTM)
          wave_stats_fine<MT, NT>(acc, p.stat_partial, p.stat_rows, m0 + wm * WTM, p.M,
                                  n0 + wn * WTN, p.N, half, l31, PL::POST);
        else
          wave_stats<MT, NT>(acc, p.stat_partial, tile_m * WM + wm, p.M - (m0 + wm * WTM), WTM,
                             n0 + wn * WTN, p.N, half, l31, PL::POST);
      }
      // -------------------------------------------------------------- epilogue from registers
      // one store = 2 rows x 32 columns = two full 128-byte lines; rows past M fall outside
      // the buffer (the row bound is folded into the descriptor's extent) only for the last
      // tile row, where the lane offset is sent out of range instead
      const int rows_left = p.M - (m0 + wm * WTM + 4 * half);
      wave_epilogue<MT, NT>(acc, e_sc, e_sh, e_voff, rows_left, p.ldc, p.act, p.residual != nullptr,
                            rsrc_c, rsrc_r, false);
    }
    __builtin_amdgcn_s_setprio(0);
#ifdef VLNCE_DBG_TIME
    if (blockIdx.x == 8 && tid == 0) {
      const long long c = clock64() - d_c0, w = wall_clock64() - d_w0;
      printf("x3 tiles %d KT %d: first K-tile after %lld cycles; total %lld cycles = %lld ticks of 100 MHz "
             "(%.2f GHz); waiting for producers %lld\n", my_tiles, KT, d_c1 - d_c0, c, w,
             (double)c / (double)w * 0.1, d_wait);
    }
#endif
  }
#endif
}

// conv_x3_kernel launch: one workgroup (16 or 12 waves) per CU, walking tiles
template <int BM, int BN, int WM, int WN, int DUAL, int MATH>
int launch_x3(const IgemmParams& p, hipStream_t stream) {
  constexpr int smem_bytes = 2 * (Planes<MATH>::NA * BM + 3 * BN) * X3_PITCH + 16;  // two stages + 4 counters
  constexpr int threads = (WM * WN + X3_PRODUCERS) * 64;
  auto kern = conv_x3_kernel<BM, BN, WM, WN, DUAL, MATH>;
  static bool attr_set = false;  // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes);
    if (e != hipSuccess) {
      vlnce_set_error("conv_x3: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return 2;
    }
    attr_set = true;
  }
  IgemmParams q = p;
  q.tiles_m = ceil_div(p.M, BM);
  q.tiles_n = ceil_div(p.N, BN);
  q.splitk = 1;
  const long nwg = (long)q.tiles_m * q.tiles_n;
  if (nwg <= 0 || nwg > 0x7fffffffL) {
    vlnce_set_error("conv_x3: bad grid %ld", nwg);
    return 1;
  }
  // one workgroup per CU walks tiles a grid apart (a multiple of 8: the XCD of a tile is fixed)
  const int cus = x3_cus();
  const unsigned grid = nwg <= cus ? (unsigned)nwg : (unsigned)cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), smem_bytes, stream, q);
  VLNCE_CHECK_LAUNCH("conv_x3");
  return 0;
}

// what conv_x3_kernel covers: the buffer-descriptor hot path (buf_ok) with whole 32-channel
// K-tiles and a plain epilogue (scale / shift / activation, statistics).  Tile: the largest of
// 128x128, 64x128, 128x64, 64x64 that keeps >= 80 % of the CUs busy over the rounds a workgroup
// per CU needs (tiles / (rounds * CUs)).
struct X3Plan {
  int bm, bn;
};
bool x3_plan(const IgemmParams& p, X3Plan* out) {
  if (!conv_math() || !p.Bsplit || !buf_ok(p) || p.splitk > 1) return false;
  if (p.accumulate || p.c_bytes >= 0x7fffffffL) return false;
  if (p.residual && (p.ldr != p.ldc || p.stat_partial || p.bn.acc)) return false;  // (register epilogue)
  const int force = vlnce_opt(VLNCE_OPT_X3_TILE);  // tuning
  const X3Plan cand[4] = {{128, 128}, {64, 128}, {128, 64}, {64, 64}};
  if (force >= 1 && force <= 4) {
    *out = cand[force - 1];
    return true;
  }
  const int cus = x3_cus();
  double best = 0.0;
  for (const X3Plan& c : cand) {
    if (c.bn == 128 && p.N <= 64) continue;
    const long tiles = (long)ceil_div(p.M, c.bm) * ceil_div(p.N, c.bn);
    const long rounds = (tiles + cus - 1) / cus;
    const double eff = (double)tiles / (double)(rounds * cus);
    if (eff >= 0.8) {
      *out = c;
      return true;
    }
    if (eff > best) {
      best = eff;
      *out = c;
    }
  }
  return best >= 0.4;  // below that the problem is a handful of tiles: split-K / small-tile path
}
template <int DUAL, int MATH>
int dispatch_x3_(const IgemmParams& p, const X3Plan& t, hipStream_t s) {
  const int tile = t.bm == 128 ? (t.bn == 128 ? 1 : 3) : (t.bn == 128 ? 2 : 4);
  note_conv_kernel(VLNCE_CONV_KERNEL(VLNCE_CONV_PATH_X3, MATH, 0, tile, DUAL, 0));
  if (t.bm == 128 && t.bn == 128) return launch_x3<128, 128, 2, 4, DUAL, MATH>(p, s);
  if (t.bm == 64 && t.bn == 128) return launch_x3<64, 128, 2, 4, DUAL, MATH>(p, s);
  if (t.bm == 128 && t.bn == 64) return launch_x3<128, 64, 4, 2, DUAL, MATH>(p, s);
  return launch_x3<64, 64, 2, 2, DUAL, MATH>(p, s);
}
template <int DUAL>
int dispatch_x3(const IgemmParams& p, const X3Plan& t, hipStream_t s) {
  return p.math == MATH_F16X3 ? dispatch_x3_<DUAL, MATH_F16X3>(p, t, s)
                              : dispatch_x3_<DUAL, MATH_BF16X6>(p, t, s);
}

}  // namespace

int x3_try_launch(const IgemmParams& p, bool dual, hipStream_t stream) {
  X3Plan t;
  if (!x3_plan(p, &t)) return -1;
  return dual ? dispatch_x3<1>(p, t, stream) : dispatch_x3<0>(p, t, stream);
}

}  // namespace vlnce_detail
