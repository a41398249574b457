// conv_p3_kernel: fp32 convolution on the bf16 matrix pipe with a PATCH-RESIDENT A operand.
//
// Same arithmetic as conv_x3_kernel (conv_x3.hip): every fp32 operand is split exactly into three
// bf16 planes and a product is the six plane products of order <= 2^-16 on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- here with a round-to-nearest split
// (v_cvt_pk_bf16_f32), so the dropped cross terms are <= 2^-26 relative.
//
// What round 2's PMC passes showed for conv_x3_kernel: the matrix waves wait for the producer
// waves about half the time, because the operand transform (previous layer's BatchNorm + ReLU,
// zero padding, three-way split, LDS writes: ~40 VALU instructions per float4) is redone for
// every filter tap (9x for a 3x3 convolution) and for every N-tile, and it shares the SIMD's issue
// port with the MFMAs.  This kernel removes both redundancies and the B operand's LDS round trip:
//   * A: the workgroup owns BM consecutive output pixels.  For a stride-1 convolution their
//     receptive field is ONE contiguous range of the zero-padded input in padded-linear pixel
//     order u = (img * Hp + hp) * Wp + wp:  tap (r, q) of output pixel m reads u0(m) + r * Wp + q.
//     Per 32-channel chunk the producers transform that range ONCE into an LDS patch
//     (rows = padded pixels incl. the zero halo, 208 bytes = 3 planes x 32 bf16 + 16 pad), and
//     the matrix waves read their A fragments for every tap from it with a wave-uniform row
//     offset -- implicit im2col out of LDS: 2.1x instead of 9x transformed elements at 64x64,
//     1.4x at 16x16.  1x1 convolutions (any stride) are the degenerate case: patch row = output
//     pixel (GATHER mode).
//   * B: the weights are pre-packed once per parameter version into MFMA fragment order
//     (vlnce_conv2d_pack_weights: [n-block][k-slab][plane][lane][8 bf16], k ordered
//     chunk-major / tap / 16-slab to match the loop here), so a matrix wave fetches a B fragment
//     with one fully coalesced 1 KB buffer_load_dwordx4 straight into registers, one slab
//     ahead -- no LDS bytes, no producer work, no hand-over for B.  The weight set of a layer
//     lives in L2 / MALL.
//   * wide tiles (BN up to 256) where the layer has the channels: the transform per MFMA halves
//     again for the 1x1 convolutions.
// A workgroup is 8 matrix waves (two per SIMD taking turns on the matrix pipe) + 4 producer waves
// (one per SIMD), 168 VGPRs each, one workgroup per CU, persistent over a strided tile list; the
// hand-over is per patch buffer (two of them) through LDS counters as in conv_x3_kernel.
// This file also holds the weight packer and the router p3_try_launch, which hands the 1x1 layers
// it finds eligible to conv_u3_kernel (conv_u3.hip) and conv_s3_kernel (conv_s3.hip).
#include "igemm_shared.h"

using namespace vlnce_detail;

namespace vlnce_detail {
namespace {

// bytes per patch row: Planes<MATH>::ROW (208 = 13 x 16 B / 144 = 9 x 16 B: consecutive rows are
// conflict-free for ds_read_b128)
constexpr int P3_PRODUCERS = 4;  // producer waves
// patch rows the KxK producers address: 12 row groups of 32 (3 items of 128), their byte offsets in
// twelve registers.  (Round 6, measured and dropped: with the 144-byte rows of the fp16 planes the LDS
// would hold 568 rows, i.e. 256-row tiles on 64x64 maps -- but 16 offsets in registers pushed the
// workgroup's register allocation (the maximum over both roles) over the edge, the MATRIX waves'
// k-loop reloaded two spilled values per 24 MFMAs behind an s_waitcnt vmcnt(0), and every 3x3
// layer ran 1.5-2.7x slower: profiles/r6_06; the offsets in LDS instead, read back with one
// ds_read_b128 per item, left 120 spilled registers: profiles/r6_07; sixteen offsets only in the
// instantiations whose matrix waves hold <= 2 accumulator blocks made exactly those instantiations
// 1.9-2.1x slower -- l1 3x3 100 -> 207 us, ResNet-18's 64-channel 3x3 at 416 frames 683 -> 1335 us --
// and left the others alone: profiles/r06_f_*.  The 64-channel 3x3 layers on 64x64 maps therefore
// stay on 128x64 tiles (one accumulator block per wave), 185-195 TF/s against 300-330 TF/s for the
// 128- to 512-channel layers.)
constexpr int P3_MAX_ROWS = 384;

enum { P3_GATHER = 0, P3_DENSE = 1 };

// Wait for an LDS counter of the hand-over.  Waits are between the waves of ONE workgroup, i.e.
// microseconds; a protocol bug must become a launch error, not a hung GPU: after ~0.2 s of
// spinning the wave traps.
__device__ __forceinline__ void p3_wait(const int* flag, int need) {
  int seen = x3_peek(flag);
  for (int spins = 0; seen < need; ++spins) {
    __builtin_amdgcn_s_sleep(1);
    seen = x3_peek(flag);
    if (spins > (1 << 22)) __builtin_trap();
  }
  asm volatile("" ::: "memory");
}

template <int BM, int BN, int WM, int WN, int DUAL, int MODE, int MATH>
__global__ __launch_bounds__((WM * WN + P3_PRODUCERS) * 64) void conv_p3_kernel(IgemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Planes<MATH> PL;
  constexpr int P3_ROW = PL::ROW, NA = PL::NA;
  constexpr int MATRIX = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN, MT = WTM / 32, NT = WTN / 32;
  static_assert(MT >= 1 && NT >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "tile");
  static_assert(!DUAL || MODE == P3_GATHER, "dual-input prologue: 1x1 convolutions only");

  // 1x1 convolutions have short reductions: their epilogue stores must not sit in front of any
  // load of the same wave (vmcnt counts stores too, in order), so there the matrix waves issue NO
  // vector loads: the producers bring a chunk's B fragments into LDS with LDS-DMA (fragment
  // order = lane order, 1 KB per instruction) next to the patch, under the same hand-over.  KxK
  // convolutions (long reductions, large patches) fetch B straight from L2 into registers.
  constexpr bool B_LDS = MODE == P3_GATHER;
  constexpr int BST = B_LDS ? BN * 192 : 0;   // bytes of one B stage: BN/32 n-blocks x 2 slabs x 3 KB
  extern __shared__ __attribute__((aligned(16))) char xsm[];
  const int pbuf = p.p3_rows * P3_ROW;                         // bytes of one patch buffer
  char* const bstage = xsm + 2 * pbuf;                         // [2][BST]
  int* const pfull = reinterpret_cast<int*>(bstage + 2 * BST);  // [2] producer waves done writing
  int* const pempty = pfull + 2;                               // [2] matrix waves done reading
  // KxK form: the prologue vectors [3][Cin] behind the counters (conv_u3_kernel's arrangement)
  float* const vlds = reinterpret_cast<float*>(pfull + 4);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int NC = p.Cin / 32;      // channel chunks
  const int T = p.KH * p.KW;      // filter taps
  const int HoWo = p.Ho * p.Wo;
  const int Hp = p.H + 2 * p.pad, Wp = p.W + 2 * p.pad;

  // ---- this workgroup's tiles: virtual block ids blockIdx.x + r * gridDim.x through the
  // XCD-aware map of igemm_kernel (gridDim.x is a multiple of 8 or the whole tile count)
  const int ntiles = p.tiles_m * p.tiles_n;
  const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  auto tile_of = [&](int round, int& m0, int& n0) {
    const int v = blockIdx.x + round * gridDim.x;
    const int q = ntiles >> 3, r = ntiles & 7, xcd = v & 7, idx = v >> 3;
    const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int tm = tile / p.tiles_n;
    m0 = tm * BM;
    n0 = (tile - tm * p.tiles_n) * BN;
  };
  // padded-linear index of output pixel m's tap (0, 0)
  auto u0_of = [&](int m) {
    const int img = m / HoWo;
    const int rem = m - img * HoWo;
    const int ho = rem / p.Wo;
    return (img * Hp + ho) * Wp + (rem - ho * p.Wo);
  };
  // rows of the patch of the tile at m0 (DENSE: padded pixels; GATHER: output pixels)
  auto patch_rows = [&](int m0) {
    const int mlast = min(m0 + BM, p.M) - 1;
    if constexpr (MODE == P3_DENSE) return u0_of(mlast) - u0_of(m0) + (p.KH - 1) * Wp + p.KW;
    return mlast - m0 + 1;
  };

  if (tid < 4) pfull[tid] = 0;
  if constexpr (MODE == P3_DENSE) {
    const bool pro = p.in_scale != nullptr;
    for (int ch = tid; ch < p.Cin; ch += (MATRIX + P3_PRODUCERS) * 64) {
      vlds[ch] = pro ? p.in_scale[ch] : 1.f;
      vlds[p.Cin + ch] = pro ? p.in_shift[ch] : 0.f;
      vlds[2 * p.Cin + ch] = (pro && p.in_center) ? p.in_center[ch] : 0.f;
    }
  }
  __syncthreads();

  if (wave >= MATRIX) {
    // ================================================================ producer waves
    // producer waves above the matrix waves: measured, a producer-bound layer (3x3 64->64 at
    // 64x64) runs 140 -> 119 us when the producers win the issue port
    constexpr int P3_PPRIO = 2;
    __builtin_amdgcn_s_setprio(P3_PPRIO);
    const int ptid = tid - MATRIX * 64;
    const int lrow = ptid >> 3;          // row inside a 32-row pass
    const int lk4 = (ptid & 7) * 4;      // first of this thread's 4 channels inside the chunk
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.A)), 0, (int)p.a_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsrc_a2 = rsrc_a;
    if constexpr (DUAL)
      rsrc_a2 = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(reinterpret_cast<const char*>(p.A2)), 0, (int)p.a_bytes, 0x00020000);
    const bool has_pro = p.in_scale != nullptr;
    const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();  // max(x, -inf) = x
    const int n_img = p.M / HoWo;
    const bool linear = p.stride == 1;   // GATHER: input pixel index = output pixel index

    // prologue vectors of a chunk (its 32 input channels): `cur` in use, `nxt` in flight a chunk ahead
    struct Vec {
      f32x4 s, t, c, s2, t2, c2;
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f}, one4 = {1.f, 1.f, 1.f, 1.f};
    Vec cur = {one4, zero4, zero4, one4, zero4, zero4}, nxt = cur;
    auto load_vec = [&](Vec& v, int ci) {
      if (has_pro) {
        v.s = ldg4(p.in_scale + ci + lk4);
        v.t = ldg4(p.in_shift + ci + lk4);
        if (p.in_center) v.c = ldg4(p.in_center + ci + lk4);
        if constexpr (DUAL) {
          if (p.in2_scale != nullptr) {
            v.s2 = ldg4(p.in2_scale + ci + lk4);
            v.t2 = ldg4(p.in2_shift + ci + lk4);
            if (p.in2_center) v.c2 = ldg4(p.in2_center + ci + lk4);
          }
        }
      }
    };
    auto next_vec = [&](int c_next) {  // at the first row group of a chunk
      cur = nxt;
      if constexpr (DUAL) {
        if (p.in2_scale != nullptr) cur.t2 = cur.t + cur.t2;  // both shifts in one add
      }
      load_vec(nxt, c_next < NC ? c_next * 32 : 0);
    };
    // one thread's float4 of a patch row: prologue, zero padding, (block output), split, LDS write
    auto transform_store = [&](f32x4 v, f32x4 v2, bool ok, char* dst, float* side_dst) {
      if (has_pro) {
        // (scalar fma / max per element: packed fp32 VALU beside MFMAs costs more issue time than
        // the two plain instructions it replaces -- MI355X_MICROARCH.md)
        if constexpr (DUAL) {
          if (p.in2_scale != nullptr) {  // downsample branch: its own BatchNorm
#pragma unroll
            for (int e = 0; e < 4; ++e)
              v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e],
                                fmaf(v2[e] - cur.c2[e], cur.s2[e], cur.t2[e])), relu_floor);
          } else {  // identity skip: added as is
#pragma unroll
            for (int e = 0; e < 4; ++e)
              v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e], cur.t[e]) + v2[e], relu_floor);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e], cur.t[e]), relu_floor);
        }
        // zero padding / rows past M come AFTER the transform
        if (!ok) v = zero4;
        if constexpr (DUAL) {
          if (side_dst != nullptr && ok) *reinterpret_cast<f32x4*>(side_dst) = v;
        }
      }
      p3_split_store<MATH>(v, dst);
    };
    DBG_T(long long d_wait = 0, d_vmw = 0, d_tr = 0, d_ld = 0; const long long d_t0 = clock64();)

    if constexpr (MODE == P3_GATHER) {
      // ---- 1x1 convolutions: patch row = output pixel, BM / 32 row groups per chunk, all of a
      // chunk's loads in flight one chunk ahead (two register sets)
      constexpr int NP = BM / 32;
      constexpr int NPI = NP < 4 ? NP : 4;   // row groups per staged item (register budget)
      constexpr int PARTS = NP / NPI;        // items per chunk: 1, or 2 for 256-row tiles
      static_assert(PARTS == 1 || PARTS == 2, "tile height");
      struct Staged {
        f32x4 a[NPI];
        f32x4 a2[DUAL ? NPI : 1];
        unsigned ok;
        int m0;  // first row of the tile if this workgroup writes side_out for it, else -1
      };
      Staged st[2];
      int a_voff[NP];
      unsigned a_ok = 0;
      int l_round = 0, l_c = 0, l_m0 = 0, l_side = 0;
      auto setup_tile = [&](int round) {
        int m0, n0;
        tile_of(round, m0, n0);
        l_m0 = m0;
        l_side = n0 == 0;  // the materialised block output: written once, by the n-tile-0 workgroups
        a_ok = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int m = m0 + i * 32 + lrow;
          a_voff[i] = BUF_OOB;
          if (m < p.M) {
            int pix = m;
            if (!linear) {
              const int img = m / HoWo;
              const int rem = m - img * HoWo;
              const int ho = rem / p.Wo;
              pix = (img * p.H + ho * p.stride) * p.W + (rem - ho * p.Wo) * p.stride;
            }
            a_voff[i] = (pix * p.lda + lk4) * 4;
            a_ok |= 1u << i;
          }
        }
      };
      // item `it` of the stream is part it % PARTS of chunk it / PARTS; it lives in set it & 1, so
      // with two parts the part index equals the set index (static register indexing)
      auto load = [&](Staged& s, int part, bool live) {
        const int soff = l_c * 128;
        s.ok = live ? (a_ok >> (part * NPI)) : 0u;
        s.m0 = l_side ? l_m0 : -1;
#pragma unroll
        for (int i = 0; i < NPI; ++i) {
          const int vo = live ? a_voff[part * NPI + i] : BUF_OOB;
          s.a[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, soff, 0));
          if constexpr (DUAL)
            s.a2[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a2, vo, soff, 0));
        }
        if (part == PARTS - 1 && ++l_c == NC) {
          l_c = 0;
          if (++l_round < my_tiles) setup_tile(l_round);
        }
      };
      int s_c = 0, s_round = 0, s_n0 = 0;
      const int KS3 = (p.K / 16) * 3072;   // bytes of one n-block's fragments
      const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(reinterpret_cast<const char*>(p.Bfrag)), 0, (int)((long)p.N * p.K * 6),
          0x00020000);
      auto stash = [&](const Staged& s, int part, int g) {   // g = chunk index of the stream
        char* const buf = xsm + (g & 1) * pbuf + (part * NPI * 32 + lrow) * P3_ROW + lk4 * 2;
        if (part == 0) {
          next_vec(s_c + 1);
          DBG_T(const long long d_a = clock64();)
          p3_wait(pempty + (g & 1), MATRIX * (g >> 1));  // chunk g-2 has been read
          DBG_T(d_wait += clock64() - d_a;)
        }
#pragma unroll
        for (int i = 0; i < NPI; ++i) {
          float* side = nullptr;
          if constexpr (DUAL) {
            if (p.side_out != nullptr && s.m0 >= 0)
              side = p.side_out + (long)(s.m0 + (part * NPI + i) * 32 + lrow) * p.lda + s_c * 32 + lk4;
          }
          transform_store(s.a[i], s.a2[DUAL ? i : 0], (s.ok >> i) & 1u, buf + i * 32 * P3_ROW, side);
        }
        if (part == PARTS - 1) {
          // this chunk's B fragments: BN/32 runs of 6 KB (2 k-slabs x 3 planes of one n-block),
          // 1 KB per instruction, instructions dealt round-robin to the producer waves
          const int pw = wave - MATRIX;
          typedef __attribute__((address_space(3))) void lds_void;
#pragma unroll
          for (int k = 0; k < 6 * (BN / 32) / P3_PRODUCERS; ++k) {
            const int f = k * P3_PRODUCERS + pw;     // fragment slot inside the stage
            const int nbl = f / 6, part6 = f - nbl * 6;
            const int nb = s_n0 / 32 + nbl;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc_b, (lds_void*)(bstage + (g & 1) * BST + f * 1024), 16,
                nb * 32 < p.N ? lane * 16 : BUF_OOB, nb * KS3 + s_c * 6144 + part6 * 1024, 0, 0);
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA has landed
          if (lane == 0) x3_signal(pfull + (g & 1));  // (in LDS order behind this wave's writes)
          if (++s_c == NC) {
            s_c = 0;
            if (++s_round < my_tiles) {
              int m0;
              tile_of(s_round, m0, s_n0);
            }
          }
        }
      };
      {
        int m0;
        tile_of(0, m0, s_n0);
      }
      const int I_total = my_tiles * NC * PARTS;
      setup_tile(0);
      load_vec(nxt, 0);
      load(st[0], 0, true);
      for (int it = 0; it < I_total; it += 2) {
        load(st[1], PARTS == 2 ? 1 : 0, it + 1 < I_total);
        stash(st[0], 0, it / PARTS);
        if (it + 1 < I_total) {
          load(st[0], 0, it + 2 < I_total);
          stash(st[1], PARTS == 2 ? 1 : 0, (it + 1) / PARTS);
        }
      }
    } else {
      // ---- KxK stride-1 convolutions: the patch is a run of padded-linear pixels, fetched and
      // transformed as a stream of items of 4 row groups (128 rows x 32 channels), two register
      // sets: 4 - 8 loads per thread in flight
      struct Staged {
        f32x4 a[4];
        unsigned ok;
      };
      Staged st[2];
      // load cursor: (tile, chunk, part) of the next item to fetch.  The byte offsets of this
      // thread's (up to 12) patch rows are decoded once per tile -- every chunk re-reads the same
      // pixels 32 channels further on (soffset)
      // (scalars and wave-uniform branches: a runtime-indexed array would live in scratch memory)
      int l_round = 0, l_c = 0, l_part = 0, l_nparts = 0;
      int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0, r8 = 0, r9 = 0, r10 = 0,
          r11 = 0;   // byte offsets of this thread's rows in row groups 0..11 (p3_rows <= P3_MAX_ROWS)
      unsigned l_ok = 0;
      auto l_setup = [&](int round) {
        int m0, n0;
        tile_of(round, m0, n0);
        const int rows = patch_rows(m0);
        l_nparts = (rows + 127) >> 7;
        const int u = u0_of(m0) + lrow;
        int img = u / (Hp * Wp);
        const int rem = u - img * (Hp * Wp);
        int hh = rem / Wp;
        int ww = rem - hh * Wp;
        l_ok = 0;
        auto next_row = [&](int g, int& vo) {
          const int hi = hh - p.pad, wi = ww - p.pad;
          const bool ok = g * 32 + lrow < rows && img < n_img && (unsigned)hi < (unsigned)p.H &&
                          (unsigned)wi < (unsigned)p.W;
          vo = ok ? (((img * p.H + hi) * p.W + wi) * p.lda + lk4) * 4 : BUF_OOB;
          l_ok |= (ok ? 1u : 0u) << g;
          ww += 32;
          while (ww >= Wp) {
            ww -= Wp;
            if (++hh == Hp) {
              hh = 0;
              ++img;
            }
          }
        };
        next_row(0, r0); next_row(1, r1); next_row(2, r2); next_row(3, r3);
        next_row(4, r4); next_row(5, r5); next_row(6, r6); next_row(7, r7);
        next_row(8, r8); next_row(9, r9); next_row(10, r10); next_row(11, r11);
      };
      auto load = [&](Staged& s) {
        const bool live = l_round < my_tiles;
        const int soff = l_c * 128;
        s.ok = live ? (l_ok >> (l_part * 4)) & 15u : 0u;
#define P3_LD(V) \
  __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, live ? (V) : BUF_OOB, soff, 0))
        if (l_part == 0) {           // (wave-uniform branches, scalar variables: no indexed array)
          s.a[0] = P3_LD(r0); s.a[1] = P3_LD(r1); s.a[2] = P3_LD(r2); s.a[3] = P3_LD(r3);
        } else if (l_part == 1) {
          s.a[0] = P3_LD(r4); s.a[1] = P3_LD(r5); s.a[2] = P3_LD(r6); s.a[3] = P3_LD(r7);
        } else {
          s.a[0] = P3_LD(r8); s.a[1] = P3_LD(r9); s.a[2] = P3_LD(r10); s.a[3] = P3_LD(r11);
        }
#undef P3_LD
        if (!live) return;
        if (++l_part == l_nparts) {  // next chunk of this tile, else next tile
          l_part = 0;
          if (++l_c == NC) {
            l_c = 0;
            if (++l_round < my_tiles) l_setup(l_round);
          }
        }
      };
      // store cursor
      int s_round = 0, s_c = 0, s_part = 0, s_nparts = 0, s_h = 0;
      auto s_setup = [&](int round) {
        int m0, n0;
        tile_of(round, m0, n0);
        s_nparts = (patch_rows(m0) + 127) >> 7;
      };
      auto stash = [&](const Staged& s) {
        char* const buf = xsm + (s_h & 1) * pbuf + lk4 * 2;
        if (s_part == 0) {
          const float* const vp = vlds + s_c * 32 + lk4;   // this chunk's vectors (LDS, staged once)
          cur.s = *reinterpret_cast<const f32x4*>(vp);
          cur.t = *reinterpret_cast<const f32x4*>(vp + p.Cin);
          cur.c = *reinterpret_cast<const f32x4*>(vp + 2 * p.Cin);
          DBG_T(const long long d_a = clock64();)
          p3_wait(pempty + (s_h & 1), MATRIX * (s_h >> 1));  // chunk h-2 has been read
          DBG_T(d_wait += clock64() - d_a;)
        }
        DBG_T(const long long d_b = clock64();
              asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // this item's 4 loads (4 newer ones fly)
              const long long d_c = clock64();
              d_vmw += d_c - d_b;)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = (s_part * 4 + i) * 32 + lrow;
          if (j < p.p3_rows)  // (the last item may reach past the rows the buffer holds)
            transform_store(s.a[i], zero4, (s.ok >> i) & 1u, buf + j * P3_ROW, nullptr);
        }
        DBG_T(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); d_tr += clock64() - d_c;)
        if (++s_part == s_nparts) {
          if (lane == 0) x3_signal(pfull + (s_h & 1));  // (in LDS order behind this wave's writes)
          s_part = 0;
          ++s_h;
          if (++s_c == NC) {
            s_c = 0;
            if (++s_round < my_tiles) s_setup(s_round);
          }
        }
      };
      l_setup(0);
      s_setup(0);
      load(st[0]);
      while (s_round < my_tiles) {
        DBG_T(const long long d_l = clock64();)
        load(st[1]);
        DBG_T(d_ld += clock64() - d_l;)
        stash(st[0]);
        if (s_round < my_tiles) {
          load(st[0]);
          stash(st[1]);
        }
      }
    }
#ifdef VLNCE_DBG_TIME
    if (blockIdx.x == 8 && ptid == 0)
      printf("p3 producer: total %lld cycles, waiting for the matrix waves %lld; KxK form: waiting for "
             "loads %lld, transform + LDS writes %lld, issuing every other item's loads %lld\n",
             (long long)(clock64() - d_t0), d_wait, d_vmw, d_tr, d_ld);
#endif
  } else {
    // ================================================================ matrix waves
    const int wm = wave / WN, wn = wave % WN;
    const int KS3 = (p.K / 16) * 3072;   // bytes of one n-block's fragments (all k-slabs, 3 planes)
    const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.Bfrag)), 0, (int)((long)p.N * p.K * 6),
        0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<char*>(p.C), 0, (int)p.c_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.residual ? p.residual : p.C)), 0,
        (int)p.c_bytes, 0x00020000);   // (ldr == ldc: the output's extent)

    // (Measured and dropped, round 4: a second A-fragment set so that the LDS reads of k-slab
    // s + 1 are issued in front of the MFMAs of slab s -- branch-free steady loop, fragments
    // carried as 128-bit integer vectors -- changes no 3x3 layer by more than 2 % on the same box
    // (profiles/r04_t_*).  Bisection builds of this loop at 256 channels, 16x16 frames: 100 us as
    // is, 96 without any hand-over wait, 84 without the B-fragment loads, 85 without the A reads,
    // 69 with neither -- against 58 us of pure MFMA issue at the 1.9 GHz the launch runs at
    // (profiles/r04_u_*): what the loop loses is the issue cost of its 9 memory instructions per
    // 12 MFMAs (768 B of operands per MFMA at these per-wave tiles), not their latency.)
    // (Round 6, measured and dropped as well: the B fragments of the one- / two-block waves two
    // (chunk, tap) steps ahead in four sets -- what paid in conv_u3: the 64-channel 3x3 layer
    // 178 -> 156 TF/s with no spill, the other instances spill 198 registers under the 168-register
    // cap of a 12-wave workgroup; profiles/r06_v_conv_p3_b_fragments_two_steps_ahead.txt.)
    bf16x8 fa[MT][NA];
    bf16x8 b0[NT][3], b1[NT][3];
    f32x16 acc[MT][NT];
    auto loadB = [&](bf16x8 (&b)[NT][3], const int (&vb)[NT], int soff) {
      if constexpr (!B_LDS) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            b[j][q] = __builtin_bit_cast(
                bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                            rsrc_b, vb[j] == BUF_OOB ? BUF_OOB : vb[j] + q * 1024, soff, 0));
      }
    };
    // B_LDS: k-slab s of the chunk in stage `st`, this wave's n-blocks, fragment (= lane) order
    auto readB = [&](bf16x8 (&b)[NT][3], int st, int s) {
      if constexpr (B_LDS) {
        const char* base = bstage + st * BST + ((wn * NT) * 2 + s) * 3072 + lane * 16;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            b[j][q] = *reinterpret_cast<const bf16x8*>(base + j * 6144 + q * 1024);
      }
    };
    auto mma = [&](const bf16x8 (&b)[NT][3]) {
#pragma unroll
      for (int q = 0; q < PL::NP; ++q)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = plane_mfma<MATH>(fa[i][PL::PA[q]], b[j][PL::PB[q]], acc[i][j]);
    };
    auto vb_of = [&](int n0, int (&vb)[NT]) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int nb = (n0 + wn * WTN) / 32 + j;
        vb[j] = nb * 32 < p.N ? nb * KS3 + lane * 16 : BUF_OOB;
      }
    };

    // the SIMD's VALU issue port is shared with the producer wave: the MFMAs must win it the
    // moment the matrix pipe frees up
    constexpr int P3_MPRIO = 1;   // (the producer waves run at 2, see there)
    __builtin_amdgcn_s_setprio(P3_MPRIO);
    DBG_T(long long d_pf = 0, d_vm = 0, d_lg = 0; const long long d_t0 = clock64(), d_w0 = wall_clock64();)
    int h = 0;
    int vb[NT], vbn[NT];
    WaveBn<NT> wbn;   // BatchNorm finished in this launch (p.bn): the wave's running column sums
    wave_bn_reset(wbn);
    {
      int m0, n0;
      tile_of(0, m0, n0);
      vb_of(n0, vb);
      loadB(b0, vb, 0);
    }
    for (int round = 0; round < my_tiles; ++round) {
      int m0, n0;
      tile_of(round, m0, n0);
      vb_of(n0, vb);
      if (round + 1 < my_tiles) {
        int m1, n1;
        tile_of(round + 1, m1, n1);
        vb_of(n1, vbn);
      } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) vbn[j] = BUF_OOB;
      }
      // LDS byte offset of this lane's patch row for tap (0, 0), per 32-row MFMA block
      int a_row[MT];
      {
        const int u_lo = MODE == P3_DENSE ? u0_of(m0) : m0;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int m = min(m0 + wm * WTM + i * 32 + l31, p.M - 1);
          a_row[i] = ((MODE == P3_DENSE ? u0_of(m) : m) - u_lo) * P3_ROW + half * 16;
        }
      }
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

      int ks3 = 0;  // byte offset of the current k-slab pair inside an n-block's fragments
      for (int c = 0; c < NC; ++c, ++h) {
        DBG_T(const long long d_a = clock64();)
        p3_wait(pfull + (h & 1), P3_PRODUCERS * ((h >> 1) + 1));
        DBG_T(d_pf += clock64() - d_a;)
        const int bufoff = (h & 1) * pbuf;
        int tr = 0, tq = 0;
        for (int t = 0; t < T; ++t) {
          const char* const abase = xsm + bufoff + (tr * Wp + tq) * P3_ROW;
          const bool last_of_chunk = t == T - 1;
          const bool last_of_tile = last_of_chunk && c == NC - 1;
          // ---- k-slab 0 of this (chunk, tap): B fragments in b0 (fetched a slab ago)
          loadB(b1, vb, ks3 + 3072);
          readB(b0, h & 1, 0);
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < NA; ++q)
              fa[i][q] = *reinterpret_cast<const bf16x8*>(abase + a_row[i] + q * 64);
          __builtin_amdgcn_sched_barrier(0);
          DBG_T({
            const long long d_0 = clock64();
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(B_LDS ? 0 : NT * 3) : "memory");
            const long long d_1 = clock64();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            d_vm += d_1 - d_0;
            d_lg += clock64() - d_1;
          } __builtin_amdgcn_sched_barrier(0);)
          mma(b0);
          __builtin_amdgcn_sched_barrier(0);
          // ---- k-slab 1: B fragments in b1; b0 <- the next step's (or the next tile's first)
          if (last_of_tile) loadB(b0, vbn, 0);
          else loadB(b0, vb, ks3 + 6144);
          readB(b1, h & 1, 1);
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int q = 0; q < NA; ++q)
              fa[i][q] = *reinterpret_cast<const bf16x8*>(abase + a_row[i] + q * 64 + 32);
          if (last_of_chunk) {
            // this wave's reads of the patch buffer are complete once they have all returned
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) x3_signal(pempty + (h & 1));
          }
          __builtin_amdgcn_sched_barrier(0);
          mma(b1);
          __builtin_amdgcn_sched_barrier(0);
          ks3 += 6144;
          if (++tq == p.KW) {
            tq = 0;
            ++tr;
          }
        }
      }

      // -------------------------------------------------------------- statistics
      if (p.bn.acc != nullptr) {
        wave_bn_tile<MT, NT>(acc, wbn, p.bn.acc, n0 + wn * WTN, p.N, p.M - (m0 + wm * WTM), half, l31,
                             PL::POST);
        if (round == my_tiles - 1) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);  // in front of the stores
      } else if (p.stat_partial != nullptr) {
        const int tile_m = m0 / BM;
        if (p.stat_rows == 32 && MT > 1) {
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
      // one store = 2 rows x 32 columns = two full 128-byte lines; rows past M get an
      // out-of-range lane offset
      const int rows_left = p.M - (m0 + wm * WTM + 4 * half);
      wave_epilogue<MT, NT>(acc, e_sc, e_sh, e_voff, rows_left, p.ldc, p.act, p.residual != nullptr,
                            rsrc_c, rsrc_r, false);
    }
    __builtin_amdgcn_s_setprio(0);
#ifdef VLNCE_DBG_TIME
    if (blockIdx.x == 8 && (tid == 0 || tid == 64 * (MATRIX - 1))) {
      const long long c = clock64() - d_t0, w = wall_clock64() - d_w0;
      printf("p3 matrix wave %d: tiles %d chunks %d taps %d: total %lld cycles = %lld ticks of 100 MHz "
             "(%.2f GHz); waiting for the patch %lld, slab-0 waits: B fragments %lld, A fragments %lld\n",
             wave, my_tiles, NC, T, c, w, (double)c / (double)w * 0.1, d_pf, d_vm, d_lg);
    }
#endif
  }
#endif
}

// w_ohwi [N][KH][KW][Cin] fp32 -> B fragments [N/32][K/16][3][64 lanes][8 bf16]: k-slab
// ks = ((chunk * T + tap) * 2 + s) holds input channels chunk*32 + s*16 + [0, 16) of that tap;
// lane (l31, half) holds output channel nb*32 + l31, channels half*8 + [0, 8) of the slab;
// plane q is the q-th term of the exact round-to-nearest three-way bf16 split.
template <int MATH>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w,
                                                           unsigned short* __restrict__ frag,
                                                           int N, int T, int Cin) {
  const long total = (long)(N / 32) * (T * Cin / 16) * 64;  // (nb, ks, lane) triples
  const int KS = T * Cin / 16;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int lane = (int)(i & 63);
    const long rest = i >> 6;
    const int ks = (int)(rest % KS);
    const int nb = (int)(rest / KS);
    const int s = ks & 1, ct = ks >> 1;
    const int t = ct % T, c = ct / T;
    const int n = nb * 32 + (lane & 31);
    const int ci = c * 32 + s * 16 + (lane >> 5) * 8;
    const float* src = w + ((long)n * T + t) * Cin + ci;
    unsigned short out[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned short o3[3];
      split_weight<MATH>(src[e], o3);
#pragma unroll
      for (int q = 0; q < 3; ++q) out[q][e] = o3[q];
    }
    unsigned short* dst = frag + ((rest * 3) * 64 + lane) * 8;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[(long)q * 512 + e] = out[q][e];
  }
}

template <int BM, int BN, int WM, int WN, int DUAL, int MODE, int MATH>
int launch_p3(const IgemmParams& p, int rows_alloc, hipStream_t stream) {
  // two patch buffers (+ two B stages for the 1x1 form) + 4 counters
  const int smem_bytes = 2 * rows_alloc * Planes<MATH>::ROW +
                         (MODE == P3_GATHER ? 2 * BN * 192 : 3 * p.Cin * 4) + 16;
  constexpr int threads = (WM * WN + P3_PRODUCERS) * 64;
  auto kern = conv_p3_kernel<BM, BN, WM, WN, DUAL, MODE, MATH>;
  static int attr_bytes = 0;  // per instantiation: the largest dynamic LDS size enabled so far
  if (smem_bytes > attr_bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, x3_lds_max());
    if (e != hipSuccess) {
      vlnce_set_error("conv_p3: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return 2;
    }
    attr_bytes = x3_lds_max();
  }
  IgemmParams q = p;
  q.tiles_m = ceil_div(p.M, BM);
  q.tiles_n = ceil_div(p.N, BN);
  q.splitk = 1;
  q.p3_rows = rows_alloc;
  const long nwg = (long)q.tiles_m * q.tiles_n;
  if (nwg <= 0 || nwg > 0x7fffffffL) {
    vlnce_set_error("conv_p3: bad grid %ld", nwg);
    return 1;
  }
  const int cus = x3_cus();
  const unsigned grid = nwg <= cus ? (unsigned)nwg : (unsigned)cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), smem_bytes, stream, q);
  VLNCE_CHECK_LAUNCH("conv_p3");
  return 0;
}

struct P3Tile {
  int bm, bn;
};

// patch rows (rounded up to whole 32-row passes) the BM-pixel tiles of this problem need: the
// exact maximum over the tiles (the pattern of tile starts repeats with the image, so at most
// Ho*Wo / gcd(BM, Ho*Wo) tiles are looked at)
int p3_rows_for(const IgemmParams& p, int bm, bool dense) {
  if (!dense) return bm;
  const int Hp = p.H + 2 * p.pad, Wp = p.W + 2 * p.pad;
  const int howo = p.Ho * p.Wo;
  auto u0 = [&](long m) {
    const long img = m / howo, rem = m - img * howo, ho = rem / p.Wo;
    return (img * Hp + ho) * Wp + (rem - ho * p.Wo);
  };
  long rows = 0;
  for (long m0 = 0; m0 < p.M; m0 += bm) {
    if (m0 > 0 && m0 % howo == 0) break;  // same tile starts as from m0 = 0 on
    const long mlast = (m0 + bm < p.M ? m0 + bm : p.M) - 1;
    const long r = u0(mlast) - u0(m0) + (p.KH - 1) * Wp + p.KW;
    if (r > rows) rows = r;
  }
  return (int)((rows + 31) / 32 * 32);
}

// Tiles: 8 matrix waves, each a (BM / WM) x 32 sub-tile.  B fragments come straight from L2 (one
// 1 KB load per plane and k-slab, used for BM / WM / 32 MFMAs), so the sub-tile is TALL: with
// 128 rows the texture path carries 16 B/clk per CU, with 32 rows it would saturate (64 B/clk).
template <int DUAL, int MODE, int MATH>
int dispatch_p3(const IgemmParams& p, int tile, int rows, hipStream_t s) {
  note_conv_kernel(VLNCE_CONV_KERNEL(VLNCE_CONV_PATH_P3, MATH, VLNCE_CONV_KERNEL_P3, tile + 1,
                                     DUAL ? VLNCE_CONV_P3_DUAL : MODE == P3_DENSE ? VLNCE_CONV_P3_DENSE
                                                                                  : VLNCE_CONV_P3_GATHER, 0));
  switch (tile) {
    case 0: return launch_p3<128, 256, 1, 8, DUAL, MODE, MATH>(p, rows, s);
    case 1: return launch_p3<64, 256, 1, 8, DUAL, MODE, MATH>(p, rows, s);
    case 2: return launch_p3<256, 128, 2, 4, DUAL, MODE, MATH>(p, rows, s);
    case 3: return launch_p3<128, 128, 2, 4, DUAL, MODE, MATH>(p, rows, s);
    case 4: return launch_p3<256, 64, 4, 2, DUAL, MODE, MATH>(p, rows, s);
    default: return launch_p3<128, 64, 4, 2, DUAL, MODE, MATH>(p, rows, s);
  }
}

template <int MATH>
int p3_try_launch_(const IgemmParams& p, hipStream_t stream) {
  constexpr int P3_ROW = Planes<MATH>::ROW;
  // option "p3": 0 = off, 1 = every layer it covers, 2 = the KxK (patch) layers only, 3 = the 1x1
  // layers only.  Default 2: measured per layer at num_envs 64 (profiles/archive/r03_*_convbench_ab.txt),
  // the patch form is 1.26-1.51x conv_x3_kernel on every stride-1 3x3 layer of the trunks, the
  // 1x1 form (4 producer waves) is within +-10 % of it and slower on most.
  const int mode_env = vlnce_opt(VLNCE_OPT_P3);
  const int force = vlnce_opt(VLNCE_OPT_P3_TILE);  // tuning
  if (!mode_env || !conv_math() || !p.Bfrag) return -1;
  if (p.Cin % 32 != 0 || p.N % 32 != 0 || p.lda % 4 != 0 || p.splitk > 1) return -1;
  if (p.accumulate || p.c_bytes >= 0x7fffffffL || p.a_bytes >= 0x7fffffffL) return -1;
  // residual (eval-mode block ends): added in the register epilogues of conv_p3 / conv_u3; it must
  // have the output's raster
  if (p.residual && (p.ldr != p.ldc || p.stat_partial || p.bn.acc)) return -1;
  if ((long)p.N * p.K * 6 >= 0x7fffffffL) return -1;
  const bool one = p.KH == 1 && p.KW == 1 && p.pad == 0;
  const bool dense = !one;
  if (dense && p.stride != 1) return -1;
  const bool dual = p.A2 != nullptr || p.side_out != nullptr;
  if (dual && !(one && p.stride == 1)) return -1;
  // 1x1 layers wide enough for 256-column tiles: conv_u3_kernel (no producer waves), where its
  // 128-row tiles fill the CUs.  option "u3": 0 = off, 1 = default, 2 / 3 = force 64- / 128-row tiles
  // for every N >= 256 1x1 layer (tests).  Measured
  // per layer at num_envs 64 (profiles/archive/r03_b_convbench_ab_u3.txt): 1.07-1.23x conv_x3_kernel on
  // every N >= 256 layer of the RGB trunk with M >= 16384.
  // short-K wide 1x1 (the bottleneck expansions): conv_s3_kernel.  option "s3": 0 = off, 1 = default
  // (where the 64-row tiles give every CU at least four), 2 = every eligible shape (tests)
  const int s3_env = vlnce_opt(VLNCE_OPT_S3);
  if (!dense && !dual && !p.residual && s3_env && p.stride == 1 && (p.Cin == 64 || p.Cin == 128) && p.K == p.Cin &&
      p.N % 256 == 0 && p.N / 256 <= 8 && (p.stat_partial == nullptr || p.stat_rows == 32) &&
      (p.act == VLNCE_ACT_NONE || p.act == VLNCE_ACT_RELU) &&
      (s3_env == 2 || (long)ceil_div(p.M, 64) * (p.N / 256) >= 4L * x3_cus()))
  {
    return s3_launch(p, stream);
  }
  const int u3_env = vlnce_opt(VLNCE_OPT_U3);
  const int u3_waves = vlnce_opt(VLNCE_OPT_U3_WAVES);
  if (!dense && u3_env && p.N >= 256 && p.Cin <= U3_MAX_CIN) {
    const int cus = x3_cus();
    auto eff = [&](int bm) {
      const long tiles = (long)ceil_div(p.M, bm) * ceil_div(p.N, 256);
      const long rounds = (tiles + cus - 1) / cus;
      return (double)tiles / (double)(rounds * cus);
    };
    // 128-row tiles where they fill the CUs; else 64-row tiles for the long-K layers whose 128-row
    // tiles would leave half of the CUs idle (the 1024 -> 256 block ends of layer 3 at num_envs 64:
    // 70.5 us on conv_x3_kernel, 59.9 us here; profiles/r04_q_convbench_dual_u3.txt)
    int bm = u3_env == 2 ? 64 : 128;
    if (u3_env == 1 && eff(128) < 0.8 && p.K >= 512 && eff(64) >= 0.8) bm = 64;
    if (eff(bm) >= 0.8 || u3_env >= 2) {
      const int kind = !dual ? 0 : (p.in2_scale != nullptr ? 2 : 1);
      // (u3_waves == 4: one wave per SIMD, always 64 x 256 tiles -- conv_u3.hip)
      return u3_launch(p, bm, kind, u3_waves == 4 ? 4 : 8, stream);
    }
  }
  if (mode_env == 2 && !dense) return -1;  // VLNCE_P3=2: only the patch (KxK) layers
  if (mode_env == 3 && dense) return -1;   // VLNCE_P3=3: only the 1x1 layers

  const P3Tile cand[6] = {{128, 256}, {64, 256}, {256, 128}, {128, 128}, {256, 64}, {128, 64}};
  const int cus = x3_cus();
  const bool forced = force >= 1 && force <= 6;
  // BN: the narrowest of 64 / 128 / 256 that covers N (256 for wider layers); 1x1 layers with
  // N <= 64 stay on conv_x3_kernel (8 producer waves: the transform per MFMA is what binds there)
  const int bn = p.N <= 64 ? 64 : p.N <= 128 ? 128 : 256;
  if (!dense && bn == 64 && !forced) return -1;
  int pick = -1, pick_rows = 0;
  double best = 0.0;
  for (int ci = 0; ci < 6; ++ci) {
    const P3Tile& c = cand[ci];
    if (forced ? ci != force - 1 : c.bn > bn) continue;  // (narrower tiles only to fill the CUs)
    const int rows = p3_rows_for(p, c.bm, dense);
    if (2L * rows * P3_ROW + (dense ? 3L * p.Cin * 4 : 2L * c.bn * 192) + 16 > x3_lds_max())
      continue;
    if (dense && rows > P3_MAX_ROWS) continue;   // (the producers' twelve row groups)
    const long tiles = (long)ceil_div(p.M, c.bm) * ceil_div(p.N, c.bn);
    const long rounds = (tiles + cus - 1) / cus;
    const double eff = (double)tiles / (double)(rounds * cus);
    if (eff > best) {
      best = eff;
      pick = ci;
      pick_rows = rows;
    }
    if (eff >= 0.8) break;
  }
  if (pick < 0 || (best < 0.4 && !forced)) return -1;
  if (dual) return dispatch_p3<1, P3_GATHER, MATH>(p, pick, pick_rows, stream);
  if (dense) return dispatch_p3<0, P3_DENSE, MATH>(p, pick, pick_rows, stream);
  return dispatch_p3<0, P3_GATHER, MATH>(p, pick, pick_rows, stream);
}

}  // namespace

int p3_try_launch(const IgemmParams& p, hipStream_t stream) {
  return p.math == MATH_F16X3 ? p3_try_launch_<MATH_F16X3>(p, stream)
                              : p3_try_launch_<MATH_BF16X6>(p, stream);
}

}  // namespace vlnce_detail

extern "C" long vlnce_conv2d_pack_bytes(const vlnce_conv_desc* d) {
  if (!d || d->Cin <= 0 || d->Cout <= 0 || d->Cin % 32 != 0 || d->Cout % 32 != 0) return 0;
  return (long)d->Cout * d->KH * d->KW * d->Cin * 6;
}

extern "C" int vlnce_conv2d_pack_weights(const float* w_ohwi, void* frag, const vlnce_conv_desc* d,
                                         int format, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(w_ohwi && frag && d, "conv2d_pack_weights: null argument");
  VLNCE_CHECK_ARG(format == MATH_BF16X6 || format == MATH_F16X3,
                  "conv2d_pack_weights: format must be 1 (three bf16 planes) or 2 (fp16 planes)");
  VLNCE_CHECK_ARG(vlnce_conv2d_pack_bytes(d) > 0,
                  "conv2d_pack_weights: needs Cin %% 32 == 0 and Cout %% 32 == 0");
  const int T = d->KH * d->KW;
  const long total = (long)(d->Cout / 32) * (T * d->Cin / 16) * 64;
  const long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(format == MATH_F16X3 ? pack_weights_kernel<MATH_F16X3>
                                          : pack_weights_kernel<MATH_BF16X6>,
                     dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), w_ohwi,
                     reinterpret_cast<unsigned short*>(frag), d->Cout, T, d->Cin);
  VLNCE_CHECK_LAUNCH("conv2d_pack_weights");
  return 0;
}
