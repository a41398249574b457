// conv_u3_kernel: 1x1 convolutions with NO producer waves (arithmetic, patch rows and fragment
// layout: conv_p3.hip).
//
// What the in-kernel timers of conv_p3_kernel / conv_x3_kernel show for the 1x1 layers (60 % of
// the trunks' convolution time): a dedicated producer wave next to two MFMA-issuing waves of its
// SIMD gets one instruction in 15-20 cycles -- it has no second wave to hide its own dependency
// and LDS latencies behind, and the matrix waves own the issue port -- so the matrix waves wait
// for the patch.  Here every wave does both jobs, and the compiler interleaves them in ONE
// instruction stream: 8 waves (two per SIMD, 256 VGPRs each), wave w owns output columns
// [32 w, 32 w + 32) of a BM x 256 tile for ALL BM rows (MT = BM / 32 MFMA blocks: a B fragment
// fetched from L2 feeds MT MFMAs), and, between the MFMAs of K-chunk g, transforms its 1/8 share
// of the rows of K-chunk g + 1 (BatchNorm + ReLU prologue, block end, three-way bf16 split) into
// the other patch buffer.  One raw s_barrier per K-chunk (48 MFMAs per wave) swaps the buffers;
// raw A rows are fetched two chunks ahead into registers, B fragments one k-slab ahead.
// (Round 6, measured and dropped: a ring of three / four raw-row sets -- inside a trunk the rows come
// from HBM, not from the Infinity Cache scripts/convbench.py keeps them in (--rotate: 1024 -> 256 block
// end 48 us cache-hot, 69 us from HBM) -- is 5-19 % SLOWER on the 128-row single-input form, cache-hot
// and from HBM alike, and changes nothing on the 64-row forms: profiles/r06_i_*.)
// WAVES = 8: two waves per SIMD, 256 registers each, a wave owns BM x 32 outputs;
// WAVES = 4: ONE wave per SIMD with the whole 512-register file, a wave owns BM x 64 outputs and
// double-buffers its A fragments (no partner wave to hide LDS latency behind).
// LINEAR: stride 1 (input pixel = output pixel).  A compile-time flag: as a runtime one the
// strided path's division constants stayed live through the chunk loop, were spilled, and were
// reloaded from scratch behind every chunk's MFMAs -- each reload followed by an
// s_waitcnt vmcnt(0) that drained the wave's whole prefetch queue (profiles/archive/r03_n_*).
// DUAL: 0 = one input; 1 = block end with an identity skip (second input added as is); 2 = block
// end whose skip path has its own BatchNorm.  Compile-time: the identity form carries half the
// prologue vectors and its chunk body has no branch.
#include "igemm_shared.h"

using namespace vlnce_detail;

namespace vlnce_detail {
namespace {

template <int BM, int DUAL, int WAVES, int LINEAR, int MATH>
__global__ __launch_bounds__(WAVES * 64) void conv_u3_kernel(IgemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Planes<MATH> PL;
  constexpr int P3_ROW = PL::ROW, NA = PL::NA;
  constexpr int BN = 256, MT = BM / 32, NT = 8 / WAVES;
  constexpr int RG = WAVES * 8;                  // rows per group of the transform's thread map
  constexpr int NPT = BM / RG;                   // float4 of a K-chunk's A rows per thread
  constexpr bool ADB = WAVES == 4;               // A fragments double-buffered across the k-slabs
  static_assert(NPT >= 1 && MT >= 1 && (WAVES == 8 || WAVES == 4), "tile");
  constexpr int PBUF = BM * P3_ROW;
  extern __shared__ __attribute__((aligned(16))) char xsm[];  // [2][PBUF] + prologue vectors [NV][Cin]
  // The prologue vectors (scale / shift / centre per input channel, twice for a skip path with its
  // own BatchNorm) live in LDS for the whole launch (round 6).  As per-chunk global loads into a
  // `cur` / `nxt` register pair they cost 24-48 VGPRs (the 128-row instances spilled) and sat in
  // the wave's one in-order vmcnt queue between the raw-row and B-fragment prefetches.
  constexpr int NV = DUAL == 2 ? 6 : 3;
  float* const vlds = reinterpret_cast<float*>(xsm + 2 * PBUF);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int NC = p.Cin / 32;
  const int HoWo = p.Ho * p.Wo;
  const int trow = tid >> 3;          // this thread's row inside a group of RG rows
  const int lk4 = (tid & 7) * 4;

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
  const int G = my_tiles * NC;  // K-chunks this workgroup streams

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.A)), 0, (int)p.a_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsrc_a2 = rsrc_a;
  if constexpr (DUAL)
    rsrc_a2 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(p.A2)), 0, (int)p.a_bytes, 0x00020000);
  const int KS3 = (p.K / 16) * 3072;
  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.Bfrag)), 0, (int)((long)p.N * p.K * 6),
      0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(p.C), 0, (int)p.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(reinterpret_cast<const char*>(p.residual ? p.residual : p.C)), 0,
      (int)p.c_bytes, 0x00020000);   // (ldr == ldc: the output's extent)
  const bool has_pro = p.in_scale != nullptr;
  const float relu_floor = p.in_relu ? 0.f : -__builtin_huge_valf();
  constexpr bool linear = LINEAR != 0;

  // ---------------------------------------------------------------- the A side (every thread)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int ch = tid; ch < p.Cin; ch += WAVES * 64) {   // neutral vectors where there is no prologue
    vlds[ch] = has_pro ? p.in_scale[ch] : 1.f;
    const float t1 = has_pro ? p.in_shift[ch] : 0.f;
    vlds[p.Cin + ch] = t1;
    vlds[2 * p.Cin + ch] = (has_pro && p.in_center) ? p.in_center[ch] : 0.f;
    if constexpr (DUAL == 2) {
      vlds[3 * p.Cin + ch] = p.in2_scale[ch];
      vlds[4 * p.Cin + ch] = t1 + p.in2_shift[ch];   // both shifts in one add
      vlds[5 * p.Cin + ch] = p.in2_center ? p.in2_center[ch] : 0.f;
    }
  }
  __syncthreads();
  struct Raw {
    f32x4 a[NPT];
    f32x4 a2[DUAL ? NPT : 1];
    unsigned ok;
    int m0;  // first row of the tile if this workgroup writes side_out for it, else -1
    int ci;  // first input channel of the chunk
  };
  int a_voff[NPT];
  unsigned a_ok = 0;
  int l_round = 0, l_c = 0, l_m0 = 0, l_side = 0;
  auto setup_tile = [&](int round) {
    int m0, n0;
    tile_of(round, m0, n0);
    l_m0 = m0;
    l_side = n0 == 0;
    a_ok = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int m = m0 + i * RG + trow;
      a_voff[i] = BUF_OOB;
      if (m < p.M) {
        int pix = m;
        if constexpr (!linear) {
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
  auto load_raw = [&](Raw& r) {   // (branch-free; advance_raw() moves the cursor afterwards)
    const bool live = l_round < my_tiles;
    const int soff = l_c * 128;
    r.ok = live ? a_ok : 0u;
    r.m0 = l_side ? l_m0 : -1;
    r.ci = l_c * 32;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const int vo = live ? a_voff[i] : BUF_OOB;
      r.a[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, soff, 0));
      if constexpr (DUAL)
        r.a2[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a2, vo, soff, 0));
    }
  };
  auto advance_raw = [&]() {
    if (l_round < my_tiles && ++l_c == NC) {
      l_c = 0;
      if (++l_round < my_tiles) setup_tile(l_round);
    }
  };
  // prologue + split of this thread's float4s of one chunk into patch buffer `buf`.  Branch-free
  // in the single-input form (neutral vectors where the convolution has no prologue: x*1+0 and
  // max(x, -inf) are exact), so that it shares ONE basic block with the MFMAs of the chunk and
  // the scheduler can interleave the two.
  auto transform = [&](const Raw& r, char* buf) {
    struct {
      f32x4 s, t, c, s2, t2, c2;
    } cur;
    const float* const vp = vlds + r.ci + lk4;
    cur.s = *reinterpret_cast<const f32x4*>(vp);
    cur.t = *reinterpret_cast<const f32x4*>(vp + p.Cin);
    cur.c = *reinterpret_cast<const f32x4*>(vp + 2 * p.Cin);
    if constexpr (DUAL == 2) {
      cur.s2 = *reinterpret_cast<const f32x4*>(vp + 3 * p.Cin);
      cur.t2 = *reinterpret_cast<const f32x4*>(vp + 4 * p.Cin);
      cur.c2 = *reinterpret_cast<const f32x4*>(vp + 5 * p.Cin);
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      f32x4 v = r.a[i];
      const bool ok = (r.ok >> i) & 1u;
      if constexpr (DUAL) {
        if constexpr (DUAL == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e],
                              fmaf(r.a2[i][e] - cur.c2[e], cur.s2[e], cur.t2[e])), relu_floor);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e], cur.t[e]) + r.a2[i][e], relu_floor);
        }
        if (!ok) v = zero4;
        if (p.side_out != nullptr && r.m0 >= 0 && ok)
          *reinterpret_cast<f32x4*>(p.side_out + (long)(r.m0 + i * RG + trow) * p.lda + r.ci + lk4) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = fmaxf(fmaf(v[e] - cur.c[e], cur.s[e], cur.t[e]), relu_floor);
          v[e] = ok ? v[e] : 0.f;
        }
      }
      p3_split_store<MATH>(v, buf + (i * RG + trow) * P3_ROW + lk4 * 2);
    }
  };

  // ---------------------------------------------------------------- the matrix side (per wave)
  constexpr int HM = MT / 2;  // row blocks per half (two-wave form)
  static_assert(ADB || HM >= 1, "tile");
  bf16x8 fa[ADB ? MT : 1][NA], fa1[ADB ? MT : 1][NA], fh0[ADB ? 1 : HM][NA], fh1[ADB ? 1 : HM][NA];
  // BA (B fragments ahead): 0 = k-slab 1's fragments requested at the start of their chunk and the
  // next chunk's slab-0 fragments half a chunk ahead (one slab of lead: 6 * MT MFMAs against an L2
  // round trip); 1 = slab 1's fragments a whole chunk ahead (a second set, alternating by chunk
  // parity); 2 = both slabs' fragments a whole chunk ahead (two more sets: the 64-row forms have
  // the registers).  Single-input forms only: 1x1 layer list 2.219 -> 2.158 ms from HBM (1024 ->
  // 256: 179 -> 207 TF/s); the dual forms measured 3 % SLOWER with it (the 128-row ones spill 6-8
  // registers) and keep one slab of lead (profiles/r06_u_conv_u3_b_fragments_a_chunk_ahead.txt).
  constexpr int U3_B_AHEAD_64 = 2, U3_B_AHEAD_128 = 1;   // (per tile height: what the registers allow)
  constexpr int BA = (ADB || DUAL != 0) ? 0 : (BM == 64 ? U3_B_AHEAD_64 : U3_B_AHEAD_128);
  bf16x8 b0[NT][3], b1[NT][3];
  bf16x8 b0x[BA == 2 ? NT : 1][3], b1x[BA >= 1 ? NT : 1][3];
  f32x16 acc[MT][NT];
  const int a_off = l31 * P3_ROW + half * 16;   // + i * 32 * P3_ROW + q * 64 + s * 32
  auto loadB = [&](bf16x8 (&b)[NT][3], const int (&vb)[NT], int soff) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        b[j][q] = __builtin_bit_cast(
            bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                        rsrc_b, vb[j] == BUF_OOB ? BUF_OOB : vb[j] + q * 1024, soff, 0));
  };
  auto readA = [&](bf16x8 (&f)[ADB ? MT : 1][NA], const char* buf, int s) {
#pragma unroll
    for (int i = 0; i < (ADB ? MT : 1); ++i)
#pragma unroll
      for (int q = 0; q < NA; ++q)
        f[i][q] = *reinterpret_cast<const bf16x8*>(buf + a_off + i * 32 * P3_ROW + q * 64 + s * 32);
  };
  auto readH = [&](bf16x8 (&f)[ADB ? 1 : HM][NA], const char* buf, int s, int h) {
#pragma unroll
    for (int i = 0; i < (ADB ? 1 : HM); ++i)
#pragma unroll
      for (int q = 0; q < NA; ++q)
        f[i][q] = *reinterpret_cast<const bf16x8*>(buf + a_off + (h * HM + i) * 32 * P3_ROW + q * 64 +
                                                   s * 32);
  };
  constexpr int NP = PL::NP;
  auto mma = [&](const bf16x8 (&f)[ADB ? MT : 1][NA], const bf16x8 (&b)[NT][3]) {
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < (ADB ? MT : 1); ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = plane_mfma<MATH>(f[i][PL::PA[q]], b[j][PL::PB[q]], acc[i][j]);
  };
  auto mmaH = [&](const bf16x8 (&f)[ADB ? 1 : HM][NA], const bf16x8 (&b)[NT][3], int h) {
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < (ADB ? 1 : HM); ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[h * HM + i][j] = plane_mfma<MATH>(f[i][PL::PA[q]], b[j][PL::PB[q]], acc[h * HM + i][j]);
  };
  auto vb_of = [&](int n0, int (&vb)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int nb = n0 / 32 + wave * NT + j;
      vb[j] = nb * 32 < p.N ? nb * KS3 + lane * 16 : BUF_OOB;
    }
  };

  // ---------------------------------------------------------------- prologue of the stream
  // vector schedule: chunk k's vectors are channels (k % NC) * 32 ..; `cur` must hold chunk k's
  // when chunk k is transformed
  //
  // (Round 6, measured and dropped: raw rows requested TWO chunks at a time, every second chunk
  // (four raw sets), so that twice the bytes are in flight behind each wait of the wave's one in-order
  // vmcnt queue: K >= 512 layers +7...15 %, 256 -> 1024 -6 %, the dual forms 1-5 % slower, the step
  // unchanged within its noise and 40 % more compile time: profiles/r06_p_conv_u3_raw_batch_ab.txt;
  // the arm itself: docs/experiments/conv_u3_raw_batch_2.patch.  Also measured and dropped: the dual
  // forms' side_out rows stored two chunks per burst instead of every chunk -- stores count in the
  // same queue -- block ends 2.870 -> 2.946 ms: profiles/r06_s_conv_u3_side_out_store_bursts.txt.)
  Raw rx, ry;   // chunk j lives in set j % 2
  setup_tile(0);
  load_raw(rx);   // chunk 0
  advance_raw();
  load_raw(ry);   // chunk 1
  advance_raw();
  int m0 = 0, n0 = 0;
  tile_of(0, m0, n0);
  int vb[NT], vbn[NT];
  vb_of(n0, vb);
#pragma unroll
  for (int j = 0; j < NT; ++j) vbn[j] = BUF_OOB;
  if (my_tiles > 1) {
    int m1, n1;
    tile_of(1, m1, n1);
    vb_of(n1, vbn);
  }
  loadB(b0, vb, 0);
  if constexpr (BA >= 1) loadB(b1, vb, 3072);
  transform(rx, xsm);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int c = 0, round = 0, ks3 = 0;
  WaveBn<NT> wbn;   // BatchNorm finished in this launch (p.bn): the wave's running column sums
  wave_bn_reset(wbn);
  DBG_T(long long d_blk = 0, d_epi = 0, d_bar = 0, d_book = 0; const long long d_t0 = clock64(), d_w0 = wall_clock64();)
  // one K-chunk: MFMAs on patch (g & 1) / transform of `rn` (chunk g + 1) into patch ((g+1) & 1) /
  // raw loads of chunk g + 2 into `rf`.  Everything up to the transform is ONE basic block.
  auto chunk = [&](int g, Raw& rn, Raw& rf, bf16x8 (&b0c)[NT][3], bf16x8 (&b1c)[NT][3], auto& b0n,
                   auto& b1n) {
    const char* const pb = xsm + (g & 1) * PBUF;
    char* const pn = xsm + ((g + 1) & 1) * PBUF;
    const bool last_of_tile = c == NC - 1;
    int vb_s0[NT];                                         // slab 0 of the next chunk
#pragma unroll
    for (int j = 0; j < NT; ++j) vb_s0[j] = last_of_tile ? vbn[j] : vb[j];
    const int so_s0 = last_of_tile ? 0 : ks3 + 6144;
    DBG_T(const long long d_0 = clock64();)
    // k-slab 1's B fragments BEFORE the raw rows of chunk g + 2: vmcnt retires in order, and the
    // fragments (L2 hits, needed half a chunk from here) would otherwise wait out the HBM latency
    // of rows that nobody reads before the next chunk
    if constexpr (BA == 0) loadB(b1c, vb, ks3 + 3072);
    if constexpr (BA == 2) loadB(b0n, vb_s0, so_s0);              // the NEXT chunk's fragments
    if constexpr (BA >= 1) loadB(b1n, vb_s0, so_s0 + 3072);
    load_raw(rf);
    if constexpr (ADB) {
      readA(fa, pb, 0);
      readA(fa1, pb, 1);
      mma(fa, b0c);
      loadB(b0n, vb_s0, so_s0);
      mma(fa1, b1c);
    } else {
      // the MT row blocks in two halves with a fragment set each: the reads of one half land
      // under the MFMAs of the other (no spare registers for a second full set)
      readH(fh0, pb, 0, 0);
      readH(fh1, pb, 0, 1);
      mmaH(fh0, b0c, 0);
      readH(fh0, pb, 1, 0);
      mmaH(fh1, b0c, 1);
      if constexpr (BA < 2) loadB(b0n, vb_s0, so_s0);
      readH(fh1, pb, 1, 1);
      mmaH(fh0, b1c, 0);
      mmaH(fh1, b1c, 1);
    }
    transform(rn, pn);
    // Instruction order of the block (the scheduler's own choice bunches the transform behind the
    // last MFMAs and issues every fragment read right in front of its MFMA): k-slab 0's fragment
    // reads and the global loads first, a few transform instructions under their latency, then
    // per MFMA two VALU instructions of the transform and at most one LDS read (k-slab 1's
    // fragments, each as soon as the MFMAs that still read its registers have issued), one LDS
    // write, one global load.
    constexpr int U3_VPM = 2;   // VALU instructions of the transform per MFMA
    if constexpr (ADB) {
#pragma unroll
      for (int k = 0; k < 2 * NP * MT * NT; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, U3_VPM, 0);
      }
    } else {
      // four phases of 6 * HM * NT MFMAs (half 0 / half 1 of k-slab 0, then of k-slab 1).  Only
      // the first half's fragments are read before the first MFMA (all eight waves read at once
      // right after the barrier: every kilobyte in front of the first MFMA is exposed); the
      // other reads trickle, one per MFMA, a phase ahead of their use.
      // (Measured and dropped, profiles/r04_a_convbench_u3_loads_first.txt: pinning the chunk's raw-row
      // and slab-1 B loads in front of the first MFMA with a VMEM-read group changes no layer by
      // more than 2 %.)
      __builtin_amdgcn_sched_group_barrier(0x100, NA * HM, 0);
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) {
#pragma unroll
        for (int k = 0; k < NP * HM * NT; ++k) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, MATH == MATH_F16X3 ? 2 * U3_VPM : U3_VPM, 0);
          if (ph < 3 && k < NA * HM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      }
    }
    // ---- bookkeeping (branches from here on)
    DBG_T(const long long d_1 = clock64(); d_blk += d_1 - d_0;)
    advance_raw();
    ks3 += 6144;
    DBG_T(const long long d_2 = clock64(); d_book += d_2 - d_1;)
    if (last_of_tile) {
      // -------------------------------------------------------------- statistics
      if (p.bn.acc != nullptr) {
        wave_bn_tile<MT, NT>(acc, wbn, p.bn.acc, n0 + wave * NT * 32, p.N, p.M - m0, half, l31, PL::POST);
        if (round == my_tiles - 1) wave_bn_flush(wbn, p.bn.acc, p.N, half, l31);  // in front of the stores
      } else if (p.stat_partial != nullptr) {
        const int col0 = n0 + wave * NT * 32;
        if (p.stat_rows == 32 && MT > 1) {
#pragma unroll
          for (int i = 0; i < MT; ++i)
            wave_stats_block<NT>(acc[i], p.stat_partial, m0 / 32 + i, p.M - (m0 + i * 32), col0, p.N,
                                 half, l31, PL::POST);
        } else if (p.stat_rows > 0 && p.stat_rows < BM)
          wave_stats_fine<MT, NT>(acc, p.stat_partial, p.stat_rows, m0, p.M, col0, p.N, half, l31,
                                  PL::POST);
        else
          wave_stats<MT, NT>(acc, p.stat_partial, m0 / BM, p.M - m0, BM, col0, p.N, half, l31, PL::POST);
      }
      // -------------------------------------------------------------- epilogue from registers
      // (Measured alternatives, round 3, profiles/archive/r03_h_*: turning each 32x32 block around in a
      // per-wave LDS square and storing 128-byte rows with 16-byte stores -- a quarter of the
      // store instructions -- changes nothing (126 vs 122 us on the 64->256 layer): the burst
      // drains at ~5.6 TB/s either way, and what is lost is that a wave's next loads queue
      // behind its own stores in the one in-order vmcnt.  64-row tiles held to 128 VGPRs so that
      // TWO workgroups share a CU and one computes while the other drains: 2x slower, 50
      // registers spilled into the chunk loop.)
      float e_sc[NT], e_sh[NT];
      int e_voff[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + (wave * NT + j) * 32 + l31;
        const bool okc = col < p.N;
        e_sc[j] = ((okc && p.scale) ? p.scale[col] : 1.f) * PL::POST;
        e_sh[j] = (okc && p.shift) ? p.shift[col] : 0.f;
        e_voff[j] = okc ? (int)((((long)(m0 + 4 * half)) * p.ldc + col) * 4) : BUF_OOB;
      }
      const int rows_left = p.M - (m0 + 4 * half);
      wave_epilogue<MT, NT>(acc, e_sc, e_sh, e_voff, rows_left, p.ldc, p.act, p.residual != nullptr,
                            rsrc_c, rsrc_r, true);
      c = 0;
      ks3 = 0;
      if (++round < my_tiles) {
        tile_of(round, m0, n0);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          vb[j] = vbn[j];
          vbn[j] = BUF_OOB;
        }
        if (round + 1 < my_tiles) {
          int m1, n1;
          tile_of(round + 1, m1, n1);
          vb_of(n1, vbn);
        }
      }
    } else {
      ++c;
    }
    DBG_T(const long long d_3 = clock64(); d_epi += d_3 - d_2;)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this thread's patch writes are in LDS
    __builtin_amdgcn_s_barrier();
    DBG_T(d_bar += clock64() - d_3;)
  };
  auto& b0alt = [&]() -> auto& { if constexpr (BA == 2) return b0x; else return b0; }();
  auto& b1alt = [&]() -> auto& { if constexpr (BA >= 1) return b1x; else return b1; }();
  for (int g = 0; g < G; g += 2) {
    // (B sets by chunk parity: BA = 0 uses b0 / b1 throughout; BA = 1 alternates b1 / b1x;
    // BA = 2 alternates both)
    chunk(g, ry, rx, b0, b1, b0alt, b1alt);
    if (g + 1 < G) chunk(g + 1, rx, ry, b0alt, b1alt, b0, b1);
  }
#ifdef VLNCE_DBG_TIME
  if (blockIdx.x == 8 && (tid == 0 || tid == (WAVES - 1) * 64)) {
    const long long cy = clock64() - d_t0, w = wall_clock64() - d_w0;
    printf("u3 wave %d: tiles %d chunks/tile %d: total %lld cycles = %lld ticks of 100 MHz (%.2f GHz): "
           "MFMA+transform blocks %lld, bookkeeping %lld, epilogues %lld, barriers %lld\n",
           wave, my_tiles, NC, cy, w, (double)cy / (double)w * 0.1, d_blk, d_book, d_epi, d_bar);
  }
#endif
#endif
}

template <int BM, int DUAL, int WAVES, int LINEAR, int MATH>
int launch_u3_(const IgemmParams& p, hipStream_t stream) {
  constexpr int NV = DUAL == 2 ? 6 : 3;   // prologue vectors kept in LDS
  const int smem_bytes = 2 * BM * Planes<MATH>::ROW + NV * p.Cin * 4;
  constexpr int smem_max = 2 * BM * Planes<MATH>::ROW + NV * U3_MAX_CIN * 4;
  auto kern = conv_u3_kernel<BM, DUAL, WAVES, LINEAR, MATH>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem_max);
    if (e != hipSuccess) {
      vlnce_set_error("conv_u3: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
      return 2;
    }
    attr_set = true;
  }
  IgemmParams q = p;
  q.tiles_m = ceil_div(p.M, BM);
  q.tiles_n = ceil_div(p.N, 256);
  q.splitk = 1;
  const long nwg = (long)q.tiles_m * q.tiles_n;
  if (nwg <= 0 || nwg > 0x7fffffffL) {
    vlnce_set_error("conv_u3: bad grid %ld", nwg);
    return 1;
  }
  const int cus = x3_cus();
  const unsigned grid = nwg <= cus ? (unsigned)nwg : (unsigned)cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), smem_bytes, stream, q);
  VLNCE_CHECK_LAUNCH("conv_u3");
  return 0;
}

template <int BM, int DUAL, int WAVES, int MATH>
int launch_u3(const IgemmParams& p, hipStream_t stream) {
  return p.stride == 1 ? launch_u3_<BM, DUAL, WAVES, 1, MATH>(p, stream)
                       : launch_u3_<BM, DUAL, WAVES, 0, MATH>(p, stream);
}

template <int MATH>
int u3_launch_(const IgemmParams& p, int bm, int dual_kind, int waves, hipStream_t stream) {
  note_conv_kernel(VLNCE_CONV_KERNEL(VLNCE_CONV_PATH_P3, MATH, VLNCE_CONV_KERNEL_U3,
                                     waves == 4 || bm != 128 ? 64 : 128, dual_kind == 2 ? 2 : dual_kind ? 1 : 0,
                                     waves == 4 ? 4 : 8));
  if (waves == 4)   // one wave per SIMD, 64 x 256 tiles (a wave owns 64 x 64): experiment
    return dual_kind == 2 ? launch_u3<64, 2, 4, MATH>(p, stream)
                          : dual_kind ? launch_u3<64, 1, 4, MATH>(p, stream) : launch_u3<64, 0, 4, MATH>(p, stream);
  if (bm == 128)
    return dual_kind == 2 ? launch_u3<128, 2, 8, MATH>(p, stream)
                          : dual_kind ? launch_u3<128, 1, 8, MATH>(p, stream) : launch_u3<128, 0, 8, MATH>(p, stream);
  return dual_kind == 2 ? launch_u3<64, 2, 8, MATH>(p, stream)
                        : dual_kind ? launch_u3<64, 1, 8, MATH>(p, stream) : launch_u3<64, 0, 8, MATH>(p, stream);
}

}  // namespace

int u3_launch(const IgemmParams& p, int bm, int dual_kind, int waves, hipStream_t stream) {
  return p.math == MATH_F16X3 ? u3_launch_<MATH_F16X3>(p, bm, dual_kind, waves, stream)
                              : u3_launch_<MATH_BF16X6>(p, bm, dual_kind, waves, stream);
}

}  // namespace vlnce_detail
