// A T-step rollout of the masked GRU / LSTM state encoder as ONE launch forward and ONE backward
// (habitat RNNStateEncoder.seq_forward semantics; call sites cma_policy.py:249-256,287-294,
// seq2seq_policy.py:128-136; the batches are the cached-feature DAgger batch,
// dagger_trainer.py:39-114, and a DD-PPO minibatch, rollout_storage.py:154-276).
//
// The recurrence h_t = cell(gi_t, mask_t * h_{t-1}) is a chain of T dependent products with a
// [GH, H] matrix (GH = 3H for a GRU, 4H for an LSTM) that is far too large for one workgroup's
// registers at H = 512 (3-4 MB) and far too small to fill the chip: as T launches the step costs a
// launch round trip each (measured: the update of a 5-episode x 100-step batch spends most of its
// time in ~600 such launches).  Here H/16 workgroups stay resident for the whole rollout:
//   * workgroup b owns hidden units [16b, 16b+16): their G x 16 rows of W_hh (forward) or their
//     16 columns (backward, rows of W_hh^T) live in REGISTERS for all T steps -- thread
//     (unit u = tid/16, slice s = tid%16) holds the k-slice [s K/16, (s+1) K/16) of its rows;
//   * per step the workgroups exchange the new state (backward: the GH recurrent gate gradients)
//     through a small double-buffered area of (value, step tag) PAIRS written with one 64-bit
//     device-scope atomic store each and polled with 64-bit atomic loads until the tag is the
//     step's: data and flag travel together, so a step costs one store -> load latency across the
//     chip and needs no fence, no counter and no second round trip (a first version with an
//     arrival counter + thread fences, the cooperative-groups grid-sync pattern, measured 6.2 us
//     per step; profiles/archive/r03_f_*);
//   * the [N, K] operand of the step (N <= 16 episodes) is staged in LDS, each thread multiplies
//     its register slice with all N rows (fp32 FMA), slice partials meet in LDS and thread (u, n)
//     finishes unit u of episode n: gates, new state, what backward needs.  The cell arithmetic
//     is rnn_cell.h's, the one the step and gates kernels of rnn.hip call: only the summation
//     order of the product differs from theirs.
// What a step reads that does not depend on the recurrence (gi; in the backward pass the saved
// gates / states / output gradient) is fetched one step ahead.
// What the LSTM adds: its cell state c is unit-local, so the thread that finishes (unit, episode)
// keeps c_t in a REGISTER for all T steps (backward: dc), and its dgi and dgh are one array.
#include <stdlib.h>

#include "common.h"
#include "rnn_cell.h"

namespace {

constexpr int RO_UNITS = 16;   // hidden units (fwd) / carry columns (bwd) per workgroup
constexpr int RO_SLICES = 16;  // k-slices per unit = lanes that share a unit
constexpr int RO_MAXN = 16;    // episodes per rollout step
constexpr int RO_PP = 20;      // pitch of a unit's 16 slice partials (conflict-free b128 reads)

// GH = 3H, gates r, z, n (GRU) | 4H, gates i, f, g, o (LSTM)
struct RolloutParams {
  const float* gi;      // [T,N,GH]  x W_ih^T + b_ih
  const float* h0;      // [N,H]
  const float* c0;      // [N,H]     LSTM
  const uint8_t* mask;  // [T,N] not-done masks
  const float* w;       // fwd: W_hh [GH,H]; bwd: W_hh^T [H,GH]
  const float* b_hh;    // [GH]
  float* hp;            // [T,N,H]   mask_t * h_{t-1}
  float* out;           // [T,N,H]
  float* gates;         // [T,N,GH]  activated
  float* aux;           // [T,N,H]   GRU: hn = W_hn hp + b_hn; LSTM: c_t
  const float* dout;    // [T,N,H] or null
  const float* dh_fin;  // [N,H] or null
  const float* dc_fin;  // [N,H] or null  LSTM
  float* dgi;           // [T,N,GH]
  float* dh0;           // [N,H]
  float* dc0;           // [N,H]     LSTM
  unsigned long long* ex;  // [2][N][K] (value, tag) pairs, zero at launch; K = H (fwd) | GH (bwd)
  int T, N;
  // GRU only; the LSTM kernels read neither
  int spread;  // 1, or 8: only every 8th workgroup works, i.e. all of them on one XCD (experiment)
  float* dgh;  // [T,N,GH]  (an LSTM's dgh is its dgi)
};

constexpr int ro_chunk(int ld) {
  int c = ld < 16 ? ld : 16;
  while (ld % c) --c;
  return c;
}

__device__ __forceinline__ void ex_store(unsigned long long* p, float v, unsigned tag) {
  const unsigned long long w = ((unsigned long long)tag << 32) | __float_as_uint(v);
  __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// stage src [N, K] (K-contiguous rows) into LDS rows of 16 slices x (SL + 4) floats, scaled per row
template <int K, int NT, bool MASKED>
__device__ __forceinline__ void stage_operand(float* __restrict__ Xs, const float* __restrict__ src,
                                              const uint8_t* __restrict__ mrow, int N) {
  constexpr int SL = K / RO_SLICES, PITCH = SL + 4, ROW = RO_SLICES * PITCH;
  constexpr int K4 = K / 4;
  constexpr int LD = (NT * K4 + 255) / 256;
  const int total = N * K4;
  f32x4 v[LD];
#pragma unroll
  for (int q = 0; q < LD; ++q) {
    const int i = threadIdx.x + q * 256;
    if (i < total) v[q] = *reinterpret_cast<const f32x4*>(src + (long)i * 4);
  }
#pragma unroll
  for (int q = 0; q < LD; ++q) {
    const int i = threadIdx.x + q * 256;
    if (i < total) {
      const int n = i / K4, k = (i - n * K4) * 4;
      f32x4 x = v[q];
      if (MASKED) x *= (float)mrow[n];
      *reinterpret_cast<f32x4*>(Xs + n * ROW + (k / SL) * PITCH + (k % SL)) = x;
    }
  }
}

// the same from the exchange area: every thread polls its share of the N*K pairs until each
// carries `tag` (bounded: a lost workgroup ends in a trap, not in a hung device)
template <int K, int NT, bool MASKED>
__device__ __forceinline__ void stage_exchanged(float* __restrict__ Xs,
                                                const unsigned long long* __restrict__ ex,
                                                unsigned tag, const uint8_t* __restrict__ mrow,
                                                int N) {
  constexpr int SL = K / RO_SLICES, PITCH = SL + 4, ROW = RO_SLICES * PITCH;
  constexpr int LD = (NT * K + 255) / 256;
  constexpr int CH = ro_chunk(LD);  // pairs in flight per thread: the largest divisor <= 16
  static_assert(LD % CH == 0, "whole chunks");
  const int total = N * K;
  long spins = 0;
  for (int c0 = 0; c0 < LD; c0 += CH) {
    if (threadIdx.x + c0 * 256 >= total) break;
    unsigned long long w[CH];
    bool again;
    do {
      again = false;
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int i = threadIdx.x + (c0 + q) * 256;
        if (i < total)
          w[q] = __hip_atomic_load(ex + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int i = threadIdx.x + (c0 + q) * 256;
        if (i < total && (unsigned)(w[q] >> 32) != tag) again = true;
      }
      if (again && ++spins > (1L << 22)) __builtin_trap();
    } while (again);
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const int i = threadIdx.x + (c0 + q) * 256;
      if (i < total) {
        const int n = i / K, k = i - n * K;
        float x = __uint_as_float((unsigned)w[q]);
        if (MASKED) x *= (float)mrow[n];
        Xs[n * ROW + (k / SL) * PITCH + (k % SL)] = x;
      }
    }
  }
}

template <bool LSTM, int H, int NT>
__global__ __launch_bounds__(256) void rnn_rollout_fwd_kernel(RolloutParams p) {
  constexpr int G = LSTM ? 4 : 3;
  constexpr int SL = H / RO_SLICES, PITCH = SL + 4, ROW = RO_SLICES * PITCH;
  static_assert(SL % 4 == 0, "slice of whole float4s");
  extern __shared__ __attribute__((aligned(16))) float ro_sm[];
  float* Xs = ro_sm;               // [NT][ROW]   masked previous state
  float* part = ro_sm + NT * ROW;  // [G][NT][16 units][RO_PP]
  const int tid = threadIdx.x;
  const int u = tid >> 4, sl = tid & 15;
  const int n_own = sl;  // final stage: this thread finishes (unit u, episode sl)
  if (!LSTM && blockIdx.x % p.spread) return;
  const int j = (LSTM ? blockIdx.x : blockIdx.x / p.spread) * RO_UNITS + u;
  const int N = p.N, T = p.T;
  const bool fin = n_own < N;

  float w[G][SL];
  float bh[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float* row = p.w + (long)(g * H + j) * H + sl * SL;
#pragma unroll
    for (int i4 = 0; i4 < SL / 4; ++i4) {
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(row + 4 * i4);
      w[g][4 * i4] = t4[0];
      w[g][4 * i4 + 1] = t4[1];
      w[g][4 * i4 + 2] = t4[2];
      w[g][4 * i4 + 3] = t4[3];
    }
    bh[g] = p.b_hh[g * H + j];
  }
  float gx[G], gnext[G];
#pragma unroll
  for (int g = 0; g < G; ++g) gx[g] = gnext[g] = 0.f;
  [[maybe_unused]] float cst = 0.f;  // LSTM: c_{t-1} of (unit j, episode n_own), never leaves this thread
  if (fin) {
#pragma unroll
    for (int g = 0; g < G; ++g) gx[g] = p.gi[(long)n_own * G * H + g * H + j];
    if constexpr (LSTM) cst = p.c0[(long)n_own * H + j];
  }

  for (int t = 0; t < T; ++t) {
    if (fin && t + 1 < T) {
#pragma unroll
      for (int g = 0; g < G; ++g) gnext[g] = p.gi[((long)(t + 1) * N + n_own) * G * H + g * H + j];
    }
    if (t == 0)
      stage_operand<H, NT, true>(Xs, p.h0, p.mask, N);
    else
      stage_exchanged<H, NT, true>(Xs, p.ex + (long)((t - 1) & 1) * N * H, (unsigned)t,
                                   p.mask + (long)t * N, N);
    __syncthreads();
    float acc[G][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g][n] = 0.f;
      if (n < N) {
        const float* xr = Xs + n * ROW + sl * PITCH;
#pragma unroll
        for (int i4 = 0; i4 < SL / 4; ++i4) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(xr + 4 * i4);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g][n] = fmaf(w[g][4 * i4 + c], x[c], acc[g][n]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) part[((g * NT + n) * RO_UNITS + u) * RO_PP + sl] = acc[g][n];
      }
    }
    __syncthreads();
    if (fin) {
      float gh[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float* pr = part + ((g * NT + n_own) * RO_UNITS + u) * RO_PP;
        f32x4 s4 = *reinterpret_cast<const f32x4*>(pr);
#pragma unroll
        for (int q = 1; q < 4; ++q) s4 += *reinterpret_cast<const f32x4*>(pr + 4 * q);
        gh[g] = (s4[0] + s4[1]) + (s4[2] + s4[3]) + bh[g];
      }
      const float hpv = Xs[n_own * ROW + (j / SL) * PITCH + (j % SL)];
      float hnew, auxv, gv[G];
      if constexpr (LSTM) {
        const float cp = cst * (float)p.mask[(long)t * N + n_own];
        const rnn_cell::LstmFwd q =
            rnn_cell::lstm_fwd(cp, gx[0] + gh[0], gx[1] + gh[1], gx[2] + gh[2], gx[3] + gh[3]);
        cst = q.c;
        hnew = q.h;
        auxv = q.c;
        gv[0] = q.i;
        gv[1] = q.f;
        gv[2] = q.g;
        gv[3] = q.o;
      } else {
        const rnn_cell::GruFwd q = rnn_cell::gru_fwd(hpv, gx[0], gh[0], gx[1], gh[1], gx[2], gh[2]);
        hnew = q.h;
        auxv = gh[2];
        gv[0] = q.r;
        gv[1] = q.z;
        gv[2] = q.n;
      }
      const long o = ((long)t * N + n_own) * H + j;
      if (t + 1 < T)  // first: the other workgroups are waiting for it
        ex_store(p.ex + (long)(t & 1) * N * H + (long)n_own * H + j, hnew, (unsigned)(t + 1));
      p.out[o] = hnew;
      p.hp[o] = hpv;
      p.aux[o] = auxv;
      float* gs = p.gates + ((long)t * N + n_own) * G * H;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        gs[g * H + j] = gv[g];
        gx[g] = gnext[g];
      }
    }
    __syncthreads();  // Xs / part are free for the next step
  }
}

template <bool LSTM, int H, int NT>
__global__ __launch_bounds__(256) void rnn_rollout_bwd_kernel(RolloutParams p) {
  constexpr int G = LSTM ? 4 : 3;
  constexpr int GH = G * H;
  constexpr int SL = GH / RO_SLICES, PITCH = SL + 4, ROW = RO_SLICES * PITCH;
  static_assert(SL % 4 == 0, "slice of whole float4s");
  extern __shared__ __attribute__((aligned(16))) float ro_sm[];
  float* Xs = ro_sm;               // [NT][ROW]  dgh of this step
  float* part = ro_sm + NT * ROW;  // [NT][16 columns][RO_PP]
  const int tid = threadIdx.x;
  const int u = tid >> 4, sl = tid & 15;
  const int n_own = sl;
  if (!LSTM && blockIdx.x % p.spread) return;
  const int j = (LSTM ? blockIdx.x : blockIdx.x / p.spread) * RO_UNITS + u;
  const int N = p.N, T = p.T;
  const bool fin = n_own < N;

  float w[SL];  // row j of W_hh^T = column j of W_hh, slice sl of the GH gate rows
  {
    const float* row = p.w + (long)j * GH + sl * SL;
#pragma unroll
    for (int i4 = 0; i4 < SL / 4; ++i4) {
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(row + 4 * i4);
      w[4 * i4] = t4[0];
      w[4 * i4 + 1] = t4[1];
      w[4 * i4 + 2] = t4[2];
      w[4 * i4 + 3] = t4[3];
    }
  }
  float cr = (fin && p.dh_fin) ? p.dh_fin[(long)n_own * H + j] : 0.f;
  [[maybe_unused]] float dc = 0.f;  // LSTM: never leaves this thread
  if constexpr (LSTM) dc = (fin && p.dc_fin) ? p.dc_fin[(long)n_own * H + j] : 0.f;

  struct Saved {
    float g0, g1, g2, g3;  // the activated gates r, z, n | i, f, g, o
    float aux, prev;       // hn, hp (GRU) | c_t, c_{t-1} before the mask (LSTM)
    float d, mk;
  };
  auto load = [&](int t) {
    Saved s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (fin && t >= 0) {
      const long b = (long)t * N + n_own;
      const float* gs = p.gates + b * GH;
      s.g0 = gs[j];
      s.g1 = gs[H + j];
      s.g2 = gs[2 * H + j];
      if constexpr (LSTM) s.g3 = gs[3 * H + j];
      s.aux = p.aux[b * H + j];
      if constexpr (LSTM)
        s.prev = t > 0 ? p.aux[(b - N) * H + j] : p.c0[(long)n_own * H + j];
      else
        s.prev = p.hp[b * H + j];
      s.d = p.dout ? p.dout[b * H + j] : 0.f;
      s.mk = (float)p.mask[b];
    }
    return s;
  };
  Saved nxt = load(T - 1);

  for (int t = T - 1; t >= 0; --t) {
    const Saved cur = nxt;
    nxt = load(t - 1);
    [[maybe_unused]] float acc0 = 0.f;  // GRU: the direct path d * z of the carry
    if (fin) {
      // Nothing but the gate math comes before the ex_stores: the other workgroups wait for them.
      const float d = cur.d + cr;
      unsigned long long* e = p.ex + (long)(t & 1) * N * GH + (long)n_own * GH;
      const unsigned tag = (unsigned)(T - t);
      if constexpr (LSTM) {
        const rnn_cell::LstmBwd q =
            rnn_cell::lstm_bwd(d, cur.g0, cur.g1, cur.g2, cur.g3, cur.prev * cur.mk, cur.aux, dc);
        ex_store(e + j, q.di, tag);
        ex_store(e + H + j, q.df, tag);
        ex_store(e + 2 * H + j, q.dg, tag);
        ex_store(e + 3 * H + j, q.do_, tag);
        float* a = p.dgi + ((long)t * N + n_own) * GH;
        a[j] = q.di;
        a[H + j] = q.df;
        a[2 * H + j] = q.dg;
        a[3 * H + j] = q.do_;
        dc = q.dcp * cur.mk;
      } else {
        const rnn_cell::GruBwd q = rnn_cell::gru_bwd(d, cur.g0, cur.g1, cur.g2, cur.prev, cur.aux);
        ex_store(e + j, q.dr, tag);
        ex_store(e + H + j, q.dz, tag);
        ex_store(e + 2 * H + j, q.dgh_n, tag);
        const long b = (long)t * N + n_own;
        float* a = p.dgi + b * GH;
        a[j] = q.dr;
        a[H + j] = q.dz;
        a[2 * H + j] = q.dn;
        float* c = p.dgh + b * GH;
        c[j] = q.dr;
        c[H + j] = q.dz;
        c[2 * H + j] = q.dgh_n;
        acc0 = d * cur.g1;
      }
    }
    stage_exchanged<GH, NT, false>(Xs, p.ex + (long)(t & 1) * N * GH, (unsigned)(T - t), nullptr, N);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if (n < N) {
        float a0 = 0.f, a1 = 0.f;
        const float* xr = Xs + n * ROW + sl * PITCH;
#pragma unroll
        for (int i4 = 0; i4 < SL / 4; ++i4) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(xr + 4 * i4);
          a0 = fmaf(w[4 * i4], x[0], a0);
          a1 = fmaf(w[4 * i4 + 1], x[1], a1);
          a0 = fmaf(w[4 * i4 + 2], x[2], a0);
          a1 = fmaf(w[4 * i4 + 3], x[3], a1);
        }
        part[(n * RO_UNITS + u) * RO_PP + sl] = a0 + a1;
      }
    }
    __syncthreads();
    if (fin) {
      const float* pr = part + (n_own * RO_UNITS + u) * RO_PP;
      f32x4 s4 = *reinterpret_cast<const f32x4*>(pr);
#pragma unroll
      for (int q = 1; q < 4; ++q) s4 += *reinterpret_cast<const f32x4*>(pr + 4 * q);
      const float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      if constexpr (LSTM)
        cr = sum * cur.mk;
      else
        cr = (acc0 + sum) * cur.mk;
    }
    __syncthreads();  // Xs / part are free for the next step
  }
  if (fin) {
    p.dh0[(long)n_own * H + j] = cr;
    if constexpr (LSTM) p.dc0[(long)n_own * H + j] = dc;
  }
}

// dynamic LDS of one workgroup: the staged operand + the slice partials
constexpr size_t rollout_lds(bool lstm, int H, int NT, bool bwd) {
  const int G = lstm ? 4 : 3, K = bwd ? G * H : H;
  return (size_t)(NT * RO_SLICES * (K / RO_SLICES + 4) + (bwd ? 1 : G) * NT * RO_UNITS * RO_PP) * 4;
}
static_assert(rollout_lds(false, 512, 16, true) == 120 * 1024, "GRU backward, N > 8, H = 512");
static_assert(rollout_lds(true, 512, 16, true) == 152 * 1024, "LSTM backward, N > 8, H = 512");

template <bool LSTM, int H, int NT>
int launch_rollout(const RolloutParams& p, bool bwd, hipStream_t s) {
  constexpr int K = (LSTM ? 4 : 3) * H;
  const size_t lds = rollout_lds(LSTM, H, NT, bwd);
  static bool attr_f = false, attr_b = false;
  bool& done = bwd ? attr_b : attr_f;
  if (!done && lds > 48 * 1024) {
    const void* fn = bwd ? reinterpret_cast<const void*>(&rnn_rollout_bwd_kernel<LSTM, H, NT>)
                         : reinterpret_cast<const void*>(&rnn_rollout_fwd_kernel<LSTM, H, NT>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return 1;
    done = true;
  }
  const long words = 2L * 2 * p.N * (bwd ? K : H);  // [2][N][K] pairs as 32-bit words
  vlnce_zero(reinterpret_cast<float*>(p.ex), 1, (int)words, words, s);
  const dim3 grid(H / RO_UNITS * (LSTM ? 1 : p.spread));
  if (bwd)
    hipLaunchKernelGGL((rnn_rollout_bwd_kernel<LSTM, H, NT>), grid, dim3(256), lds, s, p);
  else
    hipLaunchKernelGGL((rnn_rollout_fwd_kernel<LSTM, H, NT>), grid, dim3(256), lds, s, p);
  return 0;
}

template <int H>
int launch_rollout_h(bool lstm, const RolloutParams& p, bool bwd, hipStream_t s) {
  if (p.N <= 8)
    return lstm ? launch_rollout<true, H, 8>(p, bwd, s) : launch_rollout<false, H, 8>(p, bwd, s);
  return lstm ? launch_rollout<true, H, 16>(p, bwd, s) : launch_rollout<false, H, 16>(p, bwd, s);
}

int dispatch_rollout(bool lstm, const RolloutParams& p, int H, bool bwd, vlnce_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (H) {
    case 64: return launch_rollout_h<64>(lstm, p, bwd, s);
    case 128: return launch_rollout_h<128>(lstm, p, bwd, s);
    case 256: return launch_rollout_h<256>(lstm, p, bwd, s);
    case 512: return launch_rollout_h<512>(lstm, p, bwd, s);
  }
  return 1;
}

// The H / 16 workgroups of a rollout launch hand each other the state every step: all of them must
// be RESIDENT at once (up to 152 KB of LDS each, i.e. one per CU).  That is a property of the
// device, queried once per device: a part that gives one workgroup less LDS than the (N, H)
// instance stages -- the larger of its two directions -- or that has fewer CUs than workgroups
// reports "unsupported", and the host takes the per-step kernels instead of a launch that would
// spin until its poll bound traps (round-3 ADVICE).
bool rollout_supported(bool lstm, int N, int H) {
  if (N <= 0 || N > RO_MAXN || !(H == 64 || H == 128 || H == 256 || H == 512)) return false;
  static int lds_max[16], cus[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  if (cus[dev] == 0) {
    int l = 0, c = 0;
    if (hipDeviceGetAttribute(&l, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return false;
    lds_max[dev] = l;
    cus[dev] = c > 0 ? c : -1;
  }
  const int NT = N <= 8 ? 8 : 16;
  const size_t f = rollout_lds(lstm, H, NT, false), b = rollout_lds(lstm, H, NT, true);
  return lds_max[dev] > 0 && (size_t)lds_max[dev] >= (f > b ? f : b) && cus[dev] >= H / RO_UNITS;
}

int rollout_spread() { return vlnce_opt(VLNCE_OPT_ROLLOUT_ONE_XCD) ? 8 : 1; }  // a GRU-only experiment

}  // namespace

extern "C" int vlnce_gru_rollout_supported(int N, int H) { return rollout_supported(false, N, H); }
extern "C" int vlnce_lstm_rollout_supported(int N, int H) { return rollout_supported(true, N, H); }

extern "C" long vlnce_gru_rollout_workspace_bytes(int N, int H) {
  return rollout_supported(false, N, H) ? 2L * N * 3 * H * 8 : 0;
}
extern "C" long vlnce_lstm_rollout_workspace_bytes(int N, int H) {
  return rollout_supported(true, N, H) ? 2L * N * 4 * H * 8 : 0;
}

extern "C" int vlnce_gru_rollout_fwd(const float* gi, const float* h0, const uint8_t* mask,
                                     const float* w_hh, const float* b_hh, float* hp, float* out,
                                     float* gates, float* aux, void* workspace, int T, int N,
                                     int H, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(gi && h0 && mask && w_hh && b_hh && hp && out && gates && aux && workspace,
                  "gru_rollout_fwd: null argument");
  VLNCE_CHECK_ARG(T > 0, "gru_rollout_fwd: T must be positive");
  VLNCE_CHECK_ARG(rollout_supported(false, N, H), "gru_rollout_fwd: unsupported N/H (%d,%d)", N, H);
  const RolloutParams p{.gi = gi, .h0 = h0, .mask = mask, .w = w_hh, .b_hh = b_hh, .hp = hp,
                        .out = out, .gates = gates, .aux = aux,
                        .ex = static_cast<unsigned long long*>(workspace), .T = T, .N = N,
                        .spread = rollout_spread()};
  VLNCE_CHECK_ARG(dispatch_rollout(false, p, H, false, stream) == 0,
                  "gru_rollout_fwd: no kernel for H=%d", H);
  VLNCE_CHECK_LAUNCH("gru_rollout_fwd");
  return 0;
}

extern "C" int vlnce_gru_rollout_bwd(const float* dout, const float* dh_final, const float* gates,
                                     const float* aux, const float* hp, const uint8_t* mask,
                                     const float* w_hh_t, float* dgi, float* dgh, float* dh0,
                                     void* workspace, int T, int N, int H,
                                     vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(gates && aux && hp && mask && w_hh_t && dgi && dgh && dh0 && workspace,
                  "gru_rollout_bwd: null argument");
  VLNCE_CHECK_ARG(T > 0, "gru_rollout_bwd: T must be positive");
  VLNCE_CHECK_ARG(rollout_supported(false, N, H), "gru_rollout_bwd: unsupported N/H (%d,%d)", N, H);
  const RolloutParams p{.mask = mask, .w = w_hh_t, .hp = const_cast<float*>(hp),
                        .gates = const_cast<float*>(gates), .aux = const_cast<float*>(aux),
                        .dout = dout, .dh_fin = dh_final, .dgi = dgi, .dh0 = dh0,
                        .ex = static_cast<unsigned long long*>(workspace), .T = T, .N = N,
                        .spread = rollout_spread(), .dgh = dgh};
  VLNCE_CHECK_ARG(dispatch_rollout(false, p, H, true, stream) == 0,
                  "gru_rollout_bwd: no kernel for H=%d", H);
  VLNCE_CHECK_LAUNCH("gru_rollout_bwd");
  return 0;
}

extern "C" int vlnce_lstm_rollout_fwd(const float* gi, const float* h0, const float* c0,
                                      const uint8_t* mask, const float* w_hh, const float* b_hh,
                                      float* hp, float* out, float* gates, float* aux,
                                      void* workspace, int T, int N, int H, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(gi && h0 && c0 && mask && w_hh && b_hh && hp && out && gates && aux && workspace,
                  "lstm_rollout_fwd: null argument");
  VLNCE_CHECK_ARG(T > 0, "lstm_rollout_fwd: T must be positive");
  VLNCE_CHECK_ARG(rollout_supported(true, N, H), "lstm_rollout_fwd: unsupported N/H (%d,%d)", N, H);
  const RolloutParams p{.gi = gi, .h0 = h0, .c0 = c0, .mask = mask, .w = w_hh, .b_hh = b_hh,
                        .hp = hp, .out = out, .gates = gates, .aux = aux,
                        .ex = static_cast<unsigned long long*>(workspace), .T = T, .N = N,
                        .spread = 1};
  VLNCE_CHECK_ARG(dispatch_rollout(true, p, H, false, stream) == 0,
                  "lstm_rollout_fwd: no kernel for H=%d", H);
  VLNCE_CHECK_LAUNCH("lstm_rollout_fwd");
  return 0;
}

extern "C" int vlnce_lstm_rollout_bwd(const float* dout, const float* dh_final, const float* dc_final,
                                      const float* gates, const float* aux, const float* hp,
                                      const float* c0, const uint8_t* mask, const float* w_hh_t,
                                      float* dgi, float* dh0, float* dc0, void* workspace, int T,
                                      int N, int H, vlnce_stream_t stream) {
  VLNCE_CHECK_ARG(gates && aux && hp && c0 && mask && w_hh_t && dgi && dh0 && dc0 && workspace,
                  "lstm_rollout_bwd: null argument");
  VLNCE_CHECK_ARG(T > 0, "lstm_rollout_bwd: T must be positive");
  VLNCE_CHECK_ARG(rollout_supported(true, N, H), "lstm_rollout_bwd: unsupported N/H (%d,%d)", N, H);
  const RolloutParams p{.c0 = c0, .mask = mask, .w = w_hh_t, .hp = const_cast<float*>(hp),
                        .gates = const_cast<float*>(gates), .aux = const_cast<float*>(aux),
                        .dout = dout, .dh_fin = dh_final, .dc_fin = dc_final, .dgi = dgi, .dh0 = dh0,
                        .dc0 = dc0, .ex = static_cast<unsigned long long*>(workspace), .T = T,
                        .N = N, .spread = 1};
  VLNCE_CHECK_ARG(dispatch_rollout(true, p, H, true, stream) == 0,
                  "lstm_rollout_bwd: no kernel for H=%d", H);
  VLNCE_CHECK_LAUNCH("lstm_rollout_bwd");
  return 0;
}
