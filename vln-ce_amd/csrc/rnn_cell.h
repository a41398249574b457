// The GRU / LSTM cell arithmetic (torch gate order), once: on scalars, for one hidden unit of one
// row.  Every kernel that computes a cell -- the gates kernels and the fused step kernels of
// rnn.hip, the one-launch rollouts of rnn_rollout.hip -- calls these, so "the rollout equals the
// step launches up to the summation order of gh" holds by construction.  The callers own the
// loads, the stores, the mask and what they carry between steps.
// (rnn_seq.hip keeps its own sigm / tanh_fast: different arithmetic on purpose.)
#pragma once
#include <hip/hip_runtime.h>

namespace rnn_cell {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// gx*: x W_ih^T + b_ih; gh*: hp W_hh^T + b_hh; hp: the masked previous state
struct GruFwd {
  float r, z, n, h;
};
__device__ __forceinline__ GruFwd gru_fwd(float hp, float gx_r, float gh_r, float gx_z,
                                          float gh_z, float gx_n, float gh_n) {
  GruFwd o;
  o.r = sigm(gx_r + gh_r);
  o.z = sigm(gx_z + gh_z);
  o.n = tanhf(gx_n + o.r * gh_n);
  o.h = (1.f - o.z) * o.n + o.z * hp;
  return o;
}

// d: gradient of h; hp: the masked previous state; hn: the saved gh_n.  dgi = (dr, dz, dn), dgh = (dr, dz, dgh_n); the direct
// path to the previous state, d * z, stays with the caller's carry.
struct GruBwd {
  float dr, dz, dn, dgh_n;
};
__device__ __forceinline__ GruBwd gru_bwd(float d, float r, float z, float n, float hp, float hn) {
  const float dn = d * (1.f - z);
  const float dz = d * (hp - n);
  const float dnp = dn * (1.f - n * n);
  const float dr = dnp * hn;
  GruBwd o;
  o.dr = dr * r * (1.f - r);
  o.dz = dz * z * (1.f - z);
  o.dn = dnp;
  o.dgh_n = dnp * r;
  return o;
}

// g*: gi + gh per gate (i, f, g, o); cp: the masked previous cell state
struct LstmFwd {
  float i, f, g, o, c, h;
};
__device__ __forceinline__ LstmFwd lstm_fwd(float cp, float g_i, float g_f, float g_g, float g_o) {
  LstmFwd o;
  o.i = sigm(g_i);
  o.f = sigm(g_f);
  o.g = tanhf(g_g);
  o.o = sigm(g_o);
  o.c = o.f * cp + o.i * o.g;
  o.h = o.o * tanhf(o.c);
  return o;
}

// d / dc: gradients of h_t / c_t; c: the saved c_t; cp: the masked c_{t-1}.  di..do_ are the
// pre-activation gate gradients; dcp = dc_t * f is the gradient of cp (the caller masks it).
struct LstmBwd {
  float di, df, dg, do_, dcp;
};
__device__ __forceinline__ LstmBwd lstm_bwd(float d, float i, float f, float g, float o, float cp,
                                            float c, float dc) {
  const float tc = tanhf(c);
  const float dcc = dc + d * o * (1.f - tc * tc);
  LstmBwd b;
  b.di = dcc * g * i * (1.f - i);
  b.df = dcc * cp * f * (1.f - f);
  b.dg = dcc * i * (1.f - g * g);
  b.do_ = d * tc * o * (1.f - o);
  b.dcp = dcc * f;
  return b;
}

}  // namespace rnn_cell
