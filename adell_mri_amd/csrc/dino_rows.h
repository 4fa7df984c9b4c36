// What the row kernels of the DINO loss share between csrc/dino.hip (dense rows) and csrc/ibot.hip
// (rows read in place through a table): the span of a chunk, the online accumulators and their
// merge, the (row, chunk) body of the forward, the element of the backward, and the launch of the
// merge kernels, which live in dino.hip.
#pragma once
#include "common.h"

constexpr int DN_NT = 256;
constexpr float DN_NEG = -3.0e38f;   // "no element yet": finite, so that (m - m) is 0 and not NaN
constexpr int DN_CHUNK_Q = 1024;     // chunk lengths are multiples of this
constexpr int DN_BLOCKS = 512;       // blocks the plan aims at (two per CU)

// Elements [0, n) of a chunk that starts at p0: scalars [0, head), float4 at head + 4 i for
// i < nvec, scalars from head + 4 nvec on. vec false: everything scalar.
struct DnSpan {
  int n, head, nvec;
};
__device__ __forceinline__ DnSpan dn_span(const float* p0, int n, bool vec) {
  DnSpan s;
  s.n = n;
  int head = (int)(((16u - (unsigned)((uintptr_t)p0 & 15u)) & 15u) >> 2);
  head = head < n ? head : n;
  s.head = vec ? head : n;
  s.nvec = (n - s.head) >> 2;
  return s;
}
__device__ __forceinline__ bool dn_same16(const void* a, const void* b) {
  return ((((uintptr_t)a) ^ ((uintptr_t)b)) & 15u) == 0;
}
__device__ __forceinline__ f32x4 dn_ld4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v = {p[0], p[1], p[2], p[3]};
  return v;
}

// (m, z, w) <- the sums of two runs, each relative to its own maximum
__device__ __forceinline__ void dn_comb(float& m, float& z, float& w, float m2, float z2, float w2) {
  const float mn = fmaxf(m, m2);
  const float f1 = __expf(m - mn), f2 = __expf(m2 - mn);
  z = z * f1 + z2 * f2;
  w = w * f1 + w2 * f2;
  m = mn;
}

struct DnAcc {
  float ms, zs, mt, zt, w;
};
__device__ __forceinline__ void dn_acc_comb(DnAcc& a, const DnAcc& b) {
  float unused = 0.f;
  dn_comb(a.ms, a.zs, unused, b.ms, b.zs, 0.f);
  dn_comb(a.mt, a.zt, a.w, b.mt, b.zt, b.w);
}
__device__ __forceinline__ DnAcc dn_acc_wave(DnAcc a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    DnAcc b;
    b.ms = __shfl_xor(a.ms, o, 64);
    b.zs = __shfl_xor(a.zs, o, 64);
    b.mt = __shfl_xor(a.mt, o, 64);
    b.zt = __shfl_xor(a.zt, o, 64);
    b.w = __shfl_xor(a.w, o, 64);
    dn_acc_comb(a, b);
  }
  return a;
}

template <bool SCORES>
__device__ __forceinline__ void dn_acc_one(DnAcc& acc, float av, float bv, float cv, float it1,
                                           float it2) {
  const float x = av * it1;
  const float mn = fmaxf(acc.ms, x);
  acc.zs = acc.zs * __expf(acc.ms - mn) + __expf(x - mn);
  acc.ms = mn;
  if (SCORES) {
    acc.zt += bv;
    acc.w += bv * av;
  } else {
    const float y = (bv - cv) * it2;
    const float mt = fmaxf(acc.mt, y);
    const float f = __expf(acc.mt - mt), e = __expf(y - mt);
    acc.zt = acc.zt * f + e;
    acc.w = acc.w * f + e * av;
    acc.mt = mt;
  }
}

template <bool SCORES>
__device__ __forceinline__ void dn_acc_four(DnAcc& acc, f32x4 av, f32x4 bv, f32x4 cv, float it1,
                                            float it2) {
  const f32x4 x = av * it1;
  const float mn = fmaxf(fmaxf(acc.ms, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
  acc.zs = acc.zs * __expf(acc.ms - mn) +
           ((__expf(x[0] - mn) + __expf(x[1] - mn)) + (__expf(x[2] - mn) + __expf(x[3] - mn)));
  acc.ms = mn;
  if (SCORES) {
    acc.zt += (bv[0] + bv[1]) + (bv[2] + bv[3]);
    acc.w += (bv[0] * av[0] + bv[1] * av[1]) + (bv[2] * av[2] + bv[3] * av[3]);
  } else {
    const f32x4 y = (bv - cv) * it2;
    const float mt = fmaxf(fmaxf(acc.mt, fmaxf(y[0], y[1])), fmaxf(y[2], y[3]));
    const float f = __expf(acc.mt - mt);
    const float e0 = __expf(y[0] - mt), e1 = __expf(y[1] - mt), e2 = __expf(y[2] - mt),
                e3 = __expf(y[3] - mt);
    acc.zt = acc.zt * f + ((e0 + e1) + (e2 + e3));
    acc.w = acc.w * f + ((e0 * av[0] + e1 * av[1]) + (e2 * av[2] + e3 * av[3]));
    acc.mt = mt;
  }
}

// One (row, chunk) block of DN_NT threads: the five partials (m_s, Z_s, m_t, Z_t, W) of the n
// elements at ap (student), bp (teacher) and cp (centres of the chunk, or null) go to o[0..5).
template <bool SCORES>
__device__ __forceinline__ void dn_loss_part_body(const float* __restrict__ ap,
                                                  const float* __restrict__ bp,
                                                  const float* __restrict__ cp, int n, float it1,
                                                  float it2, float* __restrict__ o) {
  const int tid = threadIdx.x;
  const DnSpan sp = dn_span(ap, n, dn_same16(ap, bp));
  const bool cvec = cp != nullptr && dn_same16(ap, cp);
  DnAcc acc = {DN_NEG, 0.f, DN_NEG, 0.f, 0.f};
  for (int k = tid; k < sp.head; k += DN_NT)
    dn_acc_one<SCORES>(acc, ap[k], bp[k], cp ? cp[k] : 0.f, it1, it2);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < sp.nvec; i += DN_NT) {
    const int k = sp.head + 4 * i;
    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + k);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + k);
    const f32x4 cv = cp ? dn_ld4(cp + k, cvec) : zero;
    dn_acc_four<SCORES>(acc, av, bv, cv, it1, it2);
  }
  for (int k = sp.head + 4 * sp.nvec + tid; k < sp.n; k += DN_NT)
    dn_acc_one<SCORES>(acc, ap[k], bp[k], cp ? cp[k] : 0.f, it1, it2);

  acc = dn_acc_wave(acc);
  __shared__ DnAcc wave_part[DN_NT / 64];
  if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    DnAcc t = wave_part[0];
#pragma unroll
    for (int w = 1; w < DN_NT / 64; ++w) dn_acc_comb(t, wave_part[w]);
    o[0] = t.ms;
    o[1] = t.zs;
    o[2] = t.mt;
    o[3] = t.zt;
    o[4] = t.w;
  }
}

template <bool SCORES>
__device__ __forceinline__ void dn_bwd_one(float av, float bv, float cv, float it1, float it2,
                                           float lse_s, float second, float abar, float g, float& da,
                                           float& db) {
  const float ls = av * it1 - lse_s;
  const float ps = __expf(ls);
  const float pt = SCORES ? bv : __expf((bv - cv) * it2 - second);
  const float sum_p = SCORES ? second : 1.0f;
  da = g * (ps * sum_p - pt) * it1;
  db = -g * pt * ((av - abar) * it1) * it2;
}

// The merge of the partials of R rows (dino.hip): stats [R][4], loss_rows [R] and, with loss_mean,
// the mean of the rows in a fixed order. R <= 65535.
int dn_launch_merge(const float* part, int R, int chunks, int teacher_is_scores, float t1,
                    float* loss_rows, float* stats, float* loss_mean, hipStream_t st);
