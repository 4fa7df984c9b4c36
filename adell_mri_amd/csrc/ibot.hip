// Kernels of iBOT pretraining (adell_mri/modules/self_supervised/ibot.py, iBOTPL in pl.py): the
// masked-token objective on the prototype logits of EVERY token, s and y [B][Tt][K] (Tt = class
// token + T patch tokens). House rules of dino.hip: fp32 in and out, wave64 reductions in a fixed
// order, no float atomics -- two runs are bit-identical; rows of K floats start at any 4-byte
// address (dino_rows.h: scalar head, float4 body, scalar tail).
//   * splice: the learnable mask token written over the rows idx[0..M) (sorted, unique) of every
//     item of the embedded sequence [B][N][E], out of place; the backward zeroes those rows and sums
//     them into the token's gradient, four waves over the (item, j) pairs merged in order.
//   * token sums: out[b][k] = scale sum_{t >= first} x[b][t][k], one read of x: the "mean" reduction
//     and, unscaled and in fp64, the per-item part of the centre sum of the masked-token loss. One wave owns 256
//     columns; while B K / 256 waves do not fill the chip the token axis is split over blocks
//     (adell_ibot_token_sums_plan) and a second launch adds the partial sums in order.
//   * masked-row loss: DinoLoss over the rows (b, rows[j]) read in place through an int32 table --
//     the accumulators, partials, plan and merge of the dense loss (dn_loss_part_body,
//     adell_dino_loss_plan(B M, K), dn_launch_merge); only [B M][4] statistics are saved.
//   * one-writer backward: every element of ds [B][Tt][K] written exactly once -- the gradient of
//     the reduced output ("cls": the class row; "mean": every patch row, / T) plus, on a masked row,
//     the loss gradient recomputed from the statistics; rows with neither are written as zeros.
#include "dino_rows.h"

// ---- mask-token splice ----------------------------------------------------------------------------
__device__ __forceinline__ bool ib_masked(const int* __restrict__ idx, int M, int n) {
  int lo = 0, hi = M;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < n) lo = mid + 1;
    else hi = mid;
  }
  return lo < M && idx[lo] == n;
}

// One wave per (item, token) row of E floats, four rows per block. token null: zeros (backward).
template <bool VEC>
__global__ __launch_bounds__(256) void adell_ibot_splice_kernel(
    const float* __restrict__ x, const int* __restrict__ idx, const float* __restrict__ token,
    long rows, int N, int E, int M, float* __restrict__ y) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bool masked = ib_masked(idx, M, (int)(row % N));
  const float* xp = x + row * E;
  float* yp = y + row * E;
  if (VEC) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < (E >> 2); i += 64) {
      f32x4 v;
      if (masked) v = token ? reinterpret_cast<const f32x4*>(token)[i] : zero;
      else v = reinterpret_cast<const f32x4*>(xp)[i];
      reinterpret_cast<f32x4*>(yp)[i] = v;
    }
  } else {
    for (int e = lane; e < E; e += 64) yp[e] = masked ? (token ? token[e] : 0.f) : xp[e];
  }
}

// dtoken[e] = sum_b sum_j dy[b][idx[j]][e]: 64 columns per block, wave w takes the pairs
// r = b M + j with r % 4 == w in order, the four sums are added in the order of w.
__global__ __launch_bounds__(256) void adell_ibot_splice_dtoken_kernel(
    const float* __restrict__ dy, const int* __restrict__ idx, int B, int N, int E, int M,
    float* __restrict__ dtoken) {
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
  __shared__ float part[4][64];
  float acc = 0.f;
  if (e < E) {
    const int R = B * M;
    for (int r = wave; r < R; r += 4) {
      const int b = r / M, j = r - b * M;
      acc += dy[((size_t)b * N + idx[j]) * E + e];
    }
  }
  part[wave][threadIdx.x & 63] = acc;
  __syncthreads();
  if (wave == 0 && e < E)
    dtoken[e] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) +
                part[3][threadIdx.x];
}

static int ib_splice_args(const char* what, const void* x, const int* idx, int B, int N, int E,
                          int M) {
  ADELL_REQUIRE(x && idx && B > 0 && N > 0 && E > 0 && M > 0 && M <= N,
                "%s: bad arguments (1 <= M <= N)", what);
  ADELL_REQUIRE((long)B * N <= 0x7fffffffL,
                "%s: too many rows", what);
  return ADELL_OK;
}

extern "C" int adell_ibot_mask_tokens_fwd(const float* x, const int* idx, const float* token, int B,
                                          int N, int E, int M, float* y, void* stream) {
  const int rc = ib_splice_args("ibot_mask_tokens_fwd", x, idx, B, N, E, M);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(token && y, "ibot_mask_tokens_fwd: null token / output");
  const long rows = (long)B * N;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool vec = (E % 4 == 0) && adell_aligned16(x) && adell_aligned16(y) && adell_aligned16(token);
  if (vec)
    hipLaunchKernelGGL(adell_ibot_splice_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, idx,
                       token, rows, N, E, M, y);
  else
    hipLaunchKernelGGL(adell_ibot_splice_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, idx,
                       token, rows, N, E, M, y);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_ibot_mask_tokens_bwd(const float* dy, const int* idx, int B, int N, int E, int M,
                                          float* dx, float* dtoken, void* stream) {
  const int rc = ib_splice_args("ibot_mask_tokens_bwd", dy, idx, B, N, E, M);
  if (rc != ADELL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    const long rows = (long)B * N;
    const dim3 grid((unsigned)((rows + 3) / 4));
    const bool vec = (E % 4 == 0) && adell_aligned16(dy) && adell_aligned16(dx);
    if (vec)
      hipLaunchKernelGGL(adell_ibot_splice_kernel<true>, grid, dim3(256), 0, st, dy, idx,
                         (const float*)nullptr, rows, N, E, M, dx);
    else
      hipLaunchKernelGGL(adell_ibot_splice_kernel<false>, grid, dim3(256), 0, st, dy, idx,
                         (const float*)nullptr, rows, N, E, M, dx);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  if (dtoken) {
    hipLaunchKernelGGL(adell_ibot_splice_dtoken_kernel, dim3((unsigned)adell_cdiv(E, 64)), dim3(256), 0,
                       st, dy, idx, B, N, E, M, dtoken);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  return ADELL_OK;
}

// ---- token sums -----------------------------------------------------------------------------------
constexpr int IB_SUM_WAVES = 2048;   // one-wave blocks the plan aims at (eight per CU)
constexpr int IB_SUM_MIN_T = 8;      // a split keeps at least this many tokens

// out = {splits S, tokens per split}: split s covers tokens [s per, min(T, (s + 1) per)) of the T
extern "C" int adell_ibot_token_sums_plan(int B, int T, int K, int* out) {
  ADELL_REQUIRE(out && B > 0 && T > 0 && K > 0, "ibot_token_sums_plan: bad arguments");
  const long waves = (long)B * adell_cdiv(K, 256);
  long S = waves >= IB_SUM_WAVES ? 1 : (IB_SUM_WAVES + waves - 1) / waves;
  const long most = adell_cdiv(T, IB_SUM_MIN_T);
  S = S < most ? S : most;
  const int per = adell_cdiv(T, (int)S);
  out[0] = adell_cdiv(T, per);
  out[1] = per;
  return ADELL_OK;
}

// The sums are accumulated and kept in fp64: a centre is a sum over thousands of logits of either
// sign, and where it nearly cancels an fp32 partial sum leaves an error of one ulp of the ADDENDS
// (1e-7), three digits of a centre of 1e-4. The adds hide behind the loads.
// grid (column blocks, S, B), one wave per block. S == 1: out[b][k] = scale sum (fp32),
// raw[b][k] = sum (fp64, may be null); S > 1: part [B][S][K] takes the sums of the split.
template <bool VEC>
__global__ __launch_bounds__(64) void adell_ibot_token_sums_kernel(
    const float* __restrict__ x, int Tt, int K, int first, int per, float scale,
    float* __restrict__ out, double* __restrict__ raw, double* __restrict__ part) {
  const int b = blockIdx.z, s = blockIdx.y, S = gridDim.y;
  const int t0 = first + s * per;
  const int t1 = (t0 + per) < Tt ? (t0 + per) : Tt;
  const float* xb = x + (size_t)b * Tt * K;
  const int q = blockIdx.x * 64 + threadIdx.x;
  constexpr int W = VEC ? 4 : 1;
  if (q >= (VEC ? (K >> 2) : K)) return;
  double acc[W];
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.0;
  if (VEC) {
    const int KQ = K >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xb) + q;
#pragma unroll 8
    for (int t = t0; t < t1; ++t) {
      const f32x4 v = x4[(size_t)t * KQ];
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] += (double)v[i];
    }
  } else {
#pragma unroll 8
    for (int t = t0; t < t1; ++t) acc[0] += (double)xb[(size_t)t * K + q];
  }
  const size_t k = (size_t)q * W;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    if (S == 1) {
      out[(size_t)b * K + k + i] = (float)(acc[i] * (double)scale);
      if (raw) raw[(size_t)b * K + k + i] = acc[i];
    } else {
      part[((size_t)b * S + s) * K + k + i] = acc[i];
    }
  }
}

__global__ __launch_bounds__(256) void adell_ibot_token_sums_merge_kernel(
    const double* __restrict__ part, long total, int K, int S, float scale, float* __restrict__ out,
    double* __restrict__ raw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long b = i / K;
  const int k = (int)(i - b * K);
  const double* p = part + (size_t)b * S * K + k;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += p[(size_t)s * K];
  out[i] = (float)(acc * (double)scale);
  if (raw) raw[i] = acc;
}

extern "C" long adell_ibot_token_sums_workspace_doubles(int B, int T, int K) {
  int plan[2];
  if (adell_ibot_token_sums_plan(B, T, K, plan) != ADELL_OK) return 0;
  return plan[0] > 1 ? (long)B * plan[0] * K : 0;
}

extern "C" int adell_ibot_token_sums(const float* x, int B, int Tt, int K, int first, float scale,
                                     double* workspace, long workspace_doubles, float* out,
                                     double* raw, void* stream) {
  ADELL_REQUIRE(x && out && B > 0 && Tt > 0 && K > 0 && first >= 0 && first < Tt && B <= 65535,
                "ibot_token_sums: bad arguments (0 <= first < tokens, B <= 65535)");
  int plan[2];
  adell_ibot_token_sums_plan(B, Tt - first, K, plan);
  const int S = plan[0];
  const long need = S > 1 ? (long)B * S * K : 0;
  ADELL_REQUIRE(workspace_doubles >= need && (need == 0 || workspace),
                "ibot_token_sums: workspace of %ld doubles, the plan needs %ld", workspace_doubles,
                need);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (K % 4 == 0) && adell_aligned16(x);
  if (vec)
    hipLaunchKernelGGL(adell_ibot_token_sums_kernel<true>,
                       dim3((unsigned)adell_cdiv(K >> 2, 64), (unsigned)S, (unsigned)B), dim3(64), 0, st,
                       x, Tt, K, first, plan[1], scale, out, raw, workspace);
  else
    hipLaunchKernelGGL(adell_ibot_token_sums_kernel<false>,
                       dim3((unsigned)adell_cdiv(K, 64), (unsigned)S, (unsigned)B), dim3(64), 0, st, x,
                       Tt, K, first, plan[1], scale, out, raw, workspace);
  ADELL_CHECK_HIP(hipGetLastError());
  if (S > 1) {
    const long total = (long)B * K;
    hipLaunchKernelGGL(adell_ibot_token_sums_merge_kernel, dim3((unsigned)((total + 255) / 256)),
                       dim3(256), 0, st, (const double*)workspace, total, K, S, scale, out, raw);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  return ADELL_OK;
}

// out[k] = (float) sum_r sums[r][k] over the R rows of fp64 token sums (the items of every view), in
// order: the pending centre sum of the masked-token loss.
__global__ __launch_bounds__(256) void adell_ibot_center_sum_kernel(const double* __restrict__ sums,
                                                                    int R, int K,
                                                                    float* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double acc = 0.0;
  for (int r = 0; r < R; ++r) acc += sums[(size_t)r * K + k];
  out[k] = (float)acc;
}

extern "C" int adell_ibot_center_sum(const double* sums, int R, int K, float* out, void* stream) {
  ADELL_REQUIRE(sums && out && R > 0 && K > 0, "ibot_center_sum: bad arguments");
  hipLaunchKernelGGL(adell_ibot_center_sum_kernel, dim3((unsigned)adell_cdiv(K, 256)), dim3(256), 0,
                     (hipStream_t)stream, sums, R, K, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---- masked-row loss forward ------------------------------------------------------------------------
// grid (chunks, B M): row r = b M + j reads s (and, in centre mode, y) at token rows[j] of item b;
// given scores are the dense [B M][K] rows.
template <bool SCORES>
__global__ __launch_bounds__(DN_NT) void adell_ibot_loss_part_kernel(
    const float* __restrict__ s, const float* __restrict__ y, const float* __restrict__ c,
    const int* __restrict__ rows, int M, int Tt, int K, int len, float it1, float it2,
    float* __restrict__ part) {
  const int r = blockIdx.y, chunk = blockIdx.x;
  const int b = r / M, j = r - b * M;
  const size_t row = (size_t)b * Tt + rows[j];
  const int k0 = chunk * len;
  const int n = (K - k0) < len ? (K - k0) : len;
  const float* ap = s + row * K + k0;
  const float* bp = y + (SCORES ? (size_t)r : row) * K + k0;
  const float* cp = (SCORES || c == nullptr) ? nullptr : c + k0;
  dn_loss_part_body<SCORES>(ap, bp, cp, n, it1, it2, part + ((size_t)r * gridDim.x + chunk) * 5);
}

static int ib_loss_args(const char* what, const float* s, const float* y, int B, int Tt, int K, int M,
                        float t1, float t2) {
  ADELL_REQUIRE(s && y && B > 0 && Tt > 0 && K > 0 && M > 0 && M <= Tt,
                "%s: bad arguments (1 <= M <= tokens)", what);
  ADELL_REQUIRE((long)B * M <= 65535, "%s: %ld masked rows (at most 65535)", what, (long)B * M);
  ADELL_REQUIRE((long)B * Tt <= 0x7fffffffL, "%s: too many rows", what);
  ADELL_REQUIRE(t1 > 0.f && t2 > 0.f, "%s: temperatures must be positive", what);
  return ADELL_OK;
}

extern "C" int adell_ibot_loss_fwd(const float* s, const float* y, const float* centers,
                                   const int* rows, int B, int Tt, int K, int M, float t1, float t2,
                                   int teacher_is_scores, float* workspace, long workspace_floats,
                                   float* loss_rows, float* stats, float* loss_mean, void* stream) {
  const int rc = ib_loss_args("ibot_loss_fwd", s, y, B, Tt, K, M, t1, t2);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(rows && workspace && loss_rows && stats, "ibot_loss_fwd: null table / output");
  const int R = B * M;
  int plan[2];
  adell_dino_loss_plan(R, K, plan);
  ADELL_REQUIRE(workspace_floats >= (long)R * plan[0] * 5,
                "ibot_loss_fwd: workspace of %ld floats, the plan needs %ld", workspace_floats,
                (long)R * plan[0] * 5);
  const dim3 grid((unsigned)plan[0], (unsigned)R);
  const float it1 = (float)(1.0 / (double)t1), it2 = (float)(1.0 / (double)t2);
  hipStream_t st = (hipStream_t)stream;
  if (teacher_is_scores)
    hipLaunchKernelGGL(adell_ibot_loss_part_kernel<true>, grid, dim3(DN_NT), 0, st, s, y,
                       (const float*)nullptr, rows, M, Tt, K, plan[1], it1, it2, workspace);
  else
    hipLaunchKernelGGL(adell_ibot_loss_part_kernel<false>, grid, dim3(DN_NT), 0, st, s, y, centers,
                       rows, M, Tt, K, plan[1], it1, it2, workspace);
  ADELL_CHECK_HIP(hipGetLastError());
  return dn_launch_merge(workspace, R, plan[0], teacher_is_scores, t1, loss_rows, stats, loss_mean, st);
}

// ---- one-writer student backward ------------------------------------------------------------------
// grid (B Tt, chunks): the chunk [k0, k0 + n) of row (b, t) of ds. cr: the factor of d_red[b][:] in
// this row (0: none). j = inv[t] >= 0: masked row r = b M + j.
template <bool SCORES>
__global__ __launch_bounds__(DN_NT) void adell_ibot_bwd_kernel(
    const float* __restrict__ s, const float* __restrict__ y, const float* __restrict__ c,
    const float* __restrict__ stats, const int* __restrict__ inv, const float* __restrict__ d_red,
    const float* __restrict__ g_all, float g_scale, int M, int Tt, int K, int len, int first,
    int red_cls, float red_scale, float it1, float it2, float* __restrict__ ds) {
  const size_t row = blockIdx.x;
  const int b = (int)(row / Tt), t = (int)(row - (size_t)b * Tt), tid = threadIdx.x;
  const int k0 = blockIdx.y * len;
  const int n = (K - k0) < len ? (K - k0) : len;
  const int j = (inv != nullptr && g_all != nullptr) ? inv[t] : -1;
  float cr = 0.f;
  if (d_red != nullptr) cr = red_cls ? (t == 0 ? 1.f : 0.f) : (t >= first ? red_scale : 0.f);
  float* dsp = ds + row * K + k0;
  const float* drp = cr != 0.f ? d_red + (size_t)b * K + k0 : nullptr;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (j < 0) {   // (uniform over the block)
    const DnSpan sp = dn_span(dsp, n, drp == nullptr || dn_same16(dsp, drp));
    const int tail = sp.head + 4 * sp.nvec;
    for (int k = tid; k < sp.head + (sp.n - tail); k += DN_NT) {
      const int e = k < sp.head ? k : k - sp.head + tail;
      dsp[e] = drp ? cr * drp[e] : 0.f;
    }
    for (int i = tid; i < sp.nvec; i += DN_NT) {
      const int k = sp.head + 4 * i;
      *reinterpret_cast<f32x4*>(dsp + k) = drp ? *reinterpret_cast<const f32x4*>(drp + k) * cr : zero;
    }
    return;
  }
  const int r = b * M + j;
  const float* ap = s + row * K + k0;
  const float* bp = y + (SCORES ? (size_t)r : row) * K + k0;
  const float* cp = (SCORES || c == nullptr) ? nullptr : c + k0;
  const bool same = dn_same16(ap, bp) && dn_same16(ap, dsp) && (drp == nullptr || dn_same16(ap, drp));
  const DnSpan sp = dn_span(ap, n, same);
  const bool cvec = cp != nullptr && dn_same16(ap, cp);
  const float lse_s = stats[r * 4 + 0], second = stats[r * 4 + 1], abar = stats[r * 4 + 3];
  const float g = g_all[0] * g_scale;
  const int tail = sp.head + 4 * sp.nvec;
  for (int k = tid; k < sp.head + (sp.n - tail); k += DN_NT) {   // scalar head, then scalar tail
    const int e = k < sp.head ? k : k - sp.head + tail;
    float x, unused;
    dn_bwd_one<SCORES>(ap[e], bp[e], cp ? cp[e] : 0.f, it1, it2, lse_s, second, abar, g, x, unused);
    dsp[e] = drp ? x + cr * drp[e] : x;
  }
  for (int i = tid; i < sp.nvec; i += DN_NT) {
    const int k = sp.head + 4 * i;
    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + k);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + k);
    const f32x4 cv = cp ? dn_ld4(cp + k, cvec) : zero;
    const f32x4 dv = drp ? *reinterpret_cast<const f32x4*>(drp + k) * cr : zero;
    f32x4 x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float xa, unused;
      dn_bwd_one<SCORES>(av[q], bv[q], cv[q], it1, it2, lse_s, second, abar, g, xa, unused);
      x[q] = xa + dv[q];
    }
    *reinterpret_cast<f32x4*>(dsp + k) = x;
  }
}

extern "C" int adell_ibot_bwd(const float* s, const float* y, const float* centers, const float* stats,
                              const int* inv, const float* d_red, const float* g_loss, int B, int Tt,
                              int K, int M, int class_token, int reduce_cls, float t1, float t2,
                              int teacher_is_scores, float* ds, void* stream) {
  ADELL_REQUIRE(ds && B > 0 && Tt > 0 && K > 0 && (class_token == 0 || class_token == 1) &&
                    Tt > class_token,
                "ibot_bwd: bad arguments");
  ADELL_REQUIRE((long)B * Tt <= 0x7fffffffL, "ibot_bwd: too many rows");
  ADELL_REQUIRE(!(reduce_cls && !class_token), "ibot_bwd: the \"cls\" reduction needs a class token");
  const bool masked = g_loss != nullptr;
  if (masked) {
    const int rc = ib_loss_args("ibot_bwd", s, y, B, Tt, K, M, t1, t2);
    if (rc != ADELL_OK) return rc;
    ADELL_REQUIRE(stats && inv, "ibot_bwd: null statistics / inverse table");
  }
  int plan[2];
  adell_dino_loss_plan((int)((long)B * Tt > 65535 ? 65535 : (long)B * Tt), K, plan);
  const dim3 grid((unsigned)((long)B * Tt), (unsigned)plan[0]);
  const float it1 = masked ? (float)(1.0 / (double)t1) : 1.f;
  const float it2 = masked ? (float)(1.0 / (double)t2) : 1.f;
  const float g_scale = masked ? (float)(1.0 / ((double)B * (double)M)) : 0.f;
  const float red_scale = (float)(1.0 / (double)(Tt - class_token));
  hipStream_t st = (hipStream_t)stream;
  if (teacher_is_scores)
    hipLaunchKernelGGL(adell_ibot_bwd_kernel<true>, grid, dim3(DN_NT), 0, st, s, y,
                       (const float*)nullptr, stats, inv, d_red, g_loss, g_scale, M, Tt, K, plan[1],
                       class_token, reduce_cls, red_scale, it1, it2, ds);
  else
    hipLaunchKernelGGL(adell_ibot_bwd_kernel<false>, grid, dim3(DN_NT), 0, st, s, y, centers, stats,
                       inv, d_red, g_loss, g_scale, M, Tt, K, plan[1], class_token, reduce_cls,
                       red_scale, it1, it2, ds);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
