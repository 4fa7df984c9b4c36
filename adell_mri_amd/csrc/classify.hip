// Kernels of the classification task (adell_mri/modules/classification/losses.py, pl.py;
// adell_mri/utils/batch_preprocessing.py): the three losses on logits, the relative order
// consistency loss of the ordinal network, the mixup of a batch, and the counts behind the
// classification metrics. House rules of ijepa.hip / mae.hip: fp32 in and out, one wave per row, every
// floating-point sum merged in a fixed order in fp64, no float atomics -- two runs are bit-identical.
// The only atomics are integer adds into int64 counts, whose result does not depend on their order.
//   * loss on logits, kinds 0 (BCE with logits, K = 1), 1 (cross entropy), 2 (ordinal sigmoidal /
//     CORAL on K - 1 logits): ONE block, one launch. Wave w takes the rows w, w + 4, ...; the per-item
//     losses are written, then wave 0 adds them (lane l the items l, l + 64, ... in order, the lanes
//     by the butterfly). Batches are small and the kernel is launch-bound: one block spares the
//     second launch. A label outside [0, K) is never used as an index: that row's loss and gradient
//     are NaN. Backward: one wave per row, any number of blocks, one launch.
//   * relative order consistency: the same layout over the rows i of the [B, B] pair matrix.
//   * mixup rows: out[b] = f_b x[b] + (1 - f_b) x[partner_b], the two products and the sum rounded
//     one by one (no FMA contraction); a row that is its own partner is copied. float4 where the
//     three row pointers are 16-byte aligned (decided per row), a scalar tail for V % 4.
//   * confusion update and AUROC pair counts: int64 counts.
#include "common.h"

#include <math.h>

constexpr int CLS_NT = 256;             // threads per block
constexpr int CLS_ROWS = CLS_NT / 64;   // rows (waves) per block
constexpr int CLS_MIX_NT = 256;
constexpr int CLS_MIX_ELEMS = 4096;     // elements of one row per block of the mixup kernel

__device__ __forceinline__ float cls_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ long long cls_wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// log(1 + exp(-|x|)), sigmoid(x) and log(sigmoid(x)) without overflow
__device__ __forceinline__ float cls_softplus_neg_abs(float x) { return log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float cls_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
__device__ __forceinline__ float cls_bce_logits(float x, float t) {
  return fmaxf(x, 0.f) - x * t + cls_softplus_neg_abs(x);
}

// ---- loss on logits --------------------------------------------------------------------------------
// The unweighted loss of row b and the weight of the row; false for a label outside [0, K). All 64
// lanes of the wave call it and all hold the results. W: logits per row (1, K or K - 1).
__device__ __forceinline__ bool cls_row_loss(int kind, const float* __restrict__ xr, int W, int K,
                                             const float* __restrict__ tf,
                                             const long long* __restrict__ ti,
                                             const float* __restrict__ w, int nw, int b, int lane,
                                             double* loss, float* weight) {
  if (kind == 0) {
    *weight = w ? w[nw == 1 ? 0 : b] : 1.f;
    *loss = (double)cls_bce_logits(xr[0], tf[b]);
    return true;
  }
  const long long y = ti[b];
  if (y < 0 || y >= K) return false;
  *weight = w ? w[y] : 1.f;
  if (kind == 1) {
    float m = -INFINITY;
    for (int j = lane; j < W; j += 64) m = fmaxf(m, xr[j]);
    m = cls_wave_max(m);
    double s = 0.0;
    for (int j = lane; j < W; j += 64) s += (double)expf(xr[j] - m);
    s = adell_wave_sum_d(s);
    *loss = (double)m + log(s) - (double)xr[y];
    return true;
  }
  // kind 2: t_j = [y >= j], j = 1..K-1 at column j - 1
  double s = 0.0;
  for (int j = lane; j < W; j += 64) {
    const float p = xr[j];
    const float ls = fminf(p, 0.f) - cls_softplus_neg_abs(p);      // log sigmoid(p)
    s += (y >= j + 1) ? (double)ls : (double)(ls - p);
  }
  *loss = -adell_wave_sum_d(s);
  return true;
}

// One block. item[b] = weight_b * loss_b; red[0] = sum_b item[b] / denom, denom = sum_b weight_b for
// kind 1 and B otherwise; aux[0] = denom (kept for the backward).
__global__ __launch_bounds__(CLS_NT) void adell_cls_loss_fwd_kernel(
    int kind, const float* __restrict__ x, const float* __restrict__ tf,
    const long long* __restrict__ ti, const float* __restrict__ w, int nw, int B, int W, int K,
    float* __restrict__ item, float* __restrict__ red, double* __restrict__ aux) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ double wsum[CLS_ROWS];
  double wacc = 0.0;                      // weights of this wave's rows, in row order
  for (int b = wave; b < B; b += CLS_ROWS) {
    double l;
    float wt;
    const bool ok = cls_row_loss(kind, x + (size_t)b * W, W, K, tf, ti, w, nw, b, lane, &l, &wt);
    const float v = ok ? (float)((double)wt * l) : NAN;
    if (ok) wacc += (double)wt;
    if (lane == 0) item[b] = v;
  }
  if (lane == 0) wsum[wave] = wacc;
  __syncthreads();                        // item[] of this block is visible to wave 0
  if (wave != 0) return;
  double acc = 0.0;
  for (int b = lane; b < B; b += 64) acc += (double)item[b];
  acc = adell_wave_sum_d(acc);
  if (lane == 0) {
    double denom = (double)B;
    if (kind == 1) {
      denom = 0.0;
      for (int i = 0; i < CLS_ROWS; ++i) denom += wsum[i];
    }
    red[0] = (float)(acc / denom);
    aux[0] = denom;
  }
}

// dx[b][j] = c_b * d loss_b / d x[b][j]; c_b = g[0] weight_b / aux[0] for the gradient of the reduced
// value, g[b] weight_b for a per-item gradient.
__global__ __launch_bounds__(CLS_NT) void adell_cls_loss_bwd_kernel(
    int kind, const float* __restrict__ x, const float* __restrict__ tf,
    const long long* __restrict__ ti, const float* __restrict__ w, int nw,
    const float* __restrict__ g, int per_item, const double* __restrict__ aux, int B, int W, int K,
    float* __restrict__ dx) {
  const int b = blockIdx.x * CLS_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  const float* xr = x + (size_t)b * W;
  float* dr = dx + (size_t)b * W;
  const float gb = per_item ? g[b] : (float)((double)g[0] / aux[0]);
  if (kind == 0) {
    const float wt = w ? w[nw == 1 ? 0 : b] : 1.f;
    if (lane == 0) dr[0] = gb * wt * (cls_sigmoid(xr[0]) - tf[b]);
    return;
  }
  const long long y = ti[b];
  if (y < 0 || y >= K) {
    for (int j = lane; j < W; j += 64) dr[j] = NAN;
    return;
  }
  const float c = gb * (w ? w[y] : 1.f);
  if (kind == 1) {
    float m = -INFINITY;
    for (int j = lane; j < W; j += 64) m = fmaxf(m, xr[j]);
    m = cls_wave_max(m);
    double s = 0.0;
    for (int j = lane; j < W; j += 64) s += (double)expf(xr[j] - m);
    s = adell_wave_sum_d(s);
    const float inv = (float)(1.0 / s);
    for (int j = lane; j < W; j += 64)
      dr[j] = c * (expf(xr[j] - m) * inv - (j == y ? 1.f : 0.f));
    return;
  }
  for (int j = lane; j < W; j += 64) dr[j] = c * (cls_sigmoid(xr[j]) - (y >= j + 1 ? 1.f : 0.f));
}

static int cls_loss_args(const char* what, int kind, const void* x, const void* tf, const void* ti,
                         const void* w, int nw, int B, int K) {
  ADELL_REQUIRE(kind >= 0 && kind <= 2, "%s: kind must be 0 (bce), 1 (cross entropy) or 2 (ordinal)",
                what);
  ADELL_REQUIRE(x && B > 0 && K >= (kind == 0 ? 1 : 2), "%s: bad arguments", what);
  ADELL_REQUIRE(kind == 0 ? (tf != nullptr && K == 1) : ti != nullptr,
                "%s: kind 0 takes float targets and one logit, kinds 1 and 2 int64 labels", what);
  ADELL_REQUIRE(w == nullptr || (kind == 0 ? (nw == 1 || nw == B) : nw == K),
                "%s: %d weights (kind 0: 1 or B; kinds 1, 2: K)", what, nw);
  return ADELL_OK;
}

static inline int cls_width(int kind, int K) { return kind == 0 ? 1 : kind == 1 ? K : K - 1; }

extern "C" int adell_cls_loss_fwd(int kind, const float* x, const float* tf, const long long* ti,
                                  const float* w, int nw, int B, int K, float* item, float* red,
                                  double* aux, void* stream) {
  const int rc = cls_loss_args("cls_loss_fwd", kind, x, tf, ti, w, nw, B, K);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(item && red && aux, "cls_loss_fwd: null output");
  return adell_launch<adell_cls_loss_fwd_kernel>(dim3(1), dim3(CLS_NT), 0, (hipStream_t)stream, kind, x,
                                                 tf, ti, w, nw, B, cls_width(kind, K), K, item, red,
                                                 aux);
}

extern "C" int adell_cls_loss_bwd(int kind, const float* x, const float* tf, const long long* ti,
                                  const float* w, int nw, const float* g, int per_item,
                                  const double* aux, int B, int K, float* dx, void* stream) {
  const int rc = cls_loss_args("cls_loss_bwd", kind, x, tf, ti, w, nw, B, K);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(g && dx && (per_item || aux), "cls_loss_bwd: null pointer");
  return adell_launch<adell_cls_loss_bwd_kernel>(dim3((unsigned)adell_cdiv(B, CLS_ROWS)), dim3(CLS_NT),
                                                 0, (hipStream_t)stream, kind, x, tf, ti, w, nw, g,
                                                 per_item, aux, B, cls_width(kind, K), K, dx);
}

// ---- relative order consistency ----------------------------------------------------------------------
// One block. Row i: the sum over j with y_j != y_i of bce(p_i - p_j, [y_i > y_j]) and their number.
// loss = sum / M over the M ordered pairs; aux[0] = M. M = 0: 0 / 0 = NaN, as the reference's mean of
// an empty selection.
__global__ __launch_bounds__(CLS_NT) void adell_cls_roc_fwd_kernel(
    const float* __restrict__ p, const long long* __restrict__ y, int B, double* __restrict__ rows,
    float* __restrict__ loss, double* __restrict__ aux) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ long long wcount[CLS_ROWS];
  long long count = 0;
  for (int i = wave; i < B; i += CLS_ROWS) {
    const float pi = p[i];
    const long long yi = y[i];
    double s = 0.0;
    long long n = 0;
    for (int j = lane; j < B; j += 64) {
      const long long yj = y[j];
      if (yj == yi) continue;
      s += (double)cls_bce_logits(pi - p[j], yi > yj ? 1.f : 0.f);
      ++n;
    }
    s = adell_wave_sum_d(s);
    count += cls_wave_sum_ll(n);
    if (lane == 0) rows[i] = s;
  }
  if (lane == 0) wcount[wave] = count;
  __syncthreads();
  if (wave != 0) return;
  double acc = 0.0;
  for (int i = lane; i < B; i += 64) acc += rows[i];
  acc = adell_wave_sum_d(acc);
  if (lane == 0) {
    long long M = 0;
    for (int i = 0; i < CLS_ROWS; ++i) M += wcount[i];
    loss[0] = (float)(acc / (double)M);
    aux[0] = (double)M;
  }
}

// dp[i] = g / M * sum over j with y_j != y_i of the (i, j) term and the (j, i) term of the mean.
__global__ __launch_bounds__(CLS_NT) void adell_cls_roc_bwd_kernel(
    const float* __restrict__ p, const long long* __restrict__ y, const float* __restrict__ g,
    const double* __restrict__ aux, int B, float* __restrict__ dp) {
  const int i = blockIdx.x * CLS_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= B) return;
  const float pi = p[i];
  const long long yi = y[i];
  double s = 0.0;
  for (int j = lane; j < B; j += 64) {
    const long long yj = y[j];
    if (yj == yi) continue;
    const float d = pi - p[j], t = yi > yj ? 1.f : 0.f;
    // d bce(d, t) / dp_i of the pair (i, j), and of the pair (j, i): bce(-d, 1 - t), whose
    // derivative with respect to p_i carries a minus sign
    s += (double)(cls_sigmoid(d) - t) - (double)(cls_sigmoid(-d) - (1.f - t));
  }
  s = adell_wave_sum_d(s);
  if (lane == 0) dp[i] = (float)((double)g[0] / aux[0] * s);
}

extern "C" int adell_cls_roc_fwd(const float* p, const long long* y, int B, double* rows, float* loss,
                                 double* aux, void* stream) {
  ADELL_REQUIRE(p && y && rows && loss && aux && B > 0, "cls_roc_fwd: bad arguments");
  return adell_launch<adell_cls_roc_fwd_kernel>(dim3(1), dim3(CLS_NT), 0, (hipStream_t)stream, p, y, B,
                                                rows, loss, aux);
}

extern "C" int adell_cls_roc_bwd(const float* p, const long long* y, const float* g, const double* aux,
                                 int B, float* dp, void* stream) {
  ADELL_REQUIRE(p && y && g && aux && dp && B > 0, "cls_roc_bwd: bad arguments");
  return adell_launch<adell_cls_roc_bwd_kernel>(dim3((unsigned)adell_cdiv(B, CLS_ROWS)), dim3(CLS_NT), 0,
                                                (hipStream_t)stream, p, y, g, aux, B, dp);
}

// ---- mixup -------------------------------------------------------------------------------------------
// a f + c g with the two products and the sum rounded one by one: contraction is switched off for
// this body (the *_rn intrinsics are plain operators to the compiler, which fuses them into an FMA).
__device__ __forceinline__ float cls_mix(float f, float g, float a, float c) {
#pragma clang fp contract(off)
  const float u = a * f;
  const float v = c * g;
  return u + v;
}

// Block (chunk, b): CLS_MIX_ELEMS elements of row b. partner[b] in [0, B) is checked on the host.
__global__ __launch_bounds__(CLS_MIX_NT) void adell_cls_mixup_kernel(
    const float* __restrict__ x, const float* __restrict__ factor, const int* __restrict__ partner,
    long V, float* __restrict__ out) {
  const long b = blockIdx.y;
  const int pb = partner[b];
  const float* xa = x + (size_t)b * V;
  const float* xp = x + (size_t)pb * V;
  float* op = out + (size_t)b * V;
  const bool copy = pb == b;
  const float f = factor[b], g = 1.f - f;
  const long lo = (long)blockIdx.x * CLS_MIX_ELEMS;
  const long hi = lo + CLS_MIX_ELEMS < V ? lo + CLS_MIX_ELEMS : V;
  const bool vec = ((((uintptr_t)xa) | ((uintptr_t)xp) | ((uintptr_t)op)) & 15) == 0;
  long done = lo;                          // CLS_MIX_ELEMS % 4 == 0: a chunk starts on a float4
  if (vec) {
    const long n4 = (hi - lo) >> 2;
    const f32x4* a4 = reinterpret_cast<const f32x4*>(xa + lo);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(xp + lo);
    f32x4* o4 = reinterpret_cast<f32x4*>(op + lo);
    for (long i = threadIdx.x; i < n4; i += CLS_MIX_NT) {
      const f32x4 a = a4[i];
      if (copy) {
        o4[i] = a;
        continue;
      }
      const f32x4 c = p4[i];
      f32x4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = cls_mix(f, g, a[k], c[k]);
      o4[i] = o;
    }
    done = lo + (n4 << 2);
  }
  for (long e = done + threadIdx.x; e < hi; e += CLS_MIX_NT)
    op[e] = copy ? xa[e] : cls_mix(f, g, xa[e], xp[e]);
}

extern "C" int adell_cls_mixup(const float* x, const float* factor, const int* partner, int B, long V,
                               float* out, void* stream) {
  ADELL_REQUIRE(x && factor && partner && out && B > 0 && V > 0, "cls_mixup: bad arguments");
  ADELL_REQUIRE(B <= 65535, "cls_mixup: %d rows exceed the grid", B);
  const long chunks = (V + CLS_MIX_ELEMS - 1) / CLS_MIX_ELEMS;
  ADELL_REQUIRE(chunks <= 0x7fffffffL, "cls_mixup: rows of %ld elements exceed the grid", V);
  return adell_launch<adell_cls_mixup_kernel>(dim3((unsigned)chunks, (unsigned)B), dim3(CLS_MIX_NT), 0,
                                              (hipStream_t)stream, x, factor, partner, V, out);
}

// ---- confusion counts ----------------------------------------------------------------------------------
// counts [C][C] (row: label, column: prediction) and counts[C C]: the samples whose label, or whose
// integer prediction, lies outside [0, C) (they are counted nowhere else). mode 0: pf [N][C], argmax
// (the first maximal index; a NaN wins); mode 1: pf [N] probabilities, class [p > 0.5] (C = 2);
// mode 2: pi [N] integer classes.
__global__ __launch_bounds__(CLS_NT) void adell_cls_confusion_kernel(
    int mode, const float* __restrict__ pf, const long long* __restrict__ pi,
    const long long* __restrict__ y, long N, int C, unsigned long long* __restrict__ counts) {
  const long n = (long)blockIdx.x * CLS_NT + threadIdx.x;
  if (n >= N) return;
  long long pred;
  if (mode == 0) {
    const float* r = pf + (size_t)n * C;
    float best = r[0];
    pred = 0;
    for (int c = 1; c < C; ++c) {
      const float v = r[c];
      if (v > best || (v != v && best == best)) {
        best = v;
        pred = c;
      }
    }
  } else if (mode == 1) {
    pred = pf[n] > 0.5f ? 1 : 0;
  } else {
    pred = pi[n];
  }
  const long long label = y[n];
  const bool bad = label < 0 || label >= C || pred < 0 || pred >= C;
  atomicAdd(counts + (bad ? (size_t)C * C : (size_t)label * C + (size_t)pred), 1ull);
}

extern "C" int adell_cls_confusion_update(int mode, const float* pf, const long long* pi,
                                          const long long* y, long N, int C, long long* counts,
                                          void* stream) {
  ADELL_REQUIRE(mode >= 0 && mode <= 2 && y && counts && N > 0 && C >= 2,
                "cls_confusion_update: bad arguments");
  ADELL_REQUIRE(mode == 2 ? pi != nullptr : pf != nullptr, "cls_confusion_update: null prediction");
  ADELL_REQUIRE(mode != 1 || C == 2, "cls_confusion_update: probabilities take C = 2, got %d", C);
  const long blocks = (N + CLS_NT - 1) / CLS_NT;
  ADELL_REQUIRE(blocks <= 0x7fffffffL, "cls_confusion_update: too many samples");
  return adell_launch<adell_cls_confusion_kernel>(dim3((unsigned)blocks), dim3(CLS_NT), 0,
                                                  (hipStream_t)stream, mode, pf, pi, y, N, C,
                                                  reinterpret_cast<unsigned long long*>(counts));
}

// ---- AUROC pair counts -----------------------------------------------------------------------------------
// out[0] += 2 #{(i, j): y_i = 1, y_j = 0, s_i > s_j} + #{... s_i == s_j}; out[1] += positives,
// out[2] += negatives. One wave per sample i; a positive walks the negatives. Labels other than 0
// and 1 are skipped. The caller zeroes out.
__global__ __launch_bounds__(CLS_NT) void adell_cls_auroc_kernel(
    const float* __restrict__ s, const long long* __restrict__ y, int N,
    unsigned long long* __restrict__ out) {
  const int i = blockIdx.x * CLS_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= N) return;
  const long long yi = y[i];
  if (yi == 0) {
    if (lane == 0) atomicAdd(out + 2, 1ull);
    return;
  }
  if (yi != 1) return;
  const float si = s[i];
  long long n = 0;
  for (int j = lane; j < N; j += 64)
    if (y[j] == 0) n += si > s[j] ? 2 : (si == s[j] ? 1 : 0);
  n = cls_wave_sum_ll(n);
  if (lane == 0) {
    atomicAdd(out, (unsigned long long)n);
    atomicAdd(out + 1, 1ull);
  }
}

extern "C" int adell_cls_auroc_pairs(const float* scores, const long long* y, int N, long long* out,
                                     void* stream) {
  ADELL_REQUIRE(scores && y && out && N > 0, "cls_auroc_pairs: bad arguments");
  return adell_launch<adell_cls_auroc_kernel>(dim3((unsigned)adell_cdiv(N, CLS_ROWS)), dim3(CLS_NT), 0,
                                              (hipStream_t)stream, scores, y, N,
                                              reinterpret_cast<unsigned long long*>(out));
}
