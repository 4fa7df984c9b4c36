// Kernels of the deconfounded classifier (adell_mri/modules/classification/pl.py, DeconfoundedNetPL):
// the first n columns of the pooled features [B][F] predict the confounders and are decorrelated
// from the other M = F - n. House rules of classify.hip and batch_ensemble.hip: fp32 in and out, no
// float atomics, every sum in a fixed order in fp64 -- two runs are bit-identical. The features are
// always read IN PLACE (row stride F, column offset 0 or n): no kernel is handed a slice.
//   * deconf_split, one launch each way: the two dense halves [B][n] and [B][M]; backward writes the
//     whole [B][F] gradient from whichever halves have one (zeros for the other).
//   * deconf_corr (the wrapper's correlation_loss), one launch forward: a thread per pair (i, j) of a
//     confounded and a de-confounded column takes both batch means, the centred norms and the centred
//     dot product over the B items in item order, r = clamp(dot / max(|a| |b|, 1e-8), -1, 1); the
//     block sums r^2, the block with the last integer ticket folds the blocks in index order. Kept for
//     the backward: mean and centred norm per column, and the ratio before the clamp per pair.
//     Backward, one launch: a block per confounded column (a wave per item, the lanes over j) and a
//     block per 64 de-confounded columns (a wave per item, a lane per column, i in order) write every
//     element of the [B][F] gradient once. The gradient of sqrt at an exactly zero centred norm is
//     taken as 0: such a column has r = 0 with every partner and an exact 0 gradient.
//   * deconf_heads, one launch forward: a block per item keeps features[b][:n] in LDS, a wave per
//     output row of the heads (up to 8 categorical heads of up to 64 classes and up to 64 regression
//     outputs over n <= 1024 columns) takes the logit, then the cross entropy per head and the
//     squared error; the last ticket folds the items in order. A label outside [0, K) is never used
//     as an index: the item is NaN. Backward, two launches: per item the logits again, their
//     gradient (kept in fp64) and d features[b][:] (zeros past n); then a thread per element of every
//     dW and db over the items in order.
#include "common.h"

constexpr int DC_NT = 256;
constexpr int DC_NW = DC_NT / 64;
constexpr int DC_MAX_HEADS = ADELL_DECONF_MAX_HEADS;
constexpr int DC_MAX_K = ADELL_DECONF_MAX_CLASSES;
constexpr int DC_MAX_CONT = ADELL_DECONF_MAX_CONT;
constexpr int DC_MAX_CONF = ADELL_DECONF_MAX_CONF;
constexpr int DC_MAX_OUT = DC_MAX_HEADS * DC_MAX_K + DC_MAX_CONT;
constexpr double DC_EPS = 1e-8;

// ---- split_columns --------------------------------------------------------------------------------------
__global__ __launch_bounds__(DC_NT) void adell_deconf_split_fwd_kernel(
    const float* __restrict__ x, float* __restrict__ a, float* __restrict__ b, long BF, int F, int n) {
  const long step = (long)gridDim.x * DC_NT;
  const int M = F - n;
  for (long i = (long)blockIdx.x * DC_NT + threadIdx.x; i < BF; i += step) {
    const long r = i / F;
    const int c = (int)(i - r * F);
    const float v = x[i];
    if (c < n)
      a[r * n + c] = v;
    else
      b[r * M + (c - n)] = v;
  }
}

__global__ __launch_bounds__(DC_NT) void adell_deconf_split_bwd_kernel(
    const float* __restrict__ da, const float* __restrict__ db, float* __restrict__ dx, long BF, int F,
    int n) {
  const long step = (long)gridDim.x * DC_NT;
  const int M = F - n;
  for (long i = (long)blockIdx.x * DC_NT + threadIdx.x; i < BF; i += step) {
    const long r = i / F;
    const int c = (int)(i - r * F);
    float v = 0.f;
    if (c < n) {
      if (da != nullptr) v = da[r * n + c];
    } else if (db != nullptr) {
      v = db[r * M + (c - n)];
    }
    dx[i] = v;
  }
}

// ---- correlation loss -------------------------------------------------------------------------------------
// saved: mean [F], centred norm [F], then the ratio before the clamp [n][M]
__global__ __launch_bounds__(DC_NT) void adell_deconf_corr_fwd_kernel(
    const float* __restrict__ x, int B, int F, int n, double inv_pairs, unsigned* counter, double* part,
    double* __restrict__ saved, float* __restrict__ loss) {
  __shared__ double sw[DC_NW];
  __shared__ int last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = F - n;
  const int j = blockIdx.x * 64 + lane, i = blockIdx.y * DC_NW + wave;
  double acc = 0.0;
  if (i < n && j < M) {
    const float* xa = x + i;
    const float* xb = x + n + j;
    double ma = 0.0, mb = 0.0;
    for (int b = 0; b < B; ++b) {
      ma += (double)xa[(size_t)b * F];
      mb += (double)xb[(size_t)b * F];
    }
    ma /= (double)B;
    mb /= (double)B;
    double ssa = 0.0, ssb = 0.0, dot = 0.0;
    for (int b = 0; b < B; ++b) {
      const double va = (double)xa[(size_t)b * F] - ma, vb = (double)xb[(size_t)b * F] - mb;
      ssa += va * va;
      ssb += vb * vb;
      dot += va * vb;
    }
    const double na = sqrt(ssa), nb = sqrt(ssb);
    double d = na * nb;
    d = d < DC_EPS ? DC_EPS : d;
    const double q = dot / d;
    const double r = q < -1.0 ? -1.0 : (q > 1.0 ? 1.0 : q);
    saved[2 * (size_t)F + (size_t)i * M + j] = q;
    if (j == 0) saved[i] = ma, saved[F + i] = na;
    if (i == 0) saved[n + j] = mb, saved[F + n + j] = nb;
    acc = r * r;
  }
  acc = adell_wave_sum_d(acc);
  if (lane == 0) sw[wave] = acc;
  __syncthreads();
  const unsigned nblocks = gridDim.x * gridDim.y;
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < DC_NW; ++w) tot += sw[w];
    __hip_atomic_store(part + (blockIdx.y * gridDim.x + blockIdx.x), tot, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = ticket == nblocks - 1;
  }
  __syncthreads();
  if (!last || wave != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double tot = 0.0;
  for (unsigned b = lane; b < nblocks; b += 64)
    tot += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = adell_wave_sum_d(tot);
  if (lane == 0) loss[0] = (float)(tot * inv_pairs);
}

// d loss / d ratio of a pair, and whether the denominator was above its floor
__device__ __forceinline__ double dc_gq(double q, double coef) {
  const double r = q < -1.0 ? -1.0 : (q > 1.0 ? 1.0 : q);
  return (q >= -1.0 && q <= 1.0) ? coef * r : 0.0;
}

__global__ __launch_bounds__(DC_NT) void adell_deconf_corr_bwd_kernel(
    const float* __restrict__ x, const double* __restrict__ saved, const float* __restrict__ g, int B,
    int F, int n, double two_over_pairs, float* __restrict__ dx) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = F - n;
  const double* mean = saved;
  const double* norm = saved + F;
  const double* Q = saved + 2 * (size_t)F;
  const double coef = (double)g[0] * two_over_pairs;
  if ((int)blockIdx.x < n) {
    // a confounded column: G[b] = sum_j w_ij b'_j[b] - a'[b] s_i
    const int i = blockIdx.x;
    const double ma = mean[i], na = norm[i];
    double s = 0.0;
    for (int j = lane; j < M; j += 64) {
      const double q = Q[(size_t)i * M + j];
      if (na * norm[n + j] >= DC_EPS) s += dc_gq(q, coef) * q;
    }
    s = adell_wave_sum_d(s);
    s = na > 0.0 ? s / (na * na) : 0.0;
    for (int b = wave; b < B; b += DC_NW) {
      const float* xr = x + (size_t)b * F;
      double acc = 0.0;
      for (int j = lane; j < M; j += 64) {
        double d = na * norm[n + j];
        d = d < DC_EPS ? DC_EPS : d;
        const double w = dc_gq(Q[(size_t)i * M + j], coef) / d;
        acc += w * ((double)xr[n + j] - mean[n + j]);
      }
      acc = adell_wave_sum_d(acc);
      if (lane == 0) dx[(size_t)b * F + i] = (float)(acc - ((double)xr[i] - ma) * s);
    }
    return;
  }
  // 64 de-confounded columns: G[b] = sum_i w_ij a'_i[b] - b'[b] t_j
  const int j = ((int)blockIdx.x - n) * 64 + lane;
  if (j >= M) return;
  const double mb = mean[n + j], nb = norm[n + j];
  double t = 0.0;
  for (int i = 0; i < n; ++i) {
    const double q = Q[(size_t)i * M + j];
    if (norm[i] * nb >= DC_EPS) t += dc_gq(q, coef) * q;
  }
  t = nb > 0.0 ? t / (nb * nb) : 0.0;
  for (int b = wave; b < B; b += DC_NW) {
    const float* xr = x + (size_t)b * F;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      double d = norm[i] * nb;
      d = d < DC_EPS ? DC_EPS : d;
      const double w = dc_gq(Q[(size_t)i * M + j], coef) / d;
      acc += w * ((double)xr[i] - mean[i]);
    }
    dx[(size_t)b * F + n + j] = (float)(acc - ((double)xr[n + j] - mb) * t);
  }
}

// ---- confounder heads -------------------------------------------------------------------------------------
// output row o of the heads: its weight row, its bias, its head (n_heads: the regression) and class
struct DcRow {
  const float* w;
  float bias;
  int head, k;
};
__device__ __forceinline__ DcRow dc_row(const adell_deconf_heads& hd, int o, int n) {
  DcRow r;
  int h = 0;
  while (h < hd.n_heads && o >= hd.K[h]) o -= hd.K[h], ++h;
  const float* W = h < hd.n_heads ? hd.W[h] : hd.Wc;
  const float* bs = h < hd.n_heads ? hd.b[h] : hd.bc;
  r.w = W + (size_t)o * n;
  r.bias = bs[o];
  r.head = h;
  r.k = o;
  return r;
}

// the logits of item b into z[0, O): a wave per output row, the lanes over the columns in LDS
__device__ __forceinline__ void dc_logits(const adell_deconf_heads& hd, const float* __restrict__ x, int b,
                                          int F, int n, int O, float* xs, double* z) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int c = tid; c < n; c += DC_NT) xs[c] = x[(size_t)b * F + c];
  __syncthreads();
  for (int o = wave; o < O; o += DC_NW) {
    const DcRow r = dc_row(hd, o, n);
    double acc = 0.0;
    for (int c = lane; c < n; c += 64) acc += (double)r.w[c] * (double)xs[c];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) z[o] = acc + (double)r.bias;
  }
  __syncthreads();
}

// max and log-sum-exp of the K logits at z
__device__ __forceinline__ double dc_lse(const double* z, int K) {
  double m = z[0];
  for (int k = 1; k < K; ++k) m = z[k] > m ? z[k] : m;
  double se = 0.0;
  for (int k = 0; k < K; ++k) se += exp(z[k] - m);
  return m + log(se);
}

__global__ __launch_bounds__(DC_NT) void adell_deconf_heads_fwd_kernel(
    adell_deconf_heads hd, const float* __restrict__ x, const long long* __restrict__ cat_t,
    const float* __restrict__ cont_t, int B, int F, int n, int O, double cat_scale, double cont_scale,
    unsigned* counter, double* part, float* __restrict__ out) {
  __shared__ float xs[DC_MAX_CONF];
  __shared__ double z[DC_MAX_OUT];
  __shared__ double ce[DC_MAX_HEADS];
  __shared__ int last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  dc_logits(hd, x, b, F, n, O, xs, z);
  if (tid < hd.n_heads) {
    int off = 0;
    for (int h = 0; h < tid; ++h) off += hd.K[h];
    const int K = hd.K[tid];
    const long long t = cat_t[(size_t)tid * B + b];
    const double lse = dc_lse(z + off, K);
    ce[tid] = (t >= 0 && t < K) ? lse - z[off + (int)t] : __longlong_as_double(0x7ff8000000000000LL);
  }
  __syncthreads();
  if (tid == 0) {
    double cat = 0.0, cont = 0.0;
    for (int h = 0; h < hd.n_heads; ++h) cat += ce[h];
    const int off = O - hd.n_cont;
    for (int k = 0; k < hd.n_cont; ++k) {
      const double e = z[off + k] - (double)cont_t[(size_t)b * hd.n_cont + k];
      cont += e * e;
    }
    __hip_atomic_store(part + 2 * b, cat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + 2 * b + 1, cont, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = ticket == gridDim.x - 1;
  }
  __syncthreads();
  if (!last || wave != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double cat = 0.0, cont = 0.0;
  for (int i = lane; i < B; i += 64) {
    cat += __hip_atomic_load(part + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cont += __hip_atomic_load(part + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  cat = adell_wave_sum_d(cat);
  cont = adell_wave_sum_d(cont);
  if (lane == 0) {
    out[0] = (float)(cat * cat_scale);
    out[1] = (float)(cont * cont_scale);
  }
}

// per item: dz [B][O] (fp64) and d features[b][:]
__global__ __launch_bounds__(DC_NT) void adell_deconf_heads_bwd_kernel(
    adell_deconf_heads hd, const float* __restrict__ x, const long long* __restrict__ cat_t,
    const float* __restrict__ cont_t, const float* __restrict__ g_cat, const float* __restrict__ g_cont,
    int B, int F, int n, int O, double cat_scale, double cont_scale, double* __restrict__ dz,
    float* __restrict__ dx) {
  __shared__ float xs[DC_MAX_CONF];
  __shared__ double z[DC_MAX_OUT];
  __shared__ double gz[DC_MAX_OUT];
  const int tid = threadIdx.x, b = blockIdx.x;
  dc_logits(hd, x, b, F, n, O, xs, z);
  const double kc = g_cat != nullptr ? (double)g_cat[0] * cat_scale : 0.0;
  const double kr = g_cont != nullptr ? (double)g_cont[0] * cont_scale * 2.0 : 0.0;
  for (int o = tid; o < O; o += DC_NT) {
    int h = 0, k = o, off = 0;
    while (h < hd.n_heads && k >= hd.K[h]) k -= hd.K[h], off += hd.K[h], ++h;
    double v = 0.0;
    if (h < hd.n_heads) {
      if (g_cat != nullptr) {
        const int K = hd.K[h];
        const long long t = cat_t[(size_t)h * B + b];
        const double p = exp(z[o] - dc_lse(z + off, K));
        v = (t >= 0 && t < K) ? kc * (p - (k == (int)t ? 1.0 : 0.0))
                              : __longlong_as_double(0x7ff8000000000000LL);
      }
    } else if (g_cont != nullptr) {
      v = kr * (z[o] - (double)cont_t[(size_t)b * hd.n_cont + k]);
    }
    gz[o] = v;
    dz[(size_t)b * O + o] = v;
  }
  __syncthreads();
  if (dx == nullptr) return;
  for (int c = tid; c < F; c += DC_NT) {
    double acc = 0.0;
    if (c < n) {
      int o = 0;
      for (int h = 0; h <= hd.n_heads; ++h) {
        const float* W = h < hd.n_heads ? hd.W[h] : hd.Wc;
        const int K = h < hd.n_heads ? hd.K[h] : hd.n_cont;
        for (int k = 0; k < K; ++k, ++o) acc += gz[o] * (double)W[(size_t)k * n + c];
      }
    }
    dx[(size_t)b * F + c] = (float)acc;
  }
}

// a thread per element of every dW (c < n) and db (c == n), the items in order
__global__ __launch_bounds__(DC_NT) void adell_deconf_heads_wgrad_kernel(
    adell_deconf_head_grads gr, adell_deconf_heads hd, const float* __restrict__ x,
    const double* __restrict__ dz, int B, int F, int n, int O) {
  const long idx = (long)blockIdx.x * DC_NT + threadIdx.x;
  if (idx >= (long)O * (n + 1)) return;
  const int o = (int)(idx / (n + 1)), c = (int)(idx - (long)o * (n + 1));
  double acc = 0.0;
  for (int b = 0; b < B; ++b)
    acc += dz[(size_t)b * O + o] * (c < n ? (double)x[(size_t)b * F + c] : 1.0);
  int h = 0, k = o;
  while (h < hd.n_heads && k >= hd.K[h]) k -= hd.K[h], ++h;
  float* dW = h < hd.n_heads ? gr.dW[h] : gr.dWc;
  float* db = h < hd.n_heads ? gr.db[h] : gr.dbc;
  if (c < n) {
    if (dW != nullptr) dW[(size_t)k * n + c] = (float)acc;
  } else if (db != nullptr) {
    db[k] = (float)acc;
  }
}

// ---- host side -----------------------------------------------------------------------------------------
static int dc_args(const char* what, int B, int F, int n) {
  ADELL_REQUIRE(B >= 1 && F >= 2 && n > 0 && n < F, "%s: bad arguments (B %d, F %d, n_conf %d)", what, B, F,
                n);
  ADELL_REQUIRE((long)B * F <= 0x7fffffffL, "%s: %d x %d features are too many", what, B, F);
  return ADELL_OK;
}

static unsigned dc_flat_blocks(long n) {
  long blocks = (n + DC_NT - 1) / DC_NT;
  if (blocks > 2048) blocks = 2048;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int adell_deconf_split_fwd(const float* x, float* a, float* b, int B, int F, int n,
                                      void* stream) {
  const int rc = dc_args("deconf_split_fwd", B, F, n);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && a && b, "deconf_split_fwd: null pointer");
  const long BF = (long)B * F;
  return adell_launch<adell_deconf_split_fwd_kernel>(dim3(dc_flat_blocks(BF)), dim3(DC_NT), 0,
                                                     (hipStream_t)stream, x, a, b, BF, F, n);
}

extern "C" int adell_deconf_split_bwd(const float* da, const float* db, float* dx, int B, int F, int n,
                                      void* stream) {
  const int rc = dc_args("deconf_split_bwd", B, F, n);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dx, "deconf_split_bwd: null pointer");
  const long BF = (long)B * F;
  return adell_launch<adell_deconf_split_bwd_kernel>(dim3(dc_flat_blocks(BF)), dim3(DC_NT), 0,
                                                     (hipStream_t)stream, da, db, dx, BF, F, n);
}

static long dc_corr_blocks(int F, int n) {
  return (long)adell_cdiv(F - n, 64) * adell_cdiv(n, DC_NW);
}

extern "C" long adell_deconf_corr_workspace_doubles(int B, int F, int n) {
  if (B < 1 || F < 2 || n <= 0 || n >= F) return ADELL_E_BADARG;
  return 2 + dc_corr_blocks(F, n);
}

extern "C" long adell_deconf_corr_saved_doubles(int B, int F, int n) {
  if (B < 1 || F < 2 || n <= 0 || n >= F) return ADELL_E_BADARG;
  return 2 * (long)F + (long)n * (F - n);
}

extern "C" int adell_deconf_corr_fwd(const float* x, int B, int F, int n, double* ws, double* saved,
                                     float* loss, void* stream) {
  const int rc = dc_args("deconf_corr_fwd", B, F, n);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && ws && saved && loss && adell_aligned16(ws), "deconf_corr_fwd: bad pointer");
  ADELL_REQUIRE(adell_cdiv(n, DC_NW) <= 65535, "deconf_corr_fwd: %d confounded columns", n);
  hipStream_t st = (hipStream_t)stream;
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, 16, st));
  const dim3 grid((unsigned)adell_cdiv(F - n, 64), (unsigned)adell_cdiv(n, DC_NW));
  return adell_launch<adell_deconf_corr_fwd_kernel>(grid, dim3(DC_NT), 0, st, x, B, F, n,
                                                    1.0 / ((double)n * (double)(F - n)), (unsigned*)ws,
                                                    ws + 2, saved, loss);
}

extern "C" int adell_deconf_corr_bwd(const float* x, const double* saved, const float* g, int B, int F,
                                     int n, float* dx, void* stream) {
  const int rc = dc_args("deconf_corr_bwd", B, F, n);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && saved && g && dx, "deconf_corr_bwd: null pointer");
  const dim3 grid((unsigned)(n + adell_cdiv(F - n, 64)));
  return adell_launch<adell_deconf_corr_bwd_kernel>(grid, dim3(DC_NT), 0, (hipStream_t)stream, x, saved, g,
                                                    B, F, n, 2.0 / ((double)n * (double)(F - n)), dx);
}

// ADELL_DECONF_FUSED when the fused kernels take the heads, ADELL_DECONF_COMPOSED beyond their limits
static int dc_route(int n, int n_heads, const int* K, int n_cont) {
  if (n > DC_MAX_CONF || n_heads > DC_MAX_HEADS || n_cont > DC_MAX_CONT) return ADELL_DECONF_COMPOSED;
  for (int h = 0; h < n_heads; ++h)
    if (K[h] > DC_MAX_K) return ADELL_DECONF_COMPOSED;
  return ADELL_DECONF_FUSED;
}

extern "C" int adell_deconf_route(int n, int n_heads, const int* K, int n_cont) {
  ADELL_REQUIRE(n >= 1 && n_heads >= 0 && n_cont >= 0 && n_heads + n_cont >= 1 && (n_heads == 0 || K),
                "deconf_route: bad arguments (n_conf %d, %d heads, %d regression outputs)", n, n_heads,
                n_cont);
  for (int h = 0; h < n_heads; ++h) ADELL_REQUIRE(K[h] >= 1, "deconf_route: head %d has %d classes", h, K[h]);
  return dc_route(n, n_heads, K, n_cont);
}

static int dc_heads_args(const char* what, const adell_deconf_heads* hd, const float* x, const void* cat_t,
                         const float* cont_t, int B, int F, int n, int* O) {
  const int rc = dc_args(what, B, F, n);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(hd && x, "%s: null pointer", what);
  ADELL_REQUIRE(hd->n_heads >= 0 && hd->n_cont >= 0 && hd->n_heads + hd->n_cont >= 1, "%s: no head", what);
  ADELL_REQUIRE(hd->n_heads <= DC_MAX_HEADS && dc_route(n, hd->n_heads, hd->K, hd->n_cont) == ADELL_DECONF_FUSED,
                "%s: beyond the fused route (n_conf <= %d, <= %d heads of <= %d classes, <= %d regression "
                "outputs)", what, DC_MAX_CONF, DC_MAX_HEADS, DC_MAX_K, DC_MAX_CONT);
  int o = 0;
  for (int h = 0; h < hd->n_heads; ++h) {
    ADELL_REQUIRE(hd->K[h] >= 1 && hd->W[h] && hd->b[h], "%s: head %d is incomplete", what, h);
    o += hd->K[h];
  }
  ADELL_REQUIRE(hd->n_heads == 0 || cat_t, "%s: categorical heads without their label table", what);
  ADELL_REQUIRE(hd->n_cont == 0 || (hd->Wc && hd->bc && cont_t), "%s: the regression head is incomplete",
                what);
  ADELL_REQUIRE(B <= 65535, "%s: %d items", what, B);
  *O = o + hd->n_cont;
  return ADELL_OK;
}

extern "C" long adell_deconf_heads_workspace_doubles(int B) {
  return B < 1 ? ADELL_E_BADARG : 2 + 2 * (long)B;
}

extern "C" int adell_deconf_heads_fwd(const adell_deconf_heads* hd, const float* x, const long long* cat_t,
                                      const float* cont_t, int B, int F, int n, float conf_mult,
                                      double* ws, float* out, void* stream) {
  int O = 0;
  const int rc = dc_heads_args("deconf_heads_fwd", hd, x, cat_t, cont_t, B, F, n, &O);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(ws && out && adell_aligned16(ws), "deconf_heads_fwd: bad pointer");
  hipStream_t st = (hipStream_t)stream;
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, 16, st));
  const double cs = hd->n_heads ? (double)conf_mult / ((double)B * hd->n_heads) : 0.0;
  const double rs = hd->n_cont ? (double)conf_mult / ((double)B * hd->n_cont) : 0.0;
  return adell_launch<adell_deconf_heads_fwd_kernel>(dim3((unsigned)B), dim3(DC_NT), 0, st, *hd, x, cat_t,
                                                     cont_t, B, F, n, O, cs, rs, (unsigned*)ws, ws + 2,
                                                     out);
}

extern "C" int adell_deconf_heads_bwd(const adell_deconf_heads* hd, const adell_deconf_head_grads* gr,
                                      const float* x, const long long* cat_t, const float* cont_t,
                                      const float* g_cat, const float* g_cont, int B, int F, int n,
                                      float conf_mult, double* dz, float* dx, void* stream) {
  int O = 0;
  const int rc = dc_heads_args("deconf_heads_bwd", hd, x, cat_t, cont_t, B, F, n, &O);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dz && (dx || gr), "deconf_heads_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const double cs = hd->n_heads ? (double)conf_mult / ((double)B * hd->n_heads) : 0.0;
  const double rs = hd->n_cont ? (double)conf_mult / ((double)B * hd->n_cont) : 0.0;
  const int rc1 = adell_launch<adell_deconf_heads_bwd_kernel>(dim3((unsigned)B), dim3(DC_NT), 0, st, *hd, x,
                                                              cat_t, cont_t, g_cat, g_cont, B, F, n, O, cs,
                                                              rs, dz, dx);
  if (rc1 != ADELL_OK || gr == nullptr) return rc1;
  const long elems = (long)O * (n + 1);
  return adell_launch<adell_deconf_heads_wgrad_kernel>(dim3((unsigned)((elems + DC_NT - 1) / DC_NT)),
                                                       dim3(DC_NT), 0, st, *gr, *hd, x,
                                                       (const double*)dz, B, F, n, O);
}
