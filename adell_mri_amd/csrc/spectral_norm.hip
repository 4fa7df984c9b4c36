// Spectral normalisation of a weight (torch.nn.utils.parametrizations._SpectralNorm, which the
// reference's utils/pl_callbacks.SpectralNorm puts on every weight): n power iterations
//   u <- normalize(W v, eps), v <- normalize(W^T u, eps), normalize(x) = x / max(|x|, eps),
// then sigma = u^T W v and W_sn = W / sigma. House rules of deconfound.hip: fp32 data, every sum in
// fp64 in a fixed order, no float atomics (an integer ticket names the block that finishes last, it
// folds in index order), bit-reproducible, nothing read on the host: shapes and eps are launch
// arguments. u and v are rounded to fp32 where torch stores them, and the rounded values are what
// every later product uses.
//
// ONE index map serves both `dim` values, without a permuted copy of the weight: the matrix is
// [h][w], w = outer * inner, and element (r, c = o * inner + t) lives at (o * h + r) * inner + t.
// dim = 0 is outer = 1; a transposed-conv weight [Cin][Cout][k...] is outer = Cin, h = Cout,
// inner = prod(k). W_sn and dW are written in the weight's own layout.
//
//   * block route (sn_block_fwd / sn_block_bwd), one launch each whatever n is: one workgroup of
//     1024 threads keeps W (as [h][w] rows), u, v and the fp64 products in LDS.
//     Bound: 4 (h w + h + w) + 8 (max(h, w) + 1040) <= 158 KiB.
//   * grid route, 2 n + 1 launches forward (2 in eval mode), 2 backward:
//       sn_rows   a block per row takes (W v)[r]; the last ticket normalises into u (or, in eval
//                 mode, takes sigma = u . (W v));
//       sn_cols   a thread per column and a block row per chunk of up to 32 row chunks takes the
//                 partial (W^T u)[c] of its chunk; the last ticket folds the chunks in order,
//                 normalises into v and takes sigma = (W^T u) . v, the same number as u^T W v;
//       sn_scale  W / sigma, and the copies of u and v this forward used;
//       sn_dot    <G, W_sn> over at most 1024 blocks, the last ticket folds;
//       sn_grad   dW = (G - <G, W_sn> u v^T) / sigma.
//     Bound: h, w <= 32768.
// Training mode takes sigma from the last half-iteration: (W^T u) . v with the rounded v.
// A zero weight gives u = v = 0, sigma = 0 and NaN everywhere in W_sn, as torch does.
#include "common.h"

constexpr int SN_NT = 1024;             // block route
constexpr int SN_NW = SN_NT / 64;
constexpr int SN_GT = 256;              // grid route
constexpr int SN_GW = SN_GT / 64;
constexpr int SN_MAX_CHUNKS = 32;       // row chunks of sn_cols
constexpr int SN_DOT_BLOCKS = 1024;     // blocks of sn_dot
constexpr long SN_BLOCK_LDS = 158 * 1024;

__device__ __forceinline__ long sn_addr(int r, int c, int h, int inner) {
  const int o = c / inner, t = c - o * inner;
  return ((long)o * h + r) * inner + t;
}

// the sum over the block in a fixed order; every thread of the block calls it
template <int NW>
__device__ __forceinline__ double sn_block_sum(double v, double* sw) {
  v = adell_wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < NW; ++i) tot += sw[i];
  return tot;
}

__device__ __forceinline__ double sn_floor(double nrm2, double eps) {
  const double n = sqrt(nrm2);
  return n > eps ? n : eps;      // NaN: eps, the quotient below is NaN anyway
}

// ---- block route ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SN_NT) void adell_sn_block_fwd_kernel(
    const float* __restrict__ W, float* u, float* v, int outer, int h, int inner, int n_iter, double eps,
    float* __restrict__ u_used, float* __restrict__ v_used, double* __restrict__ sigma,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char sn_smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int w = outer * inner, m = h > w ? h : w;
  const int N = h * w, hi = h * inner;
  double* tmp = (double*)sn_smem;          // [max(h, w)]
  double* part = tmp + m;                  // [SN_NT]
  double* sw = part + SN_NT;               // [SN_NW]
  float* Ws = (float*)(sw + SN_NW);        // [h][w]
  float* us = Ws + N;
  float* vs = us + h;
  for (int i = tid; i < N; i += SN_NT) {
    const int o = i / hi, rem = i - o * hi, r = rem / inner, t = rem - r * inner;
    Ws[r * w + o * inner + t] = W[i];
  }
  for (int r = tid; r < h; r += SN_NT) us[r] = u[r];
  for (int c = tid; c < w; c += SN_NT) vs[c] = v[c];
  __syncthreads();
  // row groups of the transposed product: G threads share a column when the matrix is narrow
  int G = w <= SN_NT / 2 ? SN_NT / w : 1;
  G = G > h ? h : G;
  const int per = (h + G - 1) / G;
  double sig = 0.0;
  const int passes = n_iter > 0 ? n_iter : 1;
  for (int it = 0; it < passes; ++it) {
    // tmp[r] = (W v)[r]: a wave per row, the lanes over the columns
    for (int r = wave; r < h; r += SN_NW) {
      const float* row = Ws + r * w;
      double acc = 0.0;
      for (int c = lane; c < w; c += 64) acc += (double)row[c] * (double)vs[c];
      acc = adell_wave_sum_d(acc);
      if (lane == 0) tmp[r] = acc;
    }
    __syncthreads();
    if (n_iter == 0) {      // eval mode: sigma from the stored vectors
      double acc = 0.0;
      for (int r = tid; r < h; r += SN_NT) acc += (double)us[r] * tmp[r];
      sig = sn_block_sum<SN_NW>(acc, sw);
      break;
    }
    {
      double acc = 0.0;
      for (int r = tid; r < h; r += SN_NT) acc += tmp[r] * tmp[r];
      const double d = sn_floor(sn_block_sum<SN_NW>(acc, sw), eps);
      for (int r = tid; r < h; r += SN_NT) us[r] = (float)(tmp[r] / d);
    }
    __syncthreads();
    // tmp[c] = (W^T u)[c], the rows in order
    if (G > 1) {
      if (tid < G * w) {
        const int g = tid / w, c = tid - g * w;
        const int r1 = (g + 1) * per < h ? (g + 1) * per : h;
        double acc = 0.0;
        for (int r = g * per; r < r1; ++r) acc += (double)Ws[r * w + c] * (double)us[r];
        part[tid] = acc;
      }
      __syncthreads();
      if (tid < w) {
        double acc = 0.0;
        for (int g = 0; g < G; ++g) acc += part[g * w + tid];
        tmp[tid] = acc;
      }
    } else {
      for (int c = tid; c < w; c += SN_NT) {
        double acc = 0.0;
        for (int r = 0; r < h; ++r) acc += (double)Ws[r * w + c] * (double)us[r];
        tmp[c] = acc;
      }
    }
    __syncthreads();
    {
      double acc = 0.0;
      for (int c = tid; c < w; c += SN_NT) acc += tmp[c] * tmp[c];
      const double d = sn_floor(sn_block_sum<SN_NW>(acc, sw), eps);
      double s = 0.0;
      for (int c = tid; c < w; c += SN_NT) {
        const float vv = (float)(tmp[c] / d);
        vs[c] = vv;
        s += tmp[c] * (double)vv;
      }
      if (it == passes - 1) sig = sn_block_sum<SN_NW>(s, sw);
    }
    __syncthreads();
  }
  for (int r = tid; r < h; r += SN_NT) {
    const float x = us[r];
    if (n_iter > 0) u[r] = x;
    u_used[r] = x;
  }
  for (int c = tid; c < w; c += SN_NT) {
    const float x = vs[c];
    if (n_iter > 0) v[c] = x;
    v_used[c] = x;
  }
  if (tid == 0) sigma[0] = sig;
  for (int i = tid; i < N; i += SN_NT) {
    const int o = i / hi, rem = i - o * hi, r = rem / inner, t = rem - r * inner;
    out[i] = (float)((double)Ws[r * w + o * inner + t] / sig);
  }
}

__global__ __launch_bounds__(SN_NT) void adell_sn_block_bwd_kernel(
    const float* __restrict__ G, const float* __restrict__ Wsn, const float* __restrict__ u,
    const float* __restrict__ v, const double* __restrict__ sigma, int outer, int h, int inner,
    float* __restrict__ dW) {
  __shared__ double sw[SN_NW];
  const int tid = threadIdx.x;
  const int N = h * outer * inner, hi = h * inner;
  double acc = 0.0;
  for (int i = tid; i < N; i += SN_NT) acc += (double)G[i] * (double)Wsn[i];
  const double s = sn_block_sum<SN_NW>(acc, sw);
  const double sig = sigma[0];
  for (int i = tid; i < N; i += SN_NT) {
    const int o = i / hi, rem = i - o * hi, r = rem / inner, t = rem - r * inner;
    dW[i] = (float)(((double)G[i] - s * (double)u[r] * (double)v[o * inner + t]) / sig);
  }
}

// ---- grid route -------------------------------------------------------------------------------------------
// tid 0 of a block whose results are stored: the ticket; true in the block that finishes last
__device__ __forceinline__ bool sn_last_block(unsigned* counter, unsigned nblocks, int* last) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *last = ticket == nblocks - 1;
  }
  __syncthreads();
  if (!*last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}

__device__ __forceinline__ double sn_ld(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a [h] = W v; normalise: u <- a / max(|a|, eps); else sigma = u . a
__global__ __launch_bounds__(SN_GT) void adell_sn_rows_kernel(
    const float* __restrict__ W, const float* __restrict__ v, float* u, int outer, int h, int inner,
    int normalise, double eps, unsigned* counter, double* a, double* sigma) {
  __shared__ double sw[SN_GW];
  __shared__ int last;
  const int tid = threadIdx.x, r = blockIdx.x, w = outer * inner;
  double acc = 0.0;
  for (int c = tid; c < w; c += SN_GT) acc += (double)W[sn_addr(r, c, h, inner)] * (double)v[c];
  const double tot = sn_block_sum<SN_GW>(acc, sw);
  if (tid == 0) __hip_atomic_store(a + r, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!sn_last_block(counter, gridDim.x, &last)) return;
  if (normalise) {
    double n2 = 0.0;
    for (int i = tid; i < h; i += SN_GT) {
      const double x = sn_ld(a + i);
      n2 += x * x;
    }
    const double d = sn_floor(sn_block_sum<SN_GW>(n2, sw), eps);
    for (int i = tid; i < h; i += SN_GT) u[i] = (float)(sn_ld(a + i) / d);
  } else {
    double s = 0.0;
    for (int i = tid; i < h; i += SN_GT) s += (double)u[i] * sn_ld(a + i);
    s = sn_block_sum<SN_GW>(s, sw);
    if (tid == 0) sigma[0] = s;
  }
  if (tid == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// part [chunks][w]: the partial W^T u of each row chunk; then v <- b / max(|b|, eps), sigma = b . v
__global__ __launch_bounds__(SN_GT) void adell_sn_cols_kernel(
    const float* __restrict__ W, const float* __restrict__ u, float* v, int outer, int h, int inner,
    int per, double eps, unsigned* counter, double* part, double* b, double* sigma) {
  __shared__ double sw[SN_GW];
  __shared__ int last;
  const int tid = threadIdx.x, w = outer * inner;
  const int c = blockIdx.x * SN_GT + tid, k = blockIdx.y;
  if (c < w) {
    const int o = c / inner, t = c - o * inner;
    const int r0 = k * per, r1 = r0 + per < h ? r0 + per : h;
    const float* col = W + (long)o * h * inner + t;
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) acc += (double)col[(long)r * inner] * (double)u[r];
    __hip_atomic_store(part + (long)k * w + c, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!sn_last_block(counter, gridDim.x * gridDim.y, &last)) return;
  const int chunks = gridDim.y;
  double n2 = 0.0;
  for (int i = tid; i < w; i += SN_GT) {
    double x = 0.0;
    for (int j = 0; j < chunks; ++j) x += sn_ld(part + (long)j * w + i);
    b[i] = x;      // read again below by this thread alone
    n2 += x * x;
  }
  const double d = sn_floor(sn_block_sum<SN_GW>(n2, sw), eps);
  double s = 0.0;
  for (int i = tid; i < w; i += SN_GT) {
    const double x = b[i];
    const float vv = (float)(x / d);
    v[i] = vv;
    s += x * (double)vv;
  }
  s = sn_block_sum<SN_GW>(s, sw);
  if (tid == 0) {
    sigma[0] = s;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(SN_GT) void adell_sn_scale_kernel(
    const float* __restrict__ W, const double* __restrict__ sigma, const float* __restrict__ u,
    const float* __restrict__ v, long N, int h, int w, float* __restrict__ out,
    float* __restrict__ u_used, float* __restrict__ v_used) {
  const long step = (long)gridDim.x * SN_GT, first = (long)blockIdx.x * SN_GT + threadIdx.x;
  const double sig = sigma[0];
  for (long i = first; i < N; i += step) out[i] = (float)((double)W[i] / sig);
  for (long i = first; i < h; i += step) u_used[i] = u[i];
  for (long i = first; i < w; i += step) v_used[i] = v[i];
}

__global__ __launch_bounds__(SN_GT) void adell_sn_dot_kernel(
    const float* __restrict__ G, const float* __restrict__ Wsn, long N, unsigned* counter, double* part,
    double* dot) {
  __shared__ double sw[SN_GW];
  __shared__ int last;
  const int tid = threadIdx.x;
  const long step = (long)gridDim.x * SN_GT;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * SN_GT + tid; i < N; i += step) acc += (double)G[i] * (double)Wsn[i];
  acc = sn_block_sum<SN_GW>(acc, sw);
  if (tid == 0) __hip_atomic_store(part + blockIdx.x, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!sn_last_block(counter, gridDim.x, &last)) return;
  double tot = 0.0;
  for (unsigned j = tid; j < gridDim.x; j += SN_GT) tot += sn_ld(part + j);
  tot = sn_block_sum<SN_GW>(tot, sw);
  if (tid == 0) {
    dot[0] = tot;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(SN_GT) void adell_sn_grad_kernel(
    const float* __restrict__ G, const float* __restrict__ u, const float* __restrict__ v,
    const double* __restrict__ sigma, const double* __restrict__ dot, long N, int h, int inner,
    float* __restrict__ dW) {
  const long step = (long)gridDim.x * SN_GT, hi = (long)h * inner;
  const double sig = sigma[0], s = dot[0];
  for (long i = (long)blockIdx.x * SN_GT + threadIdx.x; i < N; i += step) {
    const long o = i / hi, rem = i - o * hi;
    const int r = (int)(rem / inner), t = (int)(rem - (long)r * inner);
    dW[i] = (float)(((double)G[i] - s * (double)u[r] * (double)v[o * inner + t]) / sig);
  }
}

// ---- host side --------------------------------------------------------------------------------------------
static size_t sn_block_lds(long h, long w) {
  return (size_t)(4 * (h * w + h + w) + 8 * ((h > w ? h : w) + SN_NT + SN_NW));
}

static int sn_route(long h, long w) {
  if (h > ADELL_SN_MAX_DIM || w > ADELL_SN_MAX_DIM) return ADELL_SN_COMPOSED;
  return sn_block_lds(h, w) <= (size_t)SN_BLOCK_LDS ? ADELL_SN_BLOCK : ADELL_SN_GRID;
}

extern "C" int adell_spectral_norm_route(long h, long w) {
  ADELL_REQUIRE(h >= 1 && w >= 1, "spectral_norm_route: bad matrix %ld x %ld", h, w);
  return sn_route(h, w);
}

static int sn_chunks(int h) {
  const int c = adell_cdiv(h, 64);
  return c > SN_MAX_CHUNKS ? SN_MAX_CHUNKS : c;
}

// the ticket counter's 16 bytes, then a [h], b [w], the chunk partials of sn_cols (or sn_dot's), its sum
extern "C" long adell_spectral_norm_workspace_doubles(long h, long w) {
  if (h < 1 || w < 1) return ADELL_E_BADARG;
  const int route = sn_route(h, w);
  if (route == ADELL_SN_COMPOSED) return ADELL_E_BADARG;
  if (route == ADELL_SN_BLOCK) return 2;
  const long parts = (long)sn_chunks((int)h) * w;
  return 2 + h + w + (parts > SN_DOT_BLOCKS ? parts : SN_DOT_BLOCKS) + 2;
}

static int sn_args(const char* what, int outer, int h, int inner, int* route) {
  ADELL_REQUIRE(outer >= 1 && h >= 1 && inner >= 1 && (long)outer * inner <= ADELL_SN_MAX_DIM,
                "%s: bad shape (outer %d, h %d, inner %d)", what, outer, h, inner);
  *route = sn_route(h, (long)outer * inner);
  ADELL_REQUIRE(*route != ADELL_SN_COMPOSED, "%s: beyond the fused routes (h, w <= %d)", what,
                ADELL_SN_MAX_DIM);
  return ADELL_OK;
}

static unsigned sn_flat_blocks(long n) {
  long blocks = (n + SN_GT * 4 - 1) / (SN_GT * 4);
  if (blocks > 2048) blocks = 2048;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int adell_spectral_norm_fwd(const float* W, float* u, float* v, int outer, int h, int inner,
                                       int n_iter, double eps, double* ws, long ws_doubles,
                                       float* u_used, float* v_used, double* sigma, float* out,
                                       void* stream) {
  int route = 0;
  const int rc = sn_args("spectral_norm_fwd", outer, h, inner, &route);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(W && u && v && u_used && v_used && sigma && out && n_iter >= 0,
                "spectral_norm_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int w = outer * inner;
  if (route == ADELL_SN_BLOCK)
    return adell_launch<adell_sn_block_fwd_kernel>(dim3(1), dim3(SN_NT), sn_block_lds(h, w), st, W, u, v,
                                                   outer, h, inner, n_iter, eps, u_used, v_used, sigma,
                                                   out);
  ADELL_REQUIRE(ws && adell_aligned16(ws) && ws_doubles >= adell_spectral_norm_workspace_doubles(h, w),
                "spectral_norm_fwd: workspace of %ld doubles, %ld needed", ws_doubles,
                adell_spectral_norm_workspace_doubles(h, w));
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, 16, st));
  unsigned* counter = (unsigned*)ws;
  double* a = ws + 2;
  double* b = a + h;
  double* part = b + w;
  const int chunks = sn_chunks(h), per = adell_cdiv(h, chunks);
  const int rows = adell_cdiv(h, per);      // chunks that hold a row
  if (n_iter == 0) {
    const int r1 = adell_launch<adell_sn_rows_kernel>(dim3((unsigned)h), dim3(SN_GT), 0, st, W,
                                                      (const float*)v, u, outer, h, inner, 0, eps,
                                                      counter, a, sigma);
    if (r1 != ADELL_OK) return r1;
  }
  for (int it = 0; it < n_iter; ++it) {
    const int r1 = adell_launch<adell_sn_rows_kernel>(dim3((unsigned)h), dim3(SN_GT), 0, st, W,
                                                      (const float*)v, u, outer, h, inner, 1, eps,
                                                      counter, a, sigma);
    if (r1 != ADELL_OK) return r1;
    const int r2 = adell_launch<adell_sn_cols_kernel>(
        dim3((unsigned)adell_cdiv(w, SN_GT), (unsigned)rows), dim3(SN_GT), 0, st, W, (const float*)u, v,
        outer, h, inner, per, eps, counter, part, b, sigma);
    if (r2 != ADELL_OK) return r2;
  }
  const long N = (long)h * w;
  return adell_launch<adell_sn_scale_kernel>(dim3(sn_flat_blocks(N)), dim3(SN_GT), 0, st, W,
                                             (const double*)sigma, (const float*)u, (const float*)v, N, h,
                                             w, out, u_used, v_used);
}

extern "C" int adell_spectral_norm_bwd(const float* G, const float* Wsn, const float* u, const float* v,
                                       const double* sigma, int outer, int h, int inner, double* ws,
                                       long ws_doubles, float* dW, void* stream) {
  int route = 0;
  const int rc = sn_args("spectral_norm_bwd", outer, h, inner, &route);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(G && Wsn && u && v && sigma && dW, "spectral_norm_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int w = outer * inner;
  if (route == ADELL_SN_BLOCK)
    return adell_launch<adell_sn_block_bwd_kernel>(dim3(1), dim3(SN_NT), 0, st, G, Wsn, u, v, sigma, outer,
                                                   h, inner, dW);
  ADELL_REQUIRE(ws && adell_aligned16(ws) && ws_doubles >= adell_spectral_norm_workspace_doubles(h, w),
                "spectral_norm_bwd: workspace of %ld doubles, %ld needed", ws_doubles,
                adell_spectral_norm_workspace_doubles(h, w));
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, 16, st));
  const long N = (long)h * w;
  long nb = (N + SN_GT * 8 - 1) / (SN_GT * 8);
  nb = nb > SN_DOT_BLOCKS ? SN_DOT_BLOCKS : nb;
  double* part = ws + 2;
  double* dot = part + SN_DOT_BLOCKS;
  const int r1 = adell_launch<adell_sn_dot_kernel>(dim3((unsigned)nb), dim3(SN_GT), 0, st, G, Wsn, N,
                                                   (unsigned*)ws, part, dot);
  if (r1 != ADELL_OK) return r1;
  return adell_launch<adell_sn_grad_kernel>(dim3(sn_flat_blocks(N)), dim3(SN_GT), 0, st, G, u, v, sigma,
                                            (const double*)dot, N, h, inner, dW);
}
