// Kernels of the ensemble classifiers (adell_mri/modules/classification/classification/ensemble.py)
// and of the Gaussian-process head they end in (adell_mri/modules/layers/gaussian_process.py, the SNGP
// head of arXiv:2006.10108). House rules of mil.hip: fp32 in and out, dense inputs, no float atomics,
// every sum in a fixed order in fp64 -- two runs are bit-identical. cosf / sinf are the accurate ones.
//   * gp_phi, ONE launch forward, a block per row: x^ = LayerNorm(x) (or x), z = -W x^ + b,
//     phi = scale cos(z), logits = phi weights^T. x^ [i] and phi [r] live in LDS (GP_MAX_I, GP_MAX_R:
//     20 KB, so eight blocks share a CU); a wave per output feature walks a row of W. Saved: phi (an
//     output anyway), the row mean and rstd. Backward, two launches: per row z again, dphi = dlogits
//     weights + the gradient that arrived on phi, dz = scale sin(z) dphi, dx^ = W^T dz... the sign:
//     d cos(z) = -sin(z) dz and dz / dx^ = -W, so dx^ = W^T (scale sin(z) dphi); then the LayerNorm
//     backward of the row. dx^ is kept [N, i]; the second launch sums dgamma, dbeta (over the rows in
//     order) and dweights = dlogits^T phi. W and b are buffers: no gradient.
//     Beyond the limits the layer is composed from layer_norm / linear and gp_cos (one launch each
//     way): phi = scale cos(b - t), dt = scale sin(b - t) dphi. adell_gp_route decides.
//   * gp_precision_update, one launch, in place: U = sum_n c_n phi_n phi_n^T over n in order, c_n the
//     sum over the row of p (1 - p); P += U or P = m P + (1 - m) U. 16 x 16 tiles of the upper
//     triangle; every entry is computed once and stored at (a, b) and (b, a): P is exactly symmetric.
//   * gp_variance, one launch: var_n = phi_n^T S phi_n, a block per row, a wave per row of S.
//   * gp_sample, one launch: samples[s][n][o] = mean + sqrt(max(var, 0)) eps, and the mean and the
//     unbiased standard deviation over s (S = 1: NaN, as torch.std).
//   * ensemble_pool, one launch each way: up to ENS_MAX members [B, V_k, C_k] (NDHWC; V_k = 1 for a
//     vector) max-pooled over the voxels into their slice of one [B, sum C_k] buffer, int32 arg-max,
//     lowest index on a tie, the first NaN wins (adell_channel_max's convention). The members'
//     pointers travel by value.
//   * ensemble_average, one launch each way: the mean of K [B, C] logit tensors, then sigmoid (C = 1)
//     or softmax.
#include "common.h"

constexpr int ENS_NT = 256;
constexpr int ENS_NW = ENS_NT / 64;
constexpr int GP_MAX_I = 1024;          // input features the fused route keeps in LDS
constexpr int GP_MAX_R = 4096;          // random features the fused route keeps in LDS
constexpr int GP_TILE = 16;             // precision update: tile edge
constexpr int GP_NCHUNK = 32;           // precision update: rows of phi staged at once
constexpr int ENS_MAX = ADELL_ENSEMBLE_MAX;

struct EnsMembers {
  const float* x[ENS_MAX];
  float* dx[ENS_MAX];
  long V[ENS_MAX];
  int C[ENS_MAX];
  int off[ENS_MAX + 1];
  int K;
};

struct EnsLogits {
  const float* x[ENS_MAX];
  float* dx[ENS_MAX];
  int K;
};

// sum of one double per thread over the block, the waves added in order; every thread gets it.
// `red` holds ENS_NW doubles; the caller's next use of `red` must follow a __syncthreads of its own.
__device__ __forceinline__ double ens_block_sum_d(double v, double* red) {
  v = adell_wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < ENS_NW; ++w) s += red[w];
  return s;
}

// The row's x^ into sx [I] (mean and rstd returned) and z into sz [R].
__device__ __forceinline__ void gp_row_z(const float* __restrict__ xr, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, const float* __restrict__ W,
                                         const float* __restrict__ bvec, int I, int R, float eps,
                                         bool norm, float* sx, float* sz, double* red, float* mean_out,
                                         float* rstd_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (norm) {
    double s = 0.0;
    for (int k = threadIdx.x; k < I; k += ENS_NT) s += (double)xr[k];
    const double mean = ens_block_sum_d(s, red) / (double)I;
    double q = 0.0;
    for (int k = threadIdx.x; k < I; k += ENS_NT) {
      const double d = (double)xr[k] - mean;
      q += d * d;
    }
    const double var = ens_block_sum_d(q, red) / (double)I;
    const float mf = (float)mean, rs = (float)(1.0 / sqrt(var + (double)eps));
    for (int k = threadIdx.x; k < I; k += ENS_NT) sx[k] = (xr[k] - mf) * rs * gamma[k] + beta[k];
    *mean_out = mf;
    *rstd_out = rs;
  } else {
    for (int k = threadIdx.x; k < I; k += ENS_NT) sx[k] = xr[k];
  }
  __syncthreads();
  for (int j = wave; j < R; j += ENS_NW) {
    const float* wr = W + (size_t)j * I;
    double acc = 0.0;
    for (int k = lane; k < I; k += 64) acc += (double)wr[k] * (double)sx[k];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) sz[j] = (float)((double)bvec[j] - acc);
  }
  __syncthreads();
}

__global__ __launch_bounds__(ENS_NT) void adell_gp_phi_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ W, const float* __restrict__ bvec, const float* __restrict__ weights,
    int I, int R, int O, float scale, float eps, float* __restrict__ phi, float* __restrict__ logits,
    float* __restrict__ mean, float* __restrict__ rstd) {
  extern __shared__ float gp_sm[];
  __shared__ double red[ENS_NW];
  float* sx = gp_sm;
  float* sz = gp_sm + I;
  const size_t n = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool norm = gamma != nullptr;
  float mf = 0.f, rs = 1.f;
  gp_row_z(x + n * I, gamma, beta, W, bvec, I, R, eps, norm, sx, sz, red, &mf, &rs);
  if (norm && threadIdx.x == 0) {
    mean[n] = mf;
    rstd[n] = rs;
  }
  for (int j = threadIdx.x; j < R; j += ENS_NT) {
    const float p = scale * cosf(sz[j]);
    sz[j] = p;
    phi[n * R + j] = p;
  }
  __syncthreads();
  if (logits == nullptr) return;
  for (int o = wave; o < O; o += ENS_NW) {
    const float* wr = weights + (size_t)o * R;
    double acc = 0.0;
    for (int j = lane; j < R; j += 64) acc += (double)sz[j] * (double)wr[j];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) logits[n * O + o] = (float)acc;
  }
}

// A block per row. dxhat [N][I] is written for the second launch (and IS dx without the norm).
__global__ __launch_bounds__(ENS_NT) void adell_gp_phi_bwd_row_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ W, const float* __restrict__ bvec, const float* __restrict__ weights,
    const float* __restrict__ dlogits, const float* __restrict__ dphi, int I, int R, int O, float scale,
    float eps, float* __restrict__ dx, float* __restrict__ dxhat) {
  extern __shared__ float gp_sm[];
  __shared__ double red[ENS_NW];
  float* sx = gp_sm;
  float* sz = gp_sm + I;
  const size_t n = blockIdx.x;
  const bool norm = gamma != nullptr;
  float mf = 0.f, rs = 1.f;
  const float* xr = x + n * I;
  gp_row_z(xr, gamma, beta, W, bvec, I, R, eps, norm, sx, sz, red, &mf, &rs);
  // sz[j] <- scale sin(z_j) (dlogits weights + dphi)_j
  for (int j = threadIdx.x; j < R; j += ENS_NT) {
    double g = dphi != nullptr ? (double)dphi[n * R + j] : 0.0;
    if (dlogits != nullptr)
      for (int o = 0; o < O; ++o) g += (double)dlogits[n * O + o] * (double)weights[(size_t)o * R + j];
    sz[j] = (float)((double)(scale * sinf(sz[j])) * g);
  }
  __syncthreads();
  // sx[k] <- dx^_k = sum_j W[j][k] sz[j], j in order (the lanes read a row of W side by side)
  for (int k = threadIdx.x; k < I; k += ENS_NT) {
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < R; ++j) acc += (double)W[(size_t)j * I + k] * (double)sz[j];
    sx[k] = (float)acc;
    if (dxhat != nullptr) dxhat[n * I + k] = (float)acc;
  }
  if (dx == nullptr || !norm) return;      // without the norm dxhat is dx
  __syncthreads();
  // LayerNorm backward of the row: g = dx^ gamma, xt = (x - mean) rstd,
  // dx = rstd (g - mean(g) - xt mean(g xt))
  double s1 = 0.0, s2 = 0.0;
  for (int k = threadIdx.x; k < I; k += ENS_NT) {
    const double g = (double)sx[k] * (double)gamma[k];
    s1 += g;
    s2 += g * (double)((xr[k] - mf) * rs);
  }
  const double m1 = ens_block_sum_d(s1, red) / (double)I;
  const double m2 = ens_block_sum_d(s2, red) / (double)I;
  for (int k = threadIdx.x; k < I; k += ENS_NT) {
    const double g = (double)sx[k] * (double)gamma[k];
    const double xt = (double)((xr[k] - mf) * rs);
    dx[n * I + k] = (float)((double)rs * (g - m1 - xt * m2));
  }
}

// Threads [0, I): dgamma[k] = sum_n dx^[n][k] xt[n][k], dbeta[k] = sum_n dx^[n][k]; threads
// [I, I + O R): dweights[o][j] = sum_n dlogits[n][o] phi[n][j]. n in order, fp64.
__global__ __launch_bounds__(ENS_NT) void adell_gp_phi_bwd_sum_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ dxhat, const float* __restrict__ dlogits, const float* __restrict__ phi,
    int N, int In, int I, int R, int O, float* __restrict__ dgamma, float* __restrict__ dbeta,
    float* __restrict__ dweights) {
  const long t = (long)blockIdx.x * ENS_NT + threadIdx.x;
  if (t < In) {
    const int k = (int)t;
    double ag = 0.0, ab = 0.0;
    for (int n = 0; n < N; ++n) {
      const float d = dxhat[(size_t)n * I + k];
      ag += (double)d * (double)((x[(size_t)n * I + k] - mean[n]) * rstd[n]);
      ab += (double)d;
    }
    dgamma[k] = (float)ag;
    dbeta[k] = (float)ab;
    return;
  }
  const long e = t - In;
  if (dweights == nullptr || e >= (long)O * R) return;
  const int o = (int)(e / R), j = (int)(e - (long)o * R);
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc += (double)dlogits[(size_t)n * O + o] * (double)phi[(size_t)n * R + j];
  dweights[e] = (float)acc;
}

// The epilogue of the composed route: t = x^ W^T [rows][R].
__global__ __launch_bounds__(ENS_NT) void adell_gp_cos_kernel(const float* __restrict__ t,
                                                              const float* __restrict__ bvec,
                                                              const float* __restrict__ dphi, long total,
                                                              int R, float scale, float* __restrict__ out) {
  const long e = (long)blockIdx.x * ENS_NT + threadIdx.x;
  if (e >= total) return;
  const float z = bvec[e % R] - t[e];
  out[e] = dphi == nullptr ? scale * cosf(z) : scale * sinf(z) * dphi[e];
}

// Block (ta, tb), ta <= tb: the 16 x 16 tile of P at rows 16 ta, columns 16 tb. Thread (a, b).
__global__ __launch_bounds__(GP_TILE* GP_TILE) void adell_gp_precision_kernel(
    const float* __restrict__ phi, const float* __restrict__ prob, int N, int R, int Cp, int momentum,
    float m, float* __restrict__ P) {
  const int ta = blockIdx.y, tb = blockIdx.x;
  if (ta > tb) return;
  __shared__ float sa[GP_NCHUNK][GP_TILE], sb[GP_NCHUNK][GP_TILE];
  __shared__ double sc[GP_NCHUNK];
  const int la = threadIdx.x / GP_TILE, lb = threadIdx.x % GP_TILE;
  const int a = ta * GP_TILE + la, b = tb * GP_TILE + lb;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += GP_NCHUNK) {
    const int nn = min(GP_NCHUNK, N - n0);
    __syncthreads();
    for (int e = threadIdx.x; e < nn * GP_TILE; e += GP_TILE * GP_TILE) {
      const int r = e / GP_TILE, c = e % GP_TILE;
      const int ca = ta * GP_TILE + c, cb = tb * GP_TILE + c;
      sa[r][c] = ca < R ? phi[(size_t)(n0 + r) * R + ca] : 0.f;
      sb[r][c] = cb < R ? phi[(size_t)(n0 + r) * R + cb] : 0.f;
    }
    if (threadIdx.x < nn) {
      const float* pr = prob + (size_t)(n0 + threadIdx.x) * Cp;
      double c = 0.0;
      for (int k = 0; k < Cp; ++k) c += (double)pr[k] * (1.0 - (double)pr[k]);
      sc[threadIdx.x] = c;
    }
    __syncthreads();
    for (int r = 0; r < nn; ++r) acc += sc[r] * (double)sa[r][la] * (double)sb[r][lb];
  }
  if (a >= R || b >= R || a > b) return;
  const size_t at = (size_t)a * R + b;
  const double old = (double)P[at];
  const float v = momentum ? (float)((double)m * old + (1.0 - (double)m) * acc) : (float)(old + acc);
  P[at] = v;
  if (a != b) P[(size_t)b * R + a] = v;
}

__global__ __launch_bounds__(ENS_NT) void adell_gp_variance_kernel(const float* __restrict__ phi,
                                                                   const float* __restrict__ cov, int R,
                                                                   float* __restrict__ var) {
  __shared__ double red[ENS_NW];
  const size_t n = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* pr = phi + n * R;
  double acc = 0.0;
  for (int a = wave; a < R; a += ENS_NW) {
    const float* cr = cov + (size_t)a * R;
    double row = 0.0;
    for (int b = lane; b < R; b += 64) row += (double)cr[b] * (double)pr[b];
    row = adell_wave_sum_d(row);
    acc += (double)pr[a] * row;
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < ENS_NW; ++w) s += red[w];
    var[n] = (float)s;
  }
}

// A thread per (n, o).
__global__ __launch_bounds__(ENS_NT) void adell_gp_sample_kernel(
    const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ eps, int S,
    long NO, int O, float* __restrict__ samples, float* __restrict__ smean, float* __restrict__ sstd) {
  const long e = (long)blockIdx.x * ENS_NT + threadIdx.x;
  if (e >= NO) return;
  const float mu = mean[e], sd = sqrtf(fmaxf(var[e / O], 0.f));
  double sum = 0.0;
  for (int s = 0; s < S; ++s) {
    const float v = mu + sd * eps[(size_t)s * NO + e];
    samples[(size_t)s * NO + e] = v;
    sum += (double)v;
  }
  const double m = sum / (double)S;
  double ss = 0.0;
  for (int s = 0; s < S; ++s) {
    const double d = (double)(mu + sd * eps[(size_t)s * NO + e]) - m;
    ss += d * d;
  }
  smean[e] = (float)m;
  sstd[e] = (float)sqrt(ss / (double)(S - 1));       // S = 1: 0 / 0, NaN as torch.std
}

// Block (chunk, b): a thread per channel of the concatenated row.
__global__ __launch_bounds__(ENS_NT) void adell_ensemble_pool_fwd_kernel(EnsMembers mb,
                                                                         float* __restrict__ out,
                                                                         int* __restrict__ arg) {
  const int Ct = mb.off[mb.K];
  const int cg = blockIdx.x * ENS_NT + threadIdx.x;
  if (cg >= Ct) return;
  const size_t b = blockIdx.y;
  int k = 0;
  while (k + 1 < mb.K && cg >= mb.off[k + 1]) ++k;
  const int C = mb.C[k], c = cg - mb.off[k];
  const long V = mb.V[k];
  const float* xb = mb.x[k] + b * (size_t)V * C;
  float best = xb[c];
  long at = 0;
  for (long v = 1; v < V; ++v) {
    const float t = xb[v * C + c];
    if (t > best || (t != t && best == best)) {
      best = t;
      at = v;
    }
  }
  out[b * Ct + cg] = best;
  arg[b * Ct + cg] = (int)at;
}

// Block (blocks, k, b): member k's dense gradient of item b.
__global__ __launch_bounds__(ENS_NT) void adell_ensemble_pool_bwd_kernel(EnsMembers mb,
                                                                         const float* __restrict__ g,
                                                                         const int* __restrict__ arg) {
  const int k = blockIdx.y;
  const size_t b = blockIdx.z;
  float* dx = mb.dx[k];
  if (dx == nullptr) return;
  const int Ct = mb.off[mb.K], C = mb.C[k];
  const long VC = mb.V[k] * C;
  const float* gb = g + b * Ct + mb.off[k];
  const int* ab = arg + b * Ct + mb.off[k];
  float* db = dx + b * (size_t)VC;
  for (long i = blockIdx.x * (long)ENS_NT + threadIdx.x; i < VC; i += (long)gridDim.x * ENS_NT) {
    const int c = (int)(i % C);
    db[i] = ab[c] == i / C ? gb[c] : 0.f;
  }
}

// A thread per item b. dy == nullptr: y = sigmoid / softmax of the members' mean. Else the gradient of
// the mean from y and dy, a K-th of it to every member.
__global__ __launch_bounds__(ENS_NT) void adell_ensemble_average_kernel(EnsLogits lg, int B, int C,
                                                                        float* __restrict__ y,
                                                                        const float* __restrict__ dy) {
  const int b = blockIdx.x * ENS_NT + threadIdx.x;
  if (b >= B) return;
  const size_t base = (size_t)b * C;
  if (dy == nullptr) {
    auto mean_of = [&](int c) {
      double s = 0.0;
      for (int k = 0; k < lg.K; ++k) s += (double)lg.x[k][base + c];
      return (float)(s / (double)lg.K);
    };
    if (C == 1) {
      y[base] = 1.0f / (1.0f + expf(-mean_of(0)));
      return;
    }
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, mean_of(c));
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += (double)expf(mean_of(c) - mx);
    for (int c = 0; c < C; ++c) y[base + c] = (float)((double)expf(mean_of(c) - mx) / sum);
    return;
  }
  double dot = 0.0;
  if (C > 1)
    for (int c = 0; c < C; ++c) dot += (double)y[base + c] * (double)dy[base + c];
  for (int c = 0; c < C; ++c) {
    const double yy = (double)y[base + c], d = (double)dy[base + c];
    const double dm = C == 1 ? yy * (1.0 - yy) * d : yy * (d - dot);
    const float each = (float)(dm / (double)lg.K);
    for (int k = 0; k < lg.K; ++k)
      if (lg.dx[k] != nullptr) lg.dx[k][base + c] = each;
  }
}

// ---- host side -----------------------------------------------------------------------------------------
extern "C" int adell_gp_route(int n, int i, int r) {
  ADELL_REQUIRE(n > 0 && i > 0 && r > 0, "gp_route: bad arguments");
  return (i <= GP_MAX_I && r <= GP_MAX_R) ? ADELL_GP_FUSED : ADELL_GP_COMPOSED;
}

static int gp_phi_args(const char* what, int N, int I, int R, int O) {
  ADELL_REQUIRE(N > 0 && I > 0 && R > 0 && O >= 0, "%s: bad arguments", what);
  ADELL_REQUIRE(I <= GP_MAX_I && R <= GP_MAX_R,
                "%s: %d inputs and %d random features, the fused route takes at most %d and %d "
                "(adell_gp_route says which route a shape takes)", what, I, R, GP_MAX_I, GP_MAX_R);
  return ADELL_OK;
}

extern "C" int adell_gp_phi_fwd(const float* x, const float* gamma, const float* beta, const float* W,
                                const float* b, const float* weights, int N, int I, int R, int O,
                                float scale, float eps, float* phi, float* logits, float* mean,
                                float* rstd, void* stream) {
  const int rc = gp_phi_args("gp_phi_fwd", N, I, R, O);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && W && b && phi, "gp_phi_fwd: null pointer");
  ADELL_REQUIRE((gamma == nullptr) == (beta == nullptr), "gp_phi_fwd: gamma and beta go together");
  ADELL_REQUIRE(gamma == nullptr || (mean && rstd), "gp_phi_fwd: the norm needs mean and rstd buffers");
  ADELL_REQUIRE(logits == nullptr || (weights && O > 0), "gp_phi_fwd: logits without weights");
  return adell_launch<adell_gp_phi_fwd_kernel>(dim3((unsigned)N), dim3(ENS_NT),
                                               (size_t)(I + R) * sizeof(float), (hipStream_t)stream, x,
                                               gamma, beta, W, b, weights, I, R, O, scale, eps, phi,
                                               logits, mean, rstd);
}

extern "C" int adell_gp_phi_bwd(const float* x, const float* gamma, const float* beta, const float* W,
                                const float* b, const float* weights, const float* phi,
                                const float* mean, const float* rstd, const float* dlogits,
                                const float* dphi, int N, int I, int R, int O, float scale, float eps,
                                float* dx, float* dxhat, float* dgamma, float* dbeta, float* dweights,
                                void* stream) {
  const int rc = gp_phi_args("gp_phi_bwd", N, I, R, O);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && W && b && (dlogits || dphi), "gp_phi_bwd: null pointer");
  ADELL_REQUIRE((gamma == nullptr) == (beta == nullptr), "gp_phi_bwd: gamma and beta go together");
  ADELL_REQUIRE(dlogits == nullptr || (weights && O > 0), "gp_phi_bwd: dlogits without weights");
  ADELL_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "gp_phi_bwd: dgamma and dbeta go together");
  ADELL_REQUIRE(dgamma == nullptr || (gamma && mean && rstd && dxhat),
                "gp_phi_bwd: dgamma needs the norm, its statistics and the dxhat buffer");
  ADELL_REQUIRE(dweights == nullptr || (dlogits && phi), "gp_phi_bwd: dweights needs dlogits and phi");
  ADELL_REQUIRE(gamma != nullptr || dx == nullptr || dx == dxhat || dxhat == nullptr,
                "gp_phi_bwd: without the norm dxhat is dx");
  hipStream_t st = (hipStream_t)stream;
  if (dx != nullptr || dxhat != nullptr) {
    // without the norm the row kernel writes its dx^ where dx is wanted
    float* hat = gamma != nullptr ? dxhat : (dx != nullptr ? dx : dxhat);
    const int rc2 = adell_launch<adell_gp_phi_bwd_row_kernel>(
        dim3((unsigned)N), dim3(ENS_NT), (size_t)(I + R) * sizeof(float), st, x, gamma, beta, W, b,
        weights, dlogits, dphi, I, R, O, scale, eps, dx, hat);
    if (rc2 != ADELL_OK) return rc2;
  }
  const int In = dgamma != nullptr ? I : 0;
  const long work = In + (dweights != nullptr ? (long)O * R : 0);
  if (work == 0) return ADELL_OK;
  return adell_launch<adell_gp_phi_bwd_sum_kernel>(dim3((unsigned)((work + ENS_NT - 1) / ENS_NT)),
                                                   dim3(ENS_NT), 0, st, x, mean, rstd,
                                                   (const float*)dxhat, dlogits, phi, N, In, I, R, O,
                                                   dgamma, dbeta, dweights);
}

extern "C" int adell_gp_cos(const float* t, const float* b, const float* dphi, long rows, int R,
                            float scale, float* out, void* stream) {
  ADELL_REQUIRE(t && b && out && rows > 0 && R > 0, "gp_cos: bad arguments");
  const long total = rows * R, blocks = (total + ENS_NT - 1) / ENS_NT;
  ADELL_REQUIRE(blocks <= 0x7fffffffL, "gp_cos: too many elements");
  return adell_launch<adell_gp_cos_kernel>(dim3((unsigned)blocks), dim3(ENS_NT), 0, (hipStream_t)stream,
                                           t, b, dphi, total, R, scale, out);
}

extern "C" int adell_gp_precision_update(const float* phi, const float* prob, int N, int R, int Cp,
                                         int use_momentum, float m, float* P, void* stream) {
  ADELL_REQUIRE(phi && prob && P && N > 0 && R > 0 && Cp > 0, "gp_precision_update: bad arguments");
  const int tiles = adell_cdiv(R, GP_TILE);
  ADELL_REQUIRE(tiles <= 65535, "gp_precision_update: too many random features");
  return adell_launch<adell_gp_precision_kernel>(dim3((unsigned)tiles, (unsigned)tiles),
                                                 dim3(GP_TILE * GP_TILE), 0, (hipStream_t)stream, phi,
                                                 prob, N, R, Cp, use_momentum ? 1 : 0, m, P);
}

extern "C" int adell_gp_variance(const float* phi, const float* cov, int N, int R, float* var,
                                 void* stream) {
  ADELL_REQUIRE(phi && cov && var && N > 0 && R > 0, "gp_variance: bad arguments");
  return adell_launch<adell_gp_variance_kernel>(dim3((unsigned)N), dim3(ENS_NT), 0, (hipStream_t)stream,
                                                phi, cov, R, var);
}

extern "C" int adell_gp_sample(const float* mean, const float* var, const float* eps, int S, int N,
                               int O, float* samples, float* smean, float* sstd, void* stream) {
  ADELL_REQUIRE(mean && var && eps && samples && smean && sstd && S > 0 && N > 0 && O > 0,
                "gp_sample: bad arguments");
  const long NO = (long)N * O, blocks = (NO + ENS_NT - 1) / ENS_NT;
  ADELL_REQUIRE(blocks <= 0x7fffffffL, "gp_sample: too many elements");
  return adell_launch<adell_gp_sample_kernel>(dim3((unsigned)blocks), dim3(ENS_NT), 0,
                                              (hipStream_t)stream, mean, var, eps, S, NO, O, samples,
                                              smean, sstd);
}

static int ens_members(const char* what, int K, int B, const int* C, const long* V, EnsMembers* mb) {
  ADELL_REQUIRE(K > 0 && K <= ENS_MAX, "%s: %d members, 1 to %d go in one launch", what, K, ENS_MAX);
  ADELL_REQUIRE(B > 0 && B <= 65535 && C && V, "%s: bad arguments", what);
  mb->K = K;
  long off = 0;
  for (int k = 0; k < K; ++k) {
    ADELL_REQUIRE(C[k] > 0 && V[k] > 0 && V[k] < (1L << 31), "%s: member %d is empty or too large", what, k);
    mb->C[k] = C[k];
    mb->V[k] = V[k];
    mb->off[k] = (int)off;
    off += C[k];
    ADELL_REQUIRE(off <= 0x7fffffffL / 2, "%s: too many channels", what);
  }
  mb->off[K] = (int)off;
  for (int k = K; k < ENS_MAX; ++k) {
    mb->x[k] = nullptr;
    mb->dx[k] = nullptr;
  }
  return ADELL_OK;
}

extern "C" int adell_ensemble_pool_fwd(const float* const* x, const int* C, const long* V, int K, int B,
                                       float* out, int* arg, void* stream) {
  EnsMembers mb;
  const int rc = ens_members("ensemble_pool_fwd", K, B, C, V, &mb);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && out && arg, "ensemble_pool_fwd: null pointer");
  for (int k = 0; k < K; ++k) {
    ADELL_REQUIRE(x[k], "ensemble_pool_fwd: member %d is null", k);
    mb.x[k] = x[k];
    mb.dx[k] = nullptr;
  }
  return adell_launch<adell_ensemble_pool_fwd_kernel>(dim3((unsigned)adell_cdiv(mb.off[K], ENS_NT),
                                                           (unsigned)B),
                                                      dim3(ENS_NT), 0, (hipStream_t)stream, mb, out, arg);
}

extern "C" int adell_ensemble_pool_bwd(const float* g, const int* arg, const int* C, const long* V,
                                       int K, int B, float* const* dx, void* stream) {
  EnsMembers mb;
  const int rc = ens_members("ensemble_pool_bwd", K, B, C, V, &mb);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(g && arg && dx, "ensemble_pool_bwd: null pointer");
  long most = 0;
  for (int k = 0; k < K; ++k) {
    mb.x[k] = nullptr;
    mb.dx[k] = dx[k];
    if (dx[k] != nullptr) most = std::max(most, V[k] * C[k]);
  }
  if (most == 0) return ADELL_OK;
  const long blocks = std::min<long>((most + ENS_NT - 1) / ENS_NT, 1024);
  return adell_launch<adell_ensemble_pool_bwd_kernel>(dim3((unsigned)blocks, (unsigned)K, (unsigned)B),
                                                      dim3(ENS_NT), 0, (hipStream_t)stream, mb, g, arg);
}

static int ens_logits(const char* what, int K, int B, int C, EnsLogits* lg) {
  ADELL_REQUIRE(K > 0 && K <= ENS_MAX, "%s: %d members, 1 to %d go in one launch", what, K, ENS_MAX);
  ADELL_REQUIRE(B > 0 && C > 0, "%s: bad arguments", what);
  lg->K = K;
  for (int k = 0; k < ENS_MAX; ++k) {
    lg->x[k] = nullptr;
    lg->dx[k] = nullptr;
  }
  return ADELL_OK;
}

extern "C" int adell_ensemble_average_fwd(const float* const* x, int K, int B, int C, float* y,
                                          void* stream) {
  EnsLogits lg;
  const int rc = ens_logits("ensemble_average_fwd", K, B, C, &lg);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && y, "ensemble_average_fwd: null pointer");
  for (int k = 0; k < K; ++k) {
    ADELL_REQUIRE(x[k], "ensemble_average_fwd: member %d is null", k);
    lg.x[k] = x[k];
  }
  return adell_launch<adell_ensemble_average_kernel>(dim3((unsigned)adell_cdiv(B, ENS_NT)), dim3(ENS_NT),
                                                     0, (hipStream_t)stream, lg, B, C, y,
                                                     (const float*)nullptr);
}

extern "C" int adell_ensemble_average_bwd(const float* y, const float* dy, int K, int B, int C,
                                          float* const* dx, void* stream) {
  EnsLogits lg;
  const int rc = ens_logits("ensemble_average_bwd", K, B, C, &lg);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(y && dy && dx, "ensemble_average_bwd: null pointer");
  for (int k = 0; k < K; ++k) lg.dx[k] = dx[k];
  return adell_launch<adell_ensemble_average_kernel>(dim3((unsigned)adell_cdiv(B, ENS_NT)), dim3(ENS_NT),
                                                     0, (hipStream_t)stream, lg, B, C,
                                                     const_cast<float*>(y), dy);
}
