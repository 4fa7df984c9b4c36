// Kernels of the DDPM diffusion path (adell_mri/modules/diffusion/unet.py, diffusion_process.py;
// modules/layers/class_attention.py). House rules of mil.hip: fp32 in and out, dense inputs, no float
// atomics, every sum in a fixed order with fp64 accumulation -- two runs are bit-identical. All of
// them are bandwidth- or launch-bound; none uses MFMA.
//   * gate logits (EfficientConditioningAttentionBlock, op_type="linear") of ALL sites of a network in
//     ONE launch: a block per (site, embedding row). The block builds the sinusoidal timestep
//     embedding (cos half, sin half, zero pad; the argument t * exp(-ln(10000) k / half) and its cosine
//     / sine in fp64, rounded once: at an integer t near 1000 an fp32 argument alone is off by 6e-5),
//     adds the class-embedding row, then runs class_to_channels -> SiLU -> Linear -> LayerNorm -> SiLU
//     -> Linear with one wave per output row (fp64 dot products, wave butterfly) and every vector in
//     LDS. What the backward needs (h0, a0, xhat, h2, a2, rstd) goes to a record per (site, row).
//     Backward, TWO launches for all sites: (1) a block per (site, row) walks the chain back (thread j
//     owns column j of the transposed products) and leaves dh0, dh1, dh2 in the record; (2) a wave per
//     parameter row adds the outer products over the rows in order (weights, biases, LayerNorm gamma /
//     beta), and one more block per embedding row adds W0^T dh0 over the sites in order: the gradient
//     of the class embedding. The sites' pointers travel as a kernel argument (at most 32 sites).
//   * gate apply: y = x * sigmoid(z[n or 0][c]) on NDHWC memory, one launch; the block keeps the C
//     sigmoids in LDS (accurate expf, C per block instead of one per element). Backward, one pass over
//     x and dy: dx = dy * s and the per-(item, tile, channel) fp64 partial sums of dy * x; a small
//     second kernel folds tiles (and items, when one gate row serves the batch) in order into dz =
//     s (1 - s) sum.
//   * noising: sqrt(ab[t_n]) x + sqrt(1 - ab[t_n]) eps per item, t read on the device; a t outside the
//     table is never an index and makes the item NaN.
//   * reverse step (DDPM / DDIM / alpha-deblending) with the classifier-free guidance blend folded in:
//     one launch; the scalar coefficients are computed by the host in fp64.
//   * mean squared error: one launch forward (fp64 partial per block; the block that takes the last
//     ticket of an integer counter folds them in index order), one launch backward.
#include "common.h"

constexpr int DIF_NT = 256;              // threads per block
constexpr int DIF_NW = DIF_NT / 64;      // waves per block
constexpr int ECA_MAX_SITES = 32;        // sites per grouped launch (a kernel argument of < 4 KiB)
constexpr int ECA_MAX_DIM = 1024;        // widest site / embedding the gate kernels keep in LDS
constexpr int ECA_APPLY_MAX_C = 16384;   // channels whose sigmoids fit the apply kernels' LDS
constexpr int MSE_MAX_BLOCKS = 1024;

// accurate expf: 1 / (1 + exp(-x)); exp(-x) overflows to +inf for x < -88 and the quotient is 0
__device__ __forceinline__ float dif_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float dif_silu(float x) { return x * dif_sigmoid(x); }
__device__ __forceinline__ float dif_silu_grad(float x) {
  const float s = dif_sigmoid(x);
  return s * (1.0f + x * (1.0f - s));
}

// ---- gate logits ---------------------------------------------------------------------------------------
// p: class_to_channels.weight [C][T], .bias [C], op.1.weight [C][C], op.1.bias, op.2.weight (gamma),
// op.2.bias (beta), op.4.weight [C][C], op.4.bias. Record of (site, row g), 8 C + 4 floats at
// rec + g (8 C + 4): h0 | a0 | xhat | h2 | a2 | dh0 | dh1 | dh2 | rstd.
struct EcaFwdSite {
  const float* p[8];
  float* z;        // [Ng][C]
  float* rec;
  long C;
};
struct EcaFwdArgs { EcaFwdSite s[ECA_MAX_SITES]; };
struct EcaBwd1Site {
  const float* p[8];
  const float* gz;   // [Ng][C] or null (no gradient arrived: zeros)
  float* rec;
  long C;
};
struct EcaBwd1Args { EcaBwd1Site s[ECA_MAX_SITES]; };
struct EcaBwd2Site {
  float* dp[8];
  const float* gz;
  const float* rec;
  const float* w0;
  long C;
};
struct EcaBwd2Args { EcaBwd2Site s[ECA_MAX_SITES]; };

// out[c] = b[c] + sum_k W[c][k] in[k]: a wave per row, lanes along k, fp64
__device__ __forceinline__ void dif_matvec(const float* __restrict__ W, const float* __restrict__ b,
                                           const float* in, float* out, int C, int K) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = wave; c < C; c += DIF_NW) {
    const float* w = W + (size_t)c * K;
    double acc = 0.0;
    for (int k = lane; k < K; k += 64) acc += (double)w[k] * (double)in[k];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) out[c] = (float)(acc + (double)b[c]);
  }
}

__global__ __launch_bounds__(DIF_NT) void adell_eca_gates_fwd_kernel(
    EcaFwdArgs a, const float* __restrict__ t, int Gt, const float* __restrict__ cls, int T, float eps,
    float* __restrict__ emb) {
  __shared__ float se[ECA_MAX_DIM], sa[ECA_MAX_DIM], sb[ECA_MAX_DIM];
  __shared__ double sred[2];
  const EcaFwdSite& site = a.s[blockIdx.x];
  const int g = blockIdx.y, C = (int)site.C, tid = threadIdx.x;
  float* rec = site.rec + (size_t)g * (8 * C + 4);
  const int half = T / 2;
  const double tv = t != nullptr ? (double)t[Gt == 1 ? 0 : g] : 0.0;
  for (int k = tid; k < T; k += DIF_NT) {
    float v = 0.f;
    if (t != nullptr && k < 2 * half) {
      const int kk = k < half ? k : k - half;
      const double arg = tv * exp(-9.210340371976184 * (double)kk / (double)half);   // ln(10000)
      v = (float)(k < half ? cos(arg) : sin(arg));
    }
    if (cls != nullptr) v += cls[(size_t)g * T + k];
    se[k] = v;
    if (blockIdx.x == 0) emb[(size_t)g * T + k] = v;
  }
  __syncthreads();
  dif_matvec(site.p[0], site.p[1], se, sa, C, T);           // h0
  __syncthreads();
  for (int c = tid; c < C; c += DIF_NT) {
    const float h = sa[c], act = dif_silu(h);
    rec[c] = h;
    rec[C + c] = act;
    sa[c] = act;
  }
  __syncthreads();
  dif_matvec(site.p[2], site.p[3], sa, sb, C, C);           // h1
  __syncthreads();
  if (tid < 64) {                                           // LayerNorm statistics, biased variance
    double s = 0.0;
    for (int c = tid; c < C; c += 64) s += (double)sb[c];
    const double mean = adell_wave_sum_d(s) / C;
    double v = 0.0;
    for (int c = tid; c < C; c += 64) {
      const double d = (double)sb[c] - mean;
      v += d * d;
    }
    v = adell_wave_sum_d(v) / C;
    if (tid == 0) {
      sred[0] = mean;
      sred[1] = 1.0 / sqrt(v + (double)eps);
    }
  }
  __syncthreads();
  const double mean = sred[0], rstd = sred[1];
  if (tid == 0) rec[8 * C] = (float)rstd;
  const float* gamma = site.p[4];
  const float* beta = site.p[5];
  for (int c = tid; c < C; c += DIF_NT) {
    const float xh = (float)(((double)sb[c] - mean) * rstd);
    const float h2 = xh * gamma[c] + beta[c];
    const float act = dif_silu(h2);
    rec[2 * C + c] = xh;
    rec[3 * C + c] = h2;
    rec[4 * C + c] = act;
    sa[c] = act;
  }
  __syncthreads();
  dif_matvec(site.p[6], site.p[7], sa, site.z + (size_t)g * C, C, C);
}

// in[j] <- sum_c W[c][j] v[c] (v in LDS), thread j owns column j, c in order, fp64
__device__ __forceinline__ double dif_matvec_t(const float* __restrict__ W, const float* v, int C,
                                               int j) {
  double acc = 0.0;
  for (int c = 0; c < C; ++c) acc += (double)W[(size_t)c * C + j] * (double)v[c];
  return acc;
}

__global__ __launch_bounds__(DIF_NT) void adell_eca_gates_bwd1_kernel(EcaBwd1Args a) {
  __shared__ float sa[ECA_MAX_DIM], sb[ECA_MAX_DIM];
  __shared__ double sred[2];
  const EcaBwd1Site& site = a.s[blockIdx.x];
  const int g = blockIdx.y, C = (int)site.C, tid = threadIdx.x;
  float* rec = site.rec + (size_t)g * (8 * C + 4);
  for (int c = tid; c < C; c += DIF_NT) sa[c] = site.gz != nullptr ? site.gz[(size_t)g * C + c] : 0.f;
  __syncthreads();
  const float* gamma = site.p[4];
  for (int j = tid; j < C; j += DIF_NT) {
    const float dh2 = (float)dif_matvec_t(site.p[6], sa, C, j) * dif_silu_grad(rec[3 * C + j]);
    rec[7 * C + j] = dh2;
    sb[j] = dh2 * gamma[j];                                // d xhat
  }
  __syncthreads();
  if (tid < 64) {
    double m1 = 0.0, m2 = 0.0;
    for (int c = tid; c < C; c += 64) {
      m1 += (double)sb[c];
      m2 += (double)sb[c] * (double)rec[2 * C + c];
    }
    m1 = adell_wave_sum_d(m1) / C;
    m2 = adell_wave_sum_d(m2) / C;
    if (tid == 0) {
      sred[0] = m1;
      sred[1] = m2;
    }
  }
  __syncthreads();
  const double m1 = sred[0], m2 = sred[1], rstd = (double)rec[8 * C];
  for (int j = tid; j < C; j += DIF_NT) {
    const float dh1 = (float)(rstd * ((double)sb[j] - m1 - (double)rec[2 * C + j] * m2));
    rec[6 * C + j] = dh1;
    sa[j] = dh1;
  }
  __syncthreads();
  for (int j = tid; j < C; j += DIF_NT)
    rec[5 * C + j] = (float)dif_matvec_t(site.p[2], sa, C, j) * dif_silu_grad(rec[j]);
}

// blockIdx.y < chunks: rows [4 y, 4 y + 4) of the site's parameters, a wave per row; above: embedding
// row y - chunks of the class-embedding gradient (site 0's column of the grid only).
__global__ __launch_bounds__(DIF_NT) void adell_eca_gates_bwd2_kernel(
    EcaBwd2Args a, int n_sites, int chunks, int Ng, int T, const float* __restrict__ emb,
    float* __restrict__ de) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if ((int)blockIdx.y >= chunks) {
    if (blockIdx.x != 0) return;
    const int g = blockIdx.y - chunks;
    for (int k = tid; k < T; k += DIF_NT) {
      double acc = 0.0;
      for (int s = 0; s < n_sites; ++s) {
        const int C = (int)a.s[s].C;
        const float* dh0 = a.s[s].rec + (size_t)g * (8 * C + 4) + 5 * C;
        const float* w0 = a.s[s].w0;
        for (int c = 0; c < C; ++c) acc += (double)w0[(size_t)c * T + k] * (double)dh0[c];
      }
      de[(size_t)g * T + k] = (float)acc;
    }
    return;
  }
  const EcaBwd2Site& site = a.s[blockIdx.x];
  const int C = (int)site.C, c = blockIdx.y * DIF_NW + wave;
  if (c >= C) return;
  const size_t RS = (size_t)8 * C + 4;
  const float* rec = site.rec;
  const float* gz = site.gz;
  for (int j = lane; j < C; j += 64) {
    double a2 = 0.0, a1 = 0.0;
    for (int g = 0; g < Ng; ++g) {
      const float* r = rec + g * RS;
      if (gz != nullptr) a2 += (double)gz[(size_t)g * C + c] * (double)r[4 * C + j];
      a1 += (double)r[6 * C + c] * (double)r[C + j];
    }
    site.dp[6][(size_t)c * C + j] = (float)a2;
    site.dp[2][(size_t)c * C + j] = (float)a1;
  }
  for (int k = lane; k < T; k += 64) {
    double a0 = 0.0;
    for (int g = 0; g < Ng; ++g) a0 += (double)rec[g * RS + 5 * C + c] * (double)emb[(size_t)g * T + k];
    site.dp[0][(size_t)c * T + k] = (float)a0;
  }
  if (lane == 0) {
    double b2 = 0.0, b1 = 0.0, b0 = 0.0, dg = 0.0, db = 0.0;
    for (int g = 0; g < Ng; ++g) {
      const float* r = rec + g * RS;
      if (gz != nullptr) b2 += (double)gz[(size_t)g * C + c];
      b1 += (double)r[6 * C + c];
      b0 += (double)r[5 * C + c];
      dg += (double)r[7 * C + c] * (double)r[2 * C + c];
      db += (double)r[7 * C + c];
    }
    site.dp[7][c] = (float)b2;
    site.dp[3][c] = (float)b1;
    site.dp[1][c] = (float)b0;
    site.dp[4][c] = (float)dg;
    site.dp[5][c] = (float)db;
  }
}

// table rows (host memory, 64-bit words): fwd C, p0..p7, z, rec; bwd C, p0..p7, gz, rec, dp0..dp7
constexpr int ECA_FWD_WORDS = 11, ECA_BWD_WORDS = 19;

static int eca_gates_dims(const char* what, const long long* table, int words, int n_sites, int Ng,
                          int T, int* maxC) {
  ADELL_REQUIRE(table && n_sites >= 1 && n_sites <= ECA_MAX_SITES, "%s: 1..%d sites per call, got %d",
                what, ECA_MAX_SITES, n_sites);
  ADELL_REQUIRE(Ng >= 1 && Ng <= 65535 && T >= 1 && T <= ECA_MAX_DIM,
                "%s: %d embedding rows of %d values (at most 65535 rows of %d)", what, Ng, T,
                ECA_MAX_DIM);
  *maxC = 0;
  for (int s = 0; s < n_sites; ++s) {
    const long long* row = table + (size_t)s * words;
    ADELL_REQUIRE(row[0] >= 1 && row[0] <= ECA_MAX_DIM, "%s: site %d has %lld channels (1..%d)", what,
                  s, row[0], ECA_MAX_DIM);
    for (int i = 1; i < words; ++i)
      ADELL_REQUIRE(row[i] != 0 || (words == ECA_BWD_WORDS && i == 9), "%s: site %d: null pointer %d",
                    what, s, i);
    if (row[0] > *maxC) *maxC = (int)row[0];
  }
  return ADELL_OK;
}

extern "C" int adell_eca_gates_fwd(const long long* table, int n_sites, const float* t, int Gt,
                                   const float* cls, int Ng, int T, float eps, float* emb,
                                   void* stream) {
  int maxC;
  const int rc = eca_gates_dims("eca_gates_fwd", table, ECA_FWD_WORDS, n_sites, Ng, T, &maxC);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(emb && (t ? (Gt == 1 || Gt == Ng) : cls != nullptr),
                "eca_gates_fwd: %d timesteps for %d rows (or no timesteps and no class rows)", Gt, Ng);
  EcaFwdArgs a = {};
  for (int s = 0; s < n_sites; ++s) {
    const long long* row = table + (size_t)s * ECA_FWD_WORDS;
    a.s[s].C = row[0];
    for (int i = 0; i < 8; ++i) a.s[s].p[i] = (const float*)(uintptr_t)row[1 + i];
    a.s[s].z = (float*)(uintptr_t)row[9];
    a.s[s].rec = (float*)(uintptr_t)row[10];
  }
  return adell_launch<adell_eca_gates_fwd_kernel>(dim3(n_sites, Ng), dim3(DIF_NT), 0,
                                                  (hipStream_t)stream, a, t, Gt, cls, T, eps, emb);
}

extern "C" int adell_eca_gates_bwd(const long long* table, int n_sites, const float* emb, float* de,
                                   int Ng, int T, void* stream) {
  int maxC;
  const int rc = eca_gates_dims("eca_gates_bwd", table, ECA_BWD_WORDS, n_sites, Ng, T, &maxC);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(emb, "eca_gates_bwd: null embedding");
  EcaBwd1Args a1 = {};
  EcaBwd2Args a2 = {};
  for (int s = 0; s < n_sites; ++s) {
    const long long* row = table + (size_t)s * ECA_BWD_WORDS;
    a1.s[s].C = a2.s[s].C = row[0];
    for (int i = 0; i < 8; ++i) {
      a1.s[s].p[i] = (const float*)(uintptr_t)row[1 + i];
      a2.s[s].dp[i] = (float*)(uintptr_t)row[11 + i];
    }
    a1.s[s].gz = a2.s[s].gz = (const float*)(uintptr_t)row[9];
    a1.s[s].rec = (float*)(uintptr_t)row[10];
    a2.s[s].rec = (const float*)(uintptr_t)row[10];
    a2.s[s].w0 = (const float*)(uintptr_t)row[1];
  }
  hipStream_t st = (hipStream_t)stream;
  const int rc1 = adell_launch<adell_eca_gates_bwd1_kernel>(dim3(n_sites, Ng), dim3(DIF_NT), 0, st, a1);
  if (rc1 != ADELL_OK) return rc1;
  const int chunks = adell_cdiv(maxC, DIF_NW);
  return adell_launch<adell_eca_gates_bwd2_kernel>(dim3(n_sites, chunks + (de != nullptr ? Ng : 0)),
                                                   dim3(DIF_NT), 0, st, a2, n_sites, chunks, Ng, T,
                                                   emb, de);
}

// ---- gate apply ------------------------------------------------------------------------------------------
// x, y [N][V][C] (NDHWC memory), z [Ng][C], Ng in {1, N}: zstride = 0 broadcasts the one gate row.
template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_eca_apply_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ z, int zstride, float* __restrict__ y,
    long VC, int C) {
  extern __shared__ __attribute__((aligned(16))) float eca_s[];
  const int n = blockIdx.y;
  const float* zb = z + (size_t)n * zstride;
  for (int c = threadIdx.x; c < C; c += DIF_NT) eca_s[c] = dif_sigmoid(zb[c]);
  __syncthreads();
  const float* xb = x + (size_t)n * VC;
  float* yb = y + (size_t)n * VC;
  const long step = (long)gridDim.x * DIF_NT * VEC;
  long i = ((long)blockIdx.x * DIF_NT + threadIdx.x) * VEC;
  int c = (int)(i % C);
  const int cstep = (int)(step % C);
  for (; i < VC; i += step) {
    if (VEC == 4) {
      const float4 v = *reinterpret_cast<const float4*>(xb + i);
      const float4 s = *reinterpret_cast<const float4*>(eca_s + c);
      *reinterpret_cast<float4*>(yb + i) = make_float4(v.x * s.x, v.y * s.y, v.z * s.z, v.w * s.w);
    } else {
      yb[i] = xb[i] * eca_s[c];
    }
    c += cstep;
    if (c >= C) c -= C;
  }
}

// Block (tile, n): voxels [tile vpt, (tile + 1) vpt) of item n. Thread (r, cl) = (tid / CGb, tid %
// CGb) owns column group cl (VEC channels) of every R-th voxel; R = 256 / CGb rows (threads past
// R CGb idle); CG = C / VEC column groups are walked CGb at a time. dx = dy s; part[n][tile][c] = the
// fp64 sum of dy x over the tile's voxels: per thread in voxel order, then over the rows in order.
template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_eca_apply_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ z,
    int zstride, float* __restrict__ dx, double* __restrict__ part, long V, int C, long vpt, int CGb,
    int R) {
  extern __shared__ __attribute__((aligned(16))) float eca_s[];
  __shared__ double sred[DIF_NT * VEC];
  const int n = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const float* zb = z + (size_t)n * zstride;
  if (dx != nullptr) {
    for (int c = tid; c < C; c += DIF_NT) eca_s[c] = dif_sigmoid(zb[c]);
    __syncthreads();
  }
  const long v0 = (long)tile * vpt;
  const long v1 = v0 + vpt < V ? v0 + vpt : V;
  const size_t base = (size_t)n * V * C;
  const int CG = C / VEC, r = tid / CGb, cl = tid - r * CGb;
  for (int cg0 = 0; cg0 < CG; cg0 += CGb) {
    const int cg = cg0 + cl;
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    if (r < R && cg < CG) {
      const int c = cg * VEC;
      for (long v = v0 + r; v < v1; v += R) {
        const size_t o = base + (size_t)v * C + c;
        if (VEC == 4) {
          const float4 xv = *reinterpret_cast<const float4*>(x + o);
          const float4 gv = *reinterpret_cast<const float4*>(dy + o);
          if (dx != nullptr) {
            const float4 s = *reinterpret_cast<const float4*>(eca_s + c);
            *reinterpret_cast<float4*>(dx + o) = make_float4(gv.x * s.x, gv.y * s.y, gv.z * s.z, gv.w * s.w);
          }
          acc[0] += (double)gv.x * (double)xv.x;
          acc[1 % VEC] += (double)gv.y * (double)xv.y;
          acc[2 % VEC] += (double)gv.z * (double)xv.z;
          acc[3 % VEC] += (double)gv.w * (double)xv.w;
        } else {
          const float gv = dy[o];
          if (dx != nullptr) dx[o] = gv * eca_s[c];
          acc[0] += (double)gv * (double)x[o];
        }
      }
    }
    if (part == nullptr) continue;
#pragma unroll
    for (int e = 0; e < VEC; ++e) sred[tid * VEC + e] = acc[e];
    __syncthreads();
    if (r == 0 && cg < CG) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double tot = 0.0;
        for (int rr = 0; rr < R; ++rr) tot += sred[(rr * CGb + cl) * VEC + e];
        part[((size_t)n * gridDim.x + tile) * C + cg * VEC + e] = tot;
      }
    }
    __syncthreads();
  }
}

// dz[g][c] = s (1 - s) sum over the rows of part that belong to gate row g (tiles of item g, or of
// every item when Ng == 1): block = 64 channels x 4 row lanes, each a fixed share of the rows.
__global__ __launch_bounds__(DIF_NT) void adell_eca_apply_fold_kernel(
    const double* __restrict__ part, const float* __restrict__ z, float* __restrict__ dz, long rows,
    int C) {
  __shared__ double sh[DIF_NW][64];
  const int g = blockIdx.y, cl = threadIdx.x & 63, vl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const double* p = part + (size_t)g * rows * C;
  double acc = 0.0;
  if (c < C)
    for (long r = vl; r < rows; r += DIF_NW) acc += p[(size_t)r * C + c];
  sh[vl][cl] = acc;
  __syncthreads();
  if (vl != 0 || c >= C) return;
  acc = 0.0;
#pragma unroll
  for (int k = 0; k < DIF_NW; ++k) acc += sh[k][cl];
  const float s = dif_sigmoid(z[(size_t)g * C + c]);
  dz[(size_t)g * C + c] = (float)((double)(s * (1.0f - s)) * acc);
}

static int eca_apply_args(const char* what, const void* x, const void* z, int Ng, int N, long V, int C) {
  ADELL_REQUIRE(x && z && N >= 1 && N <= 65535 && V >= 1 && C >= 1 && C <= ECA_APPLY_MAX_C,
                "%s: bad arguments (N %d, V %ld, C %d; C <= %d)", what, N, V, C, ECA_APPLY_MAX_C);
  ADELL_REQUIRE(Ng == 1 || Ng == N, "%s: %d gate rows for %d items (1 or %d)", what, Ng, N, N);
  return ADELL_OK;
}

extern "C" int adell_eca_apply_fwd(const float* x, const float* z, int Ng, float* y, int N, long V,
                                   int C, void* stream) {
  const int rc = eca_apply_args("eca_apply_fwd", x, z, Ng, N, V, C);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(y, "eca_apply_fwd: null output");
  const long VC = V * C;
  const bool vec = C % 4 == 0 && adell_aligned16(x) && adell_aligned16(y);
  long blocks = (VC / (vec ? 4 : 1) + DIF_NT * 4 - 1) / (DIF_NT * 4);     // ~4 elements per thread
  const long cap = 2048 / N > 1 ? 2048 / N : 1;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const int zstride = Ng == 1 ? 0 : C;
  const dim3 grid((unsigned)blocks, (unsigned)N);
  const size_t lds = (size_t)C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (vec) return adell_launch<adell_eca_apply_fwd_kernel<4>>(grid, dim3(DIF_NT), lds, st, x, z, zstride, y, VC, C);
  return adell_launch<adell_eca_apply_fwd_kernel<1>>(grid, dim3(DIF_NT), lds, st, x, z, zstride, y, VC, C);
}

// rows of the backward's thread grid and tiles per item (>= 8 voxels per thread, at most 1024 tiles)
static void eca_apply_plan(long V, int C, bool vec, int* CGb, int* R, int* tiles) {
  const int CG = C / (vec ? 4 : 1);
  *CGb = CG < DIF_NT ? CG : DIF_NT;
  *R = DIF_NT / *CGb;
  long t = (V + (long)*R * 8 - 1) / ((long)*R * 8);
  if (t > 1024) t = 1024;
  if (t < 1) t = 1;
  *tiles = (int)t;
}

extern "C" long adell_eca_apply_bwd_workspace_doubles(int N, long V, int C) {
  if (N <= 0 || V <= 0 || C <= 0) return ADELL_E_BADARG;
  int CGb, R, tiles;
  // (the scalar plan never has fewer tiles than the vector one: size for it)
  eca_apply_plan(V, C, false, &CGb, &R, &tiles);
  return (long)N * tiles * C;
}

extern "C" int adell_eca_apply_bwd(const float* x, const float* dy, const float* z, int Ng, float* dx,
                                   float* dz, double* part, int N, long V, int C, void* stream) {
  const int rc = eca_apply_args("eca_apply_bwd", x, z, Ng, N, V, C);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dy && (dx || dz) && (dz == nullptr) == (part == nullptr),
                "eca_apply_bwd: null gradient, or dz without its workspace");
  const bool vec = C % 4 == 0 && adell_aligned16(x) && adell_aligned16(dy) &&
                   (dx == nullptr || adell_aligned16(dx));
  int CGb, R, tiles;
  eca_apply_plan(V, C, vec, &CGb, &R, &tiles);
  const long vpt = (V + tiles - 1) / tiles;
  const int zstride = Ng == 1 ? 0 : C;
  const dim3 grid((unsigned)tiles, (unsigned)N);
  const size_t lds = (size_t)C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  const int rc1 =
      vec ? adell_launch<adell_eca_apply_bwd_kernel<4>>(grid, dim3(DIF_NT), lds, st, x, dy, z, zstride, dx,
                                                        part, V, C, vpt, CGb, R)
          : adell_launch<adell_eca_apply_bwd_kernel<1>>(grid, dim3(DIF_NT), lds, st, x, dy, z, zstride, dx,
                                                        part, V, C, vpt, CGb, R);
  if (rc1 != ADELL_OK || dz == nullptr) return rc1;
  const long rows = Ng == 1 ? (long)N * tiles : tiles;
  return adell_launch<adell_eca_apply_fold_kernel>(dim3((unsigned)adell_cdiv(C, 64), (unsigned)Ng),
                                                   dim3(DIF_NT), 0, st, (const double*)part,
                                                   z, dz, rows, C);
}

// ---- noising -----------------------------------------------------------------------------------------------
// y[n][i] = sqrt(ab[t[n]]) x[n][i] + sqrt(1 - ab[t[n]]) eps[n][i]; M elements per item (an item is
// one contiguous piece in either dense layout)
template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_diffusion_noise_kernel(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ ab, int S,
    const long long* __restrict__ t, float* __restrict__ y, long M) {
  const int n = blockIdx.y;
  const long long tt = t[n];
  const float a = (tt >= 0 && tt < S) ? ab[tt] : __builtin_nanf("");
  const float ca = sqrtf(a), cb = sqrtf(1.0f - a);
  const float* xb = x + (size_t)n * M;
  const float* eb = eps + (size_t)n * M;
  float* yb = y + (size_t)n * M;
  const long step = (long)gridDim.x * DIF_NT * VEC;
  for (long i = ((long)blockIdx.x * DIF_NT + threadIdx.x) * VEC; i < M; i += step) {
    if (VEC == 4) {
      const float4 v = *reinterpret_cast<const float4*>(xb + i);
      const float4 e = *reinterpret_cast<const float4*>(eb + i);
      *reinterpret_cast<float4*>(yb + i) = make_float4(ca * v.x + cb * e.x, ca * v.y + cb * e.y,
                                                       ca * v.z + cb * e.z, ca * v.w + cb * e.w);
    } else {
      yb[i] = ca * xb[i] + cb * eb[i];
    }
  }
}

static long dif_blocks(long n, int vec, long cap) {
  long blocks = (n / vec + DIF_NT * 4 - 1) / (DIF_NT * 4);
  if (blocks > cap) blocks = cap;
  return blocks < 1 ? 1 : blocks;
}

extern "C" int adell_diffusion_noise(const float* x, const float* eps, const float* alpha_bar, int S,
                                     const long long* t, float* y, int N, long M, void* stream) {
  ADELL_REQUIRE(x && eps && alpha_bar && t && y && S >= 1 && N >= 1 && N <= 65535 && M >= 1,
                "diffusion_noise: bad arguments");
  const bool vec = M % 4 == 0 && adell_aligned16(x) && adell_aligned16(eps) && adell_aligned16(y);
  const dim3 grid((unsigned)dif_blocks(M, vec ? 4 : 1, 2048 / N > 1 ? 2048 / N : 1), (unsigned)N);
  hipStream_t st = (hipStream_t)stream;
  if (vec) return adell_launch<adell_diffusion_noise_kernel<4>>(grid, dim3(DIF_NT), 0, st, x, eps, alpha_bar, S, t, y, M);
  return adell_launch<adell_diffusion_noise_kernel<1>>(grid, dim3(DIF_NT), 0, st, x, eps, alpha_bar, S, t, y, M);
}

// ---- reverse step ----------------------------------------------------------------------------------------
// e = eu + scale (eps - eu) with guidance, else eps; x0 = (x - sb e) / sa, clamped to [-1, 1] on
// request; out = c_x0 x0 + c_x x + c_e e + c_n noise. The three step kinds differ in the coefficients
// alone (include/adell_hip.h).
struct DifStepCoef { float sb, sa, c_x0, c_x, c_e, c_n, scale; int flags; };

__device__ __forceinline__ float dif_step_one(const DifStepCoef& k, float x, float e, float eu,
                                              float nz, bool guided, bool noisy) {
  if (guided) e = eu + k.scale * (e - eu);
  float out = k.c_x * x + k.c_e * e;
  if (k.flags & ADELL_DIFFUSION_X0) {
    float x0 = (x - k.sb * e) / k.sa;
    if (k.flags & ADELL_DIFFUSION_CLIP) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    out += k.c_x0 * x0;
  }
  if (noisy) out += k.c_n * nz;
  return out;
}

template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_diffusion_step_kernel(
    const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ eu,
    const float* __restrict__ noise, float* __restrict__ out, long n, DifStepCoef k) {
  const bool guided = eu != nullptr, noisy = noise != nullptr;
  const long step = (long)gridDim.x * DIF_NT * VEC;
  for (long i = ((long)blockIdx.x * DIF_NT + threadIdx.x) * VEC; i < n; i += step) {
    if (VEC == 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + i);
      const float4 ev = *reinterpret_cast<const float4*>(eps + i);
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 uv = guided ? *reinterpret_cast<const float4*>(eu + i) : z4;
      const float4 nv = noisy ? *reinterpret_cast<const float4*>(noise + i) : z4;
      *reinterpret_cast<float4*>(out + i) =
          make_float4(dif_step_one(k, xv.x, ev.x, uv.x, nv.x, guided, noisy),
                      dif_step_one(k, xv.y, ev.y, uv.y, nv.y, guided, noisy),
                      dif_step_one(k, xv.z, ev.z, uv.z, nv.z, guided, noisy),
                      dif_step_one(k, xv.w, ev.w, uv.w, nv.w, guided, noisy));
    } else {
      out[i] = dif_step_one(k, x[i], eps[i], guided ? eu[i] : 0.f, noisy ? noise[i] : 0.f, guided,
                            noisy);
    }
  }
}

extern "C" int adell_diffusion_reverse_step(const float* x, const float* eps, const float* eps_uncond,
                                            const float* noise, float* out, long n, float sb, float sa,
                                            float c_x0, float c_x, float c_e, float c_n, float scale,
                                            int flags, void* stream) {
  ADELL_REQUIRE(x && eps && out && n >= 1, "diffusion_reverse_step: bad arguments");
  const DifStepCoef k = {sb, sa, c_x0, c_x, c_e, c_n, scale, flags};
  const bool vec = n % 4 == 0 && adell_aligned16(x) && adell_aligned16(eps) && adell_aligned16(out) &&
                   adell_aligned16(eps_uncond) && adell_aligned16(noise);
  const dim3 grid((unsigned)dif_blocks(n, vec ? 4 : 1, 2048));
  hipStream_t st = (hipStream_t)stream;
  if (vec) return adell_launch<adell_diffusion_step_kernel<4>>(grid, dim3(DIF_NT), 0, st, x, eps, eps_uncond, noise, out, n, k);
  return adell_launch<adell_diffusion_step_kernel<1>>(grid, dim3(DIF_NT), 0, st, x, eps, eps_uncond, noise, out, n, k);
}

// ---- mean squared error ------------------------------------------------------------------------------------
// ws: 16 bytes of ticket counter (zeroed by a memset node in front of every launch), then one double
// per block. Every block sums its grid-stride share in fp64 (thread order, wave butterfly, waves in
// order), publishes the partial with an agent-scope atomic store and takes a ticket with an agent-scope
// acquire-release add; the block that draws the last ticket reads the partials back with agent-scope
// loads and folds them in index order -- the same order whichever block that is. Nothing spins.
template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_mse_fwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, long n, double inv_n,
    unsigned* counter, double* part, float* __restrict__ loss) {
  __shared__ double sw[DIF_NW];
  __shared__ int last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double acc = 0.0;
  const long step = (long)gridDim.x * DIF_NT * VEC;
  for (long i = ((long)blockIdx.x * DIF_NT + tid) * VEC; i < n; i += step) {
    if (VEC == 4) {
      const float4 p = *reinterpret_cast<const float4*>(pred + i);
      const float4 q = *reinterpret_cast<const float4*>(target + i);
      const double d0 = (double)p.x - (double)q.x, d1 = (double)p.y - (double)q.y;
      const double d2 = (double)p.z - (double)q.z, d3 = (double)p.w - (double)q.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    } else {
      const double d = (double)pred[i] - (double)target[i];
      acc += d * d;
    }
  }
  acc = adell_wave_sum_d(acc);
  if (lane == 0) sw[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < DIF_NW; ++w) tot += sw[w];
    __hip_atomic_store(part + blockIdx.x, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = ticket == gridDim.x - 1;
  }
  __syncthreads();
  if (!last || wave != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double tot = 0.0;
  for (int b = lane; b < (int)gridDim.x; b += 64)
    tot += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = adell_wave_sum_d(tot);
  if (lane == 0) loss[0] = (float)(tot * inv_n);
}

template <int VEC>
__global__ __launch_bounds__(DIF_NT) void adell_mse_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ g,
    float scale, long n, float* __restrict__ dpred) {
  const float k = g[0] * scale;
  const long step = (long)gridDim.x * DIF_NT * VEC;
  for (long i = ((long)blockIdx.x * DIF_NT + threadIdx.x) * VEC; i < n; i += step) {
    if (VEC == 4) {
      const float4 p = *reinterpret_cast<const float4*>(pred + i);
      const float4 q = *reinterpret_cast<const float4*>(target + i);
      *reinterpret_cast<float4*>(dpred + i) =
          make_float4(k * (p.x - q.x), k * (p.y - q.y), k * (p.z - q.z), k * (p.w - q.w));
    } else {
      dpred[i] = k * (pred[i] - target[i]);
    }
  }
}

extern "C" long adell_mse_workspace_bytes(void) { return 16 + (long)MSE_MAX_BLOCKS * sizeof(double); }

extern "C" int adell_mse_fwd(const float* pred, const float* target, long n, void* ws, float* loss,
                             void* stream) {
  ADELL_REQUIRE(pred && target && ws && loss && n >= 1 && adell_aligned16(ws), "mse_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, 16, st));
  unsigned* counter = (unsigned*)ws;
  double* part = (double*)((char*)ws + 16);
  const bool vec = n % 4 == 0 && adell_aligned16(pred) && adell_aligned16(target);
  const dim3 grid((unsigned)dif_blocks(n, vec ? 4 : 1, MSE_MAX_BLOCKS));
  if (vec) return adell_launch<adell_mse_fwd_kernel<4>>(grid, dim3(DIF_NT), 0, st, pred, target, n, 1.0 / (double)n, counter, part, loss);
  return adell_launch<adell_mse_fwd_kernel<1>>(grid, dim3(DIF_NT), 0, st, pred, target, n, 1.0 / (double)n, counter, part, loss);
}

extern "C" int adell_mse_bwd(const float* pred, const float* target, const float* g, long n,
                             float* dpred, void* stream) {
  ADELL_REQUIRE(pred && target && g && dpred && n >= 1, "mse_bwd: bad arguments");
  const float scale = (float)(2.0 / (double)n);
  const bool vec = n % 4 == 0 && adell_aligned16(pred) && adell_aligned16(target) && adell_aligned16(dpred);
  const dim3 grid((unsigned)dif_blocks(n, vec ? 4 : 1, 2048));
  hipStream_t st = (hipStream_t)stream;
  if (vec) return adell_launch<adell_mse_bwd_kernel<4>>(grid, dim3(DIF_NT), 0, st, pred, target, g, scale, n, dpred);
  return adell_launch<adell_mse_bwd_kernel<1>>(grid, dim3(DIF_NT), 0, st, pred, target, g, scale, n, dpred);
}
