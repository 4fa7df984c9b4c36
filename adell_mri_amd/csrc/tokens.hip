// Token-sequence kernels of the ViT encoder in UNETR (reference:
// adell_mri/modules/layers/vit.py:844-1002, linear_blocks.py:358-417):
//   * LayerNorm over the last dimension (torch.nn.LayerNorm) forward/backward,
//   * broadcast add (X + positional_embedding) and its reduction backward,
//   * scaled-dot-product attention forward/backward with an optional additive
//     bias (F.scaled_dot_product_attention as called at linear_blocks.py:407-414).
// The Linear layers run on the conv kernel (a Linear is a 1x1x1 convolution over
// the token axis). Sequences are short (216 tokens at config 3): these kernels
// are latency/HBM-bound fp32 VALU code, one wave per row, wavefront-shuffle
// reductions, fixed summation order.
#include "common.h"

ADELL_RNG_STEP_DEFINE(tokens)

// ---------------------------------------------------------------------------
// LayerNorm: y = (x - mean) * rstd * gamma + beta over rows of length C.
// One wave per row. mean/rstd are saved for the backward.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adell_layernorm_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd, long rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float m = adell_wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = xr[c] - m;
    v += d * d;
  }
  const float r = rsqrtf(adell_wave_sum(v) / (float)C + eps);
  float* yr = y + row * C;
  for (int c = lane; c < C; c += 64) {
    float t = (xr[c] - m) * r;
    if (gamma) t *= gamma[c];
    if (beta) t += beta[c];
    yr[c] = t;
  }
  if (lane == 0) {
    mean[row] = m;
    rstd[row] = r;
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma. One wave per row, four rows
// per block: rows are independent, so the grid is rows / 4 blocks whatever C is (the first
// version walked 64 rows per block and accumulated dgamma / dbeta by LDS read-modify-write:
// 14 blocks and 4.9 ms for the [864, 4096] rescaler tensors of UNETR).
__global__ __launch_bounds__(256) void adell_layernorm_bwd_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ dy,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dx, long rows, int C) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * C;
  const float* gr = dy + row * C;
  const float m = mean[row], r = rstd[row];
  float a = 0.f, b = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float xh = (xr[c] - m) * r;
    const float g = gr[c] * (gamma ? gamma[c] : 1.f);
    a += g;
    b += g * xh;
  }
  a = adell_wave_sum(a) / (float)C;
  b = adell_wave_sum(b) / (float)C;
  float* dr = dx + row * C;
  for (int c = lane; c < C; c += 64) {   // second read of the row comes from L1 / L2
    const float xh = (xr[c] - m) * r;
    const float g = gr[c] * (gamma ? gamma[c] : 1.f);
    dr[c] = r * (g - a - xh * b);
  }
}

// dgamma / dbeta partials: grid (column tiles of 256, row chunks); thread = one column, walks the
// rows of its chunk (consecutive threads read consecutive columns: coalesced), fixed order.
// part[chunk][2][C] = (sum dy * xhat, sum dy) over the chunk's rows.
__global__ __launch_bounds__(256) void adell_layernorm_bwd_affine_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part, long rows, int C,
    int rows_per_chunk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const long r0 = (long)blockIdx.y * rows_per_chunk;
  long r1 = r0 + rows_per_chunk;
  if (r1 > rows) r1 = rows;
  if (c >= C) return;
  float sg = 0.f, sb = 0.f;
  for (long row = r0; row < r1; ++row) {
    const float d = dy[row * C + c];
    sg += d * (x[row * C + c] - mean[row]) * rstd[row];
    sb += d;
  }
  part[((size_t)blockIdx.y * 2 + 0) * C + c] = sg;
  part[((size_t)blockIdx.y * 2 + 1) * C + c] = sb;
}

__global__ __launch_bounds__(256) void adell_rowsum_final_kernel(
    const float* __restrict__ part, int nb, int n, float* __restrict__ out0,
    float* __restrict__ out1, int half) {
  __shared__ double sh[4][64];
  const int cl = threadIdx.x & 63, vl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0.0;
  if (c < n)
    for (int b = vl; b < nb; b += 4) s += (double)part[(size_t)b * n + c];
  sh[vl][cl] = s;
  __syncthreads();
  if (vl != 0 || c >= n) return;
  s = (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
  if (c < half) {
    if (out0) out0[c] = (float)s;
  } else if (out1) {
    out1[c - half] = (float)s;
  }
}

extern "C" int adell_layernorm_fwd(const float* x, const float* gamma, const float* beta,
                                   float* y, float* mean, float* rstd, long rows, int C,
                                   float eps, void* stream) {
  ADELL_REQUIRE(x && y && mean && rstd, "layernorm_fwd: null pointer");
  ADELL_REQUIRE(rows > 0 && C > 0, "layernorm_fwd: bad dims");
  hipLaunchKernelGGL(adell_layernorm_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, x, gamma, beta, y, mean, rstd, rows, C, eps);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// rows per chunk of the affine-gradient partials: enough chunks for ~512 blocks, >= 8 rows each
static int adell_ln_rows_per_chunk(long rows, int C) {
  const long tiles = (C + 255) / 256;
  long chunks = 512 / tiles;
  if (chunks < 1) chunks = 1;
  long rpc = (rows + chunks - 1) / chunks;
  if (rpc < 8) rpc = 8;
  return (int)rpc;
}
extern "C" long adell_layernorm_bwd_workspace(long rows, int C) {
  const int rpc = adell_ln_rows_per_chunk(rows, C);
  const long nb = (rows + rpc - 1) / rpc;
  return nb * 2 * C * (long)sizeof(float);
}

extern "C" int adell_layernorm_bwd(const float* x, const float* dy, const float* gamma,
                                   const float* mean, const float* rstd, float* dx,
                                   float* dgamma, float* dbeta, long rows, int C,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  ADELL_REQUIRE(x && dy && mean && rstd && dx, "layernorm_bwd: null pointer");
  ADELL_REQUIRE(rows > 0 && C > 0, "layernorm_bwd: bad dims");
  const bool want = dgamma || dbeta;
  if (want)
    ADELL_REQUIRE(workspace && (long)workspace_bytes >= adell_layernorm_bwd_workspace(rows, C),
                  "layernorm_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adell_layernorm_bwd_dx_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     st, x, dy, gamma, mean, rstd, dx, rows, C);
  if (want) {
    const int rpc = adell_ln_rows_per_chunk(rows, C);
    const int nb = (int)((rows + rpc - 1) / rpc);
    hipLaunchKernelGGL(adell_layernorm_bwd_affine_kernel, dim3(adell_cdiv(C, 256), nb), dim3(256),
                       0, st, x, dy, mean, rstd, (float*)workspace, rows, C, rpc);
    hipLaunchKernelGGL(adell_rowsum_final_kernel, dim3(adell_cdiv(2 * C, 64)), dim3(256), 0, st,
                       (const float*)workspace, nb, 2 * C, dgamma, dbeta, C);
  }
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---------------------------------------------------------------------------
// out[i] = a[i] + b[i % period]  and its backward db[j] = sum_k dout[k*period + j]
// ---------------------------------------------------------------------------
__global__ void adell_add_bcast_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                       float* __restrict__ out, long n, long period) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    out[i] = a[i] + b[i % period];
}
__global__ void adell_sum_bcast_kernel(const float* __restrict__ g, float* __restrict__ db,
                                       long n, long period) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < period;
       j += (long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (long i = j; i < n; i += period) s += g[i];
    db[j] = s;
  }
}
extern "C" int adell_add_bcast(const float* a, const float* b, float* out, long n, long period,
                               void* stream) {
  ADELL_REQUIRE(a && b && out && n > 0 && period > 0 && n % period == 0, "add_bcast: bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adell_add_bcast_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, a, b, out, n, period);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
extern "C" int adell_sum_bcast(const float* g, float* db, long n, long period, void* stream) {
  ADELL_REQUIRE(g && db && n > 0 && period > 0 && n % period == 0, "sum_bcast: bad arguments");
  long blocks = (period + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adell_sum_bcast_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, g, db, n, period);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---------------------------------------------------------------------------
// Attention. Q,K: [BH][T][A]; V,O: [BH][T][Dv]; bias: [nbias][T][T] or null
// (bias row for sequence bh is bh % nbias). scale = 1/sqrt(A) unless given.
// One wave per query row; keys streamed through LDS in tiles of 64 with an
// online softmax; lane j owns key j of the tile for the scores, lane d owns
// output column d (and d+64, ...) for the PV product.
// ---------------------------------------------------------------------------
#define ATT_TK 64
#define ATT_ROWS 16  // query rows per block (4 waves x 4 rows)

struct AttStride { long b, h, r; };

struct AttArgs {
  const float* q;
  const float* k;
  const float* v;
  const float* bias;
  const int* labels; // [nlab][T] region labels or null: -100 between tokens whose labels differ
  const float* o;    // bwd
  const float* dout; // bwd
  const float* lse;  // bwd: [BH][T] log-sum-exp of the scaled scores
  float* out;        // fwd: O ; bwd: unused
  float* lse_out;    // fwd
  float* dq;
  float* dk;
  float* dv;
  int T, A, Dv, nbias;
  int nlab, labH;    // item bh / labH reads label row (bh / labH) % nlab
  float scale;
  float drop_p;      // attention-probability dropout (0 = off)
  uint32_t seed_lo, seed_hi, rng_offset;
  // MFMA kernels: element strides of sequence bh = b * H + h (item b, head h) and of its token
  // rows, so that Q / K / V can be read inside a packed [B][T][H][q | k | v] projection and O,
  // dQ, dK, dV land in token-major buffers (contiguous [BH][T][*]: H = 1, {T * C, 0, C})
  int H;
  AttStride sq, sk, sv, so, sg, sdq, sdk, sdv;
};

__device__ __forceinline__ size_t att_base(const AttArgs& a, const AttStride& s, int bh) {
  return (size_t)(bh / a.H) * s.b + (size_t)(bh % a.H) * s.h;
}

// label row of sequence bh (null without labels) and the additive term of one (query, key) pair
__device__ __forceinline__ const int* att_labels(const AttArgs& a, int bh) {
  return a.labels ? a.labels + (size_t)((bh / a.labH) % a.nlab) * a.T : nullptr;
}
__device__ __forceinline__ float att_label_term(int lq, int lk) { return lq != lk ? -100.f : 0.f; }

// word `i` (0..3) of a Philox block by selects (indexing a local array with a run-time index puts the
// array in scratch memory)
__device__ __forceinline__ uint32_t adell_word4(const uint4& r, unsigned i) {
  return i == 0 ? r.x : (i == 1 ? r.y : (i == 2 ? r.z : r.w));
}

// Keep decision of probability (bh, qrow, kcol): a pure function of the seed, so the two
// backward kernels regenerate the mask the forward applied.
__device__ __forceinline__ bool adell_att_keep(const AttArgs& a, int bh, int qrow, int kcol) {
  if (a.drop_p <= 0.f) return true;
  const uint64_t e = ((uint64_t)bh * a.T + qrow) * a.T + kcol;
  const uint4 r = adell_philox4((uint32_t)(e >> 2), (uint32_t)(e >> 34), a.rng_offset + g_adell_rng_step, 2u,
                                a.seed_lo, a.seed_hi);
  return (float)(adell_word4(r, (unsigned)(e & 3)) >> 8) * (1.0f / 16777216.0f) >= a.drop_p;
}

// The same decisions for the four consecutive keys kcol0 .. kcol0 + 3 of one query: element
// indices e0 .. e0 + 3 fall into at most two Philox blocks (one when e0 is a multiple of 4).
__device__ __forceinline__ void adell_att_keep4(const AttArgs& a, int bh, int qrow, int kcol0,
                                                bool keep[4]) {
  keep[0] = keep[1] = keep[2] = keep[3] = true;
  if (a.drop_p <= 0.f) return;
  const uint64_t e0 = ((uint64_t)bh * a.T + qrow) * a.T + kcol0;
  const uint64_t b0 = e0 >> 2, b1 = (e0 + 3) >> 2;
  const uint4 r0 = adell_philox4((uint32_t)b0, (uint32_t)(b0 >> 32), a.rng_offset + g_adell_rng_step, 2u, a.seed_lo,
                                 a.seed_hi);
  uint4 r1 = r0;
  if (b1 != b0)
    r1 = adell_philox4((uint32_t)b1, (uint32_t)(b1 >> 32), a.rng_offset + g_adell_rng_step, 2u, a.seed_lo, a.seed_hi);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t e = e0 + j;
    const bool first = (e >> 2) == b0;      // (component-wise: a select of the structs goes
    const unsigned i = (unsigned)(e & 3);   // through memory)
    const uint32_t w = i == 0 ? (first ? r0.x : r1.x) : (i == 1 ? (first ? r0.y : r1.y) :
                       (i == 2 ? (first ? r0.z : r1.z) : (first ? r0.w : r1.w)));
    keep[j] = (float)(w >> 8) * (1.0f / 16777216.0f) >= a.drop_p;
  }
}

__global__ __launch_bounds__(256) void adell_attention_fwd_kernel(AttArgs a) {
  extern __shared__ float sh[];
  const int AP = a.A + 1, DP = a.Dv;  // K rows padded against bank conflicts
  float* sK = sh;                       // [ATT_TK][AP]
  float* sV = sK + ATT_TK * AP;         // [ATT_TK][DP]
  float* sQ = sV + ATT_TK * DP;         // [ATT_ROWS][A]
  float* sP = sQ + ATT_ROWS * a.A;      // [4 waves][ATT_TK]
  const int bh = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * ATT_ROWS;
  const float* qb = a.q + (size_t)bh * a.T * a.A;
  const float* kb = a.k + (size_t)bh * a.T * a.A;
  const float* vb = a.v + (size_t)bh * a.T * a.Dv;
  for (int i = threadIdx.x; i < ATT_ROWS * a.A; i += 256) {
    const int r = i / a.A, c = i - r * a.A;
    sQ[i] = (row0 + r < a.T) ? qb[(size_t)(row0 + r) * a.A + c] : 0.f;
  }
  constexpr int RPW = ATT_ROWS / 4;
  constexpr int MAXD = 4;  // output columns per lane: Dv <= 256
  float m[RPW], l[RPW], acc[RPW][MAXD];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int d = 0; d < MAXD; ++d) acc[r][d] = 0.f;
  }
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  for (int k0 = 0; k0 < a.T; k0 += ATT_TK) {
    __syncthreads();
    for (int i = threadIdx.x; i < ATT_TK * a.A; i += 256) {
      const int r = i / a.A, c = i - r * a.A;
      sK[r * AP + c] = (k0 + r < a.T) ? kb[(size_t)(k0 + r) * a.A + c] : 0.f;
    }
    for (int i = threadIdx.x; i < ATT_TK * a.Dv; i += 256) {
      const int r = i / a.Dv, c = i - r * a.Dv;
      sV[r * DP + c] = (k0 + r < a.T) ? vb[(size_t)(k0 + r) * a.Dv + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int qrow = row0 + wave * RPW + r;
      const float* qr = sQ + (wave * RPW + r) * a.A;
      float s = -INFINITY;
      if (k0 + lane < a.T && qrow < a.T) {
        float t = 0.f;
        for (int c = 0; c < a.A; ++c) t += qr[c] * sK[lane * AP + c];
        s = t * a.scale;
        if (biasb) s += biasb[(size_t)qrow * a.T + k0 + lane];
        if (labb) s += att_label_term(labb[qrow], labb[k0 + lane]);
      }
      float mx = s;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      const float mnew = fmaxf(m[r], mx);
      const float p = (s == -INFINITY) ? 0.f : expf(s - mnew);
      const float corr = (m[r] == -INFINITY) ? 0.f : expf(m[r] - mnew);
      const float psum = adell_wave_sum(p);
      l[r] = l[r] * corr + psum;
      m[r] = mnew;
      // dropout acts on the normalised probabilities: l keeps the full sum, the PV product
      // sees the kept entries scaled by 1/(1-p)
      sP[wave * ATT_TK + lane] =
          (p != 0.f && adell_att_keep(a, bh, qrow, k0 + lane)) ? p * keep_scale : 0.f;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int d = 0; d < MAXD; ++d) {
        const int col = lane + 64 * d;
        if (col < a.Dv) {
          float t = 0.f;
          for (int j = 0; j < ATT_TK; ++j) t += sP[wave * ATT_TK + j] * sV[j * DP + col];
          acc[r][d] = acc[r][d] * corr + t;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int qrow = row0 + wave * RPW + r;
    if (qrow >= a.T) continue;
    const float inv = 1.0f / l[r];
#pragma unroll
    for (int d = 0; d < MAXD; ++d) {
      const int col = lane + 64 * d;
      if (col < a.Dv) a.out[((size_t)bh * a.T + qrow) * a.Dv + col] = acc[r][d] * inv;
    }
    if (lane == 0) a.lse_out[(size_t)bh * a.T + qrow] = m[r] + logf(l[r]);
  }
}

// dQ: one wave per query row (same structure as forward). ROWS: query rows per block (ATT_ROWS, or
// half of it for head dims whose 16-row block would not fit the LDS: adell_att_plan).
template <int ROWS>
__global__ __launch_bounds__(256) void adell_attention_bwd_q_kernel(AttArgs a) {
  extern __shared__ float sh[];
  const int AP = a.A + 1, DP = a.Dv + 1;
  float* sK = sh;                        // [ATT_TK][AP]
  float* sV = sK + ATT_TK * AP;          // [ATT_TK][DP]
  float* sQ = sV + ATT_TK * DP;          // [ROWS][A]
  float* sdO = sQ + ROWS * a.A;      // [ROWS][Dv]
  float* sP = sdO + ROWS * a.Dv;     // [4][ATT_TK]  (holds dS)
  const int bh = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * ROWS;
  const float* qb = a.q + (size_t)bh * a.T * a.A;
  const float* kb = a.k + (size_t)bh * a.T * a.A;
  const float* vb = a.v + (size_t)bh * a.T * a.Dv;
  const float* ob = a.o + (size_t)bh * a.T * a.Dv;
  const float* gb = a.dout + (size_t)bh * a.T * a.Dv;
  for (int i = threadIdx.x; i < ROWS * a.A; i += 256) {
    const int r = i / a.A, c = i - r * a.A;
    sQ[i] = (row0 + r < a.T) ? qb[(size_t)(row0 + r) * a.A + c] : 0.f;
  }
  for (int i = threadIdx.x; i < ROWS * a.Dv; i += 256) {
    const int r = i / a.Dv, c = i - r * a.Dv;
    sdO[i] = (row0 + r < a.T) ? gb[(size_t)(row0 + r) * a.Dv + c] : 0.f;
  }
  __syncthreads();
  constexpr int RPW = ROWS / 4;
  constexpr int MAXA = 4;  // A <= 256
  float Dr[RPW], lse[RPW], acc[RPW][MAXA];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int qrow = row0 + wave * RPW + r;
    float t = 0.f;
    if (qrow < a.T)
      for (int c = lane; c < a.Dv; c += 64)
        t += sdO[(wave * RPW + r) * a.Dv + c] * ob[(size_t)qrow * a.Dv + c];
    Dr[r] = adell_wave_sum(t);
    lse[r] = qrow < a.T ? a.lse[(size_t)bh * a.T + qrow] : 0.f;
#pragma unroll
    for (int d = 0; d < MAXA; ++d) acc[r][d] = 0.f;
  }
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  for (int k0 = 0; k0 < a.T; k0 += ATT_TK) {
    __syncthreads();
    for (int i = threadIdx.x; i < ATT_TK * a.A; i += 256) {
      const int r = i / a.A, c = i - r * a.A;
      sK[r * AP + c] = (k0 + r < a.T) ? kb[(size_t)(k0 + r) * a.A + c] : 0.f;
    }
    for (int i = threadIdx.x; i < ATT_TK * a.Dv; i += 256) {
      const int r = i / a.Dv, c = i - r * a.Dv;
      sV[r * DP + c] = (k0 + r < a.T) ? vb[(size_t)(k0 + r) * a.Dv + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int qrow = row0 + wave * RPW + r;
      const float* qr = sQ + (wave * RPW + r) * a.A;
      const float* gr = sdO + (wave * RPW + r) * a.Dv;
      float ds = 0.f;
      if (k0 + lane < a.T && qrow < a.T) {
        float t = 0.f;
        for (int c = 0; c < a.A; ++c) t += qr[c] * sK[lane * AP + c];
        float s = t * a.scale;
        if (biasb) s += biasb[(size_t)qrow * a.T + k0 + lane];
        if (labb) s += att_label_term(labb[qrow], labb[k0 + lane]);
        const float p = expf(s - lse[r]);
        float dp = 0.f;
        for (int c = 0; c < a.Dv; ++c) dp += gr[c] * sV[lane * DP + c];
        dp = adell_att_keep(a, bh, qrow, k0 + lane) ? dp * keep_scale : 0.f;
        ds = p * (dp - Dr[r]);
      }
      sP[wave * ATT_TK + lane] = ds;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int d = 0; d < MAXA; ++d) {
        const int col = lane + 64 * d;
        if (col < a.A) {
          float t = 0.f;
          for (int j = 0; j < ATT_TK; ++j) t += sP[wave * ATT_TK + j] * sK[j * AP + col];
          acc[r][d] += t;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int qrow = row0 + wave * RPW + r;
    if (qrow >= a.T) continue;
#pragma unroll
    for (int d = 0; d < MAXA; ++d) {
      const int col = lane + 64 * d;
      if (col < a.A) a.dq[((size_t)bh * a.T + qrow) * a.A + col] = acc[r][d] * a.scale;
    }
  }
}

// dK, dV: one wave per key row; queries streamed through LDS in tiles of 64.
template <int ROWS>
__global__ __launch_bounds__(256) void adell_attention_bwd_kv_kernel(AttArgs a) {
  extern __shared__ float sh[];
  const int AP = a.A + 1, DP = a.Dv + 1;
  float* sQ = sh;                        // [ATT_TK][AP]   query tile
  float* sdO = sQ + ATT_TK * AP;         // [ATT_TK][DP]
  float* sK = sdO + ATT_TK * DP;         // [ROWS][A]  this block's keys
  float* sV = sK + ROWS * a.A;       // [ROWS][Dv]
  float* sP = sV + ROWS * a.Dv;      // [4][2][ATT_TK] (p, dS)
  float* sL = sP + 4 * 2 * ATT_TK;       // [ATT_TK][2] lse, D of the query tile
  const int bh = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * ROWS;
  const float* qb = a.q + (size_t)bh * a.T * a.A;
  const float* kb = a.k + (size_t)bh * a.T * a.A;
  const float* vb = a.v + (size_t)bh * a.T * a.Dv;
  const float* ob = a.o + (size_t)bh * a.T * a.Dv;
  const float* gb = a.dout + (size_t)bh * a.T * a.Dv;
  for (int i = threadIdx.x; i < ROWS * a.A; i += 256) {
    const int r = i / a.A, c = i - r * a.A;
    sK[i] = (row0 + r < a.T) ? kb[(size_t)(row0 + r) * a.A + c] : 0.f;
  }
  for (int i = threadIdx.x; i < ROWS * a.Dv; i += 256) {
    const int r = i / a.Dv, c = i - r * a.Dv;
    sV[i] = (row0 + r < a.T) ? vb[(size_t)(row0 + r) * a.Dv + c] : 0.f;
  }
  constexpr int RPW = ROWS / 4;
  constexpr int MAXC = 4;
  float dk[RPW][MAXC], dv[RPW][MAXC];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int d = 0; d < MAXC; ++d) dk[r][d] = dv[r][d] = 0.f;
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  for (int q0 = 0; q0 < a.T; q0 += ATT_TK) {
    __syncthreads();
    for (int i = threadIdx.x; i < ATT_TK * a.A; i += 256) {
      const int r = i / a.A, c = i - r * a.A;
      sQ[r * AP + c] = (q0 + r < a.T) ? qb[(size_t)(q0 + r) * a.A + c] : 0.f;
    }
    for (int i = threadIdx.x; i < ATT_TK * a.Dv; i += 256) {
      const int r = i / a.Dv, c = i - r * a.Dv;
      sdO[r * DP + c] = (q0 + r < a.T) ? gb[(size_t)(q0 + r) * a.Dv + c] : 0.f;
    }
    __syncthreads();
    // D_i = dO_i . O_i for the query tile: wave w handles rows w, w+4, ...
    for (int r = wave; r < ATT_TK; r += 4) {
      float t = 0.f;
      if (q0 + r < a.T)
        for (int c = lane; c < a.Dv; c += 64) t += sdO[r * DP + c] * ob[(size_t)(q0 + r) * a.Dv + c];
      t = adell_wave_sum(t);
      if (lane == 0) {
        sL[r * 2 + 0] = (q0 + r < a.T) ? a.lse[(size_t)bh * a.T + q0 + r] : 0.f;
        sL[r * 2 + 1] = t;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int krow = row0 + wave * RPW + r;
      const float* kr = sK + (wave * RPW + r) * a.A;
      const float* vr = sV + (wave * RPW + r) * a.Dv;
      float p = 0.f, ds = 0.f;
      if (q0 + lane < a.T && krow < a.T) {
        float t = 0.f;
        for (int c = 0; c < a.A; ++c) t += kr[c] * sQ[lane * AP + c];
        float s = t * a.scale;
        if (biasb) s += biasb[(size_t)(q0 + lane) * a.T + krow];
        if (labb) s += att_label_term(labb[q0 + lane], labb[krow]);
        p = expf(s - sL[lane * 2 + 0]);
        float dp = 0.f;
        for (int c = 0; c < a.Dv; ++c) dp += vr[c] * sdO[lane * DP + c];
        const float km = adell_att_keep(a, bh, q0 + lane, krow) ? keep_scale : 0.f;
        ds = p * (dp * km - sL[lane * 2 + 1]);
        p *= km;  // dV sees the dropped probabilities
      }
      sP[(wave * 2 + 0) * ATT_TK + lane] = p;
      sP[(wave * 2 + 1) * ATT_TK + lane] = ds;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int d = 0; d < MAXC; ++d) {
        const int col = lane + 64 * d;
        if (col < a.Dv) {
          float t = 0.f;
          for (int j = 0; j < ATT_TK; ++j) t += sP[(wave * 2 + 0) * ATT_TK + j] * sdO[j * DP + col];
          dv[r][d] += t;
        }
        if (col < a.A) {
          float t = 0.f;
          for (int j = 0; j < ATT_TK; ++j) t += sP[(wave * 2 + 1) * ATT_TK + j] * sQ[j * AP + col];
          dk[r][d] += t;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int krow = row0 + wave * RPW + r;
    if (krow >= a.T) continue;
#pragma unroll
    for (int d = 0; d < MAXC; ++d) {
      const int col = lane + 64 * d;
      if (col < a.Dv) a.dv[((size_t)bh * a.T + krow) * a.Dv + col] = dv[r][d];
      if (col < a.A) a.dk[((size_t)bh * a.T + krow) * a.A + col] = dk[r][d] * a.scale;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MFMA attention (head dims that are multiples of 32, up to 128): QK^T and PV -- and in the
// backward dO V^T, dS K, dS^T Q, P^T dO -- on v_mfma_f32_32x32x2_f32, i.e. exact fp32 FMA chains
// (the reference op is F.scaled_dot_product_attention on fp32 tensors, linear_blocks.py:358-417).
// One wave per 32-row tile, one tile per block: 7 x BH blocks at the 216 tokens of config 3.
//
// The score tile is always computed with the SUMMATION index of the product that follows in its
// accumulator ROWS (registers): a 32x32 accumulator holds column (lane & 31) and rows
// am_row(r, lane >> 5) in its 16 registers, and the A operand of the 32x32x2 MFMA wants
// A[i = lane & 31][k = lane >> 5] -- so register r of the tile IS the A operand of k-step r of the
// next product (k = rows am_row(r, 0), am_row(r, 1)), with no lane movement and no LDS trip:
//   forward / dQ kernel:  S^T = K Q^T (rows = keys, column = query)  ->  O = P V,  dQ = dS K
//   dK/dV kernel:         S   = Q K^T (rows = queries, column = key) ->  dV = P^T dO, dK = dS^T Q
// Softmax statistics are per column (= per lane) in the first form: a max / sum over the 16
// registers plus one exchange between the two lane halves; the forward makes two passes over the
// keys (statistics, then normalised probabilities), so the output tile is never rescaled.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int am_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// rows [r0, r0 + NR) x C columns of a [T][C] matrix -> LDS rows of C + 1 floats, rows >= T zero,
// by the 256 threads of the block. All 16-byte loads are issued before the first LDS store, from
// clamped row indices (a select on the loaded value, not a branch around the load: hipcc would
// otherwise wait for every load in turn -- dependent L2 round trips).
template <int C>
__device__ __forceinline__ void am_stage32(float* dst, const float* src, long rs, int r0, int T, int tid) {
  constexpr int N4 = 32 * C / 4 / 256;   // float4 per thread for a 32-row tile
  float4 v[N4];
#pragma unroll
  for (int u = 0; u < N4; ++u) {
    const int i = tid + 256 * u, r = i / (C / 4), c4 = i - r * (C / 4);
    const int row = r0 + r < T ? r0 + r : T - 1;
    v[u] = *reinterpret_cast<const float4*>(src + (size_t)row * rs + 4 * c4);
  }
#pragma unroll
  for (int u = 0; u < N4; ++u) {
    const int i = tid + 256 * u, r = i / (C / 4), c4 = i - r * (C / 4);
    const bool ok = r0 + r < T;
    float* d = dst + r * (C + 1) + 4 * c4;
    d[0] = ok ? v[u].x : 0.f;
    d[1] = ok ? v[u].y : 0.f;
    d[2] = ok ? v[u].z : 0.f;
    d[3] = ok ? v[u].w : 0.f;
  }
}
// the whole [T][C] matrix, padded to a multiple of 32 rows (resident variants): the loads of
// four tiles are in flight together
template <int C>
__device__ __forceinline__ void am_stage_all(float* dst, const float* src, long rs, int T, int tid) {
  constexpr int N4 = 32 * C / 4 / 256, G = 4;
  const int tiles = (T + 31) / 32;
  for (int t0 = 0; t0 < tiles; t0 += G) {
    float4 v[G][N4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int u = 0; u < N4; ++u) {
        const int i = tid + 256 * u, r = i / (C / 4), c4 = i - r * (C / 4);
        int row = (t0 + g) * 32 + r;
        row = row < T ? row : T - 1;
        v[g][u] = *reinterpret_cast<const float4*>(src + (size_t)row * rs + 4 * c4);
      }
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (t0 + g < tiles) {
#pragma unroll
        for (int u = 0; u < N4; ++u) {
          const int i = tid + 256 * u, r = i / (C / 4), c4 = i - r * (C / 4);
          const bool ok = (t0 + g) * 32 + r < T;
          float* d = dst + (size_t)((t0 + g) * 32 + r) * (C + 1) + 4 * c4;
          d[0] = ok ? v[g][u].x : 0.f;
          d[1] = ok ? v[g][u].y : 0.f;
          d[2] = ok ? v[g][u].z : 0.f;
          d[3] = ok ? v[g][u].w : 0.f;
        }
      }
  }
}

// S^T tile: rows = keys k0 + am_row(r, h), column = this lane's query; -inf outside the sequence
template <int A>
__device__ __forceinline__ void am_scores_t(const AttArgs& a, const float* sK, const float* qreg,
                                            const float* biasb, const int* labb, int qrow, bool qok,
                                            int k0, int li, int h, float* val) {
  f32x16 s;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
  for (int ss = 0; ss < A / 2; ++ss)
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[li * (A + 1) + 2 * ss + h], qreg[ss], s, 0, 0, 0);
  const int qlab = labb && qok ? labb[qrow] : 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int key = k0 + am_row(r, h);
    float v = -INFINITY;
    if (qok && key < a.T) {
      v = s[r] * a.scale;
      if (biasb) v += biasb[(size_t)qrow * a.T + key];
      if (labb) v += att_label_term(qlab, labb[key]);
    }
    val[r] = v;
  }
}

// Block = 4 waves = 4 query tiles of 32 rows sharing the staged K / V. RES: every K / V row of the
// sequence is staged ONCE and stays in LDS (config 3: 216 tokens x (64 + 64) floats = 110 KB), no
// further global loads or barriers in the key loops; otherwise 32-key tiles are streamed.
template <int AT, int DT, bool RES>
__global__ __launch_bounds__(256) void adell_attn_mfma_fwd_kernel(AttArgs a) {
  constexpr int A = AT * 32, Dv = DT * 32;
  extern __shared__ float sh[];
  const int Tpad = (a.T + 31) & ~31;
  float* sK = sh;
  float* sV = sK + (size_t)(RES ? Tpad : 32) * (A + 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, q0 = (blockIdx.x * 4 + wave) * 32, qrow = q0 + li;
  const bool qok = qrow < a.T, active = q0 < a.T;   // `active` is wave-uniform
  const float* qb = a.q + att_base(a, a.sq, bh);
  const float* kb = a.k + att_base(a, a.sk, bh);
  const float* vb = a.v + att_base(a, a.sv, bh);
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  float qreg[A / 2];
#pragma unroll
  for (int ss = 0; ss < A / 2; ++ss) qreg[ss] = qok ? qb[(size_t)qrow * a.sq.r + 2 * ss + h] : 0.f;
  if (RES) {
    am_stage_all<A>(sK, kb, a.sk.r, a.T, tid);
    am_stage_all<Dv>(sV, vb, a.sv.r, a.T, tid);
    __syncthreads();
  }
  // pass 1: log-sum-exp of this lane's query
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < a.T; k0 += 32) {
    if (!RES) {
      __syncthreads();
      am_stage32<A>(sK, kb, a.sk.r, k0, a.T, tid);
      __syncthreads();
    }
    if (!active) continue;
    float val[16];
    am_scores_t<A>(a, sK + (size_t)(RES ? k0 : 0) * (A + 1), qreg, biasb, labb, qrow, qok, k0, li, h, val);
    float mt = val[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mt = fmaxf(mt, val[r]);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mnew = fmaxf(m, mt);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ps += (val[r] == -INFINITY) ? 0.f : expf(val[r] - mnew);
    ps += __shfl_xor(ps, 32, 64);
    l = l * ((m == -INFINITY) ? 0.f : expf(m - mnew)) + ps;
    m = mnew;
  }
  const float lse = m + logf(l);
  // pass 2: O = dropout(softmax) V with the normalised probabilities as the MFMA A operand
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  for (int k0 = 0; k0 < a.T; k0 += 32) {
    if (!RES) {
      __syncthreads();
      am_stage32<A>(sK, kb, a.sk.r, k0, a.T, tid);
      am_stage32<Dv>(sV, vb, a.sv.r, k0, a.T, tid);
      __syncthreads();
    }
    if (!active) continue;
    const float* sVt = sV + (size_t)(RES ? k0 : 0) * (Dv + 1);
    float val[16];
    am_scores_t<A>(a, sK + (size_t)(RES ? k0 : 0) * (A + 1), qreg, biasb, labb, qrow, qok, k0, li, h, val);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      bool keep[4];   // registers 4 r4 .. 4 r4 + 3 are four consecutive keys
      adell_att_keep4(a, bh, qrow, k0 + am_row(4 * r4, h), keep);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * r4 + j;
        const float p = (val[r] == -INFINITY) ? 0.f : expf(val[r] - lse);
        val[r] = keep[j] ? p * keep_scale : 0.f;
      }
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            val[r], sVt[am_row(r, h) * (Dv + 1) + dt * 32 + li], o[dt], 0, 0, 0);
  }
  if (!active) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = q0 + am_row(r, h);
      if (row < a.T) a.out[att_base(a, a.so, bh) + (size_t)row * a.so.r + dt * 32 + li] = o[dt][r];
    }
  if (h == 0 && qok) a.lse_out[(size_t)bh * a.T + qrow] = lse;
}

// dQ = scale * dS K with dS^T tiles (rows = keys, column = this lane's query)
template <int AT, int DT, bool RES>
__global__ __launch_bounds__(256) void adell_attn_mfma_bwd_q_kernel(AttArgs a) {
  constexpr int A = AT * 32, Dv = DT * 32;
  extern __shared__ float sh[];
  const int Tpad = (a.T + 31) & ~31;
  float* sK = sh;
  float* sV = sK + (size_t)(RES ? Tpad : 32) * (A + 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, q0 = (blockIdx.x * 4 + wave) * 32, qrow = q0 + li;
  const bool qok = qrow < a.T, active = q0 < a.T;
  const float* qb = a.q + att_base(a, a.sq, bh);
  const float* kb = a.k + att_base(a, a.sk, bh);
  const float* vb = a.v + att_base(a, a.sv, bh);
  const float* ob = a.o + att_base(a, a.so, bh);
  const float* gb = a.dout + att_base(a, a.sg, bh);
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  float qreg[A / 2], doreg[Dv / 2];
  float D = 0.f;
#pragma unroll
  for (int ss = 0; ss < A / 2; ++ss) qreg[ss] = qok ? qb[(size_t)qrow * a.sq.r + 2 * ss + h] : 0.f;
#pragma unroll
  for (int ss = 0; ss < Dv / 2; ++ss) {
    doreg[ss] = qok ? gb[(size_t)qrow * a.sg.r + 2 * ss + h] : 0.f;
    D += qok ? doreg[ss] * ob[(size_t)qrow * a.so.r + 2 * ss + h] : 0.f;
  }
  D += __shfl_xor(D, 32, 64);
  const float lse = qok ? a.lse[(size_t)bh * a.T + qrow] : 0.f;
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  f32x16 dq[AT];
#pragma unroll
  for (int at = 0; at < AT; ++at)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[at][r] = 0.f;
  if (RES) {
    am_stage_all<A>(sK, kb, a.sk.r, a.T, tid);
    am_stage_all<Dv>(sV, vb, a.sv.r, a.T, tid);
    __syncthreads();
  }
  for (int k0 = 0; k0 < a.T; k0 += 32) {
    if (!RES) {
      __syncthreads();
      am_stage32<A>(sK, kb, a.sk.r, k0, a.T, tid);
      am_stage32<Dv>(sV, vb, a.sv.r, k0, a.T, tid);
      __syncthreads();
    }
    if (!active) continue;
    const float* sKt = sK + (size_t)(RES ? k0 : 0) * (A + 1);
    const float* sVt = sV + (size_t)(RES ? k0 : 0) * (Dv + 1);
    float val[16];
    am_scores_t<A>(a, sKt, qreg, biasb, labb, qrow, qok, k0, li, h, val);
    f32x16 dp;   // dP^T = V dO^T: rows = keys, column = query
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int ss = 0; ss < Dv / 2; ++ss)
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sVt[li * (Dv + 1) + 2 * ss + h], doreg[ss], dp, 0, 0, 0);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      bool keep[4];
      adell_att_keep4(a, bh, qrow, k0 + am_row(4 * r4, h), keep);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * r4 + j;
        const float p = (val[r] == -INFINITY) ? 0.f : expf(val[r] - lse);
        const float g = keep[j] ? dp[r] * keep_scale : 0.f;
        val[r] = p * (g - D);   // dS
      }
    }
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dq[at] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            val[r], sKt[am_row(r, h) * (A + 1) + at * 32 + li], dq[at], 0, 0, 0);
  }
  if (!active) return;
#pragma unroll
  for (int at = 0; at < AT; ++at)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = q0 + am_row(r, h);
      if (row < a.T) a.dq[att_base(a, a.sdq, bh) + (size_t)row * a.sdq.r + at * 32 + li] = dq[at][r] * a.scale;
    }
}

// dV = P_drop^T dO, dK = scale * dS^T Q with S tiles (rows = queries, column = this lane's key);
// block = 4 key tiles sharing the staged Q / dO (+ D = rowsum(dO * O) and lse per query)
template <int AT, int DT, bool RES>
__global__ __launch_bounds__(256) void adell_attn_mfma_bwd_kv_kernel(AttArgs a) {
  constexpr int A = AT * 32, Dv = DT * 32;
  extern __shared__ float sh[];
  const int Tpad = (a.T + 31) & ~31;
  const int rows = RES ? Tpad : 32;
  float* sQ = sh;
  float* sG = sQ + (size_t)rows * (A + 1);     // dO
  float* sD = sG + (size_t)rows * (Dv + 1);
  float* sL = sD + rows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, k0 = (blockIdx.x * 4 + wave) * 32, krow = k0 + li;
  const bool kok = krow < a.T, active = k0 < a.T;
  const float* qb = a.q + att_base(a, a.sq, bh);
  const float* kb = a.k + att_base(a, a.sk, bh);
  const float* vb = a.v + att_base(a, a.sv, bh);
  const float* ob = a.o + att_base(a, a.so, bh);
  const float* gb = a.dout + att_base(a, a.sg, bh);
  const float* biasb = a.bias ? a.bias + (size_t)(bh % a.nbias) * a.T * a.T : nullptr;
  const int* labb = att_labels(a, bh);
  const int klab = labb && kok ? labb[krow] : 0;
  float kreg[A / 2], vreg[Dv / 2];
#pragma unroll
  for (int ss = 0; ss < A / 2; ++ss) kreg[ss] = kok ? kb[(size_t)krow * a.sk.r + 2 * ss + h] : 0.f;
#pragma unroll
  for (int ss = 0; ss < Dv / 2; ++ss) vreg[ss] = kok ? vb[(size_t)krow * a.sv.r + 2 * ss + h] : 0.f;
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  f32x16 dv[DT], dk[AT];
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dv[t][r] = 0.f;
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[t][r] = 0.f;
  // D[q] = sum_dv dO[q][dv] O[q][dv] and lse[q] of queries [r0, r0 + n): 8 threads per query
  auto stage_stats = [&](int r0, int n, float* dD, float* dL) {
    for (int qi = tid >> 3; qi < n; qi += 32) {
      const int qr = r0 + qi;
      float d = 0.f;
      if (qr < a.T)
        for (int c = (tid & 7) * 4; c < Dv; c += 32) {
          const float4 g4 = *reinterpret_cast<const float4*>(gb + (size_t)qr * a.sg.r + c);
          const float4 o4 = *reinterpret_cast<const float4*>(ob + (size_t)qr * a.so.r + c);
          d += g4.x * o4.x + g4.y * o4.y + g4.z * o4.z + g4.w * o4.w;
        }
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      if ((tid & 7) == 0) {
        dD[qi] = d;
        dL[qi] = qr < a.T ? a.lse[(size_t)bh * a.T + qr] : 0.f;
      }
    }
  };
  if (RES) {
    am_stage_all<A>(sQ, qb, a.sq.r, a.T, tid);
    am_stage_all<Dv>(sG, gb, a.sg.r, a.T, tid);
    stage_stats(0, Tpad, sD, sL);
    __syncthreads();
  }
  for (int q0 = 0; q0 < a.T; q0 += 32) {
    if (!RES) {
      __syncthreads();
      am_stage32<A>(sQ, qb, a.sq.r, q0, a.T, tid);
      am_stage32<Dv>(sG, gb, a.sg.r, q0, a.T, tid);
      stage_stats(q0, 32, sD, sL);
      __syncthreads();
    }
    if (!active) continue;
    const int base = RES ? q0 : 0;
    const float* sQt = sQ + (size_t)base * (A + 1);
    const float* sGt = sG + (size_t)base * (Dv + 1);
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
    for (int ss = 0; ss < A / 2; ++ss)
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(sQt[li * (A + 1) + 2 * ss + h], kreg[ss], s, 0, 0, 0);
#pragma unroll
    for (int ss = 0; ss < Dv / 2; ++ss)
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sGt[li * (Dv + 1) + 2 * ss + h], vreg[ss], dp, 0, 0, 0);
    float pd[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = am_row(r, h), qr = q0 + row;
      float p = 0.f;
      if (kok && qr < a.T) {
        float v = s[r] * a.scale;
        if (biasb) v += biasb[(size_t)qr * a.T + krow];
        if (labb) v += att_label_term(labb[qr], klab);
        p = expf(v - sL[base + row]);
      }
      const bool keep = adell_att_keep(a, bh, qr, krow);
      pd[r] = keep ? p * keep_scale : 0.f;
      ds[r] = p * ((keep ? dp[r] * keep_scale : 0.f) - sD[base + row]);
    }
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            pd[r], sGt[am_row(r, h) * (Dv + 1) + t * 32 + li], dv[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            ds[r], sQt[am_row(r, h) * (A + 1) + t * 32 + li], dk[t], 0, 0, 0);
  }
  if (!active) return;
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = k0 + am_row(r, h);
      if (row < a.T) a.dv[att_base(a, a.sdv, bh) + (size_t)row * a.sdv.r + t * 32 + li] = dv[t][r];
    }
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = k0 + am_row(r, h);
      if (row < a.T) a.dk[att_base(a, a.sdk, bh) + (size_t)row * a.sdk.r + t * 32 + li] = dk[t][r] * a.scale;
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient of the additive bias, reduced over the sequences that share a bias slice and never
// materialised per sequence: dbias[j] = sum over bh % nbias == j of dS[bh], dS = P o (keep dP /
// (1 - p) - D) -- the gradient of the pre-softmax additive term, so without `scale`. S, P and dS are
// rebuilt exactly as the dQ kernels build them (scale, bias, labels, the same keep mask).
// A block owns slice j (grid y), one tile of the [T][T] result (grid x) and one contiguous chunk of
// j's sequences (grid z), walks the chunk in ascending bh and accumulates in registers. With one
// chunk the tile goes straight to dbias; otherwise to partial slice z of the workspace, and
// adell_attn_dbias_fold_kernel adds the partial slices in chunk order: no atomics, the same bits on
// every run. Operands by (item, head, row) strides as in adell_attention_bwd.
// ---------------------------------------------------------------------------------------------
struct AttBiasGrad {
  float* dst;    // dbias, or the workspace [chunks][nbias][T][T]
  int BH, chunk; // sequences in all; sequences of one slice per block
  int tiles_k;   // key tiles per row of tiles (grid x = query tiles * tiles_k)
};

// MFMA form: 4 waves = 4 query tiles of 32 rows sharing the staged 32-key K / V tiles, NK key tiles
// per block (128 x 32 NK results, 16 NK accumulator registers per lane); dS^T tiles as in the dQ kernel
template <int AT, int DT, int NK>
__global__ __launch_bounds__(256) void adell_attn_mfma_dbias_kernel(AttArgs a, AttBiasGrad g) {
  constexpr int A = AT * 32, Dv = DT * 32;
  extern __shared__ float sh[];
  float* sK = sh;
  float* sV = sK + 32 * (A + 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int tq = blockIdx.x / g.tiles_k, tk = blockIdx.x - tq * g.tiles_k;
  const int q0 = (tq * 4 + wave) * 32, qrow = q0 + li, kbase = tk * 32 * NK;
  const bool qok = qrow < a.T, active = q0 < a.T;   // `active` is wave-uniform
  const int j = blockIdx.y;
  const int nj = (g.BH - j + a.nbias - 1) / a.nbias;   // sequences j, j + nbias, ...
  const int i0 = blockIdx.z * g.chunk, i1 = min(i0 + g.chunk, nj);
  const float* biasb = a.bias ? a.bias + (size_t)j * a.T * a.T : nullptr;
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  f32x16 acc[NK];
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int bh = j + i * a.nbias;
    const float* qb = a.q + att_base(a, a.sq, bh);
    const float* kb = a.k + att_base(a, a.sk, bh);
    const float* vb = a.v + att_base(a, a.sv, bh);
    const float* ob = a.o + att_base(a, a.so, bh);
    const float* gb = a.dout + att_base(a, a.sg, bh);
    const int* labb = att_labels(a, bh);
    float qreg[A / 2], doreg[Dv / 2];
    float D = 0.f;
#pragma unroll
    for (int ss = 0; ss < A / 2; ++ss) qreg[ss] = qok ? qb[(size_t)qrow * a.sq.r + 2 * ss + h] : 0.f;
#pragma unroll
    for (int ss = 0; ss < Dv / 2; ++ss) {
      doreg[ss] = qok ? gb[(size_t)qrow * a.sg.r + 2 * ss + h] : 0.f;
      D += qok ? doreg[ss] * ob[(size_t)qrow * a.so.r + 2 * ss + h] : 0.f;
    }
    D += __shfl_xor(D, 32, 64);
    const float lse = qok ? a.lse[(size_t)bh * a.T + qrow] : 0.f;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
      const int k0 = kbase + 32 * kt;
      if (k0 >= a.T) continue;   // block-uniform
      __syncthreads();
      am_stage32<A>(sK, kb, a.sk.r, k0, a.T, tid);
      am_stage32<Dv>(sV, vb, a.sv.r, k0, a.T, tid);
      __syncthreads();
      if (!active) continue;
      float val[16];
      am_scores_t<A>(a, sK, qreg, biasb, labb, qrow, qok, k0, li, h, val);
      f32x16 dp;   // dP^T = V dO^T: rows = keys, column = query
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
      for (int ss = 0; ss < Dv / 2; ++ss)
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[li * (Dv + 1) + 2 * ss + h], doreg[ss], dp, 0, 0, 0);
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        bool keep[4];
        adell_att_keep4(a, bh, qrow, k0 + am_row(4 * r4, h), keep);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int r = 4 * r4 + jj;
          const float p = (val[r] == -INFINITY) ? 0.f : expf(val[r] - lse);
          const float gd = keep[jj] ? dp[r] * keep_scale : 0.f;
          acc[kt][r] += p * (gd - D);
        }
      }
    }
  }
  if (!qok) return;
  float* dst = g.dst + ((size_t)blockIdx.z * a.nbias + j) * a.T * a.T + (size_t)qrow * a.T;
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kbase + 32 * kt + am_row(r, h);
      if (key < a.T) dst[key] = acc[kt][r];
    }
}

// vector-ALU form (the structure of adell_attention_bwd_q_kernel): one wave per query row, lane =
// key of the block's 64-key tile; block tile ROWS queries x 64 keys
template <int ROWS>
__global__ __launch_bounds__(256) void adell_attention_dbias_kernel(AttArgs a, AttBiasGrad g) {
  extern __shared__ float sh[];
  const int AP = a.A + 1, DP = a.Dv + 1;
  float* sK = sh;                        // [ATT_TK][AP]
  float* sV = sK + ATT_TK * AP;          // [ATT_TK][DP]
  float* sQ = sV + ATT_TK * DP;          // [ROWS][A]
  float* sdO = sQ + ROWS * a.A;          // [ROWS][Dv]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tq = blockIdx.x / g.tiles_k, tk = blockIdx.x - tq * g.tiles_k;
  const int row0 = tq * ROWS, k0 = tk * ATT_TK;
  const int j = blockIdx.y;
  const int nj = (g.BH - j + a.nbias - 1) / a.nbias;
  const int i0 = blockIdx.z * g.chunk, i1 = min(i0 + g.chunk, nj);
  const float* biasb = a.bias ? a.bias + (size_t)j * a.T * a.T : nullptr;
  const float keep_scale = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  constexpr int RPW = ROWS / 4;
  float acc[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int bh = j + i * a.nbias;
    const float* qb = a.q + att_base(a, a.sq, bh);
    const float* kb = a.k + att_base(a, a.sk, bh);
    const float* vb = a.v + att_base(a, a.sv, bh);
    const float* ob = a.o + att_base(a, a.so, bh);
    const float* gb = a.dout + att_base(a, a.sg, bh);
    const int* labb = att_labels(a, bh);
    __syncthreads();
    for (int e = threadIdx.x; e < ROWS * a.A; e += 256) {
      const int r = e / a.A, c = e - r * a.A;
      sQ[e] = (row0 + r < a.T) ? qb[(size_t)(row0 + r) * a.sq.r + c] : 0.f;
    }
    for (int e = threadIdx.x; e < ROWS * a.Dv; e += 256) {
      const int r = e / a.Dv, c = e - r * a.Dv;
      sdO[e] = (row0 + r < a.T) ? gb[(size_t)(row0 + r) * a.sg.r + c] : 0.f;
    }
    for (int e = threadIdx.x; e < ATT_TK * a.A; e += 256) {
      const int r = e / a.A, c = e - r * a.A;
      sK[r * AP + c] = (k0 + r < a.T) ? kb[(size_t)(k0 + r) * a.sk.r + c] : 0.f;
    }
    for (int e = threadIdx.x; e < ATT_TK * a.Dv; e += 256) {
      const int r = e / a.Dv, c = e - r * a.Dv;
      sV[r * DP + c] = (k0 + r < a.T) ? vb[(size_t)(k0 + r) * a.sv.r + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int qrow = row0 + wave * RPW + r;
      const float* qr = sQ + (wave * RPW + r) * a.A;
      const float* gr = sdO + (wave * RPW + r) * a.Dv;
      float t = 0.f;
      if (qrow < a.T)
        for (int c = lane; c < a.Dv; c += 64) t += gr[c] * ob[(size_t)qrow * a.so.r + c];
      const float Dr = adell_wave_sum(t);
      if (k0 + lane < a.T && qrow < a.T) {
        float d = 0.f;
        for (int c = 0; c < a.A; ++c) d += qr[c] * sK[lane * AP + c];
        float s = d * a.scale;
        if (biasb) s += biasb[(size_t)qrow * a.T + k0 + lane];
        if (labb) s += att_label_term(labb[qrow], labb[k0 + lane]);
        const float p = expf(s - a.lse[(size_t)bh * a.T + qrow]);
        float dp = 0.f;
        for (int c = 0; c < a.Dv; ++c) dp += gr[c] * sV[lane * DP + c];
        dp = adell_att_keep(a, bh, qrow, k0 + lane) ? dp * keep_scale : 0.f;
        acc[r] += p * (dp - Dr);
      }
    }
  }
  float* dst = g.dst + ((size_t)blockIdx.z * a.nbias + j) * a.T * a.T;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int qrow = row0 + wave * RPW + r;
    if (qrow < a.T && k0 + lane < a.T) dst[(size_t)qrow * a.T + k0 + lane] = acc[r];
  }
}

// dbias[e] = part[0][e] + part[1][e] + ... in chunk order
__global__ __launch_bounds__(256) void adell_attn_dbias_fold_kernel(
    const float* __restrict__ part, float* __restrict__ dbias, long n, int chunks) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    float s = part[e];
    for (int z = 1; z < chunks; ++z) s += part[(size_t)z * n + e];
    dbias[e] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// Launch plan of one attention pass (which: 0 forward, 1 backward dQ, 2 backward dK/dV): every
// decision the launchers below take, and what adell_attention_plan reports. Host only.
//   MFMA kernels: A, Dv in {32, 64, 128}, T >= 16, 16-byte aligned operands; resident while the
//   padded sequence fits ADELL_ATT_RES_BYTES of LDS (dK/dV rows carry D and lse: 2 floats more).
//   Vector-ALU kernels: everything else up to head dims of 256; the two backward kernels halve
//   their query / key row block when 16 rows would not fit the LDS budget (A + Dv > 502 / 507).
// ---------------------------------------------------------------------------------------------
#define ADELL_ATT_RES_BYTES (150 * 1024)
#define ADELL_ATT_LDS_MAX (160 * 1024)

struct AdellAttPlan {
  int path;     // ADELL_ATT_*
  size_t lds;   // dynamic LDS bytes
  int grid_x;   // blocks per sequence (grid y = BH)
  int rows;     // query (dK/dV: key) rows per block
};

static size_t adell_att_valu_lds(int which, int A, int Dv, int rows) {
  size_t fl = (size_t)ATT_TK * (A + 1) + (size_t)rows * A;
  if (which == 0) fl += (size_t)ATT_TK * Dv + 4 * ATT_TK;
  else fl += (size_t)ATT_TK * (Dv + 1) + (size_t)rows * Dv + (which == 1 ? 4 : 10) * ATT_TK;
  return sizeof(float) * fl;
}

static AdellAttPlan adell_att_plan(int which, int T, int A, int Dv, bool aligned) {
  AdellAttPlan p = {ADELL_ATT_REFUSED, 0, 0, 0};
  if (T <= 0 || A <= 0 || Dv <= 0 || A > 256 || Dv > 256) return p;
  const bool mfma = T >= 16 && (A == 32 || A == 64 || A == 128) && (Dv == 32 || Dv == 64 || Dv == 128) &&
                    aligned && !g_adell_tune.attn_nomfma;
  if (mfma) {
    const size_t tpad = (size_t)((T + 31) & ~31);
    const size_t per_row = (size_t)(A + 1) + (size_t)(Dv + 1) + (which == 2 ? 2 : 0);
    const size_t res = sizeof(float) * tpad * per_row;
    p.rows = 128;
    p.grid_x = adell_cdiv(T, 128);
    if (res <= ADELL_ATT_RES_BYTES) {   // the whole sequence stays in LDS
      p.path = ADELL_ATT_MFMA_RESIDENT;
      p.lds = res;
    } else {
      p.path = ADELL_ATT_MFMA_STREAMED;
      p.lds = sizeof(float) * 32 * per_row;
    }
    return p;
  }
  p.rows = ATT_ROWS;
  if (which != 0 && adell_att_valu_lds(which, A, Dv, p.rows) > ADELL_ATT_LDS_MAX) p.rows = ATT_ROWS / 2;
  p.lds = adell_att_valu_lds(which, A, Dv, p.rows);
  if (p.lds > ADELL_ATT_LDS_MAX) return p;   // (not reached with head dims <= 256)
  p.path = ADELL_ATT_VALU;
  p.grid_x = adell_cdiv(T, p.rows);
  return p;
}

template <int AT, int DT, bool RES>
static int adell_att_mfma_launch3(int which, const AttArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  if (which == 0) return adell_launch<adell_attn_mfma_fwd_kernel<AT, DT, RES>>(grid, dim3(256), lds, st, a);
  if (which == 1) return adell_launch<adell_attn_mfma_bwd_q_kernel<AT, DT, RES>>(grid, dim3(256), lds, st, a);
  return adell_launch<adell_attn_mfma_bwd_kv_kernel<AT, DT, RES>>(grid, dim3(256), lds, st, a);
}
template <int AT, int DT>
static int adell_att_mfma_launch2(int which, const AttArgs& a, int BH, const AdellAttPlan& p, hipStream_t st) {
  const dim3 grid((unsigned)p.grid_x, (unsigned)BH);
  if (p.path == ADELL_ATT_MFMA_RESIDENT)
    return adell_att_mfma_launch3<AT, DT, true>(which, a, grid, p.lds, st);
  return adell_att_mfma_launch3<AT, DT, false>(which, a, grid, p.lds, st);
}
template <int AT>
static int adell_att_mfma_launch1(int which, const AttArgs& a, int BH, const AdellAttPlan& p, hipStream_t st) {
  switch (a.Dv) {
    case 32: return adell_att_mfma_launch2<AT, 1>(which, a, BH, p, st);
    case 64: return adell_att_mfma_launch2<AT, 2>(which, a, BH, p, st);
    default: return adell_att_mfma_launch2<AT, 4>(which, a, BH, p, st);
  }
}
static int adell_att_mfma_launch(int which, const AttArgs& a, int BH, const AdellAttPlan& p, hipStream_t st) {
  switch (a.A) {
    case 32: return adell_att_mfma_launch1<1>(which, a, BH, p, st);
    case 64: return adell_att_mfma_launch1<2>(which, a, BH, p, st);
    default: return adell_att_mfma_launch1<4>(which, a, BH, p, st);
  }
}

template <auto Kern>
static int adell_att_valu_launch(const AttArgs& a, int BH, const AdellAttPlan& p, hipStream_t st) {
  return adell_launch<Kern>(dim3((unsigned)p.grid_x, (unsigned)BH), dim3(256), p.lds, st, a);
}

// one pass of the contiguous or the strided entry, as planned
static int adell_att_launch(int which, const AttArgs& a, int BH, const AdellAttPlan& p, hipStream_t st) {
  if (p.path == ADELL_ATT_MFMA_RESIDENT || p.path == ADELL_ATT_MFMA_STREAMED)
    return adell_att_mfma_launch(which, a, BH, p, st);
  ADELL_REQUIRE(p.path == ADELL_ATT_VALU, "attention: no kernel for head dims (%d, %d)", a.A, a.Dv);
  if (which == 0) return adell_att_valu_launch<adell_attention_fwd_kernel>(a, BH, p, st);
  if (which == 1)
    return p.rows == ATT_ROWS ? adell_att_valu_launch<adell_attention_bwd_q_kernel<ATT_ROWS>>(a, BH, p, st)
                              : adell_att_valu_launch<adell_attention_bwd_q_kernel<ATT_ROWS / 2>>(a, BH, p, st);
  return p.rows == ATT_ROWS ? adell_att_valu_launch<adell_attention_bwd_kv_kernel<ATT_ROWS>>(a, BH, p, st)
                            : adell_att_valu_launch<adell_attention_bwd_kv_kernel<ATT_ROWS / 2>>(a, BH, p, st);
}

// The three launching entries. Each uses the first `nops` operands of the order of
// adell_attention_desc::stride (q, k, v, out, dout, dq, dk, dv). Stride policy of strided operands:
// strict entries refuse what the MFMA kernels cannot stage with 16-byte loads (and shapes without an
// MFMA instance); the lenient one plans the vector-ALU form for it.
enum AttEntry { ATT_FWD, ATT_BWD, ATT_DBIAS };
static const struct { const char* name; int nops; bool strict; } ATT_ENTRY[] = {
    {"attention_fwd", 4, true}, {"attention_bwd", 8, true}, {"attention_bias_grad", 5, false}};
static const char* const ATT_OPERAND[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};

static bool adell_att_is_mfma(const AdellAttPlan& p) {
  return p.path == ADELL_ATT_MFMA_RESIDENT || p.path == ADELL_ATT_MFMA_STREAMED;
}

// Element strides of operand `i` (`C` values per row) of entry `e`, checked by the entry's policy.
// *aligned: what adell_att_plan is to be asked with.
static int adell_att_stride(AttEntry e, const adell_attention_desc* d, int i, const void* p, int C,
                            AttStride* out, bool* aligned) {
  const char* who = ATT_ENTRY[e].name;
  const bool a16 = (((uintptr_t)p) & 15) == 0;
  if (!d->strided) {   // contiguous [BH][T][C], any alignment
    *out = {(long)d->T * C, 0, C};
    *aligned = *aligned && a16;
    return ADELL_OK;
  }
  const int64_t* s = d->stride[i];
  const bool mult4 = s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0;
  ADELL_REQUIRE(s[0] >= 0 && s[1] >= 0 && s[2] >= C,
                "%s (strided): bad %s strides (%ld, %ld, %ld): none negative, rows at least %d apart", who,
                ATT_OPERAND[i], (long)s[0], (long)s[1], (long)s[2], C);
  if (ATT_ENTRY[e].strict) {
    ADELL_REQUIRE(a16, "%s (strided): %s must be 16-byte aligned", who, ATT_OPERAND[i]);
    ADELL_REQUIRE(mult4, "%s (strided): %s strides (%ld, %ld, %ld) must be multiples of 4 elements", who,
                  ATT_OPERAND[i], (long)s[0], (long)s[1], (long)s[2]);
  }
  *out = {(long)s[0], (long)s[1], (long)s[2]};
  *aligned = *aligned && a16 && mult4;
  return ADELL_OK;
}

// The kernels' arguments of entry `e` from its descriptor and tensors (op: the 8 operands in
// descriptor order, those past the entry's own null): every check that needs no plan, in one place.
static int adell_att_fill(AttEntry e, const adell_attention_desc* d, const float* const op[8],
                          const float* lse, AttArgs* out, bool* aligned) {
  const char* who = ATT_ENTRY[e].name;
  ADELL_REQUIRE(d, "%s: null descriptor", who);
  const int BH = d->BH, T = d->T, A = d->A, Dv = d->Dv;
  ADELL_REQUIRE(BH > 0 && T > 0 && A > 0 && Dv > 0, "%s: bad dims", who);
  ADELL_REQUIRE(A <= 256 && Dv <= 256, "%s: head dims up to 256 supported", who);
  ADELL_REQUIRE(!d->strided || (d->H > 0 && BH % d->H == 0),
                "%s (strided): %d sequences are not items of %d heads", who, BH, d->H);
  ADELL_REQUIRE(d->bias == nullptr || d->nbias > 0, "%s: bias needs nbias > 0", who);
  if (e == ATT_DBIAS) {
    ADELL_REQUIRE(d->nbias > 0 && d->nbias <= BH, "%s: nbias must be in [1, BH]", who);
    ADELL_REQUIRE(d->nbias <= 65535, "%s: at most 65535 bias slices (grid y), got %d", who, d->nbias);
  }
  ADELL_REQUIRE(!(d->strided && ATT_ENTRY[e].strict) || adell_att_is_mfma(adell_att_plan(0, T, A, Dv, true)),
                "%s (strided): head dims (%d, %d) at %d tokens have no MFMA instance", who, A, Dv, T);
  for (int i = 0; i < ATT_ENTRY[e].nops; ++i) ADELL_REQUIRE(op[i], "%s: null pointer (%s)", who, ATT_OPERAND[i]);
  ADELL_REQUIRE(lse, "%s: null pointer (lse)", who);
  ADELL_REQUIRE(d->labels == nullptr || (d->nlab > 0 && d->H > 0), "%s: labels need nlab > 0 and H > 0", who);
  ADELL_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "%s: bad dropout probability", who);
  AttArgs a = {};
  a.q = op[0]; a.k = op[1]; a.v = op[2]; a.bias = d->bias; a.labels = d->labels;
  if (e == ATT_FWD) {
    a.out = (float*)op[3]; a.lse_out = (float*)lse;
  } else {
    a.o = op[3]; a.dout = op[4]; a.lse = lse;
    a.dq = (float*)op[5]; a.dk = (float*)op[6]; a.dv = (float*)op[7];
  }
  a.T = T; a.A = A; a.Dv = Dv; a.nbias = d->nbias > 0 ? d->nbias : 1;
  a.nlab = d->nlab > 0 ? d->nlab : 1; a.labH = d->H > 0 ? d->H : 1;
  a.scale = d->scale; a.drop_p = d->drop_p;
  a.seed_lo = (uint32_t)d->seed; a.seed_hi = (uint32_t)(d->seed >> 32); a.rng_offset = d->rng_offset;
  a.H = d->strided ? d->H : 1;
  AttStride* const st[8] = {&a.sq, &a.sk, &a.sv, &a.so, &a.sg, &a.sdq, &a.sdk, &a.sdv};
  const int width[8] = {A, A, Dv, Dv, Dv, A, A, Dv};
  *aligned = true;   // the MFMA kernels stage with 16-byte loads: other operands take the vector-ALU kernels
  for (int i = 0; i < ATT_ENTRY[e].nops; ++i) {
    const int rc = adell_att_stride(e, d, i, op[i], width[i], st[i], aligned);
    if (rc != ADELL_OK) return rc;
  }
  *out = a;
  return ADELL_OK;
}

// With strided operands (sequence bh = b * H + h) Q / K / V can stay inside the packed
// [B][T][H][q | k | v] projection output, O / dO are read and written as [B][T][H * Dv] token rows,
// dQ / dK / dV land where the caller's next kernel wants them -- none of the permute / slice copies
// of linear_blocks.py:372-417 exist as launches.
extern "C" int adell_attention_fwd(const adell_attention_desc* d, const float* q, const float* k,
                                   const float* v, float* out, float* lse, void* stream) {
  const float* const op[8] = {q, k, v, out};
  AttArgs a;
  bool aligned;
  const int rc = adell_att_fill(ATT_FWD, d, op, lse, &a, &aligned);
  if (rc != ADELL_OK) return rc;
  return adell_att_launch(0, a, d->BH, adell_att_plan(0, a.T, a.A, a.Dv, aligned), (hipStream_t)stream);
}

extern "C" int adell_attention_bwd(const adell_attention_desc* d, const float* q, const float* k,
                                   const float* v, const float* out, const float* dout,
                                   const float* lse, float* dq, float* dk, float* dv, void* stream) {
  const float* const op[8] = {q, k, v, out, dout, dq, dk, dv};
  AttArgs a;
  bool aligned;
  int rc = adell_att_fill(ATT_BWD, d, op, lse, &a, &aligned);
  if (rc != ADELL_OK) return rc;
  const AdellAttPlan pq = adell_att_plan(1, a.T, a.A, a.Dv, aligned), pkv = adell_att_plan(2, a.T, a.A, a.Dv, aligned);
  ADELL_REQUIRE(pq.path != ADELL_ATT_REFUSED && pkv.path != ADELL_ATT_REFUSED,
                "attention_bwd: no kernel for head dims (%d, %d)", a.A, a.Dv);   // before the first launch
  rc = adell_att_launch(1, a, d->BH, pq, (hipStream_t)stream);
  if (rc != ADELL_OK) return rc;
  return adell_att_launch(2, a, d->BH, pkv, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Bias gradient (kernels above). The result has nbias * query tiles * key tiles block tiles; the
// sequences of a slice are split into at most ADELL_ATT_DBIAS_BLOCKS / that many chunks (and at most
// ADELL_ATT_DBIAS_CHUNKS), so the workspace is a fixed number of partial tiles whatever the number
// of sequences.
// ---------------------------------------------------------------------------------------------
#define ADELL_ATT_DBIAS_BLOCKS 512
#define ADELL_ATT_DBIAS_NK 4
#define ADELL_ATT_DBIAS_CHUNKS 16   // partial results per slice at most: the workspace is <= 16 x dbias

static int adell_att_dbias_max_chunks(int nbias, int T) {
  // the MFMA tiling (128 x 128) gives the fewest tiles: its chunk count bounds the vector-ALU form's
  const long t = adell_cdiv(T, 128), tiles = (long)nbias * t * t;
  const long c = ADELL_ATT_DBIAS_BLOCKS / tiles;
  return (int)(c < 1 ? 1 : (c > ADELL_ATT_DBIAS_CHUNKS ? ADELL_ATT_DBIAS_CHUNKS : c));
}

extern "C" long adell_attention_bias_grad_workspace_floats(int nbias, int T) {
  if (nbias <= 0 || T <= 0) return 0;
  const int c = adell_att_dbias_max_chunks(nbias, T);
  return c > 1 ? (long)c * nbias * T * T : 0;
}

template <int AT, int DT>
static int adell_att_dbias_mfma2(const AttArgs& a, const AttBiasGrad& g, dim3 grid, hipStream_t st) {
  const size_t lds = sizeof(float) * 32 * ((size_t)(AT * 32 + 1) + (size_t)(DT * 32 + 1));
  return adell_launch<adell_attn_mfma_dbias_kernel<AT, DT, ADELL_ATT_DBIAS_NK>>(grid, dim3(256), lds, st, a, g);
}
template <int AT>
static int adell_att_dbias_mfma1(const AttArgs& a, const AttBiasGrad& g, dim3 grid, hipStream_t st) {
  switch (a.Dv) {
    case 32: return adell_att_dbias_mfma2<AT, 1>(a, g, grid, st);
    case 64: return adell_att_dbias_mfma2<AT, 2>(a, g, grid, st);
    default: return adell_att_dbias_mfma2<AT, 4>(a, g, grid, st);
  }
}

extern "C" int adell_attention_bias_grad(const adell_attention_desc* d, const float* q, const float* k,
                                         const float* v, const float* out, const float* dout,
                                         const float* lse, float* dbias, float* workspace,
                                         long workspace_floats, void* stream) {
  const float* const op[8] = {q, k, v, out, dout};
  AttArgs a;
  bool aligned;
  int rc = adell_att_fill(ATT_DBIAS, d, op, lse, &a, &aligned);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dbias, "attention_bias_grad: null pointer (dbias)");
  const int BH = d->BH, T = a.T, A = a.A, Dv = a.Dv, nbias = a.nbias;
  const AdellAttPlan p = adell_att_plan(1, T, A, Dv, aligned);   // the dQ kernel's choice of form
  ADELL_REQUIRE(p.path != ADELL_ATT_REFUSED, "attention_bias_grad: no kernel for head dims (%d, %d)", A, Dv);
  const bool mfma = p.path != ADELL_ATT_VALU;
  const int nj = adell_cdiv(BH, nbias);   // sequences of slice 0, the longest list
  int chunks = adell_att_dbias_max_chunks(nbias, T);
  if (chunks > nj) chunks = nj;
  AttBiasGrad g = {dbias, BH, adell_cdiv(nj, chunks), 0};
  chunks = adell_cdiv(nj, g.chunk);
  const long n = (long)nbias * T * T;
  if (chunks > 1) {
    ADELL_REQUIRE(workspace && workspace_floats >= chunks * n, "attention_bias_grad: workspace too small");
    g.dst = workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  if (mfma) {
    g.tiles_k = adell_cdiv(T, 32 * ADELL_ATT_DBIAS_NK);
    const dim3 grid((unsigned)(adell_cdiv(T, 128) * g.tiles_k), (unsigned)nbias, (unsigned)chunks);
    switch (A) {
      case 32: rc = adell_att_dbias_mfma1<1>(a, g, grid, st); break;
      case 64: rc = adell_att_dbias_mfma1<2>(a, g, grid, st); break;
      default: rc = adell_att_dbias_mfma1<4>(a, g, grid, st); break;
    }
  } else {
    g.tiles_k = adell_cdiv(T, ATT_TK);
    const dim3 grid((unsigned)(adell_cdiv(T, p.rows) * g.tiles_k), (unsigned)nbias, (unsigned)chunks);
    rc = p.rows == ATT_ROWS
             ? adell_launch<adell_attention_dbias_kernel<ATT_ROWS>>(grid, dim3(256), p.lds, st, a, g)
             : adell_launch<adell_attention_dbias_kernel<ATT_ROWS / 2>>(grid, dim3(256), p.lds, st, a, g);
  }
  if (rc != ADELL_OK || chunks == 1) return rc;
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return adell_launch<adell_attn_dbias_fold_kernel>(dim3((unsigned)blocks), dim3(256), 0, st,
                                                    (const float*)workspace, dbias, n, chunks);
}

// Host-only launch plan of one pass of adell_attention_fwd / _bwd (strided operands: aligned = 1):
// the adell_att_plan call the launch makes (include/adell_hip.h: out[4]).
extern "C" int adell_attention_plan(int pass, int T, int A, int Dv, int aligned, int* out) {
  ADELL_REQUIRE(out && pass >= 0 && pass <= 2, "attention_plan: bad arguments");
  const AdellAttPlan p = adell_att_plan(pass, T, A, Dv, aligned != 0);
  out[0] = p.path; out[1] = (int)p.lds; out[2] = p.grid_x; out[3] = p.rows;
  return ADELL_OK;
}
