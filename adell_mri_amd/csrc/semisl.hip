// Losses of the semi-supervised U-Net beyond the local contrastive one (adell_mri/modules/
// semi_supervised_segmentation/losses.py): LocalContrastiveLossWithAnchors, NearestNeighbourLoss (its
// loss and the gather behind its queue) and PseudoLabelCrossEntropy. fp32 data, every sum that leaves a
// thread in fp64 and in a fixed order (strided per thread, xor butterflies, waves in index order), no
// float atomics, no scratch: two runs are bit-identical.
//   * anchor loss. x, a1, a2 are NDHWC rows [B][V][C]. adell_anchor_sim_kernel: a group of G = min(64,
//     pow2 <= C/4) lanes owns a voxel, each lane a channel quad, the five partial dot products are folded
//     with xor shuffles; sim_k[b][v] = cos(x, a_k) / T (each norm clamped at 1e-8 on its own, as torch's
//     cosine_similarity) and the block's online-softmax partial (max, sum of exponentials) of both rows.
//     adell_anchor_fold_kernel folds the partials of an item in index order into (max, log sum);
//     adell_anchor_rows_kernel walks the [B][V] rows once: H = sum q log q, A = sum p q per block;
//     adell_anchor_loss_kernel folds them: loss = H - A, which is what F.kl_div(p, q, "none").sum(-1) gives
//     when its input p is a probability (the reference passes one). The backward reads the two rows and
//     the six scalars of an item, d L / d sim_1 = p (A - q), d L / d sim_2 = q (log q - p - H + A),
//     recomputes the dot products and writes dx (da1, da2 when wanted):
//     d cos(x, a) / d x = rx ra (a - [|x| > 1e-8] (x.a) rx^2 x).
//   * nearest-neighbour loss. A thread per voxel; the block's NV voxel rows sit in LDS (row stride s
//     floats with s / 4 odd: the 16 lanes of a ds_read_b128 group hit 16 distinct 16-byte slots), the
//     normalised past rows pass through LDS in tiles of SS_TQ rows that every lane reads at the same
//     address (a broadcast). Four past rows per step: five 16-byte LDS reads per 16 FMAs.
//     S = sum_q exp(-d_q m_q / T), O = sum_q exp(-d_q (1 - m_q) / T), d_q = 1 - cos(x, past_q),
//     m_q = y[b][class_q][v] (re-read only when the class changes: a queue is stored class by class);
//     a NaN term counts 0 (nansum), a NaN ratio S / O leaves the mean (nanmean). S and O are kept per
//     voxel; the backward recomputes the tiles once, accumulates sum_q coef_q past_q in a second LDS
//     tile and writes dx; a voxel whose ratio is NaN gets an exact 0.
//   * queue gather. adell_nnq_count_kernel counts y > 0 per (item, class, chunk of SS_CH voxels); the
//     caller sums and scans that table; adell_nnq_gather_kernel, a wave per selected row, finds the chunk
//     of rank j by binary search in the scanned table (item-major, then voxel: the order of
//     torch.where(y > 0) within a class), the voxel inside it by ballots, and copies that row of X.
//   * pseudo-label cross entropy. pred, proba are channel-major [B][K][V]; a thread per voxel reads the K
//     planes (coalesced along v) twice: online log-sum-exp, then -sum_k w_k t_k log_softmax_k with
//     t_k = (proba_k > threshold) (1 - ls) + ls / K, the probability-target form of F.cross_entropy. The
//     backward is one launch: dz_j = g scale (softmax_j sum_k w_k t_k - w_j t_j).
#include "common.h"

constexpr int SS_NT = 256;
constexpr int SS_NW = SS_NT / 64;
constexpr float SS_COS_EPS = 1e-8f;
constexpr int SS_TQ = 32;                       // past rows per LDS tile
constexpr int SS_CH = ADELL_SEMISL_PUT_CHUNK;   // voxels per counting chunk
constexpr int SS_NV_FWD = 256, SS_NV_BWD = 128; // voxels per block of the nearest-neighbour kernels
constexpr int SS_MAX_PART = 1024;               // blocks per item of the anchor passes

static inline int ss_row_stride(int C) { return ((C >> 2) & 1) ? C : C + 4; }
static inline size_t ss_nnq_lds(int NV, int C, int tiles) {
  return ((size_t)tiles * NV * ss_row_stride(C) + (size_t)SS_TQ * C) * sizeof(float) + SS_TQ * sizeof(int);
}
static_assert(2 * adell_lds_alloc(((size_t)SS_NV_FWD * (ADELL_SEMISL_NN_MAX_C + 4) +
                                   (size_t)SS_TQ * ADELL_SEMISL_NN_MAX_C + SS_TQ) * 4 + 256) <=
                  (size_t)kAdellLdsPerCu,
              "two forward blocks of the nearest-neighbour loss must fit a CU's LDS");
static_assert(2 * adell_lds_alloc(((size_t)2 * SS_NV_BWD * (ADELL_SEMISL_NN_MAX_C + 4) +
                                   (size_t)SS_TQ * ADELL_SEMISL_NN_MAX_C + SS_TQ) * 4 + 256) <=
                  (size_t)kAdellLdsPerCu,
              "two backward blocks of the nearest-neighbour loss must fit a CU's LDS");

// Block sums in a fixed order: an xor butterfly per wave (both partners add the same two numbers, so
// every lane holds the same bits), the waves in index order. sh: one double per wave. NT threads.
template <int NT>
__device__ __forceinline__ double ss_block_sum_d(double v, double* sh) {
  v = adell_wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) t += sh[k];
  return t;
}
template <int NT>
__device__ __forceinline__ double ss_block_max_d(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
#pragma unroll
  for (int k = 1; k < NT / 64; ++k) t = fmax(t, sh[k]);
  return t;
}

// ---- anchor loss ------------------------------------------------------------------------------------
struct SsDots {
  float d1, d2, nx, n1, n2;
};

__device__ __forceinline__ SsDots ss_anchor_dots(const float4* __restrict__ X, const float4* __restrict__ A1,
                                                 const float4* __restrict__ A2, size_t row, int C4, int G,
                                                 int gl, bool ok) {
  SsDots m = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (ok) {
    for (int q = gl; q < C4; q += G) {
      const float4 x = X[row * C4 + q], u = A1[row * C4 + q], w = A2[row * C4 + q];
      m.nx += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      m.n1 += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
      m.n2 += w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w;
      m.d1 += x.x * u.x + x.y * u.y + x.z * u.z + x.w * u.w;
      m.d2 += x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
    }
  }
  for (int o = G >> 1; o > 0; o >>= 1) {
    m.d1 += __shfl_xor(m.d1, o, 64);
    m.d2 += __shfl_xor(m.d2, o, 64);
    m.nx += __shfl_xor(m.nx, o, 64);
    m.n1 += __shfl_xor(m.n1, o, 64);
    m.n2 += __shfl_xor(m.n2, o, 64);
  }
  return m;
}

__device__ __forceinline__ void ss_online(float z, float& mx, float& s) {
  if (z > mx) {
    s = s * expf(mx - z) + 1.f;
    mx = z;
  } else {
    s += expf(z - mx);
  }
}

// grid (blocks, B), grid-strided over the voxels of item blockIdx.y; part [B][gridDim.x][4] =
// (max_1, sum_1, max_2, sum_2) of the block's voxels
__global__ __launch_bounds__(SS_NT) void adell_anchor_sim_kernel(
    const float* __restrict__ x, const float* __restrict__ a1, const float* __restrict__ a2, long V, int C,
    int G, float invT, float* __restrict__ sim1, float* __restrict__ sim2, double* __restrict__ part) {
  __shared__ double sh[SS_NW];
  const int C4 = C >> 2, gl = threadIdx.x & (G - 1), vpb = SS_NT / G;
  const size_t b = blockIdx.y;
  const long stride = (long)gridDim.x * vpb;
  const long rounds = (V + stride - 1) / stride;  // every thread runs every round (shuffles)
  const float4* X = reinterpret_cast<const float4*>(x);
  const float4* A1 = reinterpret_cast<const float4*>(a1);
  const float4* A2 = reinterpret_cast<const float4*>(a2);
  float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f;
  for (long r = 0; r < rounds; ++r) {
    const long v = r * stride + (long)blockIdx.x * vpb + threadIdx.x / G;
    const bool ok = v < V;
    const size_t row = b * (size_t)V + (size_t)(ok ? v : 0);
    const SsDots m = ss_anchor_dots(X, A1, A2, row, C4, G, gl, ok);
    if (!ok || gl != 0) continue;
    const float rx = 1.f / fmaxf(sqrtf(m.nx), SS_COS_EPS);
    const float z1 = m.d1 * rx * (1.f / fmaxf(sqrtf(m.n1), SS_COS_EPS)) * invT;
    const float z2 = m.d2 * rx * (1.f / fmaxf(sqrtf(m.n2), SS_COS_EPS)) * invT;
    sim1[row] = z1;
    sim2[row] = z2;
    ss_online(z1, m1, s1);
    ss_online(z2, m2, s2);
  }
  const double M1 = ss_block_max_d<SS_NT>((double)m1, sh);
  const double M2 = ss_block_max_d<SS_NT>((double)m2, sh);
  const double t1 = ss_block_sum_d<SS_NT>(s1 > 0.f || s1 != s1 ? (double)s1 * exp((double)m1 - M1) : 0.0, sh);
  const double t2 = ss_block_sum_d<SS_NT>(s2 > 0.f || s2 != s2 ? (double)s2 * exp((double)m2 - M2) : 0.0, sh);
  if (threadIdx.x == 0) {
    double* o = part + (b * gridDim.x + blockIdx.x) * 4;
    o[0] = M1;
    o[1] = t1;
    o[2] = M2;
    o[3] = t2;
  }
}

// a block per item: stats[b][0 .. 4) = (max_1, log sum_1, max_2, log sum_2) over the nblk partials
__global__ __launch_bounds__(SS_NT) void adell_anchor_fold_kernel(const double* __restrict__ part, int nblk,
                                                                  double* __restrict__ stats) {
  __shared__ double sh[SS_NW];
  const double* p = part + (size_t)blockIdx.x * nblk * 4;
  for (int k = 0; k < 2; ++k) {
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += SS_NT) mx = fmax(mx, p[i * 4 + 2 * k]);
    mx = ss_block_max_d<SS_NT>(mx, sh);
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += SS_NT) s += p[i * 4 + 2 * k + 1] * exp(p[i * 4 + 2 * k] - mx);
    s = ss_block_sum_d<SS_NT>(s, sh);
    if (threadIdx.x == 0) {
      stats[blockIdx.x * 6 + 2 * k] = mx;
      stats[blockIdx.x * 6 + 2 * k + 1] = log(s);
    }
  }
}

// grid (blocks, B), a thread per voxel: part2 [B][gridDim.x][2] = (sum q log q, sum p q)
__global__ __launch_bounds__(SS_NT) void adell_anchor_rows_kernel(const float* __restrict__ sim1,
                                                                  const float* __restrict__ sim2, long V,
                                                                  const double* __restrict__ stats,
                                                                  double* __restrict__ part2) {
  __shared__ double sh[SS_NW];
  const size_t b = blockIdx.y;
  const double* st = stats + b * 6;
  const double M1 = st[0], L1 = st[1], M2 = st[2], L2 = st[3];
  double h = 0.0, a = 0.0;
  for (long v = (long)blockIdx.x * SS_NT + threadIdx.x; v < V; v += (long)gridDim.x * SS_NT) {
    const double p = exp((double)sim1[b * V + v] - M1 - L1);
    const double lq = (double)sim2[b * V + v] - M2 - L2;
    const double q = exp(lq);
    h += q > 0.0 || q != q ? q * lq : 0.0;  // xlogy(q, q): 0 at q = 0
    a += p * q;
  }
  h = ss_block_sum_d<SS_NT>(h, sh);
  a = ss_block_sum_d<SS_NT>(a, sh);
  if (threadIdx.x == 0) {
    part2[(b * gridDim.x + blockIdx.x) * 2] = h;
    part2[(b * gridDim.x + blockIdx.x) * 2 + 1] = a;
  }
}

// a block per item: stats[b][4] = H, stats[b][5] = A, loss[b] = H - A
__global__ __launch_bounds__(SS_NT) void adell_anchor_loss_kernel(const double* __restrict__ part2, int nblk,
                                                                  double* __restrict__ stats,
                                                                  float* __restrict__ loss) {
  __shared__ double sh[SS_NW];
  const double* p = part2 + (size_t)blockIdx.x * nblk * 2;
  double h = 0.0, a = 0.0;
  for (int i = threadIdx.x; i < nblk; i += SS_NT) {
    h += p[i * 2];
    a += p[i * 2 + 1];
  }
  h = ss_block_sum_d<SS_NT>(h, sh);
  a = ss_block_sum_d<SS_NT>(a, sh);
  if (threadIdx.x == 0) {
    stats[blockIdx.x * 6 + 4] = h;
    stats[blockIdx.x * 6 + 5] = a;
    loss[blockIdx.x] = (float)(h - a);
  }
}

__global__ __launch_bounds__(SS_NT) void adell_anchor_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ a1, const float* __restrict__ a2,
    const float* __restrict__ sim1, const float* __restrict__ sim2, const double* __restrict__ stats,
    const float* __restrict__ gloss, long V, int C, int G, float invT, float* __restrict__ dx,
    float* __restrict__ da1, float* __restrict__ da2) {
  const int C4 = C >> 2, gl = threadIdx.x & (G - 1), vpb = SS_NT / G;
  const size_t b = blockIdx.y;
  const long stride = (long)gridDim.x * vpb;
  const long rounds = (V + stride - 1) / stride;
  const float4* X = reinterpret_cast<const float4*>(x);
  const float4* A1 = reinterpret_cast<const float4*>(a1);
  const float4* A2 = reinterpret_cast<const float4*>(a2);
  const double* st = stats + b * 6;
  const double M1 = st[0], L1 = st[1], M2 = st[2], L2 = st[3], H = st[4], A = st[5];
  const double g = (double)gloss[b] * (double)invT;
  for (long r = 0; r < rounds; ++r) {
    const long v = r * stride + (long)blockIdx.x * vpb + threadIdx.x / G;
    const bool ok = v < V;
    const size_t row = b * (size_t)V + (size_t)(ok ? v : 0);
    const SsDots m = ss_anchor_dots(X, A1, A2, row, C4, G, gl, ok);
    if (!ok) continue;
    const double p = exp((double)sim1[row] - M1 - L1);
    const double lq = (double)sim2[row] - M2 - L2;
    const double q = exp(lq);
    const float ds1 = (float)(g * p * (A - q));
    const float ds2 = q > 0.0 || q != q ? (float)(g * q * (lq - p - H + A)) : 0.f;
    const float ax = sqrtf(m.nx), an1 = sqrtf(m.n1), an2 = sqrtf(m.n2);
    const float rx = 1.f / fmaxf(ax, SS_COS_EPS);
    const float r1 = 1.f / fmaxf(an1, SS_COS_EPS), r2 = 1.f / fmaxf(an2, SS_COS_EPS);
    const float kx = ax > SS_COS_EPS ? rx * rx : 0.f;
    const float k1 = an1 > SS_COS_EPS ? r1 * r1 : 0.f, k2 = an2 > SS_COS_EPS ? r2 * r2 : 0.f;
    const float c1 = ds1 * rx * r1, c2 = ds2 * rx * r2;
    const float sx = kx * (c1 * m.d1 + c2 * m.d2), s1 = c1 * k1 * m.d1, s2 = c2 * k2 * m.d2;
    for (int qd = gl; qd < C4; qd += G) {
      const float4 xv = X[row * C4 + qd], u = A1[row * C4 + qd], w = A2[row * C4 + qd];
      reinterpret_cast<float4*>(dx)[row * C4 + qd] =
          make_float4(c1 * u.x + c2 * w.x - sx * xv.x, c1 * u.y + c2 * w.y - sx * xv.y,
                      c1 * u.z + c2 * w.z - sx * xv.z, c1 * u.w + c2 * w.w - sx * xv.w);
      if (da1)
        reinterpret_cast<float4*>(da1)[row * C4 + qd] = make_float4(
            c1 * xv.x - s1 * u.x, c1 * xv.y - s1 * u.y, c1 * xv.z - s1 * u.z, c1 * xv.w - s1 * u.w);
      if (da2)
        reinterpret_cast<float4*>(da2)[row * C4 + qd] = make_float4(
            c2 * xv.x - s2 * w.x, c2 * xv.y - s2 * w.y, c2 * xv.z - s2 * w.z, c2 * xv.w - s2 * w.w);
    }
  }
}

static int ss_group(int C) {
  int G = 1;
  while (2 * G <= C / 4 && 2 * G <= 64) G *= 2;
  return G;
}
static int ss_anchor_blocks(long V, int per_block) {
  long b = (V + per_block - 1) / per_block;
  if (b > SS_MAX_PART) b = SS_MAX_PART;
  return (int)(b < 1 ? 1 : b);
}

extern "C" int adell_semisl_route(int kind, int C, int K) {
  switch (kind) {
    case ADELL_SEMISL_ANCHOR:
      ADELL_REQUIRE(C >= 1, "semisl_route: C = %d", C);
      return (C & 3) == 0 && C <= ADELL_SEMISL_ANCHOR_MAX_C ? ADELL_SEMISL_FUSED : ADELL_SEMISL_COMPOSED;
    case ADELL_SEMISL_NN:
      ADELL_REQUIRE(C >= 1 && K >= 1, "semisl_route: C = %d, K = %d", C, K);
      return (C & 3) == 0 && C <= ADELL_SEMISL_NN_MAX_C && K <= ADELL_SEMISL_MAX_CLASSES
                 ? ADELL_SEMISL_FUSED
                 : ADELL_SEMISL_COMPOSED;
    case ADELL_SEMISL_PSEUDO_LABEL:
      ADELL_REQUIRE(K >= 1, "semisl_route: K = %d", K);
      return K <= ADELL_SEMISL_MAX_CLASSES ? ADELL_SEMISL_FUSED : ADELL_SEMISL_COMPOSED;
    default:
      ADELL_REQUIRE(false, "semisl_route: kind %d", kind);
  }
  return ADELL_E_BADARG;
}

static int ss_anchor_check(const char* what, int B, long V, int C, float temperature) {
  ADELL_REQUIRE(B >= 1 && B <= 65535 && V >= 1, "%s: bad shape (B %d, V %ld)", what, B, V);
  ADELL_REQUIRE(C >= 4 && (C & 3) == 0 && C <= ADELL_SEMISL_ANCHOR_MAX_C,
                "%s: need C %% 4 == 0 and C <= %d (C = %d)", what, ADELL_SEMISL_ANCHOR_MAX_C, C);
  ADELL_REQUIRE(temperature > 0.f, "%s: temperature must be positive", what);
  return ADELL_OK;
}

extern "C" long adell_loco_anchor_workspace_doubles(int B, long V, int C) {
  if (ss_anchor_check("loco_anchor_workspace", B, V, C, 1.f) != ADELL_OK) return ADELL_E_BADARG;
  const long n1 = ss_anchor_blocks(V, SS_NT / ss_group(C)), n2 = ss_anchor_blocks(V, SS_NT);
  return (long)B * (4 * n1 + 2 * n2);
}

extern "C" int adell_loco_anchor_fwd(const float* x, const float* a1, const float* a2, int B, long V, int C,
                                     float temperature, float* sim1, float* sim2, double* stats,
                                     float* loss, double* workspace, long workspace_doubles, void* stream) {
  ADELL_REQUIRE(x && a1 && a2 && sim1 && sim2 && stats && loss && workspace, "loco_anchor_fwd: null pointer");
  if (ss_anchor_check("loco_anchor_fwd", B, V, C, temperature) != ADELL_OK) return ADELL_E_BADARG;
  ADELL_REQUIRE((((uintptr_t)x | (uintptr_t)a1 | (uintptr_t)a2) & 15) == 0, "loco_anchor_fwd: unaligned rows");
  ADELL_REQUIRE(workspace_doubles >= adell_loco_anchor_workspace_doubles(B, V, C),
                "loco_anchor_fwd: workspace too small");
  const int G = ss_group(C), n1 = ss_anchor_blocks(V, SS_NT / G), n2 = ss_anchor_blocks(V, SS_NT);
  hipStream_t st = (hipStream_t)stream;
  double* part = workspace;
  double* part2 = workspace + (size_t)B * 4 * n1;
  int rc = adell_launch<adell_anchor_sim_kernel>(dim3(n1, B), dim3(SS_NT), 0, st, x, a1, a2, V, C, G,
                                                 1.f / temperature, sim1, sim2, part);
  if (rc != ADELL_OK) return rc;
  rc = adell_launch<adell_anchor_fold_kernel>(dim3(B), dim3(SS_NT), 0, st, (const double*)part, n1, stats);
  if (rc != ADELL_OK) return rc;
  rc = adell_launch<adell_anchor_rows_kernel>(dim3(n2, B), dim3(SS_NT), 0, st, (const float*)sim1,
                                              (const float*)sim2, V, (const double*)stats, part2);
  if (rc != ADELL_OK) return rc;
  return adell_launch<adell_anchor_loss_kernel>(dim3(B), dim3(SS_NT), 0, st, (const double*)part2, n2, stats,
                                                loss);
}

extern "C" int adell_loco_anchor_bwd(const float* x, const float* a1, const float* a2, const float* sim1,
                                     const float* sim2, const double* stats, const float* gloss, int B,
                                     long V, int C, float temperature, float* dx, float* da1, float* da2,
                                     void* stream) {
  ADELL_REQUIRE(x && a1 && a2 && sim1 && sim2 && stats && gloss && dx, "loco_anchor_bwd: null pointer");
  if (ss_anchor_check("loco_anchor_bwd", B, V, C, temperature) != ADELL_OK) return ADELL_E_BADARG;
  ADELL_REQUIRE((((uintptr_t)x | (uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)dx | (uintptr_t)da1 |
                  (uintptr_t)da2) & 15) == 0,
                "loco_anchor_bwd: unaligned pointer");
  const int G = ss_group(C), n1 = ss_anchor_blocks(V, SS_NT / G);
  return adell_launch<adell_anchor_bwd_kernel>(dim3(n1, B), dim3(SS_NT), 0, (hipStream_t)stream, x, a1, a2,
                                               sim1, sim2, stats, gloss, V, C, G, 1.f / temperature, dx, da1,
                                               da2);
}

// ---- nearest-neighbour loss ---------------------------------------------------------------------------
// a wave per past row: out = row / max(|row|, 1e-8)
__global__ __launch_bounds__(SS_NT) void adell_nnq_normalize_kernel(const float* __restrict__ past, int Q,
                                                                    int C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * SS_NW + (threadIdx.x >> 6);
  if (q >= Q) return;  // whole waves leave: the shuffles below stay complete
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += past[q * C + c] * past[q * C + c];
  s = adell_wave_sum(s);
  const float r = 1.f / fmaxf(sqrtf(s), SS_COS_EPS);
  for (int c = lane; c < C; c += 64) out[q * C + c] = past[q * C + c] * r;
}

struct SsTile {
  float* xl;   // [NV][xs] the block's voxel rows
  float* acc;  // [NV][xs] (backward only)
  float* pl;   // [SS_TQ][C] past rows of the tile, zero beyond Q
  int* pc;     // [SS_TQ] their classes
};

template <int NV>
__device__ __forceinline__ SsTile ss_tile(float* lds, int C, int xs, bool with_acc) {
  SsTile t;
  t.xl = lds;
  t.acc = lds + (size_t)NV * xs;
  t.pl = lds + (size_t)(with_acc ? 2 : 1) * NV * xs;
  t.pc = reinterpret_cast<int*>(t.pl + (size_t)SS_TQ * C);
  return t;
}

// the block's rows of x into LDS (rows past N as zeros); returns the squared norm of this thread's row
template <int NV>
__device__ __forceinline__ float ss_load_x(const SsTile& t, const float* __restrict__ x, long n0, long N,
                                           int C, int xs) {
  const int C4 = C >> 2;
  const float4* X = reinterpret_cast<const float4*>(x) + (size_t)n0 * C4;
  for (int i = threadIdx.x; i < NV * C4; i += NV) {
    const int row = i / C4, col = i - row * C4;
    const float4 v = n0 + row < N ? X[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(t.xl + (size_t)row * xs + 4 * col) = v;
  }
  __syncthreads();
  float nx = 0.f;
  const float4* mine = reinterpret_cast<const float4*>(t.xl + (size_t)threadIdx.x * xs);
  for (int c = 0; c < C4; ++c) {
    const float4 v = mine[c];
    nx += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  return nx;
}

template <int NV>
__device__ __forceinline__ void ss_load_past(const SsTile& t, const float* __restrict__ pastn,
                                             const int* __restrict__ pcls, int q0, int Q, int C) {
  const int C4 = C >> 2, tq = min(SS_TQ, Q - q0);
  const float4* P = reinterpret_cast<const float4*>(pastn) + (size_t)q0 * C4;
  __syncthreads();  // the previous tile has been read
  for (int i = threadIdx.x; i < SS_TQ * C4; i += NV)
    reinterpret_cast<float4*>(t.pl)[i] = i < tq * C4 ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x; i < SS_TQ; i += NV) t.pc[i] = i < tq ? pcls[q0 + i] : -1;
  __syncthreads();
}

// dot products of this thread's row with the past rows j .. j + 3 of the tile
__device__ __forceinline__ void ss_dots4(const SsTile& t, int xs, int C4, int j, float d[4]) {
  const float4* mine = reinterpret_cast<const float4*>(t.xl + (size_t)threadIdx.x * xs);
  const float4* P = reinterpret_cast<const float4*>(t.pl);
  d[0] = d[1] = d[2] = d[3] = 0.f;
  for (int c = 0; c < C4; ++c) {
    const float4 v = mine[c];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float4 p = P[(size_t)(j + jj) * C4 + c];
      d[jj] += v.x * p.x + v.y * p.y + v.z * p.z + v.w * p.w;
    }
  }
}

// y [B][K][V]; S, O [B V]; part [gridDim.x][2] = (sum of the ratios that are not NaN, their count)
__global__ __launch_bounds__(SS_NV_FWD) void adell_nnq_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ pastn,
    const int* __restrict__ pcls, long N, long V, int C, int K, int Q, int xs, float invT,
    float* __restrict__ S, float* __restrict__ O, double* __restrict__ part) {
  constexpr int NV = SS_NV_FWD;
  extern __shared__ __attribute__((aligned(16))) float ss_lds[];
  __shared__ double sh[NV / 64];
  const SsTile t = ss_tile<NV>(ss_lds, C, xs, false);
  const long n0 = (long)blockIdx.x * NV, n = n0 + threadIdx.x;
  const bool ok = n < N;
  const long b = ok ? n / V : 0, v = ok ? n - b * V : 0;
  const float rx = 1.f / fmaxf(sqrtf(ss_load_x<NV>(t, x, n0, N, C, xs)), SS_COS_EPS);
  const int C4 = C >> 2;
  float s = 0.f, o = 0.f, m = 0.f;
  int last = -1;
  for (int q0 = 0; q0 < Q; q0 += SS_TQ) {
    ss_load_past<NV>(t, pastn, pcls, q0, Q, C);
    const int tq = min(SS_TQ, Q - q0);
    for (int j = 0; j < tq; j += 4) {
      float d[4];
      ss_dots4(t, xs, C4, j, d);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (j + jj >= tq) break;
        const int cls = t.pc[j + jj];
        if (cls != last) {
          last = cls;
          m = ok && cls >= 0 && cls < K ? y[((size_t)b * K + cls) * V + v] : 0.f;
        }
        const float dist = 1.f - d[jj] * rx;
        const float es = expf(-dist * m * invT), eo = expf(-dist * (1.f - m) * invT);
        s += es != es ? 0.f : es;
        o += eo != eo ? 0.f : eo;
      }
    }
  }
  const float ratio = s / o;
  const bool valid = ok && ratio == ratio;
  if (ok) {
    S[n] = s;
    O[n] = o;
  }
  const double sum = ss_block_sum_d<NV>(valid ? (double)ratio : 0.0, sh);
  const double cnt = ss_block_sum_d<NV>(valid ? 1.0 : 0.0, sh);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 2] = sum;
    part[(size_t)blockIdx.x * 2 + 1] = cnt;
  }
}

// stats = (sum, count), loss = sum / count (NaN when no ratio counts, as nanmean)
__global__ __launch_bounds__(SS_NT) void adell_nnq_fold_kernel(const double* __restrict__ part, long nblk,
                                                               double* __restrict__ stats,
                                                               float* __restrict__ loss) {
  __shared__ double sh[SS_NW];
  double s = 0.0, c = 0.0;
  for (long i = threadIdx.x; i < nblk; i += SS_NT) {
    s += part[i * 2];
    c += part[i * 2 + 1];
  }
  s = ss_block_sum_d<SS_NT>(s, sh);
  c = ss_block_sum_d<SS_NT>(c, sh);
  if (threadIdx.x == 0) {
    stats[0] = s;
    stats[1] = c;
    loss[0] = (float)(s / c);
  }
}

__global__ __launch_bounds__(SS_NV_BWD) void adell_nnq_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ pastn,
    const int* __restrict__ pcls, const float* __restrict__ S, const float* __restrict__ O,
    const double* __restrict__ stats, const float* __restrict__ g, long N, long V, int C, int K, int Q,
    int xs, float invT, float* __restrict__ dx) {
  constexpr int NV = SS_NV_BWD;
  extern __shared__ __attribute__((aligned(16))) float ss_lds[];
  const SsTile t = ss_tile<NV>(ss_lds, C, xs, true);
  const long n0 = (long)blockIdx.x * NV, n = n0 + threadIdx.x;
  const bool ok = n < N;
  const long b = ok ? n / V : 0, v = ok ? n - b * V : 0;
  const float ax = sqrtf(ss_load_x<NV>(t, x, n0, N, C, xs));
  const float rx = 1.f / fmaxf(ax, SS_COS_EPS), kx = ax > SS_COS_EPS ? rx * rx : 0.f;
  const int C4 = C >> 2;
  float4* acc = reinterpret_cast<float4*>(t.acc + (size_t)threadIdx.x * xs);
  float4* mine = reinterpret_cast<float4*>(t.xl + (size_t)threadIdx.x * xs);
  for (int c = 0; c < C4; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float s = ok ? S[n] : 0.f, o = ok ? O[n] : 1.f;
  const float ratio = s / o;
  const bool valid = ok && ratio == ratio;
  const float gs = valid ? g[0] * (float)(1.0 / stats[1]) * invT : 0.f;
  const float coef_s = gs / o, coef_o = gs * ratio / o;
  float sc = 0.f, m = 0.f;
  int last = -1;
  for (int q0 = 0; q0 < Q; q0 += SS_TQ) {
    ss_load_past<NV>(t, pastn, pcls, q0, Q, C);
    const int tq = min(SS_TQ, Q - q0);
    for (int j = 0; j < tq; j += 4) {
      float d[4], w[4];
      ss_dots4(t, xs, C4, j, d);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        w[jj] = 0.f;
        if (j + jj >= tq || !valid) continue;
        const int cls = t.pc[j + jj];
        if (cls != last) {
          last = cls;
          m = cls >= 0 && cls < K ? y[((size_t)b * K + cls) * V + v] : 0.f;
        }
        const float cs = d[jj] * rx, dist = 1.f - cs;
        const float es = expf(-dist * m * invT), eo = expf(-dist * (1.f - m) * invT);
        const float ws = m * es * coef_s, wo = (1.f - m) * eo * coef_o;
        w[jj] = (es != es || ws != ws ? 0.f : ws) - (eo != eo || wo != wo ? 0.f : wo);
        sc += w[jj] * cs;
      }
      const float4* P = reinterpret_cast<const float4*>(t.pl);
      for (int c = 0; c < C4; ++c) {
        float4 a = acc[c];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float4 p = P[(size_t)(j + jj) * C4 + c];
          a.x += w[jj] * p.x;
          a.y += w[jj] * p.y;
          a.z += w[jj] * p.z;
          a.w += w[jj] * p.w;
        }
        acc[c] = a;
      }
    }
  }
  // d cos / d x = rx past - [|x| > eps] cos rx^2 x, summed with the coefficients; 0 where the ratio is NaN
  const float sx = kx * sc;
  for (int c = 0; c < C4; ++c) {
    const float4 a = acc[c], xv = mine[c];
    acc[c] = valid ? make_float4(rx * a.x - sx * xv.x, rx * a.y - sx * xv.y, rx * a.z - sx * xv.z,
                                 rx * a.w - sx * xv.w)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  float4* DX = reinterpret_cast<float4*>(dx) + (size_t)n0 * C4;
  for (int i = threadIdx.x; i < NV * C4; i += NV) {
    const int row = i / C4, col = i - row * C4;
    if (n0 + row < N) DX[i] = *reinterpret_cast<const float4*>(t.acc + (size_t)row * xs + 4 * col);
  }
}

static int ss_nnq_check(const char* what, int B, long V, int C, int K, int Q, float temperature) {
  ADELL_REQUIRE(B >= 1 && V >= 1 && Q >= 1 && K >= 1 && K <= ADELL_SEMISL_MAX_CLASSES,
                "%s: bad shape (B %d, V %ld, K %d, Q %d; K <= %d)", what, B, V, K, Q,
                ADELL_SEMISL_MAX_CLASSES);
  ADELL_REQUIRE(C >= 4 && (C & 3) == 0 && C <= ADELL_SEMISL_NN_MAX_C,
                "%s: need C %% 4 == 0 and C <= %d (C = %d)", what, ADELL_SEMISL_NN_MAX_C, C);
  ADELL_REQUIRE((long)B * V / SS_NV_BWD < 2147483647L, "%s: too many voxels (%ld)", what, (long)B * V);
  ADELL_REQUIRE(temperature > 0.f, "%s: temperature must be positive", what);
  return ADELL_OK;
}

extern "C" long adell_nn_queue_workspace_doubles(int B, long V) {
  ADELL_REQUIRE(B >= 1 && V >= 1, "nn_queue_workspace: bad shape (B %d, V %ld)", B, V);
  return 2 * (((long)B * V + SS_NV_FWD - 1) / SS_NV_FWD);
}

extern "C" int adell_nn_queue_normalize(const float* past, int Q, int C, float* out, void* stream) {
  ADELL_REQUIRE(past && out && Q >= 1 && C >= 1, "nn_queue_normalize: bad arguments (Q %d, C %d)", Q, C);
  return adell_launch<adell_nnq_normalize_kernel>(dim3((unsigned)adell_cdiv(Q, SS_NW)), dim3(SS_NT), 0,
                                                  (hipStream_t)stream, past, Q, C, out);
}

extern "C" int adell_nn_queue_loss_fwd(const float* x, const float* y, const float* pastn,
                                       const int* past_class, int B, long V, int C, int K, int Q,
                                       float temperature, float* S, float* O, double* stats, float* loss,
                                       double* workspace, long workspace_doubles, void* stream) {
  ADELL_REQUIRE(x && y && pastn && past_class && S && O && stats && loss && workspace,
                "nn_queue_loss_fwd: null pointer");
  if (ss_nnq_check("nn_queue_loss_fwd", B, V, C, K, Q, temperature) != ADELL_OK) return ADELL_E_BADARG;
  ADELL_REQUIRE((((uintptr_t)x | (uintptr_t)pastn) & 15) == 0, "nn_queue_loss_fwd: unaligned rows");
  ADELL_REQUIRE(workspace_doubles >= adell_nn_queue_workspace_doubles(B, V),
                "nn_queue_loss_fwd: workspace too small");
  const long N = (long)B * V, nblk = (N + SS_NV_FWD - 1) / SS_NV_FWD;
  hipStream_t st = (hipStream_t)stream;
  int rc = adell_launch<adell_nnq_fwd_kernel>(dim3((unsigned)nblk), dim3(SS_NV_FWD),
                                              ss_nnq_lds(SS_NV_FWD, C, 1), st, x, y, pastn, past_class, N, V,
                                              C, K, Q, ss_row_stride(C), 1.f / temperature, S, O, workspace);
  if (rc != ADELL_OK) return rc;
  return adell_launch<adell_nnq_fold_kernel>(dim3(1), dim3(SS_NT), 0, st, (const double*)workspace, nblk,
                                             stats, loss);
}

extern "C" int adell_nn_queue_loss_bwd(const float* x, const float* y, const float* pastn,
                                       const int* past_class, const float* S, const float* O,
                                       const double* stats, const float* g, int B, long V, int C, int K,
                                       int Q, float temperature, float* dx, void* stream) {
  ADELL_REQUIRE(x && y && pastn && past_class && S && O && stats && g && dx,
                "nn_queue_loss_bwd: null pointer");
  if (ss_nnq_check("nn_queue_loss_bwd", B, V, C, K, Q, temperature) != ADELL_OK) return ADELL_E_BADARG;
  ADELL_REQUIRE((((uintptr_t)x | (uintptr_t)pastn | (uintptr_t)dx) & 15) == 0,
                "nn_queue_loss_bwd: unaligned rows");
  const long N = (long)B * V, nblk = (N + SS_NV_BWD - 1) / SS_NV_BWD;
  return adell_launch<adell_nnq_bwd_kernel>(dim3((unsigned)nblk), dim3(SS_NV_BWD),
                                            ss_nnq_lds(SS_NV_BWD, C, 2), (hipStream_t)stream, x, y, pastn,
                                            past_class, S, O, stats, g, N, V, C, K, Q, ss_row_stride(C),
                                            1.f / temperature, dx);
}

// ---- queue gather -------------------------------------------------------------------------------------
// grid (chunks, B K): cc[(b K + k) chunks + chunk] = #{v in the chunk: y[b][k][v] > 0}
__global__ __launch_bounds__(SS_NT) void adell_nnq_count_kernel(const float* __restrict__ y, long V,
                                                                int* __restrict__ cc) {
  __shared__ int sh[SS_NW];
  const size_t bk = blockIdx.y;
  const long v0 = (long)blockIdx.x * SS_CH, v1 = min(v0 + (long)SS_CH, V);
  int c = 0;
  for (long v = v0 + threadIdx.x; v < v1; v += SS_NT) c += y[bk * V + v] > 0.f ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int k = 0; k < SS_NW; ++k) t += sh[k];
    cc[bk * gridDim.x + blockIdx.x] = t;
  }
}

// A wave per selected row r: class sel_class[r], rank sel_rank[r] among the positives of that class.
// incl [K][B chunks]: the inclusive scan of the counts of a class over (item, chunk). x is read through
// the element strides (sb, sc, sv) of its [B][C][V] view. A rank beyond the positives writes zeros.
__global__ __launch_bounds__(64) void adell_nnq_gather_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const long long* __restrict__ incl,
    const int* __restrict__ sel_class, const long long* __restrict__ sel_rank, int B, int K, long V, int C,
    int chunks, long sb, long sc, long sv, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const size_t r = blockIdx.x;
  const int cl = sel_class[r];
  const long long j = sel_rank[r];
  const long T = (long)B * chunks;
  bool found = cl >= 0 && cl < K && j >= 0;
  long lo = 0;
  const long long* row = incl + (size_t)(found ? cl : 0) * T;
  if (found) {
    long hi = T;  // the first t with row[t] > j
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (row[mid] > j) hi = mid; else lo = mid + 1;
    }
    found = lo < T;
  }
  long b = 0, vsel = 0;
  if (found) {
    b = lo / chunks;
    const long v0 = (lo - b * chunks) * (long)SS_CH, v1 = min(v0 + (long)SS_CH, V);
    long long local = j - (lo > 0 ? row[lo - 1] : 0);
    found = false;
    for (long base = v0; base < v1; base += 64) {  // uniform trip count: the ballots stay complete
      const long v = base + lane;
      const bool flag = v < v1 && y[((size_t)b * K + cl) * V + v] > 0.f;
      const unsigned long long mask = __ballot(flag);
      const int cnt = __popcll(mask);
      if (local < cnt) {
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        const unsigned long long hit = __ballot(flag && before == (int)local);
        vsel = base + (__ffsll((long long)hit) - 1);
        found = hit != 0ull;
        break;
      }
      local -= cnt;
    }
  }
  for (int c = lane; c < C; c += 64)
    out[r * C + c] = found ? x[(size_t)b * sb + (size_t)c * sc + (size_t)vsel * sv] : 0.f;
}

extern "C" int adell_nn_queue_count(const float* y, int B, int K, long V, int* cc, void* stream) {
  ADELL_REQUIRE(y && cc && B >= 1 && K >= 1 && V >= 1 && (long)B * K <= 65535,
                "nn_queue_count: bad arguments (B %d, K %d, V %ld)", B, K, V);
  const long chunks = (V + SS_CH - 1) / SS_CH;
  return adell_launch<adell_nnq_count_kernel>(dim3((unsigned)chunks, (unsigned)(B * K)), dim3(SS_NT), 0,
                                              (hipStream_t)stream, y, V, cc);
}

extern "C" int adell_nn_queue_gather(const float* x, const float* y, const long long* incl,
                                     const int* sel_class, const long long* sel_rank, int n_sel, int B,
                                     int K, long V, int C, long sb, long sc, long sv, float* out,
                                     void* stream) {
  ADELL_REQUIRE(x && y && incl && sel_class && sel_rank && out && n_sel >= 1 && B >= 1 && K >= 1 &&
                    V >= 1 && C >= 1,
                "nn_queue_gather: bad arguments (n %d, B %d, K %d, V %ld, C %d)", n_sel, B, K, V, C);
  const bool rows = sb == V * C && sc == 1 && sv == C, planes = sb == (long)C * V && sc == V && sv == 1;
  ADELL_REQUIRE(rows || planes, "nn_queue_gather: x must be dense, channel-major or channels-last");
  const int chunks = (int)((V + SS_CH - 1) / SS_CH);
  return adell_launch<adell_nnq_gather_kernel>(dim3((unsigned)n_sel), dim3(64), 0, (hipStream_t)stream, x, y,
                                               incl, sel_class, sel_rank, B, K, V, C, chunks, sb, sc, sv,
                                               out);
}

// ---- pseudo-label cross entropy -----------------------------------------------------------------------
__device__ __forceinline__ float ss_pl_target(float proba, float thr, float keep, float floor_) {
  return (proba > thr ? keep : 0.f) + floor_;
}

// pred, proba [B][K][V]; part [gridDim.x]: the block's sum of the per-voxel losses. The block that
// finishes last (an integer ticket in *counter, zero on entry and left zero) adds the partials in
// index order: loss = scale * their sum.
__global__ __launch_bounds__(SS_NT) void adell_pl_ce_fwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ proba, const float* __restrict__ weight,
    long N, long V, int K, float thr, float ls, double scale, double* part, int* counter,
    float* __restrict__ out) {
  __shared__ double sh[SS_NW];
  __shared__ int last;
  const float keep = 1.f - ls, floor_ = ls / (float)K;
  double total = 0.0;
  for (long n = (long)blockIdx.x * SS_NT + threadIdx.x; n < N; n += (long)gridDim.x * SS_NT) {
    const long b = n / V, v = n - b * V;
    const float* z = pred + (size_t)b * K * V + v;
    const float* pr = proba + (size_t)b * K * V + v;
    float mx = -INFINITY, s = 0.f;
    for (int k = 0; k < K; ++k) ss_online(z[(size_t)k * V], mx, s);
    const float lse = mx + logf(s);
    float loss = 0.f;
    for (int k = 0; k < K; ++k) {
      const float t = ss_pl_target(pr[(size_t)k * V], thr, keep, floor_) * (weight ? weight[k] : 1.f);
      loss -= t * (z[(size_t)k * V] - lse);
    }
    total += (double)loss;
  }
  total = ss_block_sum_d<SS_NT>(total, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = total;
    __threadfence();
    last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  const volatile double* vp = part;
  double s = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += SS_NT) s += vp[i];
  s = ss_block_sum_d<SS_NT>(s, sh);
  if (threadIdx.x == 0) {
    out[0] = (float)(s * scale);
    *counter = 0;
  }
}

__global__ __launch_bounds__(SS_NT) void adell_pl_ce_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ proba, const float* __restrict__ weight,
    const float* __restrict__ g, long N, long V, int K, float thr, float ls, float scale,
    float* __restrict__ dpred) {
  const float keep = 1.f - ls, floor_ = ls / (float)K;
  const float gs = g[0] * scale;
  for (long n = (long)blockIdx.x * SS_NT + threadIdx.x; n < N; n += (long)gridDim.x * SS_NT) {
    const long b = n / V, v = n - b * V;
    const float* z = pred + (size_t)b * K * V + v;
    const float* pr = proba + (size_t)b * K * V + v;
    float* dz = dpred + (size_t)b * K * V + v;
    float mx = -INFINITY, s = 0.f, wsum = 0.f;
    for (int k = 0; k < K; ++k) {
      ss_online(z[(size_t)k * V], mx, s);
      wsum += ss_pl_target(pr[(size_t)k * V], thr, keep, floor_) * (weight ? weight[k] : 1.f);
    }
    const float inv = 1.f / s;
    for (int k = 0; k < K; ++k) {
      const float t = ss_pl_target(pr[(size_t)k * V], thr, keep, floor_) * (weight ? weight[k] : 1.f);
      dz[(size_t)k * V] = gs * (expf(z[(size_t)k * V] - mx) * inv * wsum - t);
    }
  }
}

static int ss_pl_blocks(long N) {
  long b = (N + SS_NT - 1) / SS_NT;
  if (b > 4096) b = 4096;
  return (int)b;
}
static int ss_pl_check(const char* what, int B, int K, long V, float ls) {
  ADELL_REQUIRE(B >= 1 && V >= 1 && K >= 1 && K <= ADELL_SEMISL_MAX_CLASSES,
                "%s: bad shape (B %d, K %d, V %ld; K <= %d)", what, B, K, V, ADELL_SEMISL_MAX_CLASSES);
  ADELL_REQUIRE(ls >= 0.f && ls <= 1.f, "%s: label_smoothing %g outside [0, 1]", what, (double)ls);
  return ADELL_OK;
}

extern "C" long adell_pseudo_label_ce_workspace_doubles(int B, long V) {
  ADELL_REQUIRE(B >= 1 && V >= 1, "pseudo_label_ce_workspace: bad shape (B %d, V %ld)", B, V);
  return 1 + ss_pl_blocks((long)B * V);  // the ticket's word, then a partial per block
}

extern "C" int adell_pseudo_label_ce_fwd(const float* pred, const float* proba, const float* weight, int B,
                                         int K, long V, float threshold, float label_smoothing, int mean,
                                         float* loss, double* workspace, long workspace_doubles,
                                         void* stream) {
  // workspace[0] holds the ticket: zero on entry (the caller clears it once), left zero
  ADELL_REQUIRE(pred && proba && loss && workspace, "pseudo_label_ce_fwd: null pointer");
  if (ss_pl_check("pseudo_label_ce_fwd", B, K, V, label_smoothing) != ADELL_OK) return ADELL_E_BADARG;
  ADELL_REQUIRE(workspace_doubles >= adell_pseudo_label_ce_workspace_doubles(B, V),
                "pseudo_label_ce_fwd: workspace too small");
  const long N = (long)B * V;
  const int blocks = ss_pl_blocks(N);
  return adell_launch<adell_pl_ce_fwd_kernel>(dim3(blocks), dim3(SS_NT), 0, (hipStream_t)stream, pred, proba,
                                              weight, N, V, K, threshold, label_smoothing,
                                              mean ? 1.0 / (double)N : 1.0, workspace + 1,
                                              reinterpret_cast<int*>(workspace), loss);
}

extern "C" int adell_pseudo_label_ce_bwd(const float* pred, const float* proba, const float* weight,
                                         const float* g, int B, int K, long V, float threshold,
                                         float label_smoothing, int mean, float* dpred, void* stream) {
  ADELL_REQUIRE(pred && proba && g && dpred, "pseudo_label_ce_bwd: null pointer");
  if (ss_pl_check("pseudo_label_ce_bwd", B, K, V, label_smoothing) != ADELL_OK) return ADELL_E_BADARG;
  const long N = (long)B * V;
  return adell_launch<adell_pl_ce_bwd_kernel>(dim3(ss_pl_blocks(N)), dim3(SS_NT), 0, (hipStream_t)stream,
                                              pred, proba, weight, g, N, V, K, threshold, label_smoothing,
                                              mean ? (float)(1.0 / (double)N) : 1.f, dpred);
}
