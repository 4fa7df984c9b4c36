// Kernels of DINO pretraining (adell_mri/modules/self_supervised/dino.py, losses/dino.py): fp32 in
// and out, wave64 reductions in a fixed order, no float atomics -- two runs are bit-identical.
//   * loss: -sum_k p_t[r,k] log_softmax(a / t1)[r,k] with p_t = softmax((b - centers) / t2), or p_t = b
//     as given (Sinkhorn-Knopp scores). One pass over a and b: per row the online accumulators
//     (m_s, Z_s) of the student and (m_t, Z_t, W = sum e_t a) of the teacher, so that
//     loss_r = lse_s - W / (Z_t t1) (scores: lse_s sum_b - sum(b a) / t1). The default shape has fewer
//     rows (2B, a few dozen) than the chip has CUs and 65536 columns: a row is split into the chunks of
//     adell_dino_loss_plan, every (row, chunk) block writes its five partials, a one-wave-per-row
//     launch merges them with the max-rescale (one block merges all rows and takes
//     their mean while there are at most 16) and leaves (lse_s, lse_t | sum_b, loss_r) for the
//     backward, which recomputes both probabilities from them: no [R][K] tensor is saved.
//   * rows of K floats start at any 4-byte address (K = 37): a chunk is a scalar head up to the first
//     16-byte boundary, float4 body, scalar tail; tensors that disagree about the boundary take the
//     scalar form throughout. The span, the accumulators and the (row, chunk) body live in
//     dino_rows.h: csrc/ibot.hip runs them over rows it reads through a table.
//   * column reductions over the R rows (centre sum, Sinkhorn prototype sums, gradient of the
//     per-column scale): one thread per column quad walks the rows in order.
//   * Sinkhorn-Knopp in factored form Q[k][r] = u_k E[k][r] v_r, E = exp(x / t2) recomputed per pass:
//     only u [K] and v [R] live between launches, the scores are written once.
//   * head: row L2 normalisation, g_k / ||v_k|| of a weight-normalised Linear (the normalised weight
//     is never formed) with its gradient to v, the per-column scale of the GEMM output, and the mean
//     over the feature axis of DINO.forward_encoder.
#include "dino_rows.h"

extern "C" int adell_dino_loss_plan(int R, int K, int* out) {
  ADELL_REQUIRE(out && R > 0 && K > 0, "dino_loss_plan: bad arguments");
  const int target = R >= DN_BLOCKS ? 1 : DN_BLOCKS / R;
  long len = ((long)K + target - 1) / target;
  len = (len + DN_CHUNK_Q - 1) / DN_CHUNK_Q * DN_CHUNK_Q;
  const int chunks = (int)(((long)K + len - 1) / len);
  out[0] = chunks;
  out[1] = (int)len;
  return ADELL_OK;
}

// grid (chunks, R): part[(r chunks + chunk) 5 + (m_s, Z_s, m_t, Z_t, W)]
template <bool SCORES>
__global__ __launch_bounds__(DN_NT) void adell_dino_loss_part_kernel(
    const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int K,
    int len, float it1, float it2, float* __restrict__ part) {
  const int r = blockIdx.y, chunk = blockIdx.x;
  const int k0 = chunk * len;
  const int n = (K - k0) < len ? (K - k0) : len;
  const float* ap = a + (size_t)r * K + k0;
  const float* bp = b + (size_t)r * K + k0;
  const float* cp = (SCORES || c == nullptr) ? nullptr : c + k0;
  dn_loss_part_body<SCORES>(ap, bp, cp, n, it1, it2, part + ((size_t)r * gridDim.x + chunk) * 5);
}

// Up to this many rows (one round of the four waves of a block ... four rounds) ONE block merges
// them all and takes the mean; beyond it the rows of a wave would queue behind each other's load
// and fp64 log latency, so the merge spreads over blocks and the mean is a launch of its own.
constexpr int DN_MERGE_ROWS = 16;

// mean[0] = sum_r loss[r] / R in a fixed order (fp64); all DN_NT threads of ONE block
__device__ __forceinline__ void dn_mean_rows(const float* loss, int R, float* __restrict__ mean) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int r = tid; r < R; r += DN_NT) acc += (double)loss[r];
  acc = adell_wave_sum_d(acc);
  __shared__ double wave_part[DN_NT / 64];
  if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = wave_part[0];
#pragma unroll
    for (int w = 1; w < DN_NT / 64; ++w) t += wave_part[w];
    mean[0] = (float)(t / (double)R);
  }
}

// One wave per row, four rows per block and round: stats[r] = (lse_s, lse_t | sum_b, loss_r,
// sum_k p_t a | 0). A grid of one block (R <= DN_MERGE_ROWS) also leaves the mean of the rows.
__global__ __launch_bounds__(DN_NT) void adell_dino_loss_merge_kernel(
    const float* __restrict__ part, int R, int chunks, int scores, float t1,
    float* __restrict__ loss_rows, float* __restrict__ stats, float* __restrict__ mean) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float row_loss[DN_MERGE_ROWS];
  for (int r = blockIdx.x * (DN_NT / 64) + wave; r < R; r += gridDim.x * (DN_NT / 64)) {
    DnAcc acc = {DN_NEG, 0.f, DN_NEG, 0.f, 0.f};
    for (int ch = lane; ch < chunks; ch += 64) {
      const float* p = part + ((size_t)r * chunks + ch) * 5;
      const DnAcc o = {p[0], p[1], p[2], p[3], p[4]};
      dn_acc_comb(acc, o);
    }
    acc = dn_acc_wave(acc);
    if (lane == 0) {
      const double lse_s = (double)acc.ms + log((double)acc.zs);
      double second, loss;
      if (scores) {
        second = (double)acc.zt;
        loss = lse_s * second - (double)acc.w / (double)t1;
      } else {
        second = (double)acc.mt + log((double)acc.zt);
        loss = lse_s - (double)acc.w / ((double)acc.zt * (double)t1);
      }
      stats[r * 4 + 0] = (float)lse_s;
      stats[r * 4 + 1] = (float)second;
      stats[r * 4 + 2] = (float)loss;
      // sum_k p_t a: the backward's db needs log_softmax_s - sum_k p_t log_softmax_s = (a - this) / t1,
      // in which lse_s (and its rounding) cancels
      stats[r * 4 + 3] = scores ? 0.f : (float)((double)acc.w / (double)acc.zt);
      loss_rows[r] = (float)loss;
      if (gridDim.x == 1 && r < DN_MERGE_ROWS) row_loss[r] = (float)loss;
    }
  }
  if (mean != nullptr && gridDim.x == 1) {   // (uniform over the block)
    __syncthreads();
    dn_mean_rows(row_loss, R, mean);
  }
}

__global__ __launch_bounds__(DN_NT) void adell_dino_loss_mean_kernel(const float* __restrict__ loss_rows,
                                                                     int R, float* __restrict__ mean) {
  dn_mean_rows(loss_rows, R, mean);
}

// grid (chunks, R); da / db may be null (db: centre mode only)
template <bool SCORES>
__global__ __launch_bounds__(DN_NT) void adell_dino_loss_bwd_kernel(
    const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
    const float* __restrict__ stats, const float* __restrict__ g_rows, const float* __restrict__ g_all,
    float g_scale, int K, int len, float it1, float it2, float* __restrict__ da,
    float* __restrict__ db) {
  const int r = blockIdx.y, tid = threadIdx.x;
  const int k0 = blockIdx.x * len;
  const int n = (K - k0) < len ? (K - k0) : len;
  const size_t off = (size_t)r * K + k0;
  const float* ap = a + off;
  const float* bp = b + off;
  const float* cp = (SCORES || c == nullptr) ? nullptr : c + k0;
  float* dap = da ? da + off : nullptr;
  float* dbp = db ? db + off : nullptr;
  const bool same = dn_same16(ap, bp) && (!dap || dn_same16(ap, dap)) && (!dbp || dn_same16(ap, dbp));
  const DnSpan sp = dn_span(ap, n, same);
  const bool cvec = cp != nullptr && dn_same16(ap, cp);
  const float lse_s = stats[r * 4 + 0], second = stats[r * 4 + 1], abar = stats[r * 4 + 3];
  const float g = g_rows ? g_rows[r] : g_all[0] * g_scale;
  const int tail = sp.head + 4 * sp.nvec;
  for (int k = tid; k < sp.head + (sp.n - tail); k += DN_NT) {   // scalar head, then scalar tail
    const int e = k < sp.head ? k : k - sp.head + tail;
    float x, y;
    dn_bwd_one<SCORES>(ap[e], bp[e], cp ? cp[e] : 0.f, it1, it2, lse_s, second, abar, g, x, y);
    if (dap) dap[e] = x;
    if (dbp) dbp[e] = y;
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < sp.nvec; i += DN_NT) {
    const int k = sp.head + 4 * i;
    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + k);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + k);
    const f32x4 cv = cp ? dn_ld4(cp + k, cvec) : zero;
    f32x4 x, y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xa, ya;
      dn_bwd_one<SCORES>(av[j], bv[j], cv[j], it1, it2, lse_s, second, abar, g, xa, ya);
      x[j] = xa;
      y[j] = ya;
    }
    if (dap) *reinterpret_cast<f32x4*>(dap + k) = x;
    if (dbp) *reinterpret_cast<f32x4*>(dbp + k) = y;
  }
}

// out[r][k] = x[r][k] it - lse[r] (mode 0: log-softmax) or exp((x[r][k] - c[k]) it - lse[r]) (mode 1);
// lse[r] = stats[r 4 + slot]. Not on the hot path: scalar, grid-strided.
__global__ __launch_bounds__(DN_NT) void adell_dino_scores_kernel(
    const float* __restrict__ x, const float* __restrict__ c, const float* __restrict__ stats,
    int slot, int mode, long total, int K, float it, float* __restrict__ out) {
  const long stride = (long)gridDim.x * DN_NT;
  for (long i = (long)blockIdx.x * DN_NT + threadIdx.x; i < total; i += stride) {
    const long r = i / K;
    const int k = (int)(i - r * K);
    const float lse = stats[r * 4 + slot];
    out[i] = mode == 0 ? x[i] * it - lse : expf((x[i] - (c ? c[k] : 0.f)) * it - lse);
  }
}

static int dn_loss_args(const char* what, const float* a, const float* b, int R, int K, float t1,
                        float t2) {
  ADELL_REQUIRE(a && b && R > 0 && K > 0 && R <= 65535, "%s: bad arguments (1 <= rows <= 65535)", what);
  ADELL_REQUIRE(t1 > 0.f && t2 > 0.f, "%s: temperatures must be positive", what);
  return ADELL_OK;
}

extern "C" long adell_dino_loss_workspace_floats(int R, int K) {
  int plan[2];
  if (adell_dino_loss_plan(R, K, plan) != ADELL_OK) return 0;
  return (long)R * plan[0] * 5;
}

extern "C" int adell_dino_loss_fwd(const float* a, const float* b, const float* centers, int R, int K,
                                   float t1, float t2, int teacher_is_scores, float* workspace,
                                   long workspace_floats, float* loss_rows, float* stats,
                                   float* loss_mean, void* stream) {
  const int rc = dn_loss_args("dino_loss_fwd", a, b, R, K, t1, t2);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(workspace && loss_rows && stats, "dino_loss_fwd: null output");
  int plan[2];
  adell_dino_loss_plan(R, K, plan);
  ADELL_REQUIRE(workspace_floats >= (long)R * plan[0] * 5,
                "dino_loss_fwd: workspace of %ld floats, the plan needs %ld", workspace_floats,
                (long)R * plan[0] * 5);
  const dim3 grid((unsigned)plan[0], (unsigned)R);
  const float it1 = (float)(1.0 / (double)t1), it2 = (float)(1.0 / (double)t2);
  hipStream_t st = (hipStream_t)stream;
  if (teacher_is_scores)
    hipLaunchKernelGGL(adell_dino_loss_part_kernel<true>, grid, dim3(DN_NT), 0, st, a, b,
                       (const float*)nullptr, K, plan[1], it1, it2, workspace);
  else
    hipLaunchKernelGGL(adell_dino_loss_part_kernel<false>, grid, dim3(DN_NT), 0, st, a, b, centers, K,
                       plan[1], it1, it2, workspace);
  ADELL_CHECK_HIP(hipGetLastError());
  return dn_launch_merge(workspace, R, plan[0], teacher_is_scores, t1, loss_rows, stats, loss_mean, st);
}

int dn_launch_merge(const float* part, int R, int chunks, int teacher_is_scores, float t1,
                    float* loss_rows, float* stats, float* loss_mean, hipStream_t st) {
  const int merge_blocks = R <= DN_MERGE_ROWS ? 1 : adell_cdiv(R, DN_NT / 64);
  hipLaunchKernelGGL(adell_dino_loss_merge_kernel, dim3((unsigned)merge_blocks), dim3(DN_NT), 0, st,
                     part, R, chunks, teacher_is_scores ? 1 : 0, t1, loss_rows, stats, loss_mean);
  ADELL_CHECK_HIP(hipGetLastError());
  if (loss_mean != nullptr && merge_blocks > 1) {
    hipLaunchKernelGGL(adell_dino_loss_mean_kernel, dim3(1), dim3(DN_NT), 0, st,
                       (const float*)loss_rows, R, loss_mean);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  return ADELL_OK;
}

extern "C" int adell_dino_loss_bwd(const float* a, const float* b, const float* centers,
                                   const float* stats, const float* g_rows, const float* g_all,
                                   float g_scale, int R, int K, float t1, float t2,
                                   int teacher_is_scores, float* da, float* db, void* stream) {
  const int rc = dn_loss_args("dino_loss_bwd", a, b, R, K, t1, t2);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(stats && (g_rows || g_all), "dino_loss_bwd: null statistics / gradient");
  ADELL_REQUIRE(!(teacher_is_scores && db), "dino_loss_bwd: given scores take no gradient");
  if (!da && !db) return ADELL_OK;
  int plan[2];
  adell_dino_loss_plan(R, K, plan);
  const dim3 grid((unsigned)plan[0], (unsigned)R);
  const float it1 = (float)(1.0 / (double)t1), it2 = (float)(1.0 / (double)t2);
  hipStream_t st = (hipStream_t)stream;
  if (teacher_is_scores)
    hipLaunchKernelGGL(adell_dino_loss_bwd_kernel<true>, grid, dim3(DN_NT), 0, st, a, b,
                       (const float*)nullptr, stats, g_rows, g_all, g_scale, K, plan[1], it1, it2, da, db);
  else
    hipLaunchKernelGGL(adell_dino_loss_bwd_kernel<false>, grid, dim3(DN_NT), 0, st, a, b, centers,
                       stats, g_rows, g_all, g_scale, K, plan[1], it1, it2, da, db);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_dino_scores(const float* x, const float* centers, const float* stats, int slot,
                                 int mode, int R, int K, float t, float* out, void* stream) {
  ADELL_REQUIRE(x && stats && out && R > 0 && K > 0 && t > 0.f && slot >= 0 && slot < 4 &&
                    (mode == 0 || mode == 1),
                "dino_scores: bad arguments");
  const long total = (long)R * K;
  long blocks = (total + DN_NT * 4 - 1) / (DN_NT * 4);
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(adell_dino_scores_kernel, dim3((unsigned)blocks), dim3(DN_NT), 0,
                     (hipStream_t)stream, x, centers, stats, slot, mode, total, K,
                     (float)(1.0 / (double)t), out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---- column reductions over the rows ---------------------------------------------------------------
// MODE 0: out[k] = sum_r x[r][k]; 1: sum_r exp(x[r][k] it) v[r]; 2: sum_r x[r][k] y[r][k].
// VEC: one thread owns four columns (K % 4 == 0, 16-byte aligned tensors), else one.
template <int MODE, bool VEC>
__global__ __launch_bounds__(64) void adell_dino_colreduce_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ v, int R, int K,
    float it, float* __restrict__ out) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (VEC) {
    const int KQ = K >> 2;
    if (q >= KQ) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x) + q;
    const f32x4* y4 = reinterpret_cast<const f32x4*>(y) + q;
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
      const f32x4 xv = x4[(size_t)r * KQ];
      if (MODE == 0) {
        acc += xv;
      } else if (MODE == 1) {
        const float w = v[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += expf(xv[j] * it) * w;
      } else {
        acc += xv * y4[(size_t)r * KQ];
      }
    }
    reinterpret_cast<f32x4*>(out)[q] = acc;
  } else {
    if (q >= K) return;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) {
      const float xv = x[(size_t)r * K + q];
      if (MODE == 0) acc += xv;
      else if (MODE == 1) acc += expf(xv * it) * v[r];
      else acc += xv * y[(size_t)r * K + q];
    }
    out[q] = acc;
  }
}

template <int MODE>
static int dn_colreduce(const float* x, const float* y, const float* v, int R, int K, float it,
                        float* out, hipStream_t st) {
  const bool vec = (K % 4 == 0) && adell_aligned16(x) && adell_aligned16(out) &&
                   (MODE != 2 || adell_aligned16(y));
  if (vec)
    hipLaunchKernelGGL((adell_dino_colreduce_kernel<MODE, true>), dim3((unsigned)adell_cdiv(K >> 2, 64)),
                       dim3(64), 0, st, x, y, v, R, K, it, out);
  else
    hipLaunchKernelGGL((adell_dino_colreduce_kernel<MODE, false>), dim3((unsigned)adell_cdiv(K, 64)),
                       dim3(64), 0, st, x, y, v, R, K, it, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_dino_center_sum(const float* x, int R, int K, float* out, void* stream) {
  ADELL_REQUIRE(x && out && R > 0 && K > 0, "dino_center_sum: bad arguments");
  return dn_colreduce<0>(x, nullptr, nullptr, R, K, 0.f, out, (hipStream_t)stream);
}

// centers <- centers m + (batch_sum / denom) rest, rest = 1 - m formed by the caller in double as the
// reference's Python forms it; each step rounded as the reference's fp32 rounds it
__global__ __launch_bounds__(DN_NT) void adell_dino_center_apply_kernel(
    float* __restrict__ centers, const float* __restrict__ batch_sum, int K, float m, float rest,
    float denom) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * DN_NT + threadIdx.x;
  if (k >= K) return;
  const float t = batch_sum[k] / denom;
  const float keep = centers[k] * m;
  const float add = t * rest;
  centers[k] = keep + add;
}

extern "C" int adell_dino_center_apply(float* centers, const float* batch_sum, int K, float m,
                                       float rest, float denom, void* stream) {
  ADELL_REQUIRE(centers && batch_sum && K > 0 && denom > 0.f, "dino_center_apply: bad arguments");
  hipLaunchKernelGGL(adell_dino_center_apply_kernel, dim3((unsigned)adell_cdiv(K, DN_NT)), dim3(DN_NT),
                     0, (hipStream_t)stream, centers, batch_sum, K, m, rest, denom);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---- Sinkhorn-Knopp ---------------------------------------------------------------------------------
// t[k] = sum_r exp(x[r][k] / t2) v[r]: the total weight of prototype k (the caller all-reduces it).
extern "C" int adell_dino_sk_proto_sums(const float* x, const float* v, int R, int K, float t2,
                                        float* t, void* stream) {
  ADELL_REQUIRE(x && v && t && R > 0 && K > 0 && t2 > 0.f, "dino_sk_proto_sums: bad arguments");
  return dn_colreduce<1>(x, nullptr, v, R, K, (float)(1.0 / (double)t2), t, (hipStream_t)stream);
}

// grid R: v[r] = 1 / (samples sum_k exp(x[r][k] / t2) / (K t[k]))
__global__ __launch_bounds__(DN_NT) void adell_dino_sk_sample_kernel(
    const float* __restrict__ x, const float* __restrict__ t, int K, float it, float samples,
    float* __restrict__ v) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* xp = x + (size_t)r * K;
  const DnSpan sp = dn_span(xp, K, dn_same16(xp, t));
  const float fk = (float)K;
  float acc = 0.f;
  for (int k = tid; k < sp.head; k += DN_NT) acc += expf(xp[k] * it) / (t[k] * fk);
  for (int i = tid; i < sp.nvec; i += DN_NT) {
    const int k = sp.head + 4 * i;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + k);
    const f32x4 tv = *reinterpret_cast<const f32x4*>(t + k);
    acc += (expf(xv[0] * it) / (tv[0] * fk) + expf(xv[1] * it) / (tv[1] * fk)) +
           (expf(xv[2] * it) / (tv[2] * fk) + expf(xv[3] * it) / (tv[3] * fk));
  }
  for (int k = sp.head + 4 * sp.nvec + tid; k < sp.n; k += DN_NT) acc += expf(xp[k] * it) / (t[k] * fk);
  acc = adell_wave_sum(acc);
  __shared__ float wave_part[DN_NT / 64];
  if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = wave_part[0];
#pragma unroll
    for (int w = 1; w < DN_NT / 64; ++w) s += wave_part[w];
    v[r] = 1.0f / (samples * s);
  }
}

extern "C" int adell_dino_sk_sample_weights(const float* x, const float* t, int R, int K, float t2,
                                            float samples, float* v, void* stream) {
  ADELL_REQUIRE(x && t && v && R > 0 && K > 0 && t2 > 0.f && samples > 0.f,
                "dino_sk_sample_weights: bad arguments");
  hipLaunchKernelGGL(adell_dino_sk_sample_kernel, dim3((unsigned)R), dim3(DN_NT), 0,
                     (hipStream_t)stream, x, t, K, (float)(1.0 / (double)t2), samples, v);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// out[r][k] = exp(x[r][k] / t2) / (K t[k]) v[r] samples
__global__ __launch_bounds__(DN_NT) void adell_dino_sk_final_kernel(
    const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ v, long total,
    int K, float it, float samples, float* __restrict__ out) {
  const long stride = (long)gridDim.x * DN_NT;
  const float fk = (float)K;
  for (long i = (long)blockIdx.x * DN_NT + threadIdx.x; i < total; i += stride) {
    const long r = i / K;
    const int k = (int)(i - r * K);
    out[i] = expf(x[i] * it) / (t[k] * fk) * v[r] * samples;
  }
}

extern "C" int adell_dino_sk_final(const float* x, const float* t, const float* v, int R, int K,
                                   float t2, float samples, float* out, void* stream) {
  ADELL_REQUIRE(x && t && v && out && R > 0 && K > 0 && t2 > 0.f, "dino_sk_final: bad arguments");
  const long total = (long)R * K;
  long blocks = (total + DN_NT * 4 - 1) / (DN_NT * 4);
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(adell_dino_sk_final_kernel, dim3((unsigned)blocks), dim3(DN_NT), 0,
                     (hipStream_t)stream, x, t, v, total, K, (float)(1.0 / (double)t2), samples, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---- head ---------------------------------------------------------------------------------------------
// One wave per row of C floats, four rows per block.
// MODE 0: y = x / max(||x||, eps), aux[row] = 1 / max(||x||, eps)   (F.normalize, p = 2)
// MODE 1: aux[row] = g[row] / ||x||                                  (weight norm, dim 0)
// MODE 2: aux[row] = mean(x)
template <int MODE>
__global__ __launch_bounds__(256) void adell_dino_rows_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ g, int rows, int C, float eps,
    float* __restrict__ y, float* __restrict__ aux) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xp = x + (size_t)row * C;
  float acc = 0.f;
  for (int k = lane; k < C; k += 64) acc += MODE == 2 ? xp[k] : xp[k] * xp[k];
  acc = adell_wave_sum(acc);
  if (MODE == 2) {
    if (lane == 0) aux[row] = acc / (float)C;
    return;
  }
  const float norm = sqrtf(acc);
  if (MODE == 1) {
    if (lane == 0) aux[row] = g[row] / norm;
    return;
  }
  const float inv = 1.0f / fmaxf(norm, eps);
  if (lane == 0) aux[row] = inv;
  float* yp = y + (size_t)row * C;
  for (int k = lane; k < C; k += 64) yp[k] = xp[k] * inv;
}

// MODE 0: dx = (dy - y (y . dy)) inv, or dy inv where the norm was clamped (inv == 1 / eps)
// MODE 1: dv[row] = -ds[row] g[row] / ||v||^3 v[row]         (x = v, dy = ds [rows], aux = g)
// MODE 2: dx[row][:] = dy[row] / C
template <int MODE>
__global__ __launch_bounds__(256) void adell_dino_rows_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ aux, int rows,
    int C, float eps, float* __restrict__ dx) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float* dxp = dx + (size_t)row * C;
  if (MODE == 2) {
    const float v = dy[row] / (float)C;
    for (int k = lane; k < C; k += 64) dxp[k] = v;
    return;
  }
  const float* xp = x + (size_t)row * C;   // MODE 0: y
  if (MODE == 1) {
    float acc = 0.f;
    for (int k = lane; k < C; k += 64) acc += xp[k] * xp[k];
    acc = adell_wave_sum(acc);
    const float coef = -dy[row] * aux[row] / (acc * sqrtf(acc));
    for (int k = lane; k < C; k += 64) dxp[k] = coef * xp[k];
    return;
  }
  const float* dyp = dy + (size_t)row * C;
  const float inv = aux[row];
  if (inv >= 1.0f / eps) {
    for (int k = lane; k < C; k += 64) dxp[k] = dyp[k] * inv;
    return;
  }
  float dot = 0.f;
  for (int k = lane; k < C; k += 64) dot += xp[k] * dyp[k];
  dot = adell_wave_sum(dot);
  for (int k = lane; k < C; k += 64) dxp[k] = (dyp[k] - xp[k] * dot) * inv;
}

#define DN_ROWS_GRID(rows) dim3((unsigned)adell_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream

extern "C" int adell_l2_normalize_rows_fwd(const float* x, int rows, int C, float eps, float* y,
                                           float* inv, void* stream) {
  ADELL_REQUIRE(x && y && inv && rows > 0 && C > 0 && eps > 0.f, "l2_normalize_rows_fwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_fwd_kernel<0>, DN_ROWS_GRID(rows), x, (const float*)nullptr, rows,
                     C, eps, y, inv);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_l2_normalize_rows_bwd(const float* y, const float* dy, const float* inv, int rows,
                                           int C, float eps, float* dx, void* stream) {
  ADELL_REQUIRE(y && dy && inv && dx && rows > 0 && C > 0 && eps > 0.f,
                "l2_normalize_rows_bwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_bwd_kernel<0>, DN_ROWS_GRID(rows), y, dy, inv, rows, C, eps, dx);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_row_inv_norm_fwd(const float* v, const float* g, int rows, int C, float* s,
                                      void* stream) {
  ADELL_REQUIRE(v && g && s && rows > 0 && C > 0, "row_inv_norm_fwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_fwd_kernel<1>, DN_ROWS_GRID(rows), v, g, rows, C, 0.f,
                     (float*)nullptr, s);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_row_inv_norm_bwd(const float* v, const float* g, const float* ds, int rows, int C,
                                      float* dv, void* stream) {
  ADELL_REQUIRE(v && g && ds && dv && rows > 0 && C > 0, "row_inv_norm_bwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_bwd_kernel<1>, DN_ROWS_GRID(rows), v, ds, g, rows, C, 0.f, dv);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_row_mean_fwd(const float* x, int rows, int C, float* out, void* stream) {
  ADELL_REQUIRE(x && out && rows > 0 && C > 0, "row_mean_fwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_fwd_kernel<2>, DN_ROWS_GRID(rows), x, (const float*)nullptr, rows,
                     C, 0.f, (float*)nullptr, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_row_mean_bwd(const float* dout, int rows, int C, float* dx, void* stream) {
  ADELL_REQUIRE(dout && dx && rows > 0 && C > 0, "row_mean_bwd: bad arguments");
  hipLaunchKernelGGL(adell_dino_rows_bwd_kernel<2>, DN_ROWS_GRID(rows), (const float*)nullptr, dout,
                     (const float*)nullptr, rows, C, 0.f, dx);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// y[r][k] = x[r][k] s[k]: the weight-normalised Linear's scale on the GEMM output, and dY -> d(GEMM
// output) in its backward
__global__ __launch_bounds__(DN_NT) void adell_dino_colscale_kernel(
    const float* __restrict__ x, const float* __restrict__ s, long total, int K, int vec,
    float* __restrict__ y) {
  const long stride = (long)gridDim.x * DN_NT;
  if (vec) {
    const long n4 = total >> 2;
    const int KQ = K >> 2;
    for (long i = (long)blockIdx.x * DN_NT + threadIdx.x; i < n4; i += stride)
      reinterpret_cast<f32x4*>(y)[i] =
          reinterpret_cast<const f32x4*>(x)[i] * reinterpret_cast<const f32x4*>(s)[i % KQ];
  } else {
    for (long i = (long)blockIdx.x * DN_NT + threadIdx.x; i < total; i += stride)
      y[i] = x[i] * s[i % K];
  }
}

extern "C" int adell_col_scale(const float* x, const float* s, int R, int K, float* y, void* stream) {
  ADELL_REQUIRE(x && s && y && R > 0 && K > 0, "col_scale: bad arguments");
  const long total = (long)R * K;
  const int vec = (K % 4 == 0) && adell_aligned16(x) && adell_aligned16(s) && adell_aligned16(y);
  long blocks = (total + DN_NT * 4 - 1) / (DN_NT * 4);
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(adell_dino_colscale_kernel, dim3((unsigned)blocks), dim3(DN_NT), 0,
                     (hipStream_t)stream, x, s, total, K, vec, y);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ds[k] = sum_r dy[r][k] y0[r][k]
extern "C" int adell_col_scale_dscale(const float* dy, const float* y0, int R, int K, float* ds,
                                      void* stream) {
  ADELL_REQUIRE(dy && y0 && ds && R > 0 && K > 0, "col_scale_dscale: bad arguments");
  return dn_colreduce<2>(dy, y0, nullptr, R, K, 0.f, ds, (hipStream_t)stream);
}
