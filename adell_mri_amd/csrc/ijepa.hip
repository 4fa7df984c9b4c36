// Kernels of I-JEPA pretraining (adell_mri/modules/self_supervised/jepa.py, IJEPAPL in pl.py): the
// token plumbing the reference does with fancy indexing, cat, expand and a full-size layer norm, and
// its loss. House rules of ibot.hip: fp32 in and out, no float atomics, every sum in a fixed order --
// two runs are bit-identical. One wave owns one row of E floats (four rows per block of 256
// threads); a row wider than one pass (256 floats as float4, 64 as scalars) is walked with a strided
// loop. float4 or scalar is decided per LAUNCH (E % 4 == 0 and every base 16-byte aligned, so every
// row is). Index tables are int32, sorted, unique and range-checked by the caller on the host
// (ops.TokenRows: rows[j] -> token, inv[token] -> j or -1); the kernels read them unchecked.
//   * token-row gather: y[b][j] = x[b][rows[j]]. The backward is the same kernel through the inverse
//     table: every row of dx [B][N][E] is written once, a gradient row or zeros -- no memset, no
//     scatter.
//   * predictor input: out[b][j] = e[b][j] + pos[ctx[j]] (j < nc), out[b][nc + j] = mask +
//     pos[tgt[j]], one launch. Backward, one launch: de = dout[:, :nc] and the WHOLE dpos [T][P], row
//     t the sum over b (in order) of the one dout row that maps to it, or zeros. dmask is the sum of
//     the target rows of dpos in the order of the target table (accumulated in fp64): a second launch
//     over nt rows of P floats.
//   * block loss: SmoothL1Loss()(pred, layer_norm(h)[:, rows]) (beta 1, mean; no affine, eps 1e-5,
//     biased variance) without writing the normalised h or the gathered target. Per row: mean, then
//     the variance about it (two passes over a row that is hot in the vector L1), the row's partial
//     loss; a one-wave second stage adds the B nt partials in a fixed order in fp64. The forward
//     SAVES two floats per row (mean, rstd); the backward, dpred = g clamp(pred - target, -1, 1) /
//     (B nt E), reads them instead of reducing the row again. h takes no gradient.
#include "common.h"

constexpr int IJ_NT = 256;            // threads per block
constexpr int IJ_ROWS = IJ_NT / 64;   // rows (waves) per block
constexpr float IJ_LN_EPS = 1e-5f;

__device__ __forceinline__ f32x4 ij_ld4(const float* p, int i) {
  return reinterpret_cast<const f32x4*>(p)[i];
}
__device__ __forceinline__ void ij_st4(float* p, int i, f32x4 v) {
  reinterpret_cast<f32x4*>(p)[i] = v;
}

static inline dim3 ij_grid(long rows) { return dim3((unsigned)((rows + IJ_ROWS - 1) / IJ_ROWS)); }

// ---- token-row gather ------------------------------------------------------------------------------
// Row (b, o) of out [B][No][E] = row (b, tab[o]) of in [B][Ni][E], zeros where tab[o] < 0.
template <bool VEC>
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_rows_kernel(
    const float* __restrict__ in, const int* __restrict__ tab, long rows, int No, int Ni, int E,
    float* __restrict__ out) {
  const long row = (long)blockIdx.x * IJ_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / No;
  const int src = tab[(int)(row - b * No)];
  const float* ip = in + ((size_t)b * Ni + (src < 0 ? 0 : src)) * E;
  float* op = out + (size_t)row * E;
  if (VEC) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < (E >> 2); i += 64) ij_st4(op, i, src < 0 ? zero : ij_ld4(ip, i));
  } else {
    for (int e = lane; e < E; e += 64) op[e] = src < 0 ? 0.f : ip[e];
  }
}

static int ij_rows_launch(const char* what, const float* in, const int* tab, int B, int No, int Ni,
                          int E, float* out, hipStream_t st) {
  ADELL_REQUIRE(in && tab && out && B > 0 && No > 0 && Ni > 0 && E > 0, "%s: bad arguments", what);
  ADELL_REQUIRE((long)B * No <= 0x7fffffffL && (long)B * Ni <= 0x7fffffffL, "%s: too many rows",
                what);
  const long rows = (long)B * No;
  if ((E % 4 == 0) && adell_aligned16(in) && adell_aligned16(out))
    return adell_launch<adell_ijepa_rows_kernel<true>>(ij_grid(rows), dim3(IJ_NT), 0, st, in, tab, rows,
                                                       No, Ni, E, out);
  return adell_launch<adell_ijepa_rows_kernel<false>>(ij_grid(rows), dim3(IJ_NT), 0, st, in, tab, rows,
                                                      No, Ni, E, out);
}

extern "C" int adell_ijepa_gather_fwd(const float* x, const int* rows, int B, int N, int E, int M,
                                      float* y, void* stream) {
  ADELL_REQUIRE(M <= N, "ijepa_gather_fwd: %d rows of %d", M, N);
  return ij_rows_launch("ijepa_gather_fwd", x, rows, B, M, N, E, y, (hipStream_t)stream);
}

extern "C" int adell_ijepa_gather_bwd(const float* dy, const int* inv, int B, int N, int E, int M,
                                      float* dx, void* stream) {
  ADELL_REQUIRE(M <= N, "ijepa_gather_bwd: %d rows of %d", M, N);
  return ij_rows_launch("ijepa_gather_bwd", dy, inv, B, N, M, E, dx, (hipStream_t)stream);
}

// ---- predictor input -------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_predictor_fwd_kernel(
    const float* __restrict__ e, const float* __restrict__ pos, const float* __restrict__ mask,
    const int* __restrict__ ctx, const int* __restrict__ tgt, long rows, int nc, int nt, int P,
    float* __restrict__ out) {
  const long row = (long)blockIdx.x * IJ_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / (nc + nt);
  const int j = (int)(row - b * (nc + nt));
  const bool context = j < nc;
  const float* ap = context ? e + ((size_t)b * nc + j) * P : mask;
  const float* pp = pos + (size_t)(context ? ctx[j] : tgt[j - nc]) * P;
  float* op = out + (size_t)row * P;
  if (VEC) {
    for (int i = lane; i < (P >> 2); i += 64) ij_st4(op, i, ij_ld4(ap, i) + ij_ld4(pp, i));
  } else {
    for (int k = lane; k < P; k += 64) op[k] = ap[k] + pp[k];
  }
}

extern "C" int adell_ijepa_predictor_fwd(const float* e, const float* pos, const float* mask,
                                         const int* ctx, const int* tgt, int B, int nc, int nt, int T,
                                         int P, float* out, void* stream) {
  ADELL_REQUIRE(e && pos && mask && ctx && tgt && out && B > 0 && nc > 0 && nt > 0 && P > 0 &&
                    (long)nc + nt <= T,
                "ijepa_predictor_fwd: bad arguments (nc, nt >= 1, nc + nt <= T)");
  ADELL_REQUIRE((long)B * ((long)nc + nt) <= 0x7fffffffL, "ijepa_predictor_fwd: too many rows");
  const long rows = (long)B * (nc + nt);
  hipStream_t st = (hipStream_t)stream;
  if ((P % 4 == 0) && adell_aligned16(e) && adell_aligned16(pos) && adell_aligned16(mask) &&
      adell_aligned16(out))
    return adell_launch<adell_ijepa_predictor_fwd_kernel<true>>(ij_grid(rows), dim3(IJ_NT), 0, st, e, pos,
                                                                mask, ctx, tgt, rows, nc, nt, P, out);
  return adell_launch<adell_ijepa_predictor_fwd_kernel<false>>(ij_grid(rows), dim3(IJ_NT), 0, st, e, pos,
                                                               mask, ctx, tgt, rows, nc, nt, P, out);
}

// Rows [0, copy): de row (b, j) = dout row (b, j), j < nc (copy = B nc, or 0 without de). Rows
// [copy, copy + T): dpos row t = sum_b dout[b][jj] for the jj that maps to t -- inv_ctx[t], else
// nc + inv_tgt[t] -- or zeros.
template <bool VEC>
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_predictor_bwd_kernel(
    const float* __restrict__ dout, const int* __restrict__ inv_ctx, const int* __restrict__ inv_tgt,
    long copy, int B, int nc, int nt, int T, int P, float* __restrict__ de,
    float* __restrict__ dpos) {
  const long row = (long)blockIdx.x * IJ_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const size_t item = (size_t)(nc + nt) * P;
  if (row < copy) {
    const long b = row / nc;
    const float* ip = dout + (size_t)b * item + (size_t)(row - b * nc) * P;
    float* op = de + (size_t)row * P;
    if (VEC) {
      for (int i = lane; i < (P >> 2); i += 64) ij_st4(op, i, ij_ld4(ip, i));
    } else {
      for (int k = lane; k < P; k += 64) op[k] = ip[k];
    }
    return;
  }
  const long t = row - copy;
  if (t >= T || dpos == nullptr) return;
  const int jc = inv_ctx[t], jt = inv_tgt[t];
  const int jj = jc >= 0 ? jc : (jt >= 0 ? nc + jt : -1);
  const float* ip = dout + (size_t)(jj < 0 ? 0 : jj) * P;
  float* op = dpos + (size_t)t * P;
  if (VEC) {
    for (int i = lane; i < (P >> 2); i += 64) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (jj >= 0)
        for (int b = 0; b < B; ++b) acc += ij_ld4(ip + (size_t)b * item, i);
      ij_st4(op, i, acc);
    }
  } else {
    for (int k = lane; k < P; k += 64) {
      float acc = 0.f;
      if (jj >= 0)
        for (int b = 0; b < B; ++b) acc += ip[(size_t)b * item + k];
      op[k] = acc;
    }
  }
}

// dmask[k] = sum_j dpos[tgt[j]][k], j in order, in fp64
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_predictor_dmask_kernel(
    const float* __restrict__ dpos, const int* __restrict__ tgt, int nt, int P,
    float* __restrict__ dmask) {
  const int k = blockIdx.x * IJ_NT + threadIdx.x;
  if (k >= P) return;
  double acc = 0.0;
  for (int j = 0; j < nt; ++j) acc += (double)dpos[(size_t)tgt[j] * P + k];
  dmask[k] = (float)acc;
}

extern "C" int adell_ijepa_predictor_bwd(const float* dout, const int* tgt, const int* inv_ctx,
                                         const int* inv_tgt, int B, int nc, int nt, int T, int P,
                                         float* de, float* dpos, float* dmask, void* stream) {
  ADELL_REQUIRE(dout && tgt && inv_ctx && inv_tgt && B > 0 && nc > 0 && nt > 0 && P > 0 &&
                    (long)nc + nt <= T,
                "ijepa_predictor_bwd: bad arguments (nc, nt >= 1, nc + nt <= T)");
  ADELL_REQUIRE((long)B * ((long)nc + nt) <= 0x7fffffffL, "ijepa_predictor_bwd: too many rows");
  ADELL_REQUIRE(dmask == nullptr || dpos != nullptr,
                "ijepa_predictor_bwd: dmask is summed from dpos, which is null");
  hipStream_t st = (hipStream_t)stream;
  const long copy = de ? (long)B * nc : 0;
  const long rows = copy + (dpos ? T : 0);
  if (rows > 0) {
    int rc;
    if ((P % 4 == 0) && adell_aligned16(dout) && adell_aligned16(de) && adell_aligned16(dpos))
      rc = adell_launch<adell_ijepa_predictor_bwd_kernel<true>>(ij_grid(rows), dim3(IJ_NT), 0, st, dout,
                                                                inv_ctx, inv_tgt, copy, B, nc, nt, T, P,
                                                                de, dpos);
    else
      rc = adell_launch<adell_ijepa_predictor_bwd_kernel<false>>(ij_grid(rows), dim3(IJ_NT), 0, st, dout,
                                                                 inv_ctx, inv_tgt, copy, B, nc, nt, T, P,
                                                                 de, dpos);
    if (rc != ADELL_OK) return rc;
  }
  if (dmask)
    return adell_launch<adell_ijepa_predictor_dmask_kernel>(dim3((unsigned)adell_cdiv(P, IJ_NT)),
                                                            dim3(IJ_NT), 0, st, (const float*)dpos, tgt,
                                                            nt, P, dmask);
  return ADELL_OK;
}

// ---- block loss ------------------------------------------------------------------------------------
__device__ __forceinline__ float ij_smooth_l1(float d) {
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

// One wave per row r = b nt + j: stats[r] = (mean, rstd) of h[b][rows[j]][:], part[r] = the sum
// over the row of smooth_l1(pred - (h - mean) rstd).
template <bool VEC>
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_loss_rows_kernel(
    const float* __restrict__ pred, const float* __restrict__ h, const int* __restrict__ rows, int R,
    int nt, int N, int E, float* __restrict__ stats, float* __restrict__ part) {
  const int r = blockIdx.x * IJ_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = r / nt;
  const float* hp = h + ((size_t)b * N + rows[r - b * nt]) * E;
  const float* pp = pred + (size_t)r * E;
  float s = 0.f;
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 v = ij_ld4(hp, i);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int e = lane; e < E; e += 64) s += hp[e];
  }
  const float mean = adell_wave_sum(s) / (float)E;
  float q = 0.f;
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 v = ij_ld4(hp, i) - mean;
      q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
  } else {
    for (int e = lane; e < E; e += 64) q += (hp[e] - mean) * (hp[e] - mean);
  }
  const float rstd = 1.0f / sqrtf(adell_wave_sum(q) / (float)E + IJ_LN_EPS);
  float l = 0.f;
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 d = ij_ld4(pp, i) - (ij_ld4(hp, i) - mean) * rstd;
      l += (ij_smooth_l1(d[0]) + ij_smooth_l1(d[1])) + (ij_smooth_l1(d[2]) + ij_smooth_l1(d[3]));
    }
  } else {
    for (int e = lane; e < E; e += 64) l += ij_smooth_l1(pp[e] - (hp[e] - mean) * rstd);
  }
  l = adell_wave_sum(l);
  if (lane == 0) {
    stats[2 * r] = mean;
    stats[2 * r + 1] = rstd;
    part[r] = l;
  }
}

// One wave: lane l adds the rows l, l + 64, ... in order, the 64 sums are folded in the fixed order
// of the butterfly; loss = sum / (R E).
__global__ __launch_bounds__(64) void adell_ijepa_loss_merge_kernel(const float* __restrict__ part,
                                                                    int R, double inv_count,
                                                                    float* __restrict__ loss) {
  double acc = 0.0;
  for (int r = threadIdx.x; r < R; r += 64) acc += (double)part[r];
  acc = adell_wave_sum_d(acc);
  if (threadIdx.x == 0) loss[0] = (float)(acc * inv_count);
}

static int ij_loss_args(const char* what, const float* pred, const float* h, const int* rows, int B,
                        int nt, int N, int E) {
  ADELL_REQUIRE(pred && h && rows && B > 0 && nt > 0 && N > 0 && E > 0 && nt <= N,
                "%s: bad arguments (1 <= nt <= N)", what);
  ADELL_REQUIRE((long)B * N <= 0x7fffffffL, "%s: too many rows", what);
  return ADELL_OK;
}

extern "C" int adell_ijepa_loss_fwd(const float* pred, const float* h, const int* rows, int B, int nt,
                                    int N, int E, float* stats, float* part, float* loss,
                                    void* stream) {
  const int rc = ij_loss_args("ijepa_loss_fwd", pred, h, rows, B, nt, N, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(stats && part && loss, "ijepa_loss_fwd: null output");
  const int R = B * nt;
  hipStream_t st = (hipStream_t)stream;
  int rc2;
  if ((E % 4 == 0) && adell_aligned16(pred) && adell_aligned16(h))
    rc2 = adell_launch<adell_ijepa_loss_rows_kernel<true>>(ij_grid(R), dim3(IJ_NT), 0, st, pred, h, rows,
                                                           R, nt, N, E, stats, part);
  else
    rc2 = adell_launch<adell_ijepa_loss_rows_kernel<false>>(ij_grid(R), dim3(IJ_NT), 0, st, pred, h, rows,
                                                            R, nt, N, E, stats, part);
  if (rc2 != ADELL_OK) return rc2;
  return adell_launch<adell_ijepa_loss_merge_kernel>(dim3(1), dim3(64), 0, st, (const float*)part, R,
                                                     1.0 / ((double)R * (double)E), loss);
}

template <bool VEC>
__global__ __launch_bounds__(IJ_NT) void adell_ijepa_loss_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ h, const int* __restrict__ rows,
    const float* __restrict__ stats, const float* __restrict__ g, float scale, int R, int nt, int N,
    int E, float* __restrict__ dpred) {
  const int r = blockIdx.x * IJ_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = r / nt;
  const float* hp = h + ((size_t)b * N + rows[r - b * nt]) * E;
  const float* pp = pred + (size_t)r * E;
  float* dp = dpred + (size_t)r * E;
  const float mean = stats[2 * r], rstd = stats[2 * r + 1];
  const float gs = g[0] * scale;
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 d = ij_ld4(pp, i) - (ij_ld4(hp, i) - mean) * rstd;
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = gs * fminf(fmaxf(d[c], -1.f), 1.f);
      ij_st4(dp, i, o);
    }
  } else {
    for (int e = lane; e < E; e += 64)
      dp[e] = gs * fminf(fmaxf(pp[e] - (hp[e] - mean) * rstd, -1.f), 1.f);
  }
}

extern "C" int adell_ijepa_loss_bwd(const float* pred, const float* h, const int* rows,
                                    const float* stats, const float* g, int B, int nt, int N, int E,
                                    float* dpred, void* stream) {
  const int rc = ij_loss_args("ijepa_loss_bwd", pred, h, rows, B, nt, N, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(stats && g && dpred, "ijepa_loss_bwd: null statistics / gradient");
  const int R = B * nt;
  const float scale = (float)(1.0 / ((double)R * (double)E));
  hipStream_t st = (hipStream_t)stream;
  if ((E % 4 == 0) && adell_aligned16(pred) && adell_aligned16(h) && adell_aligned16(dpred))
    return adell_launch<adell_ijepa_loss_bwd_kernel<true>>(ij_grid(R), dim3(IJ_NT), 0, st, pred, h, rows,
                                                           stats, g, scale, R, nt, N, E, dpred);
  return adell_launch<adell_ijepa_loss_bwd_kernel<false>>(ij_grid(R), dim3(IJ_NT), 0, st, pred, h, rows,
                                                          stats, g, scale, R, nt, N, E, dpred);
}
