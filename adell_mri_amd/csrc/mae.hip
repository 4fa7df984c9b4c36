// Kernels of the ViT masked autoencoder (adell_mri/modules/self_supervised/autoencoders.py,
// ViTMaskedAutoEncoderPL in pl.py): the per-item token shuffle the reference does with argsort and
// torch.gather, the un-shuffle that splices in the scaled mask token and the positional embedding, and
// the reconstruction loss taken through the reference's view / permute. House rules of ijepa.hip: fp32
// in and out, no float atomics, every sum in a fixed order -- two runs are bit-identical. One wave
// owns one row of E floats (four rows per block of 256 threads); a row wider than one pass is walked
// with a strided loop. float4 or scalar is decided per LAUNCH (E % 4 == 0 and every base 16-byte
// aligned, so every row is). Index tables are int32, PER ITEM and not sorted, and are checked by the
// caller on the host (ops.MaeShuffle: every row of ids_shuffle a permutation); the kernels read them
// unchecked.
//   * per-item row gather: out[b][o] = in[b][tab[b][o]], zeros where tab[b][o] < 0. "Keep" is the
//     table ids_keep [B][K]; its backward is the same kernel through the inverse table [B][L] (-1 on
//     the masked tokens) and writes the whole dx -- no memset, no scatter.
//   * restore: out[b][l] = (r = restore[b][l]) < K ? enc[b][r] : scale * mask_token, plus pos[l], one
//     launch; scale is read from device memory. Backward: one launch for denc (rows of dout through
//     ids_keep) and the whole dpos (row l summed over b in order); the masked rows of dout are summed
//     per chunk of MAE_CHUNK (b, l) rows in fp64 (second launch) and the chunks in order by one block
//     (third launch), which writes dmask_token = scale S and dscale = sum_e mask_token[e] S[e].
//   * reconstruction loss: mean((pred[b][l][p C + c] - x[b][c][l P + p])^2), the reference's
//     view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).view(B, C, H, W) as an index map: the permuted tensor
//     is never written. Per-row partials, then a one-wave second stage in fp64. Backward one launch.
//   * image layout: the same index map as a copy, both ways (C > 1 only; C == 1 is a view).
#include "common.h"

constexpr int MAE_NT = 256;             // threads per block
constexpr int MAE_ROWS = MAE_NT / 64;   // rows (waves) per block
constexpr int MAE_CHUNK = 32;           // (b, l) rows per fp64 partial of the mask-token gradient

__device__ __forceinline__ f32x4 mae_ld4(const float* p, int i) {
  return reinterpret_cast<const f32x4*>(p)[i];
}
__device__ __forceinline__ void mae_st4(float* p, int i, f32x4 v) {
  reinterpret_cast<f32x4*>(p)[i] = v;
}

static inline dim3 mae_grid(long rows) {
  return dim3((unsigned)((rows + MAE_ROWS - 1) / MAE_ROWS));
}

// ---- per-item row gather ---------------------------------------------------------------------------
// Row (b, o) of out [B][No][E] = row (b, tab[b][o]) of in [B][Ni][E], zeros where tab[b][o] < 0.
template <bool VEC>
__global__ __launch_bounds__(MAE_NT) void adell_mae_rows_kernel(
    const float* __restrict__ in, const int* __restrict__ tab, long rows, int No, int Ni, int E,
    float* __restrict__ out) {
  const long row = (long)blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / No;
  const int src = tab[row];
  const float* ip = in + ((size_t)b * Ni + (src < 0 ? 0 : src)) * E;
  float* op = out + (size_t)row * E;
  if (VEC) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < (E >> 2); i += 64) mae_st4(op, i, src < 0 ? zero : mae_ld4(ip, i));
  } else {
    for (int e = lane; e < E; e += 64) op[e] = src < 0 ? 0.f : ip[e];
  }
}

extern "C" int adell_mae_gather_rows(const float* in, const int* tab, int B, int No, int Ni, int E,
                                     float* out, void* stream) {
  ADELL_REQUIRE(in && tab && out && B > 0 && No > 0 && Ni > 0 && E > 0,
                "mae_gather_rows: bad arguments");
  ADELL_REQUIRE((long)B * No <= 0x7fffffffL && (long)B * Ni <= 0x7fffffffL,
                "mae_gather_rows: too many rows");
  const long rows = (long)B * No;
  hipStream_t st = (hipStream_t)stream;
  if ((E % 4 == 0) && adell_aligned16(in) && adell_aligned16(out))
    return adell_launch<adell_mae_rows_kernel<true>>(mae_grid(rows), dim3(MAE_NT), 0, st, in, tab, rows,
                                                     No, Ni, E, out);
  return adell_launch<adell_mae_rows_kernel<false>>(mae_grid(rows), dim3(MAE_NT), 0, st, in, tab, rows,
                                                    No, Ni, E, out);
}

// ---- restore -----------------------------------------------------------------------------------------
// (the product scale * mask_token is rounded before pos is added, as the reference's two torch ops)
template <bool VEC>
__global__ __launch_bounds__(MAE_NT) void adell_mae_restore_fwd_kernel(
    const float* __restrict__ enc, const float* __restrict__ mask, const float* __restrict__ scale,
    const float* __restrict__ pos, const int* __restrict__ restore, long rows, int L, int K, int E,
    float* __restrict__ out) {
  const long row = (long)blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / L;
  const int l = (int)(row - b * L);
  const int r = restore[row];
  const bool visible = r < K;
  const float* ap = visible ? enc + ((size_t)b * K + r) * E : mask;
  const float* pp = pos + (size_t)l * E;
  float* op = out + (size_t)row * E;
  const float s = visible ? 1.f : scale[0];
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 a = mae_ld4(ap, i), p = mae_ld4(pp, i);
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = __fadd_rn(__fmul_rn(s, a[c]), p[c]);
      mae_st4(op, i, o);
    }
  } else {
    for (int e = lane; e < E; e += 64) op[e] = __fadd_rn(__fmul_rn(s, ap[e]), pp[e]);
  }
}

static int mae_restore_args(const char* what, int B, int L, int K, int E) {
  ADELL_REQUIRE(B > 0 && L > 0 && E > 0 && K >= 1 && K <= L, "%s: bad arguments (1 <= K <= L)", what);
  ADELL_REQUIRE((long)B * L <= 0x7fffffffL, "%s: too many rows", what);
  return ADELL_OK;
}

extern "C" int adell_mae_restore_fwd(const float* enc, const float* mask_token, const float* scale,
                                     const float* pos, const int* restore, int B, int L, int K, int E,
                                     float* out, void* stream) {
  const int rc = mae_restore_args("mae_restore_fwd", B, L, K, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(enc && mask_token && scale && pos && restore && out, "mae_restore_fwd: null pointer");
  const long rows = (long)B * L;
  hipStream_t st = (hipStream_t)stream;
  if ((E % 4 == 0) && adell_aligned16(enc) && adell_aligned16(mask_token) && adell_aligned16(pos) &&
      adell_aligned16(out))
    return adell_launch<adell_mae_restore_fwd_kernel<true>>(mae_grid(rows), dim3(MAE_NT), 0, st, enc,
                                                            mask_token, scale, pos, restore, rows, L, K,
                                                            E, out);
  return adell_launch<adell_mae_restore_fwd_kernel<false>>(mae_grid(rows), dim3(MAE_NT), 0, st, enc,
                                                           mask_token, scale, pos, restore, rows, L, K,
                                                           E, out);
}

// Rows [0, copy): denc row (b, j) = dout row (b, keep[b][j]) (copy = B K, or 0 without denc). Rows
// [copy, copy + L): dpos row l = sum_b dout[b][l], b in order.
template <bool VEC>
__global__ __launch_bounds__(MAE_NT) void adell_mae_restore_bwd_kernel(
    const float* __restrict__ dout, const int* __restrict__ keep, long copy, int B, int L, int K, int E,
    float* __restrict__ denc, float* __restrict__ dpos) {
  const long row = (long)blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const size_t item = (size_t)L * E;
  if (row < copy) {
    const long b = row / K;
    const float* ip = dout + (size_t)b * item + (size_t)keep[row] * E;
    float* op = denc + (size_t)row * E;
    if (VEC) {
      for (int i = lane; i < (E >> 2); i += 64) mae_st4(op, i, mae_ld4(ip, i));
    } else {
      for (int e = lane; e < E; e += 64) op[e] = ip[e];
    }
    return;
  }
  const long l = row - copy;
  if (l >= L || dpos == nullptr) return;
  const float* ip = dout + (size_t)l * E;
  float* op = dpos + (size_t)l * E;
  if (VEC) {
    for (int i = lane; i < (E >> 2); i += 64) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b) acc += mae_ld4(ip + (size_t)b * item, i);
      mae_st4(op, i, acc);
    }
  } else {
    for (int e = lane; e < E; e += 64) {
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += ip[(size_t)b * item + e];
      op[e] = acc;
    }
  }
}

// part[c][e] = sum of dout[row][e] over the masked rows (restore[row] >= K) of chunk c, rows
// [c MAE_CHUNK, (c + 1) MAE_CHUNK) of the B L rows, in order, in fp64. One thread per feature; the
// test on the table is the same in every lane.
__global__ __launch_bounds__(MAE_NT) void adell_mae_mask_partial_kernel(
    const float* __restrict__ dout, const int* __restrict__ restore, long rows, int K, int E,
    double* __restrict__ part) {
  const int e = blockIdx.x * MAE_NT + threadIdx.x;
  if (e >= E) return;
  const long lo = (long)blockIdx.y * MAE_CHUNK;
  const long hi = lo + MAE_CHUNK < rows ? lo + MAE_CHUNK : rows;
  double acc = 0.0;
  for (long row = lo; row < hi; ++row)
    if (restore[row] >= K) acc += (double)dout[(size_t)row * E + e];
  part[(size_t)blockIdx.y * E + e] = acc;
}

// One block: S[e] = sum_c part[c][e] (c in order); dmask[e] = scale S[e]; dscale = sum_e mask[e] S[e],
// thread t adding e = t, t + 256, ... in order, the 64 lanes of a wave folded by the butterfly, the
// four waves added in order.
__global__ __launch_bounds__(MAE_NT) void adell_mae_mask_merge_kernel(
    const double* __restrict__ part, const float* __restrict__ mask, const float* __restrict__ scale,
    int chunks, int E, float* __restrict__ dmask, float* __restrict__ dscale) {
  __shared__ double wave_sum[MAE_ROWS];
  const double s = (double)scale[0];
  double acc = 0.0;
  for (int e = threadIdx.x; e < E; e += MAE_NT) {
    double S = 0.0;
    for (int c = 0; c < chunks; ++c) S += part[(size_t)c * E + e];
    if (dmask) dmask[e] = (float)(s * S);
    acc += (double)mask[e] * S;
  }
  acc = adell_wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0 && dscale) {
    double total = 0.0;
    for (int w = 0; w < MAE_ROWS; ++w) total += wave_sum[w];
    dscale[0] = (float)total;
  }
}

extern "C" int adell_mae_restore_bwd_chunks(int B, int L) {
  if (B <= 0 || L <= 0 || (long)B * L > 0x7fffffffL) return 0;
  return (int)(((long)B * L + MAE_CHUNK - 1) / MAE_CHUNK);
}

extern "C" int adell_mae_restore_bwd(const float* dout, const float* mask_token, const float* scale,
                                     const int* keep, const int* restore, int B, int L, int K, int E,
                                     float* denc, float* dpos, float* dmask, float* dscale,
                                     double* part, int part_rows, void* stream) {
  const int rc = mae_restore_args("mae_restore_bwd", B, L, K, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dout && keep && restore, "mae_restore_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const long copy = denc ? (long)B * K : 0;
  const long rows = copy + (dpos ? L : 0);
  if (rows > 0) {
    int rc2;
    if ((E % 4 == 0) && adell_aligned16(dout) && adell_aligned16(denc) && adell_aligned16(dpos))
      rc2 = adell_launch<adell_mae_restore_bwd_kernel<true>>(mae_grid(rows), dim3(MAE_NT), 0, st, dout,
                                                             keep, copy, B, L, K, E, denc, dpos);
    else
      rc2 = adell_launch<adell_mae_restore_bwd_kernel<false>>(mae_grid(rows), dim3(MAE_NT), 0, st, dout,
                                                              keep, copy, B, L, K, E, denc, dpos);
    if (rc2 != ADELL_OK) return rc2;
  }
  if (dmask == nullptr && dscale == nullptr) return ADELL_OK;
  const int chunks = adell_mae_restore_bwd_chunks(B, L);
  ADELL_REQUIRE(mask_token && scale && part, "mae_restore_bwd: the mask-token gradients need "
                                             "mask_token, scale and the partial-sum buffer");
  ADELL_REQUIRE_ROWS(part, part_rows, chunks, "mae_restore_bwd");
  ADELL_REQUIRE(chunks <= 65535, "mae_restore_bwd: %d chunks of rows exceed the grid", chunks);
  const int rc3 = adell_launch<adell_mae_mask_partial_kernel>(
      dim3((unsigned)adell_cdiv(E, MAE_NT), (unsigned)chunks), dim3(MAE_NT), 0, st, dout, restore,
      (long)B * L, K, E, part);
  if (rc3 != ADELL_OK) return rc3;
  return adell_launch<adell_mae_mask_merge_kernel>(dim3(1), dim3(MAE_NT), 0, st, (const double*)part,
                                                   mask_token, scale, chunks, E, dmask, dscale);
}

// ---- reconstruction loss -----------------------------------------------------------------------------
// Element i = p C + c of token row (b, l) of pred [B][L][P C] sits at x[b][c][l P + p] of the image
// x [B][C][L P]. With one channel the two rows are the same P floats.
__device__ __forceinline__ size_t mae_image_at(long b, int l, int i, int C, int L, int P) {
  const int p = i / C, c = i - p * C;
  return ((size_t)b * C + c) * ((size_t)L * P) + (size_t)l * P + p;
}

// One wave per row r = b L + l: part[r] = sum over the row of (pred - x)^2. ONE: C == 1, float4.
template <bool ONE>
__global__ __launch_bounds__(MAE_NT) void adell_mae_loss_rows_kernel(
    const float* __restrict__ pred, const float* __restrict__ x, int R, int C, int L, int P,
    float* __restrict__ part) {
  const int r = blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int E = P * C;
  const float* pp = pred + (size_t)r * E;
  float s = 0.f;
  if (ONE) {
    const float* xp = x + (size_t)r * E;
    for (int i = lane; i < (E >> 2); i += 64) {
      const f32x4 d = mae_ld4(pp, i) - mae_ld4(xp, i);
      s += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  } else {
    const long b = r / L;
    const int l = (int)(r - b * L);
    for (int i = lane; i < E; i += 64) {
      const float d = pp[i] - x[mae_image_at(b, l, i, C, L, P)];
      s += d * d;
    }
  }
  s = adell_wave_sum(s);
  if (lane == 0) part[r] = s;
}

// One wave: lane l adds the rows l, l + 64, ... in order, the 64 sums are folded in the fixed order
// of the butterfly; loss = sum / (B C H W).
__global__ __launch_bounds__(64) void adell_mae_loss_merge_kernel(const float* __restrict__ part, int R,
                                                                  double inv_count,
                                                                  float* __restrict__ loss) {
  double acc = 0.0;
  for (int r = threadIdx.x; r < R; r += 64) acc += (double)part[r];
  acc = adell_wave_sum_d(acc);
  if (threadIdx.x == 0) loss[0] = (float)(acc * inv_count);
}

static int mae_image_args(const char* what, int B, int C, int L, int P) {
  ADELL_REQUIRE(B > 0 && C > 0 && L > 0 && P > 0, "%s: bad arguments", what);
  ADELL_REQUIRE((long)B * L <= 0x7fffffffL && (long)P * C <= 0x7fffffffL, "%s: too many rows", what);
  return ADELL_OK;
}

static bool mae_one_channel_vec(int C, int P, const void* a, const void* b, const void* c) {
  return C == 1 && (P % 4 == 0) && adell_aligned16(a) && adell_aligned16(b) && adell_aligned16(c);
}

extern "C" int adell_mae_loss_fwd(const float* pred, const float* x, int B, int C, int L, int P,
                                  float* part, float* loss, void* stream) {
  const int rc = mae_image_args("mae_loss_fwd", B, C, L, P);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(pred && x && part && loss, "mae_loss_fwd: null pointer");
  const int R = B * L;
  hipStream_t st = (hipStream_t)stream;
  int rc2;
  if (mae_one_channel_vec(C, P, pred, x, nullptr))
    rc2 = adell_launch<adell_mae_loss_rows_kernel<true>>(mae_grid(R), dim3(MAE_NT), 0, st, pred, x, R, C,
                                                         L, P, part);
  else
    rc2 = adell_launch<adell_mae_loss_rows_kernel<false>>(mae_grid(R), dim3(MAE_NT), 0, st, pred, x, R,
                                                          C, L, P, part);
  if (rc2 != ADELL_OK) return rc2;
  return adell_launch<adell_mae_loss_merge_kernel>(
      dim3(1), dim3(64), 0, st, (const float*)part, R,
      1.0 / ((double)R * (double)P * (double)C), loss);
}

template <bool ONE>
__global__ __launch_bounds__(MAE_NT) void adell_mae_loss_bwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ x, const float* __restrict__ g,
    float scale, int R, int C, int L, int P, float* __restrict__ dpred) {
  const int r = blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int E = P * C;
  const float* pp = pred + (size_t)r * E;
  float* dp = dpred + (size_t)r * E;
  const float gs = g[0] * scale;
  if (ONE) {
    const float* xp = x + (size_t)r * E;
    for (int i = lane; i < (E >> 2); i += 64) mae_st4(dp, i, (mae_ld4(pp, i) - mae_ld4(xp, i)) * gs);
  } else {
    const long b = r / L;
    const int l = (int)(r - b * L);
    for (int i = lane; i < E; i += 64) dp[i] = gs * (pp[i] - x[mae_image_at(b, l, i, C, L, P)]);
  }
}

extern "C" int adell_mae_loss_bwd(const float* pred, const float* x, const float* g, int B, int C,
                                  int L, int P, float* dpred, void* stream) {
  const int rc = mae_image_args("mae_loss_bwd", B, C, L, P);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(pred && x && g && dpred, "mae_loss_bwd: null pointer");
  const int R = B * L;
  const float scale = (float)(2.0 / ((double)R * (double)P * (double)C));
  hipStream_t st = (hipStream_t)stream;
  if (mae_one_channel_vec(C, P, pred, x, dpred))
    return adell_launch<adell_mae_loss_bwd_kernel<true>>(mae_grid(R), dim3(MAE_NT), 0, st, pred, x, g,
                                                         scale, R, C, L, P, dpred);
  return adell_launch<adell_mae_loss_bwd_kernel<false>>(mae_grid(R), dim3(MAE_NT), 0, st, pred, x, g,
                                                        scale, R, C, L, P, dpred);
}

// ---- image layout ------------------------------------------------------------------------------------
// TO_IMAGE: image[b][c][l P + p] = tokens[b][l][p C + c]; else the inverse copy (its gradient).
template <bool TO_IMAGE>
__global__ __launch_bounds__(MAE_NT) void adell_mae_image_kernel(const float* __restrict__ in, int R,
                                                                 int C, int L, int P,
                                                                 float* __restrict__ out) {
  const int r = blockIdx.x * MAE_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int E = P * C;
  const long b = r / L;
  const int l = (int)(r - b * L);
  for (int i = lane; i < E; i += 64) {
    const size_t tok = (size_t)r * E + i, img = mae_image_at(b, l, i, C, L, P);
    if (TO_IMAGE)
      out[img] = in[tok];
    else
      out[tok] = in[img];
  }
}

extern "C" int adell_mae_to_image(const float* tokens, int B, int C, int L, int P, float* image,
                                  void* stream) {
  const int rc = mae_image_args("mae_to_image", B, C, L, P);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(tokens && image, "mae_to_image: null pointer");
  return adell_launch<adell_mae_image_kernel<true>>(mae_grid((long)B * L), dim3(MAE_NT), 0,
                                                    (hipStream_t)stream, tokens, B * L, C, L, P, image);
}

extern "C" int adell_mae_from_image(const float* image, int B, int C, int L, int P, float* tokens,
                                    void* stream) {
  const int rc = mae_image_args("mae_from_image", B, C, L, P);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(image && tokens, "mae_from_image: null pointer");
  return adell_launch<adell_mae_image_kernel<false>>(mae_grid((long)B * L), dim3(MAE_NT), 0,
                                                     (hipStream_t)stream, image, B * L, C, L, P, tokens);
}
