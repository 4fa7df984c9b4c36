// Kernels of the multiple-instance classifiers
// (adell_mri/modules/classification/classification/multiple_instance_learning.py): a 2-D module runs on
// every slice of a volume and the volume is classified from the stack of slice vectors. House rules of
// mae.hip: fp32 in and out, dense inputs, no float atomics, every sum in a fixed order -- two runs are
// bit-identical.
//   * volume to slices: "b c h w s -> (b s) c h w". For fixed (b, c) a [P = H W][S] -> [S][P]
//     transpose, a 64 x 64 tile through LDS (rows padded to 65 floats: the transposed side walks a
//     column at a stride of 65 dwords, so the 32 lanes of a half hit 32 different banks). Global reads
//     run along s (with S <= 64 the tile's rows are one contiguous piece of 64 S floats), global
//     writes along p. The backward is the inverse copy of the same kernel. Both are copies: bit-equal to permute().contiguous().
//   * gated-attention pooling (MILAttention + MultipleInstanceClassifier.get_prediction), ONE launch
//     forward: a block per item and chunk of 64 features. score[s] = sum_n w[n] tanh(hv[s][n])
//     sigmoid(hu[s][n]) + bias, one wave per slice row; A = softmax over s (max-subtracted) by wave 0
//     (every chunk's block repeats this for its item, in the same order); then one thread per feature
//     walks the slices in order: "mean" sum_s feat A, "max" max_s feat A (lowest s on a tie, a NaN
//     wins as in torch.max; arg-max saved as int32), "vocabulary" sum_s softmax_F(feat[s]) A (row max
//     and log-sum saved per (b, s), the softmax matrix is not). Neither the gate product nor feat A is
//     written. Without gate inputs A = 1 / S. With F = 0 only A is computed (calculate_attention).
//     Backward, two launches (one without the gate): per item dfeat, dA (with the gradient that
//     arrived on A), dscore = A (dA - sum A dA), dhv, dhu and the item's fp64 partials of dw and db;
//     then the partials are added over the items in order.
//   * slice tokens (TransformableTransformer): out row 0 = the class token, row 1 + s = x[b][s] +
//     pos[s], pos one scalar per slice; one launch. Backward, one launch: dx copied whole, dpos[s] and
//     dclass_token summed over the batch in order in fp64.
#include "common.h"

constexpr int MIL_NT = 256;             // threads per block
constexpr int MIL_NW = MIL_NT / 64;     // waves per block
constexpr int MIL_TILE = 64;            // transpose tile edge
constexpr int MIL_MAX_S = 8192;         // slices per item the pooling kernels keep in LDS
constexpr int MIL_FCHUNK = 64;          // features per block of the pooling forward

// ---- volume <-> slices -------------------------------------------------------------------------------
// vol [BC = B C][P][S] (b, c outermost), sl [B][S][C][P]. TO_SLICES: sl = transpose(vol), else back.
template <bool TO_SLICES>
__global__ __launch_bounds__(MIL_NT) void adell_mil_slices_kernel(
    const float* __restrict__ in, int C, int P, int S, int tiles_p, int tiles_s,
    float* __restrict__ out) {
  __shared__ float tile[MIL_TILE][MIL_TILE + 1];      // [p][s]
  long blk = blockIdx.x;
  const int tp = (int)(blk % tiles_p);
  blk /= tiles_p;
  const int ts = (int)(blk % tiles_s);
  const long bc = blk / tiles_s;
  const long b = bc / C;
  const int c = (int)(bc - b * C);
  const int p0 = tp * MIL_TILE, s0 = ts * MIL_TILE;
  const int np = min(MIL_TILE, P - p0), ns = min(MIL_TILE, S - s0);
  const int n = np * ns;
  const size_t vol_base = (size_t)bc * P * S;
  // element (p, s) of the tile: vol_base + (p0 + p) S + s0 + s in the volume,
  // ((b S + s0 + s) C + c) P + p0 + p in the slices
  if (TO_SLICES) {
    for (int i = threadIdx.x; i < n; i += MIL_NT) {
      const int p = i / ns, s = i - p * ns;
      tile[p][s] = in[vol_base + (size_t)(p0 + p) * S + s0 + s];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MIL_NT) {
      const int s = i / np, p = i - s * np;
      out[(((size_t)b * S + s0 + s) * C + c) * P + p0 + p] = tile[p][s];
    }
  } else {
    for (int i = threadIdx.x; i < n; i += MIL_NT) {
      const int s = i / np, p = i - s * np;
      tile[p][s] = in[(((size_t)b * S + s0 + s) * C + c) * P + p0 + p];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += MIL_NT) {
      const int p = i / ns, s = i - p * ns;
      out[vol_base + (size_t)(p0 + p) * S + s0 + s] = tile[p][s];
    }
  }
}

static int mil_slices(const char* what, bool to_slices, const float* in, int B, int C, int P, int S,
                      float* out, void* stream) {
  ADELL_REQUIRE(in && out && B > 0 && C > 0 && P > 0 && S > 0, "%s: bad arguments", what);
  const long tiles_p = adell_cdiv(P, MIL_TILE), tiles_s = adell_cdiv(S, MIL_TILE);
  const long blocks = tiles_p * tiles_s * (long)B * C;
  ADELL_REQUIRE((long)B * C <= 0x7fffffffL && blocks <= 0x7fffffffL, "%s: too many tiles", what);
  hipStream_t st = (hipStream_t)stream;
  if (to_slices)
    return adell_launch<adell_mil_slices_kernel<true>>(dim3((unsigned)blocks), dim3(MIL_NT), 0, st, in, C,
                                                       P, S, (int)tiles_p, (int)tiles_s, out);
  return adell_launch<adell_mil_slices_kernel<false>>(dim3((unsigned)blocks), dim3(MIL_NT), 0, st, in, C,
                                                      P, S, (int)tiles_p, (int)tiles_s, out);
}

extern "C" int adell_mil_volume_to_slices(const float* vol, int B, int C, int P, int S, float* slices,
                                          void* stream) {
  return mil_slices("mil_volume_to_slices", true, vol, B, C, P, S, slices, stream);
}

extern "C" int adell_mil_slices_to_volume(const float* slices, int B, int C, int P, int S, float* vol,
                                          void* stream) {
  return mil_slices("mil_slices_to_volume", false, slices, B, C, P, S, vol, stream);
}

// ---- gated-attention pooling -------------------------------------------------------------------------
__device__ __forceinline__ float mil_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// 1 / (1 + exp(-x)): exp(-x) overflows to +inf for x < -88 and the quotient is 0, no NaN
__device__ __forceinline__ float mil_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Block (b, c): item b, features [c MIL_FCHUNK, (c + 1) MIL_FCHUNK). Every block of an item computes
// the item's A (and row statistics) for itself -- S N gate values, cheaper than a second launch -- in
// the same order, so they agree bit for bit; block c = 0 writes them out. "vocabulary" repeats the row
// max and log-sum over ALL F per chunk as well, S F ceil(F / 64) exponentials per item, and only 64 of
// the 256 threads walk the slices: the layout assumes the few features that mode has (vocabulary_size,
// 10 by default), and hundreds of features elsewhere. LDS: A [S], row max [S], row log-sum [S].
__global__ __launch_bounds__(MIL_NT) void adell_mil_pool_fwd_kernel(
    int mode, const float* __restrict__ hv, const float* __restrict__ hu, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ feat, int S, int N, int F,
    float* __restrict__ A, float* __restrict__ pooled, int* __restrict__ arg,
    float* __restrict__ rowstat) {
  extern __shared__ float mil_sm[];
  float* sA = mil_sm;
  float* sM = mil_sm + S;
  float* sL = mil_sm + 2 * S;
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool first = blockIdx.y == 0;
  if (hv != nullptr) {
    const float bb = bias[0];
    for (int s = wave; s < S; s += MIL_NW) {
      const float* pv = hv + ((size_t)b * S + s) * N;
      const float* pu = hu + ((size_t)b * S + s) * N;
      float acc = 0.f;
      for (int n = lane; n < N; n += 64) acc += w[n] * (tanhf(pv[n]) * mil_sigmoid(pu[n]));
      acc = adell_wave_sum(acc);
      if (lane == 0) sA[s] = acc + bb;
    }
    __syncthreads();
    if (wave == 0) {
      float mx = -INFINITY;
      for (int s = lane; s < S; s += 64) mx = fmaxf(mx, sA[s]);
      mx = mil_wave_max(mx);
      float sum = 0.f;
      for (int s = lane; s < S; s += 64) {
        const float e = expf(sA[s] - mx);
        sA[s] = e;
        sum += e;
      }
      sum = adell_wave_sum(sum);
      for (int s = lane; s < S; s += 64) {
        const float a = sA[s] / sum;
        sA[s] = a;
        if (first) A[(size_t)b * S + s] = a;
      }
    }
  } else {
    const float a = 1.0f / (float)S;
    for (int s = threadIdx.x; s < S; s += MIL_NT) {
      sA[s] = a;
      if (first) A[(size_t)b * S + s] = a;
    }
  }
  if (F == 0) return;
  if (mode == ADELL_MIL_VOCABULARY) {
    for (int s = wave; s < S; s += MIL_NW) {
      const float* pf = feat + ((size_t)b * S + s) * F;
      float mx = -INFINITY;
      for (int f = lane; f < F; f += 64) mx = fmaxf(mx, pf[f]);
      mx = mil_wave_max(mx);
      float sum = 0.f;
      for (int f = lane; f < F; f += 64) sum += expf(pf[f] - mx);
      sum = adell_wave_sum(sum);
      if (lane == 0) {
        const float l = logf(sum);
        sM[s] = mx;
        sL[s] = l;
        if (first) {
          rowstat[((size_t)b * S + s) * 2] = mx;
          rowstat[((size_t)b * S + s) * 2 + 1] = l;
        }
      }
    }
  }
  __syncthreads();
  const float* pf = feat + (size_t)b * S * F;
  const int f1 = min(F, ((int)blockIdx.y + 1) * MIL_FCHUNK);
  for (int f = blockIdx.y * MIL_FCHUNK + threadIdx.x; f < f1; f += MIL_NT) {
    if (mode == ADELL_MIL_MAX) {
      float best = pf[f] * sA[0];
      int at = 0;
#pragma unroll 8
      for (int s = 1; s < S; ++s) {
        const float v = pf[(size_t)s * F + f] * sA[s];
        if (v > best || (v != v && best == best)) {
          best = v;
          at = s;
        }
      }
      pooled[(size_t)b * F + f] = best;
      arg[(size_t)b * F + f] = at;
    } else if (mode == ADELL_MIL_VOCABULARY) {
      float acc = 0.f;
#pragma unroll 4
      for (int s = 0; s < S; ++s) acc += expf(pf[(size_t)s * F + f] - sM[s] - sL[s]) * sA[s];
      pooled[(size_t)b * F + f] = acc;
    } else {
      float acc = 0.f;
#pragma unroll 8
      for (int s = 0; s < S; ++s) acc += pf[(size_t)s * F + f] * sA[s];
      pooled[(size_t)b * F + f] = acc;
    }
  }
}

// One block per item b. LDS: A [S], dA [S] (dscore afterwards). part [B][N + 1] doubles: the item's
// sum_s dscore tanh sigmoid per n, and sum_s dscore at [N].
__global__ __launch_bounds__(MIL_NT) void adell_mil_pool_bwd_kernel(
    int mode, const float* __restrict__ hv, const float* __restrict__ hu, const float* __restrict__ w,
    const float* __restrict__ feat, const float* __restrict__ A, const int* __restrict__ arg,
    const float* __restrict__ rowstat, const float* __restrict__ g, const float* __restrict__ gA, int S,
    int N, int F, float* __restrict__ dfeat, float* __restrict__ dhv, float* __restrict__ dhu,
    double* __restrict__ part) {
  extern __shared__ float mil_sm[];
  float* sA = mil_sm;
  float* sD = mil_sm + S;
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int s = threadIdx.x; s < S; s += MIL_NT) sA[s] = A[(size_t)b * S + s];
  __syncthreads();
  const float* pg = g + (size_t)b * F;
  for (int s = wave; s < S; s += MIL_NW) {
    const size_t row = (size_t)b * S + s;
    const float a = sA[s];
    float q = 0.f;
    if (F > 0) {
      const float* pf = feat + row * F;
      float* pd = dfeat + row * F;
      if (mode == ADELL_MIL_VOCABULARY) {
        // p = softmax_F(feat[s]) again from the saved row max and log-sum, as the forward took it
        const float m = rowstat[row * 2], l = rowstat[row * 2 + 1];
        for (int f = lane; f < F; f += 64) q += pg[f] * expf(pf[f] - m - l);
        q = adell_wave_sum(q);
        for (int f = lane; f < F; f += 64) pd[f] = expf(pf[f] - m - l) * a * (pg[f] - q);
      } else if (mode == ADELL_MIL_MAX) {
        const int* pa = arg + (size_t)b * F;
        for (int f = lane; f < F; f += 64) {
          const bool hit = pa[f] == s;
          q += hit ? pg[f] * pf[f] : 0.f;
          pd[f] = hit ? pg[f] * a : 0.f;
        }
        q = adell_wave_sum(q);
      } else {
        for (int f = lane; f < F; f += 64) {
          q += pg[f] * pf[f];
          pd[f] = pg[f] * a;
        }
        q = adell_wave_sum(q);
      }
    }
    if (lane == 0) sD[s] = q + (gA != nullptr ? gA[row] : 0.f);
  }
  if (hv == nullptr) return;
  __syncthreads();
  if (wave == 0) {
    float dot = 0.f;
    double sum = 0.0;
    for (int s = lane; s < S; s += 64) dot += sA[s] * sD[s];
    dot = adell_wave_sum(dot);
    for (int s = lane; s < S; s += 64) {
      const float d = sA[s] * (sD[s] - dot);
      sD[s] = d;
      sum += (double)d;
    }
    sum = adell_wave_sum_d(sum);
    if (lane == 0) part[(size_t)b * (N + 1) + N] = sum;
  }
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += MIL_NT) {
    const float wn = w[n];
    double acc = 0.0;
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
      const size_t at = ((size_t)b * S + s) * N + n;
      const float t = tanhf(hv[at]), sg = mil_sigmoid(hu[at]), d = sD[s];
      dhv[at] = d * wn * sg * (1.0f - t * t);
      dhu[at] = d * wn * t * sg * (1.0f - sg);
      acc += (double)(d * (t * sg));
    }
    part[(size_t)b * (N + 1) + n] = acc;
  }
}

// dw[n] = sum_b part[b][n] (b in order), n < N; db = the same at n = N.
__global__ __launch_bounds__(MIL_NT) void adell_mil_pool_merge_kernel(const double* __restrict__ part,
                                                                      int B, int N,
                                                                      float* __restrict__ dw,
                                                                      float* __restrict__ db) {
  const int n = blockIdx.x * MIL_NT + threadIdx.x;
  if (n > N) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += part[(size_t)b * (N + 1) + n];
  if (n < N)
    dw[n] = (float)acc;
  else
    db[0] = (float)acc;
}

static int mil_pool_args(const char* what, int mode, int B, int S, int N, int F, bool gated) {
  ADELL_REQUIRE(mode == ADELL_MIL_MEAN || mode == ADELL_MIL_MAX || mode == ADELL_MIL_VOCABULARY,
                "%s: mode %d is none of ADELL_MIL_MEAN / _MAX / _VOCABULARY", what, mode);
  ADELL_REQUIRE(B > 0 && S > 0 && F >= 0 && (!gated || N > 0), "%s: bad arguments", what);
  ADELL_REQUIRE(S <= MIL_MAX_S, "%s: %d slices per item, at most %d", what, S, MIL_MAX_S);
  ADELL_REQUIRE(gated || F > 0, "%s: neither gate inputs nor features", what);
  return ADELL_OK;
}

extern "C" int adell_mil_pool_fwd(int mode, const float* hv, const float* hu, const float* w,
                                  const float* bias, const float* feat, int B, int S, int N, int F,
                                  float* A, float* pooled, int* arg, float* rowstat, void* stream) {
  const bool gated = hv != nullptr;
  const int rc = mil_pool_args("mil_pool_fwd", mode, B, S, N, F, gated);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(A && (!gated || (hu && w && bias)), "mil_pool_fwd: null pointer");
  ADELL_REQUIRE(F == 0 || (feat && pooled), "mil_pool_fwd: features without an output");
  ADELL_REQUIRE(F == 0 || mode != ADELL_MIL_MAX || arg, "mil_pool_fwd: \"max\" needs the arg-max buffer");
  ADELL_REQUIRE(F == 0 || mode != ADELL_MIL_VOCABULARY || rowstat,
                "mil_pool_fwd: \"vocabulary\" needs the row-statistics buffer");
  ADELL_REQUIRE(F <= 65535 * MIL_FCHUNK, "mil_pool_fwd: too many features");
  const unsigned chunks = F > 0 ? (unsigned)adell_cdiv(F, MIL_FCHUNK) : 1u;
  return adell_launch<adell_mil_pool_fwd_kernel>(dim3((unsigned)B, chunks), dim3(MIL_NT),
                                                 3 * (size_t)S * sizeof(float), (hipStream_t)stream, mode,
                                                 hv, hu, w, bias, feat, S, N, F, A, pooled, arg, rowstat);
}

extern "C" int adell_mil_pool_bwd(int mode, const float* hv, const float* hu, const float* w,
                                  const float* feat, const float* A, const int* arg, const float* rowstat,
                                  const float* g, const float* gA, int B, int S, int N, int F,
                                  float* dfeat, float* dhv, float* dhu, float* dw, float* db, double* part,
                                  void* stream) {
  const bool gated = hv != nullptr;
  const int rc = mil_pool_args("mil_pool_bwd", mode, B, S, N, F, gated);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(A && (!gated || (hu && w && dhv && dhu && dw && db && part)), "mil_pool_bwd: null pointer");
  ADELL_REQUIRE(F == 0 || (feat && g && dfeat), "mil_pool_bwd: features without their gradients");
  ADELL_REQUIRE(F == 0 || mode != ADELL_MIL_MAX || arg, "mil_pool_bwd: \"max\" needs the arg-max buffer");
  ADELL_REQUIRE(F == 0 || mode != ADELL_MIL_VOCABULARY || rowstat,
                "mil_pool_bwd: \"vocabulary\" needs the row-statistics buffer");
  hipStream_t st = (hipStream_t)stream;
  const int rc2 = adell_launch<adell_mil_pool_bwd_kernel>(
      dim3((unsigned)B), dim3(MIL_NT), 2 * (size_t)S * sizeof(float), st, mode, hv, hu, w, feat, A, arg,
      rowstat, g, gA, S, N, F, dfeat, dhv, dhu, part);
  if (rc2 != ADELL_OK || !gated) return rc2;
  return adell_launch<adell_mil_pool_merge_kernel>(dim3((unsigned)adell_cdiv(N + 1, MIL_NT)), dim3(MIL_NT),
                                                   0, st, (const double*)part, B, N, dw, db);
}

// ---- slice tokens ------------------------------------------------------------------------------------
// One wave per output row (b, r), r < T = S + ct.
__global__ __launch_bounds__(MIL_NT) void adell_mil_tokens_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ pos, const float* __restrict__ cls, long rows,
    int S, int E, int ct, float* __restrict__ out) {
  const long row = (long)blockIdx.x * MIL_NW + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int T = S + ct;
  const long b = row / T;
  const int r = (int)(row - b * T);
  float* op = out + (size_t)row * E;
  if (r < ct) {
    for (int e = lane; e < E; e += 64) op[e] = cls[e];
    return;
  }
  const int s = r - ct;
  const float* ip = x + ((size_t)b * S + s) * E;
  if (pos != nullptr) {
    const float p = pos[s];
    for (int e = lane; e < E; e += 64) op[e] = __fadd_rn(ip[e], p);
  } else {
    for (int e = lane; e < E; e += 64) op[e] = ip[e];
  }
}

// Rows [0, B S): dx row (b, s) = dout row (b, ct + s). Rows [B S, B S + np) (np = S with dpos): dpos[s]
// = sum_b sum_e dout[b][ct + s][e], lane l adding e = l, l + 64, ... of item 0, then of item 1, ... in
// fp64, the lanes folded by the butterfly. The rows behind (with dcls): wave k sums features
// e = 64 k + lane of dout[b][0] over b in order in fp64.
__global__ __launch_bounds__(MIL_NT) void adell_mil_tokens_bwd_kernel(
    const float* __restrict__ dout, long copy, int np, int B, int S, int E, int ct,
    float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls) {
  const long row = (long)blockIdx.x * MIL_NW + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int T = S + ct;
  if (row < copy) {
    const long b = row / S;
    const int s = (int)(row - b * S);
    const float* ip = dout + ((size_t)b * T + ct + s) * E;
    float* op = dx + (size_t)row * E;
    for (int e = lane; e < E; e += 64) op[e] = ip[e];
    return;
  }
  const long k = row - copy;
  if (k < np) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      const float* ip = dout + ((size_t)b * T + ct + k) * E;
      for (int e = lane; e < E; e += 64) acc += (double)ip[e];
    }
    acc = adell_wave_sum_d(acc);
    if (lane == 0) dpos[k] = (float)acc;
    return;
  }
  if (dcls == nullptr) return;
  const long e = (k - np) * 64 + lane;
  if (e >= E) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += (double)dout[(size_t)b * T * E + e];
  dcls[e] = (float)acc;
}

static int mil_tokens_args(const char* what, int B, int S, int E) {
  ADELL_REQUIRE(B > 0 && S > 0 && E > 0, "%s: bad arguments", what);
  ADELL_REQUIRE((long)B * (S + 1) + S + E <= 0x7fffffffL, "%s: too many rows", what);
  return ADELL_OK;
}

extern "C" int adell_mil_slice_tokens_fwd(const float* x, const float* pos, const float* class_token,
                                          int B, int S, int E, float* out, void* stream) {
  const int rc = mil_tokens_args("mil_slice_tokens_fwd", B, S, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && out, "mil_slice_tokens_fwd: null pointer");
  const int ct = class_token != nullptr ? 1 : 0;
  const long rows = (long)B * (S + ct);
  return adell_launch<adell_mil_tokens_fwd_kernel>(dim3((unsigned)((rows + MIL_NW - 1) / MIL_NW)),
                                                   dim3(MIL_NT), 0, (hipStream_t)stream, x, pos,
                                                   class_token, rows, S, E, ct, out);
}

extern "C" int adell_mil_slice_tokens_bwd(const float* dout, int B, int S, int E, int has_class_token,
                                          float* dx, float* dpos, float* dclass_token, void* stream) {
  const int rc = mil_tokens_args("mil_slice_tokens_bwd", B, S, E);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dout, "mil_slice_tokens_bwd: null pointer");
  ADELL_REQUIRE(has_class_token || dclass_token == nullptr,
                "mil_slice_tokens_bwd: a class-token gradient without a class token");
  const int ct = has_class_token ? 1 : 0;
  const long copy = dx ? (long)B * S : 0;
  const int np = dpos ? S : 0;
  const long rows = copy + np + (dclass_token ? adell_cdiv(E, 64) : 0);
  if (rows == 0) return ADELL_OK;
  return adell_launch<adell_mil_tokens_bwd_kernel>(dim3((unsigned)((rows + MIL_NW - 1) / MIL_NW)),
                                                   dim3(MIL_NT), 0, (hipStream_t)stream, dout, copy, np, B,
                                                   S, E, ct, dx, dpos, dclass_token);
}
