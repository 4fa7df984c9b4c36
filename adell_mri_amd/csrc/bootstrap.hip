// Evaluation with uncertainty (adell_mri/utils/bootstrap_metrics.py, modules/conformal_prediction):
// the AUC of every bootstrap resample from one launch, and the cumulative probabilities of adaptive
// prediction sets. Integer or fixed-order fp64 arithmetic, no float atomics: two runs are bit-identical.
//   * boot_auroc_pairs. The caller sorts the n scores once (stable, ascending) and hands over pos[i],
//     the sorted position of sample i, the tie group [gstart[p], gend[p]) of every sorted position p
//     and the labels in sorted order (1 positive, 0 negative, anything else skipped). A block per
//     resample r builds two bitmasks of n bits in LDS from its m indices, one of the selected negatives
//     and one of the selected positives (atomicOr on 32-bit words; a bit that is already set is a
//     duplicate index, an index outside [0, n) is counted with them), takes the exclusive prefix
//     popcount of the negative mask per word, and adds negBefore(gstart[p]) + negBefore(gend[p]) over
//     the selected positives p, negBefore(q) = prefix[q >> 5] + popc(mask[q >> 5] & lowbits(q & 31)):
//     the negatives strictly below the tie group count twice and those inside it once, that is
//     2 #{pos > neg} + #{pos == neg}, the statistic of adell_cls_auroc_pairs (classify.hip).
//     out[r] = (that sum, positives, negatives, bad indices) as int64, every element written. A
//     duplicate of a skipped sample is not counted: it cannot change the other three.
//     LDS: three words per 32 samples, 3 n / 8 bytes. n <= ADELL_BOOT_MAX_N = 196608 keeps a block at
//     72 KiB, two blocks per CU within the 160 KiB of gfx950; beyond it adell_boot_auroc_route says
//     ADELL_BOOT_LOOP and the launcher refuses.
//   * aps_cumulative. A wave per row of p [N][C], C <= ADELL_APS_MAX_CLASSES = 64, a lane per class:
//     rank[c] = #{j: p[j] > p[c], or p[j] == p[c] and j < c} (the stable descending order), the row is
//     laid out by rank in LDS and cum[c] = fp32(the fp64 sum of the ranks 0 .. rank[c] in rank order),
//     which is what an fp32 cumsum with an fp64 accumulator gives. score[i] = cum[i][y[i]] when labels
//     are given; a label outside [0, C) is never used as an index and gives NaN. A row with a NaN has
//     no such order: its cum is unspecified (every LDS index stays inside the row).
#include "common.h"

constexpr int BT_NT = 256;
constexpr int BT_NW = BT_NT / 64;
constexpr int BT_MAX_N = ADELL_BOOT_MAX_N;
constexpr int APS_MAX_C = ADELL_APS_MAX_CLASSES;
static_assert(2 * adell_lds_alloc((size_t)3 * (BT_MAX_N / 32) * 4 + 2048) <= (size_t)kAdellLdsPerCu,
              "two bootstrap blocks must fit a CU's LDS");

__device__ __forceinline__ long long bt_wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// negatives selected at sorted positions < q (q in [0, n]); q == n reads no word past the masks
__device__ __forceinline__ unsigned bt_neg_before(const unsigned* neg, const unsigned* pre, unsigned q,
                                                  unsigned n, unsigned total) {
  if (q >= n) return total;
  const unsigned w = q >> 5, b = q & 31u;
  return pre[w] + __popc(neg[w] & ((1u << b) - 1u));
}

__global__ __launch_bounds__(BT_NT) void adell_boot_auroc_kernel(
    const int* __restrict__ idx, int m, const int* __restrict__ pos, const int* __restrict__ gstart,
    const int* __restrict__ gend, const int* __restrict__ lab, int n, long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned bt_lds[];
  __shared__ unsigned part[BT_NT];
  __shared__ long long red[3][BT_NW];
  __shared__ unsigned tot;
  const int W = (n + 31) >> 5;
  unsigned* neg = bt_lds;
  unsigned* psel = bt_lds + W;
  unsigned* pre = bt_lds + 2 * W;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t r = blockIdx.x;

  for (int w = t; w < 2 * W; w += BT_NT) bt_lds[w] = 0u;
  __syncthreads();

  // the two masks
  long long bad = 0;
  const int* row = idx + r * (size_t)m;
  for (int j = t; j < m; j += BT_NT) {
    const int i = row[j];
    if (i < 0 || i >= n) {
      ++bad;
      continue;
    }
    const int p = pos[i];
    if (p < 0 || p >= n) {
      ++bad;
      continue;
    }
    const int l = lab[p];
    if (l != 0 && l != 1) continue;
    const unsigned bit = 1u << (p & 31);
    const unsigned old = atomicOr((l == 1 ? psel : neg) + (p >> 5), bit);
    if (old & bit) ++bad;
  }
  __syncthreads();

  // exclusive prefix popcount of the negative mask: a run of words per thread, then the runs' sums
  const int chunk = (W + BT_NT - 1) / BT_NT;
  const int w0 = min(t * chunk, W), w1 = min(w0 + chunk, W);
  unsigned mine = 0;
  for (int w = w0; w < w1; ++w) mine += __popc(neg[w]);
  part[t] = mine;
  __syncthreads();
  if (wave == 0) {
    unsigned v[BT_NW], s = 0;
#pragma unroll
    for (int k = 0; k < BT_NW; ++k) {
      v[k] = part[lane * BT_NW + k];
      s += v[k];
    }
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) tot = incl;
    unsigned run = incl - s;
#pragma unroll
    for (int k = 0; k < BT_NW; ++k) {
      part[lane * BT_NW + k] = run;
      run += v[k];
    }
  }
  __syncthreads();
  unsigned run = part[t];
  for (int w = w0; w < w1; ++w) {
    pre[w] = run;
    run += __popc(neg[w]);
  }
  const unsigned total = tot;
  __syncthreads();

  // every selected positive, in sorted order
  long long num = 0, npos = 0;
  for (int w = t; w < W; w += BT_NT) {
    unsigned bits = psel[w];
    npos += __popc(bits);
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1u;
      const int p = (w << 5) + b;
      const unsigned gs = (unsigned)max(gstart[p], 0), ge = (unsigned)max(gend[p], 0);
      num += (long long)bt_neg_before(neg, pre, gs, (unsigned)n, total) +
             (long long)bt_neg_before(neg, pre, ge, (unsigned)n, total);
    }
  }
  num = bt_wave_sum_ll(num);
  npos = bt_wave_sum_ll(npos);
  bad = bt_wave_sum_ll(bad);
  if (lane == 0) {
    red[0][wave] = num;
    red[1][wave] = npos;
    red[2][wave] = bad;
  }
  __syncthreads();
  if (t == 0) {
    long long a = 0, b = 0, c = 0;
    for (int k = 0; k < BT_NW; ++k) {
      a += red[0][k];
      b += red[1][k];
      c += red[2][k];
    }
    long long* o = out + r * 4;
    o[0] = a;
    o[1] = b;
    o[2] = (long long)total;
    o[3] = c;
  }
}

extern "C" int adell_boot_auroc_route(int n) {
  ADELL_REQUIRE(n > 0, "boot_auroc_route: n = %d", n);
  return n <= BT_MAX_N ? ADELL_BOOT_BITMASK : ADELL_BOOT_LOOP;
}

extern "C" int adell_boot_auroc_pairs(const int* idx, int R, int m, const int* pos, const int* gstart,
                                      const int* gend, const int* lab, int n, long long* out,
                                      void* stream) {
  ADELL_REQUIRE(idx && pos && gstart && gend && lab && out && R > 0 && m > 0 && n > 0,
                "boot_auroc_pairs: bad arguments (R %d, m %d, n %d)", R, m, n);
  ADELL_REQUIRE(n <= BT_MAX_N, "boot_auroc_pairs: n = %d is beyond the %d samples the bitmasks take", n,
                BT_MAX_N);
  const size_t lds = (size_t)3 * ((n + 31) / 32) * sizeof(unsigned);
  return adell_launch<adell_boot_auroc_kernel>(dim3((unsigned)R), dim3(BT_NT), lds, (hipStream_t)stream,
                                               idx, m, pos, gstart, gend, lab, n, out);
}

// ---- adaptive prediction sets -----------------------------------------------------------------------------
__global__ __launch_bounds__(BT_NT) void adell_aps_cumulative_kernel(
    const float* __restrict__ p, const long long* __restrict__ y, int N, int C, float* __restrict__ cum,
    float* __restrict__ score) {
  __shared__ float raw[BT_NW][APS_MAX_C];
  __shared__ float byrank[BT_NW][APS_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * BT_NW + wave;
  const bool row = i < N;        // every thread reaches both barriers
  const float v = row && lane < C ? p[i * C + lane] : 0.f;
  raw[wave][lane] = v;
  byrank[wave][lane] = 0.f;
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < C; ++j) {
    const float u = raw[wave][j];
    rank += (u > v || (u == v && j < lane)) ? 1 : 0;
  }
  if (lane < C) byrank[wave][rank] = v;      // rank <= j's counted < C
  __syncthreads();
  if (!row) return;
  float mine = 0.f;
  if (lane < C) {
    double s = 0.0;
    for (int k = 0; k <= rank; ++k) s += (double)byrank[wave][k];
    mine = (float)s;
    cum[i * C + lane] = mine;
  }
  if (score != nullptr) {
    const long long label = y[i];
    const bool ok = label >= 0 && label < C;
    const float got = __shfl(mine, ok ? (int)label : 0, 64);
    if (lane == 0) score[i] = ok ? got : __builtin_nanf("");
  }
}

extern "C" int adell_aps_cumulative(const float* p, const long long* y, int N, int C, float* cum,
                                    float* score, void* stream) {
  ADELL_REQUIRE(p && cum && N > 0 && C >= 1, "aps_cumulative: bad arguments (N %d, C %d)", N, C);
  ADELL_REQUIRE(C <= APS_MAX_C, "aps_cumulative: %d classes, the kernel takes at most %d", C, APS_MAX_C);
  ADELL_REQUIRE((y == nullptr) == (score == nullptr),
                "aps_cumulative: labels and scores come together");
  return adell_launch<adell_aps_cumulative_kernel>(dim3((unsigned)adell_cdiv(N, BT_NW)), dim3(BT_NT), 0,
                                                   (hipStream_t)stream, p, y, N, C, cum, score);
}
