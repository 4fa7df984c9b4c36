// Kernels of the local VICReg loss (VICRegLocalLoss, adell_mri/modules/self_supervised/losses/
// vicreg.py:168-404): the loss takes, per batch item, the gamma LARGEST entries of a T x T distance
// matrix between the tokens of two views (feature distances, or distances of the token grid mapped
// into each view's box), gathers the token rows they name and feeds the gathered [B gamma][C] rows to
// the VICReg terms (csrc/ssl.hip).
//   * top-gamma pairs: the T x T matrix is never written. A block owns a strip of 64 rows x a run of
//     64-column tiles; a tile of squared distances sum_k (a_ik - b_jk)^2 (fp32, difference form, the
//     channels in the same order for every pair) lives in registers, 4 x 4 per thread, the operands
//     in LDS in chunks of 32 channels. Every distance is packed with its flat index i T + j into one
//     64-bit key (distance bits high, ~index low): a larger key is a better candidate, and keys are
//     unique, so the order (distance descending, flat index ascending) is total and the result does
//     not depend on the order of arrival. The block keeps its candidates in an LDS buffer behind a
//     threshold (its gamma-th best key so far); the buffer is compacted by a bitonic sort when it
//     could overflow. A second kernel (one block per item) merges the blocks' candidates.
//   * location mode: the operands are the token coordinates grid * (hi - lo) + lo of the two boxes,
//     computed while the LDS tile is filled; no coordinate tensor exists.
//   * row gather and its backward: one thread owns a (item, channel) column and walks the gamma
//     entries in order -- duplicates are the rule (one outlier token is far from everything), and
//     there is no float atomic: two runs are bit-identical.
#include "common.h"

typedef unsigned long long tg_u64;
constexpr int TG_TI = 64, TG_TJ = 64, TG_CK = 32, TG_LD = 68, TG_CAP = 1024, TG_NT = 256;
constexpr int TG_MAXG = 64, TG_MAXT = 65535;   // flat indices i T + j stay below 2^32 - 1

struct TopgArgs {
  const float* a;      // [B][T][C] (feature mode) or null (location mode)
  const float* b;
  const float* box1;   // [B][2 ndim] (lo..., hi...) of view 1 / view 2 (location mode)
  const float* box2;
  int B, T, C, gamma;
  int ndim, dims[3];   // location mode: the token grid, row-major, dims[0 .. ndim)
  int strips, splits, tilesPerSplit, jtiles;
  tg_u64* cand;        // [B][strips * splits][gamma]
};

struct TopgState {
  tg_u64 buf[TG_CAP];
  tg_u64 thr;
  int cnt;
  int pend[2];
};

// Sort the buffer (descending), keep the gamma best, set the threshold. Called by all threads after
// a barrier; s->cnt is stable.
__device__ void adell_tg_compact(TopgState* s, int gamma) {
  const int tid = threadIdx.x;
  const int n = s->cnt;
  for (int i = tid; i < TG_CAP; i += TG_NT)
    if (i >= n) s->buf[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= TG_CAP; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < TG_CAP / 2; t += TG_NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const tg_u64 x = s->buf[i], y = s->buf[l];
        const bool desc = (i & k) == 0;
        if (desc ? (x < y) : (x > y)) {
          s->buf[i] = y;
          s->buf[l] = x;
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    s->cnt = n < gamma ? n : gamma;
    s->thr = n >= gamma ? s->buf[gamma - 1] : 0ull;
  }
  __syncthreads();
}

// One candidate per thread at most. ub: an upper bound of s->cnt that every thread carries (the
// count itself changes under the threads' feet). Ends with a barrier.
__device__ __forceinline__ void adell_tg_round(TopgState* s, int gamma, bool has, tg_u64 key,
                                               int& ub) {
  if (ub + TG_NT > TG_CAP) {
    adell_tg_compact(s, gamma);
    ub = gamma;
  }
  if (has && key > s->thr) {
    const int pos = atomicAdd(&s->cnt, 1);
    if (pos < TG_CAP) s->buf[pos] = key;   // (pos < TG_CAP always: ub + 256 <= TG_CAP)
  }
  ub += TG_NT;
  __syncthreads();
}

__device__ __forceinline__ float adell_tg_coord(const float* __restrict__ box, int ndim,
                                                const int* dims, int t, int d) {
#pragma clang fp contract(off)
  int idx = 0;
  for (int q = ndim - 1; q >= 0; --q) {
    const int v = t % dims[q];
    t /= dims[q];
    if (q == d) idx = v;
  }
  const float lo = box[d], hi = box[ndim + d];
  // the reference's order of operations: (grid * (hi - lo)) + lo, each step rounded
  const float size = hi - lo;
  const float scaled = (float)idx * size;
  return scaled + lo;
}

// Fill one [TG_CK][TG_LD] LDS tile with rows r0 .. r0 + 64 and channels k0 .. k0 + 32 of src
// (transposed: channel-major); rows / channels beyond the tensor are zero.
__device__ __forceinline__ void adell_tg_fill(const TopgArgs& g, const float* __restrict__ src,
                                              const float* __restrict__ box, int item, int r0, int k0,
                                              float* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < (TG_TI * TG_CK) / TG_NT; ++u) {
    const int e = tid + TG_NT * u;
    const int kk = e & (TG_CK - 1), ii = e / TG_CK;
    const int r = r0 + ii, k = k0 + kk;
    float v = 0.f;
    if (r < g.T && k < g.C) {
      if (src)
        v = src[((size_t)item * g.T + r) * g.C + k];
      else
        v = adell_tg_coord(box + (size_t)item * 2 * g.ndim, g.ndim, g.dims, r, k);
    }
    lds[kk * TG_LD + ii] = v;
  }
}

__global__ __launch_bounds__(TG_NT) void adell_topg_tile_kernel(TopgArgs g) {
  __shared__ __attribute__((aligned(16))) float As[TG_CK * TG_LD];
  __shared__ __attribute__((aligned(16))) float Bs[TG_CK * TG_LD];
  __shared__ TopgState st;
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int split = blk % g.splits; blk /= g.splits;
  const int strip = blk % g.strips;
  const int item = blk / g.strips;
  if (tid == 0) {
    st.cnt = 0;
    st.thr = 0ull;
    st.pend[0] = 0;
    st.pend[1] = 0;
  }
  __syncthreads();
  const int i0 = strip * TG_TI;
  const int ti = tid >> 4, tj = tid & 15;
  int ub = 0;
  const int jt0 = split * g.tilesPerSplit;
  int jt1 = jt0 + g.tilesPerSplit;
  if (jt1 > g.jtiles) jt1 = g.jtiles;
  for (int jt = jt0; jt < jt1; ++jt) {
    const int j0 = jt * TG_TJ;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < g.C; k0 += TG_CK) {
      __syncthreads();   // the previous chunk's readers are done
      adell_tg_fill(g, g.a, g.box1, item, i0, k0, As);
      adell_tg_fill(g, g.b, g.box2, item, j0, k0, Bs);
      __syncthreads();
      const int kmax = (g.C - k0 < TG_CK) ? g.C - k0 : TG_CK;
#pragma unroll 4
      for (int kk = 0; kk < kmax; ++kk) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(As + kk * TG_LD + ti * 4);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(Bs + kk * TG_LD + tj * 4);
        const float ar[4] = {av.x, av.y, av.z, av.w};
        const float bc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float d = ar[r] - bc[c];
            acc[r][c] = fmaf(d, d, acc[r][c]);
          }
      }
    }
    // candidates of this tile
    tg_u64 key[16];
    const tg_u64 thr = st.thr;   // stable: the last barrier is behind every writer
    int np = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + ti * 4 + r, j = j0 + tj * 4 + c;
        tg_u64 k = 0ull;   // 0: no candidate (every real key is larger)
        if (i < g.T && j < g.T) {
          const unsigned flat = (unsigned)i * (unsigned)g.T + (unsigned)j;
          k = ((tg_u64)__float_as_uint(acc[r][c]) << 32) | (tg_u64)(0xFFFFFFFFu - flat);
        }
        key[r * 4 + c] = k;
        np += (k > thr) ? 1 : 0;
      }
    int* pend = &st.pend[jt & 1];
    if (np) atomicAdd(pend, np);
    __syncthreads();
    const int p = *pend;
    if (tid == 0) st.pend[(jt + 1) & 1] = 0;
    if (p == 0) continue;   // (uniform)
    if (ub + p <= TG_CAP) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (key[q] > thr) {
          const int pos = atomicAdd(&st.cnt, 1);
          if (pos < TG_CAP) st.buf[pos] = key[q];
        }
      ub += p;
      __syncthreads();
    } else {
#pragma unroll 1
      for (int q = 0; q < 16; ++q) {
        tg_u64 kq = 0ull;
#pragma unroll
        for (int w = 0; w < 16; ++w) kq = (w == q) ? key[w] : kq;
        adell_tg_round(&st, g.gamma, kq != 0ull, kq, ub);
      }
    }
  }
  __syncthreads();
  adell_tg_compact(&st, g.gamma);
  tg_u64* out = g.cand + ((size_t)item * g.strips * g.splits + (size_t)strip * g.splits + split) *
                             g.gamma;
  for (int k = tid; k < g.gamma; k += TG_NT) out[k] = st.buf[k];   // zero keys past the block's count
}

// One block per item: the gamma best of its n candidate keys, as (i, j) pairs and squared distances.
__global__ __launch_bounds__(TG_NT) void adell_topg_merge_kernel(const tg_u64* __restrict__ cand,
                                                                 long n, int T, int gamma,
                                                                 int* __restrict__ pairs,
                                                                 float* __restrict__ dist2) {
  __shared__ TopgState st;
  const int tid = threadIdx.x, item = blockIdx.x;
  if (tid == 0) {
    st.cnt = 0;
    st.thr = 0ull;
  }
  __syncthreads();
  int ub = 0;
  const tg_u64* src = cand + (size_t)item * n;
  for (long base = 0; base < n; base += TG_NT) {
    const long e = base + tid;
    const tg_u64 k = e < n ? src[e] : 0ull;
    adell_tg_round(&st, gamma, k != 0ull, k, ub);
  }
  adell_tg_compact(&st, gamma);
  for (int k = tid; k < gamma; k += TG_NT) {
    const tg_u64 key = st.buf[k];
    int i = 0, j = 0;
    float d = 0.f;
    if (key != 0ull) {
      const unsigned flat = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
      i = (int)(flat / (unsigned)T);
      j = (int)(flat % (unsigned)T);
      d = __uint_as_float((unsigned)(key >> 32));
    }
    pairs[((size_t)item * gamma + k) * 2] = i;
    pairs[((size_t)item * gamma + k) * 2 + 1] = j;
    if (dist2) dist2[(size_t)item * gamma + k] = d;
  }
}

// grid of the tile kernel: strips of 64 rows; the 64-column tiles of a strip are cut into runs (at
// least 4 tiles each) until ~512 blocks exist
static void adell_topg_plan(int B, int T, TopgArgs* g) {
  g->strips = adell_cdiv(T, TG_TI);
  g->jtiles = adell_cdiv(T, TG_TJ);
  const long base = (long)B * g->strips;
  long splits = base >= 512 ? 1 : (512 + base - 1) / base;
  const int most = adell_cdiv(g->jtiles, 4);
  if (splits > most) splits = most;
  if (splits < 1) splits = 1;
  g->tilesPerSplit = adell_cdiv(g->jtiles, (int)splits);
  g->splits = adell_cdiv(g->jtiles, g->tilesPerSplit);
}

static int adell_topg_check(int B, int T, int C, int gamma) {
  ADELL_REQUIRE(B > 0 && T > 0 && C > 0 && gamma > 0, "top_pairs: need B, T, C, gamma > 0");
  if (gamma > TG_MAXG || (long)gamma > (long)T * T || T > TG_MAXT) {
    adell_set_error("top_pairs: gamma %d of %d tokens: 1 <= gamma <= %d, gamma <= T^2 and T <= %d "
                    "are supported", gamma, T, TG_MAXG, TG_MAXT);
    return ADELL_E_UNSUPPORTED;
  }
  return ADELL_OK;
}

extern "C" long adell_top_pairs_workspace_words(int B, int T, int gamma) {
  if (B <= 0 || T <= 0 || gamma <= 0) return 0;
  TopgArgs g = {};
  adell_topg_plan(B, T, &g);
  return (long)B * g.strips * g.splits * gamma;
}

static int adell_topg_run(TopgArgs g, void* workspace, long workspace_words, int* pairs,
                          float* dist2, hipStream_t st) {
  adell_topg_plan(g.B, g.T, &g);
  const long per_item = (long)g.strips * g.splits * g.gamma;
  ADELL_REQUIRE(workspace && workspace_words >= (long)g.B * per_item,
                "top_pairs: workspace of adell_top_pairs_workspace_words() 8-byte words required");
  ADELL_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "top_pairs: workspace not 8-byte aligned");
  const long blocks = (long)g.B * g.strips * g.splits;
  ADELL_REQUIRE(blocks <= 0x7fffffffL, "top_pairs: too many blocks");
  g.cand = static_cast<tg_u64*>(workspace);
  hipLaunchKernelGGL(adell_topg_tile_kernel, dim3((unsigned)blocks), dim3(TG_NT), 0, st, g);
  ADELL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(adell_topg_merge_kernel, dim3((unsigned)g.B), dim3(TG_NT), 0, st,
                     (const tg_u64*)g.cand, per_item, g.T, g.gamma, pairs, dist2);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_top_pairs(const float* a, const float* b, int B, int T, int C, int gamma,
                               void* workspace, long workspace_words, int* pairs, float* dist2,
                               void* stream) {
  const int rc = adell_topg_check(B, T, C, gamma);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(a && b && pairs, "top_pairs: null pointer");
  TopgArgs g = {};
  g.a = a; g.b = b; g.B = B; g.T = T; g.C = C; g.gamma = gamma;
  return adell_topg_run(g, workspace, workspace_words, pairs, dist2, (hipStream_t)stream);
}

extern "C" int adell_top_pairs_boxes(const float* box1, const float* box2, int B, int ndim,
                                     const int* dims, int gamma, void* workspace,
                                     long workspace_words, int* pairs, float* dist2, void* stream) {
  ADELL_REQUIRE(box1 && box2 && dims && pairs, "top_pairs_boxes: null pointer");
  ADELL_REQUIRE(ndim == 2 || ndim == 3, "top_pairs_boxes: 2 or 3 spatial dimensions");
  long T = 1;
  for (int d = 0; d < ndim; ++d) {
    ADELL_REQUIRE(dims[d] > 0, "top_pairs_boxes: bad grid");
    T *= dims[d];
    if (T > TG_MAXT) T = TG_MAXT + 1L;
  }
  const int rc = adell_topg_check(B, (int)T, ndim, gamma);
  if (rc != ADELL_OK) return rc;
  TopgArgs g = {};
  g.box1 = box1; g.box2 = box2; g.B = B; g.T = (int)T; g.C = ndim; g.gamma = gamma;
  g.ndim = ndim;
  for (int d = 0; d < 3; ++d) g.dims[d] = d < ndim ? dims[d] : 1;
  return adell_topg_run(g, workspace, workspace_words, pairs, dist2, (hipStream_t)stream);
}

// out[b gamma + k][c] = x[b][pairs[b][k][col]][c]
__global__ __launch_bounds__(256) void adell_gather_rows_kernel(const float* __restrict__ x,
                                                                const int* __restrict__ pairs,
                                                                int col, int B, int T, int C,
                                                                int gamma, float* __restrict__ out) {
  const long total = (long)B * gamma * C;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int c = (int)(e % C);
    const long rk = e / C;   // b gamma + k
    const int b = (int)(rk / gamma);
    const int row = pairs[rk * 2 + col];
    out[e] = (row >= 0 && row < T) ? x[((size_t)b * T + row) * C + c] : 0.f;
  }
}

// dx[b][pairs[b][k][col]][c] += dout[b gamma + k][c], k in order; dx is zero on entry
__global__ __launch_bounds__(256) void adell_gather_rows_bwd_kernel(const float* __restrict__ dout,
                                                                    const int* __restrict__ pairs,
                                                                    int col, int B, int T, int C,
                                                                    int gamma, float* __restrict__ dx) {
  const long total = (long)B * C;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
    const int c = (int)(e % C);
    const int b = (int)(e / C);
    for (int k = 0; k < gamma; ++k) {
      const long rk = (long)b * gamma + k;
      const int row = pairs[rk * 2 + col];
      if (row < 0 || row >= T) continue;
      float* p = dx + ((size_t)b * T + row) * C + c;
      *p = *p + dout[rk * C + c];
    }
  }
}

static int adell_gather_rows_check(int col, int B, int T, int C, int gamma) {
  ADELL_REQUIRE(B > 0 && T > 0 && C > 0 && gamma > 0 && (col == 0 || col == 1),
                "gather_rows: need B, T, C, gamma > 0 and col in {0, 1}");
  return ADELL_OK;
}

extern "C" int adell_gather_rows_fwd(const float* x, const int* pairs, int col, int B, int T, int C,
                                     int gamma, float* out, void* stream) {
  const int rc = adell_gather_rows_check(col, B, T, C, gamma);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && pairs && out, "gather_rows_fwd: null pointer");
  long blocks = ((long)B * gamma * C + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adell_gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, x, pairs, col, B, T, C, gamma, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_gather_rows_bwd(const float* dout, const int* pairs, int col, int B, int T,
                                     int C, int gamma, float* dx, void* stream) {
  const int rc = adell_gather_rows_check(col, B, T, C, gamma);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(dout && pairs && dx, "gather_rows_bwd: null pointer");
  ADELL_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)B * T * C * sizeof(float), (hipStream_t)stream));
  long blocks = ((long)B * C + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adell_gather_rows_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, dout, pairs, col, B, T, C, gamma, dx);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
