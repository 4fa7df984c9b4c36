// Kernels of the batch-ensemble layers (adell_mri/modules/layers/batch_ensemble.py, arXiv:2002.06715):
// n rank-1 members scale the channels before and after one shared body. House rules of diffusion.hip
// and ensemble.hip: fp32 in and out, dense inputs, no float atomics, every sum in a fixed order in
// fp64 -- two runs are bit-identical. Activations are [B][V][C] (NDHWC memory, as the conv kernels
// leave them; V = 1 for rows [B][C]); tables are [n][C]. Nothing is gathered, stacked or expanded.
//   * be_expand, one launch: out[k B + b] = x[b] * table[row] * scale for k < K, x read once. With
//     item indices (K = 1) row = idx[b]: the training scale. Without, row = m0 + k: the members
//     [m0, m0 + K) of the eval mean side by side in one batch (K = 1, m0 = 0: one row broadcast). A
//     NULL table is all ones (the scale alone). An index outside [0, n) is never used as one: the item
//     comes out NaN.
//   * be_members_sum, one launch: out[b] = acc[b] + sum_k table[m0 + k] y[k B + b], ONE fma chain
//     in member order from acc (or 0), times `scale` at the end. The chain's value between two calls
//     is an fp32 tensor, so the result does not depend on how the members were cut into calls.
//   * be_tgrad, two launches: part[k B + b][tile][c] = the fp64 sum over the tile's voxels of
//     p[k B + b] q[b] (and, for the training scale, dx[b] = p[b] table[idx[b]] in the same pass:
//     its whole backward), then the fold: dtable[m][c] = scale * the sum of the rows of part that belong
//     to member m -- items in ascending order, tiles in a fixed order. A member without rows gets an
//     exact 0.
#include "common.h"

constexpr int BE_NT = 256;
constexpr int BE_NW = BE_NT / 64;
constexpr int BE_MAX_TILES = 1024;      // tiles per item of the table-gradient pass
constexpr int BE_TGRAD_BLOCKS = 2048;   // ... and about this many blocks in all: the fold walks every tile

// the table row of item b's copy k, or -1 (index out of range)
__device__ __forceinline__ int be_row(const int* __restrict__ idx, int b, int m0, int k, int n) {
  const int r = idx != nullptr ? idx[b] : m0 + k;
  return (unsigned)r < (unsigned)n ? r : -1;
}

template <int VEC>
__global__ __launch_bounds__(BE_NT) void adell_be_expand_kernel(
    const float* __restrict__ x, const float* __restrict__ table, const int* __restrict__ idx, int m0,
    int K, int n, float scale, float* __restrict__ out, long VC, int C) {
  const int b = blockIdx.y, B = gridDim.y;
  const float* xb = x + (size_t)b * VC;
  const long step = (long)gridDim.x * BE_NT * VEC;
  long i = ((long)blockIdx.x * BE_NT + threadIdx.x) * VEC;
  int c = (int)(i % C);
  const int cstep = (int)(step % C);
  const float nan = __int_as_float(0x7fc00000);
  for (; i < VC; i += step) {
    float xv[VEC];
    if (VEC == 4) {
      const float4 v = *reinterpret_cast<const float4*>(xb + i);
      xv[0] = v.x, xv[1 % VEC] = v.y, xv[2 % VEC] = v.z, xv[3 % VEC] = v.w;
    } else {
      xv[0] = xb[i];
    }
    for (int k = 0; k < K; ++k) {
      const int row = be_row(idx, b, m0, k, n);
      float t[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        t[e] = row < 0 ? nan : (table != nullptr ? table[(size_t)row * C + c + e] * scale : scale);
      float* ob = out + ((size_t)k * B + b) * VC + i;
      if (VEC == 4) {
        *reinterpret_cast<float4*>(ob) =
            make_float4(xv[0] * t[0], xv[1 % VEC] * t[1 % VEC], xv[2 % VEC] * t[2 % VEC],
                        xv[3 % VEC] * t[3 % VEC]);
      } else {
        ob[0] = xv[0] * t[0];
      }
    }
    c += cstep;
    if (c >= C) c -= C;
  }
}

template <int VEC>
__global__ __launch_bounds__(BE_NT) void adell_be_members_sum_kernel(
    const float* __restrict__ y, const float* __restrict__ table, const float* __restrict__ acc, int m0,
    int K, float scale, int scaled, float* __restrict__ out, long VC, int C) {
  const int b = blockIdx.y, B = gridDim.y;
  const long step = (long)gridDim.x * BE_NT * VEC;
  long i = ((long)blockIdx.x * BE_NT + threadIdx.x) * VEC;
  int c = (int)(i % C);
  const int cstep = (int)(step % C);
  const size_t base = (size_t)b * VC;
  for (; i < VC; i += step) {
    float s[VEC];
    if (acc != nullptr) {
      if (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(acc + base + i);
        s[0] = a.x, s[1 % VEC] = a.y, s[2 % VEC] = a.z, s[3 % VEC] = a.w;
      } else {
        s[0] = acc[base + i];
      }
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] = 0.f;
    }
    for (int k = 0; k < K; ++k) {
      const float* yb = y + ((size_t)k * B + b) * VC + i;
      const float* tr = table + (size_t)(m0 + k) * C + c;
      if (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4*>(yb);
        const float4 t = *reinterpret_cast<const float4*>(tr);
        s[0] = fmaf(t.x, v.x, s[0]);
        s[1 % VEC] = fmaf(t.y, v.y, s[1 % VEC]);
        s[2 % VEC] = fmaf(t.z, v.z, s[2 % VEC]);
        s[3 % VEC] = fmaf(t.w, v.w, s[3 % VEC]);
      } else {
        s[0] = fmaf(tr[0], yb[0], s[0]);
      }
    }
    if (scaled) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] *= scale;
    }
    if (VEC == 4) {
      *reinterpret_cast<float4*>(out + base + i) = make_float4(s[0], s[1 % VEC], s[2 % VEC], s[3 % VEC]);
    } else {
      out[base + i] = s[0];
    }
    c += cstep;
    if (c >= C) c -= C;
  }
}

// Block (tile, k B + b): voxels [tile vpt, (tile + 1) vpt) of row k B + b of p against item b of q.
// Thread (r, cl) = (tid / CGb, tid % CGb) owns column group cl (VEC channels) of every R-th voxel;
// R = 256 / CGb rows (threads past R CGb idle); the CG = C / VEC column groups are walked CGb at a
// time. part[row][tile][c]: per thread in voxel order, then over the thread rows in order.
template <int VEC>
__global__ __launch_bounds__(BE_NT) void adell_be_tgrad_kernel(
    const float* __restrict__ p, const float* __restrict__ q, const float* __restrict__ table,
    const int* __restrict__ idx, int n, int B, float* __restrict__ dx, double* __restrict__ part, long V,
    int C, long vpt, int CGb, int R) {
  __shared__ double sred[BE_NT * VEC];
  const int row = blockIdx.y, b = row % B, tile = blockIdx.x, tid = threadIdx.x;
  const long v0 = (long)tile * vpt;
  const long v1 = v0 + vpt < V ? v0 + vpt : V;
  const size_t pbase = (size_t)row * V * C, qbase = (size_t)b * V * C;
  const int CG = C / VEC, r = tid / CGb, cl = tid - r * CGb;
  const int trow = dx != nullptr ? be_row(idx, b, 0, 0, n) : 0;
  const float nan = __int_as_float(0x7fc00000);
  for (int cg0 = 0; cg0 < CG; cg0 += CGb) {
    const int cg = cg0 + cl;
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    if (r < R && cg < CG) {
      const int c = cg * VEC;
      float t[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        t[e] = dx == nullptr ? 0.f : (trow < 0 ? nan : table[(size_t)trow * C + c + e]);
      for (long v = v0 + r; v < v1; v += R) {
        const size_t o = (size_t)v * C + c;
        if (VEC == 4) {
          const float4 pv = *reinterpret_cast<const float4*>(p + pbase + o);
          const float4 qv = *reinterpret_cast<const float4*>(q + qbase + o);
          if (dx != nullptr)
            *reinterpret_cast<float4*>(dx + pbase + o) =
                make_float4(pv.x * t[0], pv.y * t[1 % VEC], pv.z * t[2 % VEC], pv.w * t[3 % VEC]);
          acc[0] += (double)pv.x * (double)qv.x;
          acc[1 % VEC] += (double)pv.y * (double)qv.y;
          acc[2 % VEC] += (double)pv.z * (double)qv.z;
          acc[3 % VEC] += (double)pv.w * (double)qv.w;
        } else {
          const float pv = p[pbase + o];
          if (dx != nullptr) dx[pbase + o] = pv * t[0];
          acc[0] += (double)pv * (double)q[qbase + o];
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
        part[((size_t)row * gridDim.x + tile) * C + cg * VEC + e] = tot;
      }
    }
    __syncthreads();
  }
}

// Block (64 channels, member m): 64 channels x 4 tile lanes. Member m owns the rows of part
//   K == 0 (the training scale): of every item b with idx[b] == m (no idx: member 0 owns them all);
//   K > 0  (members side by side): of copy k = m - m0, every item; none outside [m0, m0 + K).
// Items in ascending order, each lane a fixed share of the tiles, the lanes added in order.
__global__ __launch_bounds__(BE_NT) void adell_be_tgrad_fold_kernel(
    const double* __restrict__ part, const int* __restrict__ idx, int B, int tiles, int C, int m0, int K,
    double scale, float* __restrict__ dtable) {
  __shared__ double sh[BE_NW][64];
  const int m = blockIdx.y, cl = threadIdx.x & 63, vl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int k = m - m0;
  double acc = 0.0;
  if (c < C && (K == 0 || (k >= 0 && k < K))) {
    for (int b = 0; b < B; ++b) {
      if (K == 0 && (idx != nullptr ? idx[b] : 0) != m) continue;
      const double* pr = part + ((size_t)(K == 0 ? 0 : k) * B + b) * tiles * C + c;
      for (int t = vl; t < tiles; t += BE_NW) acc += pr[(size_t)t * C];
    }
  }
  sh[vl][cl] = acc;
  __syncthreads();
  if (vl != 0 || c >= C) return;
  acc = 0.0;
#pragma unroll
  for (int w = 0; w < BE_NW; ++w) acc += sh[w][cl];
  dtable[(size_t)m * C + c] = (float)(scale * acc);
}

// ---- host side -----------------------------------------------------------------------------------------
static int be_args(const char* what, int B, long V, int C, int K) {
  ADELL_REQUIRE(B >= 1 && V >= 1 && C >= 1 && K >= 1, "%s: bad arguments (B %d, V %ld, C %d, K %d)", what,
                B, V, C, K);
  ADELL_REQUIRE((long)B * K <= 65535, "%s: %d items x %d members, at most 65535 rows go in one launch",
                what, B, K);
  ADELL_REQUIRE(V <= 0x7fffffffL * 16 / C, "%s: item of %ld x %d elements is too large", what, V, C);
  return ADELL_OK;
}

// blocks along an item of VC elements: ~4 vectors per thread, the grid capped near 2048 blocks
static unsigned be_blocks(long VC, bool vec, int B) {
  long blocks = (VC / (vec ? 4 : 1) + BE_NT * 4 - 1) / (BE_NT * 4);
  const long cap = 2048 / B > 1 ? 2048 / B : 1;
  if (blocks > cap) blocks = cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int adell_be_expand(const float* x, const float* table, const int* idx, int m0, int K, int n,
                               float scale, float* out, int B, long V, int C, void* stream) {
  const int rc = be_args("be_expand", B, V, C, K);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(x && out && n >= 1, "be_expand: null pointer or an empty table");
  ADELL_REQUIRE(idx == nullptr || (K == 1 && table != nullptr),
                "be_expand: item indices pick one row of a table per item (K = 1)");
  ADELL_REQUIRE(idx != nullptr || (m0 >= 0 && m0 + K <= n), "be_expand: members [%d, %d) of %d", m0,
                m0 + K, n);
  const long VC = V * C;
  const bool vec = C % 4 == 0 && adell_aligned16(x) && adell_aligned16(out) &&
                   (table == nullptr || adell_aligned16(table));
  const dim3 grid(be_blocks(VC, vec, B), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    return adell_launch<adell_be_expand_kernel<4>>(grid, dim3(BE_NT), 0, st, x, table, idx, m0, K, n,
                                                   scale, out, VC, C);
  return adell_launch<adell_be_expand_kernel<1>>(grid, dim3(BE_NT), 0, st, x, table, idx, m0, K, n, scale,
                                                 out, VC, C);
}

extern "C" int adell_be_members_sum(const float* y, const float* table, const float* acc, int m0, int K,
                                    int n, float scale, int scaled, float* out, int B, long V, int C,
                                    void* stream) {
  const int rc = be_args("be_members_sum", B, V, C, K);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(y && table && out, "be_members_sum: null pointer");
  ADELL_REQUIRE(m0 >= 0 && m0 + K <= n, "be_members_sum: members [%d, %d) of %d", m0, m0 + K, n);
  const long VC = V * C;
  const bool vec = C % 4 == 0 && adell_aligned16(y) && adell_aligned16(out) && adell_aligned16(table) &&
                   (acc == nullptr || adell_aligned16(acc));
  const dim3 grid(be_blocks(VC, vec, B), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    return adell_launch<adell_be_members_sum_kernel<4>>(grid, dim3(BE_NT), 0, st, y, table, acc, m0, K,
                                                        scale, scaled ? 1 : 0, out, VC, C);
  return adell_launch<adell_be_members_sum_kernel<1>>(grid, dim3(BE_NT), 0, st, y, table, acc, m0, K,
                                                      scale, scaled ? 1 : 0, out, VC, C);
}

// rows of the pass's thread grid and tiles per item: >= 8 voxels per thread, at most BE_MAX_TILES,
// and no more than make about BE_TGRAD_BLOCKS blocks over the `rows` items (a few blocks per CU
// fill the chip; every further tile is a row of partial sums the fold has to walk)
static void be_tgrad_plan(int rows, long V, int C, bool vec, int* CGb, int* R, int* tiles) {
  const int CG = C / (vec ? 4 : 1);
  *CGb = CG < BE_NT ? CG : BE_NT;
  *R = BE_NT / *CGb;
  long t = (V + (long)*R * 8 - 1) / ((long)*R * 8);
  const long cap = BE_TGRAD_BLOCKS / rows > 1 ? BE_TGRAD_BLOCKS / rows : 1;
  if (t > cap) t = cap;
  if (t > BE_MAX_TILES) t = BE_MAX_TILES;
  if (t < 1) t = 1;
  *tiles = (int)t;
}

extern "C" long adell_be_tgrad_workspace_doubles(int B, long V, int C, int K) {
  if (B <= 0 || V <= 0 || C <= 0 || K <= 0) return ADELL_E_BADARG;
  int CGb, R, tiles;
  // (the scalar plan never has fewer tiles than the vector one: size for it)
  be_tgrad_plan(B * K, V, C, false, &CGb, &R, &tiles);
  return (long)B * K * tiles * C;
}

extern "C" int adell_be_tgrad(const float* p, const float* q, const float* table, const int* idx, int m0,
                              int K, int n, float scale, float* dx, float* dtable, double* part, int B,
                              long V, int C, void* stream) {
  const int copies = K > 0 ? K : 1;
  const int rc = be_args("be_tgrad", B, V, C, copies);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(p && q && n >= 1 && (dx || dtable) && (dtable == nullptr) == (part == nullptr),
                "be_tgrad: null pointer, or a table gradient without its workspace");
  ADELL_REQUIRE(K >= 0 && (K == 0 || (m0 >= 0 && m0 + K <= n)), "be_tgrad: members [%d, %d) of %d", m0,
                m0 + K, n);
  ADELL_REQUIRE(dx == nullptr || (K == 0 && table != nullptr),
                "be_tgrad: dx comes with the training scale (K = 0) and its table");
  ADELL_REQUIRE(idx == nullptr || K == 0, "be_tgrad: item indices belong to the training scale (K = 0)");
  const bool vec = C % 4 == 0 && adell_aligned16(p) && adell_aligned16(q) &&
                   (dx == nullptr || (adell_aligned16(dx) && adell_aligned16(table)));
  int CGb, R, tiles;
  be_tgrad_plan(B * copies, V, C, vec, &CGb, &R, &tiles);
  const long vpt = (V + tiles - 1) / tiles;
  const dim3 grid((unsigned)tiles, (unsigned)(B * copies));
  hipStream_t st = (hipStream_t)stream;
  const int rc1 = vec ? adell_launch<adell_be_tgrad_kernel<4>>(grid, dim3(BE_NT), 0, st, p, q, table, idx,
                                                               n, B, dx, part, V, C, vpt, CGb, R)
                      : adell_launch<adell_be_tgrad_kernel<1>>(grid, dim3(BE_NT), 0, st, p, q, table, idx,
                                                               n, B, dx, part, V, C, vpt, CGb, R);
  if (rc1 != ADELL_OK || dtable == nullptr) return rc1;
  ADELL_REQUIRE(n <= 65535, "be_tgrad: %d members", n);
  return adell_launch<adell_be_tgrad_fold_kernel>(dim3((unsigned)adell_cdiv(C, 64), (unsigned)n),
                                                  dim3(BE_NT), 0, st, (const double*)part, idx, B, tiles,
                                                  C, m0, K, (double)scale, dtable);
}
