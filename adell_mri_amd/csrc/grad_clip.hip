// Gradient-norm clipping and gradient accumulation over the flat fp32 gradient buffers of the
// fused optimisers (HBM-bound):
//   * torch.nn.utils.clip_grad_norm_(norm_type 2 or inf), which Lightning's Trainer calls for
//     gradient_clip_val (entrypoints/segmentation/train.py:807, ssl/train_3d.py:354): a
//     per-run partial pass, a one-block finalize that leaves the clip coefficient on the device,
//     and an in-place scale that reads it (no host synchronisation anywhere);
//   * the accumulate_grad_batches fold (train.py:811, ssl/train_3d.py:355): the per-parameter
//     gradients of a micro-batch ADDED into the flat slots.
// Bitwise reproducible: fixed grids that depend only on the element count, fixed-order sums, no
// float atomics.
#include "common.h"

#define ADELL_GN_BLOCKS 2048    // partial slots per run (the grid cap of the partial pass)
#define ADELL_GN_THREADS 256

// max that propagates NaN from either side (fmaxf drops it; torch's inf-norm does not)
__device__ __forceinline__ double adell_nanmax(double m, double a) {
  return (m >= a || m != m) ? m : a;
}

__device__ __forceinline__ double adell_gn_acc(double acc, float v, int norm_inf) {
  const double a = (double)v;
  return norm_inf ? adell_nanmax(acc, fabs(a)) : fma(a, a, acc);
}

// One partial per block: sum of squares (fp64) or max |g| of the block's grid-strided f32x4
// chunks; block 0 also takes the scalar tail. Blocks past the grid leave 0 in their slots (the
// neutral element of both reductions), so the finalize always reads ADELL_GN_BLOCKS per run.
__global__ __launch_bounds__(ADELL_GN_THREADS) void adell_grad_norm_partials_kernel(
    const float* __restrict__ g, long n, int norm_inf, double* __restrict__ partials) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * ADELL_GN_THREADS;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  double acc = 0.0;
  long i = (long)blockIdx.x * ADELL_GN_THREADS + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {      // two loads in flight per lane
    const f32x4 a = g4[i], b = g4[i + stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = adell_gn_acc(acc, a[k], norm_inf);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = adell_gn_acc(acc, b[k], norm_inf);
  }
  if (i < n4) {
    const f32x4 a = g4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = adell_gn_acc(acc, a[k], norm_inf);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc = adell_gn_acc(acc, g[(n4 << 2) + threadIdx.x], norm_inf);

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(acc, o, 64);
    acc = norm_inf ? adell_nanmax(acc, other) : acc + other;
  }
  __shared__ double wave_part[ADELL_GN_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = wave_part[0];
#pragma unroll
    for (int w = 1; w < ADELL_GN_THREADS / 64; ++w)
      r = norm_inf ? adell_nanmax(r, wave_part[w]) : r + wave_part[w];
    partials[blockIdx.x] = r;
    for (int s = blockIdx.x + gridDim.x; s < ADELL_GN_BLOCKS; s += gridDim.x) partials[s] = 0.0;
  }
}

// One block: the runs x ADELL_GN_BLOCKS partials in a fixed order, then torch's
//   total = ||s g||,  coef = clamp(max_norm / (total + 1e-6), max = 1)   (fp32, NaN kept).
__global__ __launch_bounds__(ADELL_GN_THREADS) void adell_grad_norm_finalize_kernel(
    const double* __restrict__ partials, long count, int norm_inf, float scale, float max_norm,
    float* __restrict__ out) {
  double acc = 0.0;
  for (long i = threadIdx.x; i < count; i += ADELL_GN_THREADS)
    acc = norm_inf ? adell_nanmax(acc, partials[i]) : acc + partials[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(acc, o, 64);
    acc = norm_inf ? adell_nanmax(acc, other) : acc + other;
  }
  __shared__ double wave_part[ADELL_GN_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = wave_part[0];
#pragma unroll
    for (int w = 1; w < ADELL_GN_THREADS / 64; ++w)
      r = norm_inf ? adell_nanmax(r, wave_part[w]) : r + wave_part[w];
    // ||s g|| = |s| ||g|| for both norms (scale > 0)
    const float total = norm_inf ? (float)((double)scale * r) : (float)((double)scale * sqrt(r));
    // torch: max_norm / (total + 1e-6) is Tensor.__rdiv__ = reciprocal(total + 1e-6) * max_norm
    float coef = (1.0f / (total + 1e-6f)) * max_norm;
    coef = coef > 1.0f ? 1.0f : coef;             // clamp(max=1): NaN stays NaN
    out[0] = total;
    out[1] = coef;
  }
}

// g *= coef (device scalar); nothing to do (and no traffic) when coef == 1 -- bit-identical to
// torch's multiply by one, and NaN never compares equal to 1.
__global__ __launch_bounds__(ADELL_GN_THREADS) void adell_grad_scale_by_kernel(
    float* __restrict__ g, long n, const float* __restrict__ coef_dev) {
  const float c = *coef_dev;
  if (c == 1.0f) return;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * ADELL_GN_THREADS;
  f32x4* g4 = reinterpret_cast<f32x4*>(g);
  for (long i = (long)blockIdx.x * ADELL_GN_THREADS + threadIdx.x; i < n4; i += stride)
    g4[i] = g4[i] * c;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[(n4 << 2) + threadIdx.x] *= c;
}

static unsigned adell_gn_grid(long n) {
  // ~4 f32x4 per lane below the cap (8 blocks per CU from 8 M elements up): the grid depends on n
  // alone (reproducible partials)
  long blocks = ((n >> 2) + ADELL_GN_THREADS * 4 - 1) / (ADELL_GN_THREADS * 4);
  if (blocks < 1) blocks = 1;
  if (blocks > ADELL_GN_BLOCKS) blocks = ADELL_GN_BLOCKS;
  return (unsigned)blocks;
}

extern "C" long adell_grad_norm_workspace(int runs) {
  if (runs < 1) return 0;
  return (long)runs * ADELL_GN_BLOCKS * (long)sizeof(double);
}

extern "C" int adell_grad_norm_partials(const float* g, long n, int norm_inf, double* partials,
                                        int run, void* stream) {
  ADELL_REQUIRE(g && partials && n > 0 && run >= 0, "grad_norm_partials: bad arguments");
  ADELL_REQUIRE((((uintptr_t)g) & 15) == 0, "grad_norm_partials: the buffer must be 16-byte aligned");
  hipLaunchKernelGGL(adell_grad_norm_partials_kernel, dim3(adell_gn_grid(n)), dim3(ADELL_GN_THREADS),
                     0, (hipStream_t)stream, g, n, norm_inf ? 1 : 0,
                     partials + (size_t)run * ADELL_GN_BLOCKS);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_grad_norm_finalize(const double* partials, int runs, int norm_inf, float scale,
                                        float max_norm, float* out, void* stream) {
  ADELL_REQUIRE(partials && out && runs > 0, "grad_norm_finalize: bad arguments");
  ADELL_REQUIRE(scale > 0.0f, "grad_norm_finalize: scale must be positive");
  hipLaunchKernelGGL(adell_grad_norm_finalize_kernel, dim3(1), dim3(ADELL_GN_THREADS), 0,
                     (hipStream_t)stream, partials, (long)runs * ADELL_GN_BLOCKS, norm_inf ? 1 : 0,
                     scale, max_norm, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_grad_scale_by(float* g, long n, const float* coef_dev, void* stream) {
  ADELL_REQUIRE(g && coef_dev && n > 0, "grad_scale_by: bad arguments");
  ADELL_REQUIRE((((uintptr_t)g) & 15) == 0, "grad_scale_by: the buffer must be 16-byte aligned");
  hipLaunchKernelGGL(adell_grad_scale_by_kernel, dim3(adell_gn_grid(n)), dim3(ADELL_GN_THREADS), 0,
                     (hipStream_t)stream, g, n, coef_dev);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// dst[off_r + i] += src_r[i]: adell_multi_copy's table (csrc/layout.hip), accumulating.
__global__ __launch_bounds__(256) void adell_multi_accumulate_kernel(const long* __restrict__ table,
                                                                     float* __restrict__ dst) {
  const long* row = table + (size_t)blockIdx.x * 3;
  const float* src = reinterpret_cast<const float*>(row[0]);
  float* d = dst + row[1];
  const long n = row[2];
  if (((((uintptr_t)src) | ((uintptr_t)d)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256)
      reinterpret_cast<f32x4*>(d)[i] += reinterpret_cast<const f32x4*>(src)[i];
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) d[i] += src[i];
  } else {
    for (long i = threadIdx.x; i < n; i += 256) d[i] += src[i];
  }
}

extern "C" int adell_multi_accumulate(const long* table, int rows, float* dst, void* stream) {
  ADELL_REQUIRE(table && dst && rows > 0, "multi_accumulate: bad arguments");
  hipLaunchKernelGGL(adell_multi_accumulate_kernel, dim3((unsigned)rows), dim3(256), 0,
                     (hipStream_t)stream, table, dst);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
