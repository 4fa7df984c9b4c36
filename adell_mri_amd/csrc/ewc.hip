// Elastic-weight-consolidation penalty of the reference's continual-learning package
// (continuous_learning/regularization.py:38-45):
//   penalty = sum_k || p_k - p0_k ||_p     over the selected parameter tensors k,
// value and gradient, over ANY number of tensors in three launches (HBM-bound for p = 1 and 2):
//   * partials: one block per chunk of ADELL_EWC_CHUNK elements -> sum |p - p0|^p in fp64;
//   * finalize: one block -> norm_k = S_k^(1/p) per tensor (fp32, kept for the backward pass) and
//     total = sum_k norm_k (fp64 in tensor order, stored as one fp32);
//   * gradient: one block per chunk -> g = c sgn(d) |d|^(p-1) / norm_k^(p-1), WRITTEN to or ADDED
//     into base[offset + i] (a fresh flat buffer for autograd / the flat gradient slots of a fused
//     optimiser).
// The chunks are rows of a DEVICE table the host builds and uploads once (5 longs per row: parameter
// pointer, anchor pointer, element count <= ADELL_EWC_CHUNK, tensor index, destination offset in
// elements); the chunks of a tensor are consecutive rows, and
// tensor_first[k] .. tensor_first[k + 1] are the rows of tensor k.
// The difference d is taken in fp32: that is what the reference's `param - anchor` does, and it is
// correctly rounded. p == 1 and p == 2 are instances of their own without pow; any other finite
// p >= 1 takes the generic instance, which calls the fp64 pow once per element and is therefore
// bound by the vector ALU, not by HBM -- accepted: the reference's default is 2.
// Bitwise reproducible: fixed grids (one block per chunk), fixed-order sums, no float atomics.
#include <math.h>

#include "common.h"

#define ADELL_EWC_CHUNK 8192
#define ADELL_EWC_THREADS 256
#define ADELL_EWC_FIN_THREADS 1024
#define ADELL_EWC_COLS 5

enum { EWC_P1 = 1, EWC_P2 = 2, EWC_PGEN = 0 };

template <int MODE>
__device__ __forceinline__ double adell_ewc_acc(double acc, float a, float b, double p) {
  const float d = a - b;                           // fp32, as the reference subtracts
  if (MODE == EWC_P1) return acc + (double)fabsf(d);
  if (MODE == EWC_P2) return fma((double)d, (double)d, acc);
  return acc + pow((double)fabsf(d), p);           // pow(0, p) = 0 for p >= 1
}

// Block sum of `acc` in a fixed order (shuffle tree, then the waves in turn); valid in thread 0.
template <int THREADS>
__device__ __forceinline__ double adell_ewc_block_sum(double acc, double* wave_part) {
  acc = adell_wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    r = wave_part[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) r += wave_part[w];
  }
  return r;
}

template <int MODE>
__global__ __launch_bounds__(ADELL_EWC_THREADS) void adell_ewc_partials_kernel(
    const long* __restrict__ table, double p, double* __restrict__ partials) {
  const long* row = table + (size_t)blockIdx.x * ADELL_EWC_COLS;
  const float* a = reinterpret_cast<const float*>(row[0]);
  const float* b = reinterpret_cast<const float*>(row[1]);
  const long n = row[2];
  double acc = 0.0;
  if (((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += ADELL_EWC_THREADS) {
      const f32x4 x = reinterpret_cast<const f32x4*>(a)[i];
      const f32x4 y = reinterpret_cast<const f32x4*>(b)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = adell_ewc_acc<MODE>(acc, x[k], y[k], p);
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += ADELL_EWC_THREADS)
      acc = adell_ewc_acc<MODE>(acc, a[i], b[i], p);
  } else {
    for (long i = threadIdx.x; i < n; i += ADELL_EWC_THREADS)
      acc = adell_ewc_acc<MODE>(acc, a[i], b[i], p);
  }
  __shared__ double wave_part[ADELL_EWC_THREADS / 64];
  const double r = adell_ewc_block_sum<ADELL_EWC_THREADS>(acc, wave_part);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// One block. Each wave takes every 16th tensor: its lanes fold the tensor's chunk partials (lane l
// the rows first + l, first + l + 64, ... in table order, then the shuffle tree), lane 0 takes the
// root. The norms stay in fp64 behind the partials (norm64) for the total, which wave 0 sums the
// same way in tensor order.
__global__ __launch_bounds__(ADELL_EWC_FIN_THREADS) void adell_ewc_finalize_kernel(
    const long* __restrict__ tensor_first, int tensors, double p, const double* __restrict__ partials,
    double* __restrict__ norm64, float* __restrict__ norms, float* __restrict__ total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < tensors; k += ADELL_EWC_FIN_THREADS / 64) {
    const long lo = tensor_first[k], hi = tensor_first[k + 1];
    double acc = 0.0;
    for (long i = lo + lane; i < hi; i += 64) acc += partials[i];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) {
      const double nrm = p == 1.0 ? acc : (p == 2.0 ? sqrt(acc) : pow(acc, 1.0 / p));
      norm64[k] = nrm;
      norms[k] = (float)nrm;
    }
  }
  __syncthreads();      // the block's own global writes are visible to it behind the barrier
  if (wave == 0) {
    double acc = 0.0;
    for (int k = lane; k < tensors; k += 64) acc += norm64[k];
    acc = adell_wave_sum_d(acc);
    if (lane == 0) total[0] = (float)acc;
  }
}

// The per-element factor of the gradient: g = scale * d (p = 2), scale * sgn(d) (p = 1),
// scale * sgn(d) |d|^(p-1) (generic, fp64), with d == 0 -> exactly 0 for every p.
template <int MODE>
__device__ __forceinline__ float adell_ewc_g(float a, float b, double scale, double pm1) {
  const float d = a - b;
  if (MODE == EWC_P2) return d * (float)scale;
  if (d == 0.0f) return 0.0f;
  if (MODE == EWC_P1) return d > 0.0f ? (float)scale : -(float)scale;
  const double v = scale * pow((double)fabsf(d), pm1);
  return (float)(d > 0.0f ? v : -v);
}

template <int MODE, int ADD>
__global__ __launch_bounds__(ADELL_EWC_THREADS) void adell_ewc_grad_kernel(
    const long* __restrict__ table, double p, const float* __restrict__ norms, float c_host,
    const float* __restrict__ c_dev, float* __restrict__ base) {
  // g is rounded to fp32 BEFORE it is added (no fused multiply-add into the slot): the add mode leaves
  // the bits the write mode followed by an fp32 addition leaves, so the two routes differ only by the
  // order in which a slot's contributions are added
#pragma clang fp contract(off)
  const long* row = table + (size_t)blockIdx.x * ADELL_EWC_COLS;
  const float* a = reinterpret_cast<const float*>(row[0]);
  const float* b = reinterpret_cast<const float*>(row[1]);
  const long n = row[2];
  float* dst = base + row[4];
  const float nrm = norms[row[3]];
  const float c = c_dev ? c_host * c_dev[0] : c_host;
  // torch's masked forms: a tensor that sits on its anchor (norm 0: every tensor at the first step
  // of a fine-tuning run) has gradient exactly 0, not 0 / 0
  double scale = 0.0;
  if (nrm != 0.0f) {
    if (MODE == EWC_P1) scale = (double)c;
    else if (MODE == EWC_P2) scale = (double)(c / nrm);
    else scale = (double)c / pow((double)nrm, p - 1.0);
  }
  const bool zero = nrm == 0.0f;
  if (zero && ADD) return;
  const double pm1 = p - 1.0;
  if (((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)dst)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += ADELL_EWC_THREADS) {
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (!zero) {
        const f32x4 x = reinterpret_cast<const f32x4*>(a)[i];
        const f32x4 y = reinterpret_cast<const f32x4*>(b)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = adell_ewc_g<MODE>(x[k], y[k], scale, pm1);
      }
      if (ADD) reinterpret_cast<f32x4*>(dst)[i] += g;
      else reinterpret_cast<f32x4*>(dst)[i] = g;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += ADELL_EWC_THREADS) {
      const float g = zero ? 0.0f : adell_ewc_g<MODE>(a[i], b[i], scale, pm1);
      if (ADD) dst[i] += g;
      else dst[i] = g;
    }
  } else {
    for (long i = threadIdx.x; i < n; i += ADELL_EWC_THREADS) {
      const float g = zero ? 0.0f : adell_ewc_g<MODE>(a[i], b[i], scale, pm1);
      if (ADD) dst[i] += g;
      else dst[i] = g;
    }
  }
}

static bool adell_ewc_p_ok(double p) { return isfinite(p) && p >= 1.0; }
static int adell_ewc_mode(double p) { return p == 1.0 ? EWC_P1 : (p == 2.0 ? EWC_P2 : EWC_PGEN); }

extern "C" int adell_ewc_chunk(void) { return ADELL_EWC_CHUNK; }

extern "C" long adell_ewc_workspace_doubles(int chunks, int tensors) {
  if (chunks < 1 || tensors < 1 || tensors > chunks) return 0;
  return (long)chunks + (long)tensors;
}

extern "C" int adell_ewc_partials(const long* table, int chunks, double p, double* workspace,
                                  void* stream) {
  ADELL_REQUIRE(table && workspace && chunks > 0, "ewc_partials: bad arguments");
  ADELL_REQUIRE(adell_ewc_p_ok(p), "ewc_partials: p must be a finite number >= 1, got %g", p);
  const dim3 grid((unsigned)chunks), block(ADELL_EWC_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  switch (adell_ewc_mode(p)) {
    case EWC_P1: hipLaunchKernelGGL(adell_ewc_partials_kernel<EWC_P1>, grid, block, 0, st, table, p, workspace); break;
    case EWC_P2: hipLaunchKernelGGL(adell_ewc_partials_kernel<EWC_P2>, grid, block, 0, st, table, p, workspace); break;
    default: hipLaunchKernelGGL(adell_ewc_partials_kernel<EWC_PGEN>, grid, block, 0, st, table, p, workspace); break;
  }
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_ewc_finalize(const long* tensor_first, int tensors, int chunks, double p,
                                  double* workspace, float* norms, float* total, void* stream) {
  ADELL_REQUIRE(tensor_first && workspace && norms && total && chunks > 0 && tensors > 0 &&
                    tensors <= chunks,
                "ewc_finalize: bad arguments");
  ADELL_REQUIRE(adell_ewc_p_ok(p), "ewc_finalize: p must be a finite number >= 1, got %g", p);
  hipLaunchKernelGGL(adell_ewc_finalize_kernel, dim3(1), dim3(ADELL_EWC_FIN_THREADS), 0,
                     (hipStream_t)stream, tensor_first, tensors, p, workspace, workspace + chunks,
                     norms, total);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

template <int ADD>
static void adell_ewc_grad_launch(const long* table, int chunks, double p, const float* norms,
                                  float c, const float* c_dev, float* base, hipStream_t st) {
  const dim3 grid((unsigned)chunks), block(ADELL_EWC_THREADS);
  switch (adell_ewc_mode(p)) {
    case EWC_P1: hipLaunchKernelGGL((adell_ewc_grad_kernel<EWC_P1, ADD>), grid, block, 0, st, table, p, norms, c, c_dev, base); break;
    case EWC_P2: hipLaunchKernelGGL((adell_ewc_grad_kernel<EWC_P2, ADD>), grid, block, 0, st, table, p, norms, c, c_dev, base); break;
    default: hipLaunchKernelGGL((adell_ewc_grad_kernel<EWC_PGEN, ADD>), grid, block, 0, st, table, p, norms, c, c_dev, base); break;
  }
}

extern "C" int adell_ewc_grad(const long* table, int chunks, double p, const float* norms, float c,
                              const float* c_dev, int add, float* base, void* stream) {
  ADELL_REQUIRE(table && norms && base && chunks > 0, "ewc_grad: bad arguments");
  ADELL_REQUIRE(adell_ewc_p_ok(p), "ewc_grad: p must be a finite number >= 1, got %g", p);
  if (add) adell_ewc_grad_launch<1>(table, chunks, p, norms, c, c_dev, base, (hipStream_t)stream);
  else adell_ewc_grad_launch<0>(table, chunks, p, norms, c, c_dev, base, (hipStream_t)stream);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
