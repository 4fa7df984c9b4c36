// Segmentation metrics on the device (HBM-bound): the confusion counts behind the reference's
// torchmetrics dicts (adell_mri/modules/segmentation/pl.py:100-187, fed from training_step,
// validation_step and test_step :403, :467, :513):
//   * a partial pass: one int32 row of counts per block (tp / fp / fn of every class, plus the
//     out-of-range-prediction and bad-target flags) over the network output [B][C][S] and the
//     target [B][S];
//   * a one-block finalize: the rows folded into int64 and ADDED into up to 8 metric states at once
//     (one pass serves every metric of a dict);
//   * a one-block compute: IoU / precision / F-beta / Dice of a state, in fp64, as an fp32 scalar.
// No host synchronisation, no allocation, no float atomics: the grid depends only on B * S and
// integer sums are exact, so the same tensors give the same counts whatever the schedule.
#include "common.h"

#define ADELL_SM_THREADS 256
#define ADELL_SM_BLOCKS 2048    // partial rows at most (the grid cap of the partial pass)
#define ADELL_SM_MAX_C 32
#define ADELL_SM_MAX_STATES 8

enum { ADELL_SM_T_F32 = 0, ADELL_SM_T_U8 = 1, ADELL_SM_T_I64 = 2 };

// Partial row width in int32: binary [tpA fpA fnA tpB fpB fnB oor bad]; C classes [tp fp fn] x C,
// then [oor bad].
static inline int adell_sm_row(int C) { return C == 1 ? 8 : 3 * C + 2; }

static unsigned adell_sm_grid(long n) {
  // ~4 chunks of 4 voxels per lane below the cap: the grid depends on n = B * S alone
  long blocks = ((n >> 2) + ADELL_SM_THREADS * 4 - 1) / (ADELL_SM_THREADS * 4);
  if (blocks < 1) blocks = 1;
  if (blocks > ADELL_SM_BLOCKS) blocks = ADELL_SM_BLOCKS;
  return (unsigned)blocks;
}

// integer sibling of adell_wave_sum (common.h)
__device__ __forceinline__ int adell_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The target class: rint (round-half-even, torch.round) of a float target; -1 outside [0, C)
// (NaN included).
__device__ __forceinline__ int adell_sm_tclass(float t, int C) {
  const float r = rintf(t);
  return (r >= 0.0f && r < (float)C) ? (int)r : -1;
}
__device__ __forceinline__ int adell_sm_tclass(uint8_t t, int C) { return (int)t < C ? (int)t : -1; }
__device__ __forceinline__ int adell_sm_tclass(int64_t t, int C) {
  return (t >= 0 && t < (int64_t)C) ? (int)t : -1;
}

// four consecutive targets, 16 B per load (4 B for uint8)
__device__ __forceinline__ void adell_sm_load4(const float* t, long i, int C, int* tc) {
  const f32x4 v = reinterpret_cast<const f32x4*>(t)[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) tc[k] = adell_sm_tclass(v[k], C);
}
__device__ __forceinline__ void adell_sm_load4(const uint8_t* t, long i, int C, int* tc) {
  const uint32_t v = reinterpret_cast<const uint32_t*>(t)[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) tc[k] = adell_sm_tclass((uint8_t)(v >> (8 * k)), C);
}
__device__ __forceinline__ void adell_sm_load4(const int64_t* t, long i, int C, int* tc) {
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  const i64x2 a = reinterpret_cast<const i64x2*>(t)[2 * i], b = reinterpret_cast<const i64x2*>(t)[2 * i + 1];
  tc[0] = adell_sm_tclass((int64_t)a[0], C);
  tc[1] = adell_sm_tclass((int64_t)a[1], C);
  tc[2] = adell_sm_tclass((int64_t)b[0], C);
  tc[3] = adell_sm_tclass((int64_t)b[1], C);
}

struct AdellSmBin {
  int c[6];     // tpA fpA fnA (p > 0.5) tpB fpB fnB (sigmoid(p) > 0.5)
  int oor, bad;
};

__device__ __forceinline__ void adell_sm_bin_voxel(AdellSmBin& a, float p, int tc) {
  a.bad |= tc < 0;
  a.oor |= !(p >= 0.0f && p <= 1.0f);                // NaN counts as out of range
  const int t = tc == 1;
  const int ma = p > 0.5f;
  // the fp32 sigmoid (IEEE expf and division) > 0.5; for |p| >= 1e-3 it lies 2.5e-4 or more away
  // from 0.5, so the test is p > 0 there (NaN included: negative either way), and the ~40-instruction
  // sigmoid, which made this pass VALU-bound, runs only for the few voxels near 0
  int mb = p > 0.0f;
  if (fabsf(p) < 1e-3f) mb = 1.0f / (1.0f + expf(-p)) > 0.5f;
  a.c[0] += ma & t;
  a.c[1] += ma & (1 - t);
  a.c[2] += (1 - ma) & t;
  a.c[3] += mb & t;
  a.c[4] += mb & (1 - t);
  a.c[5] += (1 - mb) & t;
}

// Binary (C = 1): pred and target are flat over the n = B * S voxels. VEC: 16-byte-aligned pred
// (and target at its own width): f32x4 chunks, block 0 takes the scalar tail; otherwise scalar.
template <typename T, bool VEC>
__global__ __launch_bounds__(ADELL_SM_THREADS) void adell_seg_confusion_partials_bin_kernel(
    const float* __restrict__ pred, const T* __restrict__ target, long n, int* __restrict__ rows) {
  AdellSmBin a = {{0, 0, 0, 0, 0, 0}, 0, 0};
  const long stride = (long)gridDim.x * ADELL_SM_THREADS;
  if (VEC) {
    const long n4 = n >> 2;
    const f32x4* p4 = reinterpret_cast<const f32x4*>(pred);
    long i = (long)blockIdx.x * ADELL_SM_THREADS + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {      // two chunks in flight per lane
      const f32x4 p = p4[i], q = p4[i + stride];
      int tc[4], uc[4];
      adell_sm_load4(target, i, 2, tc);
      adell_sm_load4(target, i + stride, 2, uc);
#pragma unroll
      for (int k = 0; k < 4; ++k) adell_sm_bin_voxel(a, p[k], tc[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) adell_sm_bin_voxel(a, q[k], uc[k]);
    }
    if (i < n4) {
      const f32x4 p = p4[i];
      int tc[4];
      adell_sm_load4(target, i, 2, tc);
#pragma unroll
      for (int k = 0; k < 4; ++k) adell_sm_bin_voxel(a, p[k], tc[k]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
      const long v = (n4 << 2) + threadIdx.x;
      adell_sm_bin_voxel(a, pred[v], adell_sm_tclass(target[v], 2));
    }
  } else {
    for (long v = (long)blockIdx.x * ADELL_SM_THREADS + threadIdx.x; v < n; v += stride)
      adell_sm_bin_voxel(a, pred[v], adell_sm_tclass(target[v], 2));
  }
  __shared__ int wave_part[ADELL_SM_THREADS / 64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int s = adell_wave_sum_i(a.c[k]);
    if (lane == 0) wave_part[wave][k] = s;
  }
  const int oor = __any(a.oor), bad = __any(a.bad);
  if (lane == 0) {
    wave_part[wave][6] = oor;
    wave_part[wave][7] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < ADELL_SM_THREADS / 64; ++w)
      s = threadIdx.x < 6 ? s + wave_part[w][threadIdx.x] : (s | wave_part[w][threadIdx.x]);
    rows[(size_t)blockIdx.x * 8 + threadIdx.x] = s;
  }
}

// Multi-class (2 <= C <= 32): the predicted class is torch.argmax over the C channels (first
// maximal index, a NaN wins). Counting uses wave ballots: lane c of every wave owns class c's
// (predicted, target, tp) counters, so the loops are wave-uniform (lanes past the end carry the
// class -1, which matches nothing).
//   cl = 0: pred [B][C][S] (NCDHW / NCHW); VEC additionally needs S % 4 == 0 and 16-byte-aligned
//           pred and target: 4 voxels per lane per step, f32x4 per channel.
//   cl = 1: pred [B][S][C] (channels-last memory): one voxel per lane per step.
__device__ __forceinline__ void adell_sm_argmax_step(float v, int c, float& best, int& idx) {
  if (v > best || (v != v && best == best)) {
    best = v;
    idx = c;
  }
}

__device__ __forceinline__ void adell_sm_count(int pc, int tc, int C, int lane, int& np, int& nt,
                                               int& ntp) {
  for (int c = 0; c < C; ++c) {
    const unsigned long long mp = __ballot(pc == c), mt = __ballot(tc == c);
    if (lane == c) {
      np += __popcll(mp);
      nt += __popcll(mt);
      ntp += __popcll(mp & mt);
    }
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(ADELL_SM_THREADS) void adell_seg_confusion_partials_mc_kernel(
    const float* __restrict__ pred, const T* __restrict__ target, long S, int C, long n, int cl,
    int* __restrict__ rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long stride = (long)gridDim.x * ADELL_SM_THREADS;
  int np = 0, nt = 0, ntp = 0, bad = 0;
  // wave-uniform loop: the wave's first item decides
  const long first = (long)blockIdx.x * ADELL_SM_THREADS + (wave << 6);
  if (VEC) {
    const long n4 = n >> 2;
    for (long w0 = first; w0 < n4; w0 += stride) {
      const long i = w0 + lane;
      int pc[4] = {-1, -1, -1, -1}, tc[4] = {-1, -1, -1, -1};
      if (i < n4) {
        const long v0 = i << 2, b = v0 / S;
        const float* p = pred + v0 + b * (long)(C - 1) * S;    // b * C * S + (v0 - b * S)
        f32x4 best = *reinterpret_cast<const f32x4*>(p);
        int idx[4] = {0, 0, 0, 0};
        for (int c = 1; c < C; ++c) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(p + (long)c * S);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float bk = best[k];
            adell_sm_argmax_step(v[k], c, bk, idx[k]);
            best[k] = bk;
          }
        }
        adell_sm_load4(target, i, C, tc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pc[k] = idx[k];
          bad |= tc[k] < 0;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) adell_sm_count(pc[k], tc[k], C, lane, np, nt, ntp);
    }
  } else {
    for (long w0 = first; w0 < n; w0 += stride) {
      const long v = w0 + lane;
      int pc = -1, tc = -1;
      if (v < n) {
        const float* p;
        long cs;
        if (cl) {
          p = pred + v * C;
          cs = 1;
        } else {
          const long b = v / S;
          p = pred + v + b * (long)(C - 1) * S;
          cs = S;
        }
        float best = p[0];
        pc = 0;
        for (int c = 1; c < C; ++c) adell_sm_argmax_step(p[(long)c * cs], c, best, pc);
        tc = adell_sm_tclass(target[v], C);
        bad |= tc < 0;
      }
      adell_sm_count(pc, tc, C, lane, np, nt, ntp);
    }
  }
  __shared__ int wave_part[ADELL_SM_THREADS / 64][ADELL_SM_MAX_C][3];
  __shared__ int wave_bad[ADELL_SM_THREADS / 64];
  if (lane < ADELL_SM_MAX_C) {
    wave_part[wave][lane][0] = np;
    wave_part[wave][lane][1] = nt;
    wave_part[wave][lane][2] = ntp;
  }
  const int any_bad = __any(bad);
  if (lane == 0) wave_bad[wave] = any_bad;
  __syncthreads();
  const int W = 3 * C + 2;
  int* row = rows + (size_t)blockIdx.x * W;
  if (threadIdx.x < C) {
    int p = 0, t = 0, tp = 0;
#pragma unroll
    for (int w = 0; w < ADELL_SM_THREADS / 64; ++w) {
      p += wave_part[w][threadIdx.x][0];
      t += wave_part[w][threadIdx.x][1];
      tp += wave_part[w][threadIdx.x][2];
    }
    row[3 * threadIdx.x + 0] = tp;
    row[3 * threadIdx.x + 1] = p - tp;    // fp
    row[3 * threadIdx.x + 2] = t - tp;    // fn
  } else if (threadIdx.x == ADELL_SM_MAX_C) {
    int b = 0;
#pragma unroll
    for (int w = 0; w < ADELL_SM_THREADS / 64; ++w) b |= wave_bad[w];
    row[3 * C] = 0;                        // no out-of-range rule for C > 1
    row[3 * C + 1] = b;
  }
}

struct AdellSmStates {
  long long* s[ADELL_SM_MAX_STATES];
};

// One block: column sums of the G partial rows in int64, then state[k][j] += count[j] for every
// state (binary: mask B's counts when any prediction of THIS update lies outside [0, 1]) and the
// bad-target flag ORed into state[k][3C].
__global__ __launch_bounds__(ADELL_SM_THREADS) void adell_seg_confusion_finalize_kernel(
    const int* __restrict__ rows, int G, int C, AdellSmStates states, int nstates) {
  const int W = C == 1 ? 8 : 3 * C + 2;
  const int per = ADELL_SM_THREADS / W;          // threads per column (>= 2: W <= 98)
  const int col = threadIdx.x / per, sub = threadIdx.x % per;
  long long acc = 0;
  if (col < W) {
    const int* c = rows + col;
    int r = sub;
    for (; r + 3 * per < G; r += 4 * per)     // four loads in flight per thread
      acc += (long long)c[(size_t)r * W] + (long long)c[(size_t)(r + per) * W] +
             (long long)c[(size_t)(r + 2 * per) * W] + (long long)c[(size_t)(r + 3 * per) * W];
    for (; r < G; r += per) acc += c[(size_t)r * W];
  }
  __shared__ long long part[ADELL_SM_THREADS];
  __shared__ long long tot[3 * ADELL_SM_MAX_C + 2];
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < W) {
    long long s = 0;
    for (int k = 0; k < per; ++k) s += part[threadIdx.x * per + k];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
  const int nc = 3 * C;
  const int off = (C == 1 && tot[6] > 0) ? 3 : 0;   // binary: the sigmoid mask for this update
  const long long bad = tot[C == 1 ? 7 : nc + 1] > 0;
  for (int k = 0; k < nstates; ++k) {
    long long* st = states.s[k];
    if (threadIdx.x < nc) st[threadIdx.x] += tot[off + threadIdx.x];
    else if (threadIdx.x == nc) st[nc] |= bad;
  }
}

// One thread: the metric of a state, fp64 from the int64 counts, averaged over the classes with
// tp + fp + fn > 0 (0 when there are none; a zero denominator gives 0).
__global__ void adell_seg_metric_compute_kernel(const long long* __restrict__ st, int C, int kind,
                                                double beta, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  int classes = 0;
  const double b2 = beta * beta;
  for (int c = 0; c < C; ++c) {
    const double tp = (double)st[3 * c], fp = (double)st[3 * c + 1], fn = (double)st[3 * c + 2];
    if (st[3 * c] + st[3 * c + 1] + st[3 * c + 2] == 0) continue;
    double num, den;
    switch (kind) {
      case ADELL_SEG_IOU: num = tp; den = tp + fp + fn; break;
      case ADELL_SEG_PRECISION: num = tp; den = tp + fp; break;
      case ADELL_SEG_FBETA: num = (1.0 + b2) * tp; den = (1.0 + b2) * tp + b2 * fn + fp; break;
      default: num = 2.0 * tp; den = 2.0 * tp + fp + fn; break;
    }
    sum += den > 0.0 ? num / den : 0.0;
    ++classes;
  }
  out[0] = (float)(classes ? sum / classes : 0.0);
}

extern "C" long adell_seg_confusion_workspace(long n, int C) {
  if (n < 1 || C < 1 || C > ADELL_SM_MAX_C) return 0;
  return (long)adell_sm_grid(n) * adell_sm_row(C) * (long)sizeof(int);
}

template <typename T>
static void adell_sm_launch(const float* pred, const T* target, long B, int C, long S, int cl,
                            int* rows, unsigned grid, hipStream_t stream) {
  const long n = B * S;
  const bool pa = (((uintptr_t)pred) & 15) == 0;
  const bool ta = (((uintptr_t)target) & (sizeof(T) == 1 ? 3 : 15)) == 0;
  if (C == 1) {
    if (pa && ta)
      hipLaunchKernelGGL((adell_seg_confusion_partials_bin_kernel<T, true>), dim3(grid),
                         dim3(ADELL_SM_THREADS), 0, stream, pred, target, n, rows);
    else
      hipLaunchKernelGGL((adell_seg_confusion_partials_bin_kernel<T, false>), dim3(grid),
                         dim3(ADELL_SM_THREADS), 0, stream, pred, target, n, rows);
  } else if (!cl && pa && ta && (S & 3) == 0) {
    hipLaunchKernelGGL((adell_seg_confusion_partials_mc_kernel<T, true>), dim3(grid),
                       dim3(ADELL_SM_THREADS), 0, stream, pred, target, S, C, n, cl, rows);
  } else {
    hipLaunchKernelGGL((adell_seg_confusion_partials_mc_kernel<T, false>), dim3(grid),
                       dim3(ADELL_SM_THREADS), 0, stream, pred, target, S, C, n, cl, rows);
  }
}

extern "C" int adell_seg_confusion_update(const float* pred, const void* target, int target_type,
                                          long B, int C, long S, int channels_last, int* workspace,
                                          long workspace_bytes, long long* const* states,
                                          int nstates, void* stream) {
  ADELL_REQUIRE(pred && target && workspace && states && B > 0 && S > 0,
                "seg_confusion_update: bad arguments");
  ADELL_REQUIRE(C >= 1 && C <= ADELL_SM_MAX_C, "seg_confusion_update: %d classes (1..%d supported)",
                C, ADELL_SM_MAX_C);
  ADELL_REQUIRE(nstates >= 1 && nstates <= ADELL_SM_MAX_STATES,
                "seg_confusion_update: %d states (1..%d per update)", nstates, ADELL_SM_MAX_STATES);
  ADELL_REQUIRE(target_type >= ADELL_SM_T_F32 && target_type <= ADELL_SM_T_I64,
                "seg_confusion_update: unknown target type %d", target_type);
  const long n = B * S;
  ADELL_REQUIRE(workspace_bytes >= adell_seg_confusion_workspace(n, C),
                "seg_confusion_update: workspace of %ld bytes, %ld needed", workspace_bytes,
                adell_seg_confusion_workspace(n, C));
  AdellSmStates st;
  for (int k = 0; k < ADELL_SM_MAX_STATES; ++k) st.s[k] = k < nstates ? states[k] : nullptr;
  for (int k = 0; k < nstates; ++k) ADELL_REQUIRE(st.s[k], "seg_confusion_update: null state %d", k);
  const unsigned grid = adell_sm_grid(n);
  const hipStream_t s = (hipStream_t)stream;
  const int cl = channels_last && C > 1;
  switch (target_type) {
    case ADELL_SM_T_F32: adell_sm_launch(pred, (const float*)target, B, C, S, cl, workspace, grid, s); break;
    case ADELL_SM_T_U8: adell_sm_launch(pred, (const uint8_t*)target, B, C, S, cl, workspace, grid, s); break;
    default: adell_sm_launch(pred, (const int64_t*)target, B, C, S, cl, workspace, grid, s); break;
  }
  ADELL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(adell_seg_confusion_finalize_kernel, dim3(1), dim3(ADELL_SM_THREADS), 0, s,
                     workspace, (int)grid, C, st, nstates);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

extern "C" int adell_seg_metric_compute(const long long* state, int C, int kind, float beta,
                                        float* out, void* stream) {
  ADELL_REQUIRE(state && out, "seg_metric_compute: bad arguments");
  ADELL_REQUIRE(C >= 1 && C <= ADELL_SM_MAX_C, "seg_metric_compute: %d classes (1..%d supported)",
                C, ADELL_SM_MAX_C);
  ADELL_REQUIRE(kind >= ADELL_SEG_IOU && kind <= ADELL_SEG_DICE, "seg_metric_compute: unknown kind %d",
                kind);
  ADELL_REQUIRE(beta > 0.0f, "seg_metric_compute: beta must be positive");
  hipLaunchKernelGGL(adell_seg_metric_compute_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     state, C, kind, (double)beta, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}
