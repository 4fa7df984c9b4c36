// Connected components on the device and the PI-CAI lesion tables built on them (integer,
// HBM-bound, atomic-heavy). They replace the host route of the reference's validation
// (adell_mri/modules/segmentation/pl.py:446-452, 503-509, 609-652 -> picai_eval/eval.py:51-251):
// scipy.ndimage.label with the full 3x3x3 structure on every detection map and target, then an
// O(N_gt * N_cand * V) loop of full-volume masks for the overlaps.
//
// Labelling, bit-identical to ndimage.label(x, np.ones((3, 3, 3))) on a batch [NV][D][H][W]:
//   1. local: one block per 8 x 16 x 32 tile; union-find in LDS over the 13 backward neighbours,
//      root = the set's minimum index; writes the global parent array P (volume-linear index of
//      the tile root, -1 for background);
//   2. merge: global union across tile faces, edges and corners by atomicMin on P (Playne and
//      Hawick). Parents only ever decrease and every value P ever held is an ancestor, so a stale
//      plain load is a valid (older) ancestor: correctness rests on the values the atomics return;
//   3. flatten (after the kernel boundary): P[v] = root; root flags counted per 4096-voxel chunk;
//   4. one block per volume: exclusive scan of the chunk counts, N = the total;
//   5. roots get 1 + their rank in raster order. A root is its component's first voxel in raster
//      order, which is exactly scipy's numbering;
//   6. every other voxel takes its root's label; optionally the voxel count of every component and
//      the maximum of the detection map over it.
// Component statistics and pair intersections are summed per thread along runs, then per block in
// an LDS hash, and only then added to global memory: a component covering half a volume costs one
// global atomic per block, not per voxel. Integer atomics only: the same input gives the same bits.
//
// PI-CAI tables (per case b of B): the labels of the thresholded prediction (volume b) and of the
// truncated target (volume B + b) in one labelling launch sequence; a global hash of the
// (GT lesion, candidate) intersections; the pairs with 10 * inter >= union (every pair whose IoU can
// reach min_overlap >= 0.1; at most 10 * min(N_gt, N_cand)); and one packed int32 record per case.
//
// Lesion candidates (the reference's extract_lesion_candidates.py, at the end of this file): the same
// labelling sequence with a fourth foreground predicate, x >= thr and x != 0 with a threshold per
// volume in device memory, and an optional per-volume flag that makes the blocks of a finished
// volume exit at once (the rounds of the dynamic mode).
#include "common.h"

#include <vector>

#define CC_THREADS 256
#define CC_TZ 8
#define CC_TY 16
#define CC_TX 32
#define CC_TILE (CC_TZ * CC_TY * CC_TX)
#define CC_PER 16                           // consecutive voxels per thread in the linear passes
#define CC_CHUNK (CC_THREADS * CC_PER)      // voxels per block in the linear passes
#define CC_HS 4096                          // LDS hash slots of the aggregating passes

enum { CC_MODE_GT = 0, CC_MODE_NONZERO = 1, CC_MODE_TRUNC = 2, CC_MODE_GE = 3 };

struct CcSrc {
  const float* x0;
  const float* x1;
  long n0;             // volumes from x0; the rest from x1
  int mode0, mode1;
  float thr;
  const float* thr_v;  // CC_MODE_GE: the threshold of every volume (device memory); null: thr
  const int* act;      // null, or [NV]: the blocks of a volume with act[vol] == 0 exit at once
};

__device__ __forceinline__ bool cc_fg(float v, int mode, float thr) {
  if (mode == CC_MODE_GT) return v > thr;
  if (mode == CC_MODE_NONZERO) return v != 0.0f;     // NaN is foreground, as for numpy
  if (mode == CC_MODE_GE) return !(v < thr) && v != 0.0f;   // x[x < thr] = 0, then x != 0
  return !(v > -1.0f && v < 1.0f);                   // astype(int32) != 0 (NaN, +-inf included)
}

// the detection value of a foreground voxel: 1 for a thresholded map (x > thr is boolean)
__device__ __forceinline__ float cc_det(float v, int mode) { return mode == CC_MODE_GT ? 1.0f : v; }

// float -> unsigned int with the same order (0 is below every float: "no value")
__device__ __forceinline__ unsigned cc_ord(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cc_unord(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// 13 backward neighbours (lexicographically negative offsets) of the 3x3x3 structure
__constant__ signed char cc_off[13][3] = {
    {-1, -1, -1}, {-1, -1, 0}, {-1, -1, 1}, {-1, 0, -1}, {-1, 0, 0}, {-1, 0, 1}, {-1, 1, -1},
    {-1, 1, 0},   {-1, 1, 1},  {0, -1, -1}, {0, -1, 0},  {0, -1, 1}, {0, 0, -1}};

// ---- union-find: parents decrease monotonically; links only by atomicMin on a root ----------
__device__ __forceinline__ int cc_find_lds(int* p, int x) {
  int y;
  while ((y = __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = y;
  return x;
}
__device__ __forceinline__ void cc_union_lds(int* p, int a, int b) {
  while (true) {
    a = cc_find_lds(p, a);
    b = cc_find_lds(p, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + b, a);
    if (old == b) return;
    b = old;
  }
}
// Path halving: x's parent is lowered to its grandparent z by atomicMin. x is no root (its parent
// was read as y != x, and a non-root never becomes one), z is an ancestor of x and z < y, so the
// entry stays a valid, smaller parent and parents keep decreasing monotonically. Without it, a
// component spanning every tile leaves chains of tile roots hundreds long behind the merge.
__device__ __forceinline__ int cc_find_g(int* p, int x) {
  while (true) {
    const int y = __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (y == x) return x;
    const int z = __hip_atomic_load(p + y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (z == y) return y;
    atomicMin(p + x, z);
    x = z;
  }
}
__device__ __forceinline__ void cc_union_g(int* p, int a, int b) {
  while (true) {
    a = cc_find_g(p, a);
    b = cc_find_g(p, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + b, a);    // device scope: the value returned is the truth
    if (old == b) return;
    b = old;
  }
}

struct CcGeom {
  int D, H, W;
  int ty, tx;          // tiles along y and x
  long V;              // voxels per volume
};

// 1. tile-local union-find
__global__ __launch_bounds__(CC_THREADS) void adell_cc_local_kernel(CcSrc src, CcGeom g, int* P) {
  __shared__ int par[CC_TILE];
  const long vol = blockIdx.y;
  if (src.act && !src.act[vol]) return;
  const int tz = blockIdx.x / (g.ty * g.tx), rem = blockIdx.x % (g.ty * g.tx);
  const int z0 = tz * CC_TZ, y0 = (rem / g.tx) * CC_TY, x0 = (rem % g.tx) * CC_TX;
  const float* x = vol < src.n0 ? src.x0 + vol * g.V : src.x1 + (vol - src.n0) * g.V;
  const int mode = vol < src.n0 ? src.mode0 : src.mode1;
  const float thr = src.thr_v ? src.thr_v[vol] : src.thr;
  for (int t = threadIdx.x; t < CC_TILE; t += CC_THREADS) {
    const int lx = t % CC_TX, ly = (t / CC_TX) % CC_TY, lz = t / (CC_TX * CC_TY);
    const int zz = z0 + lz, yy = y0 + ly, xx = x0 + lx;
    bool fg = false;
    if (zz < g.D && yy < g.H && xx < g.W)
      fg = cc_fg(x[((long)zz * g.H + yy) * g.W + xx], mode, thr);
    par[t] = fg ? t : -1;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CC_TILE; t += CC_THREADS) {
    if (par[t] < 0) continue;     // foreground status never changes
    const int lx = t % CC_TX, ly = (t / CC_TX) % CC_TY, lz = t / (CC_TX * CC_TY);
    for (int k = 0; k < 13; ++k) {
      const int nz = lz + cc_off[k][0], ny = ly + cc_off[k][1], nx = lx + cc_off[k][2];
      if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;
      const int n = (nz * CC_TY + ny) * CC_TX + nx;
      if (par[n] >= 0) cc_union_lds(par, t, n);
    }
  }
  __syncthreads();
  int* Pv = P + vol * g.V;
  for (int t = threadIdx.x; t < CC_TILE; t += CC_THREADS) {
    const int lx = t % CC_TX, ly = (t / CC_TX) % CC_TY, lz = t / (CC_TX * CC_TY);
    const int zz = z0 + lz, yy = y0 + ly, xx = x0 + lx;
    if (zz >= g.D || yy >= g.H || xx >= g.W) continue;
    int r = par[t];
    if (r >= 0) {
      r = cc_find_lds(par, t);
      const int rx = r % CC_TX, ry = (r / CC_TX) % CC_TY, rz = r / (CC_TX * CC_TY);
      r = (int)(((long)(z0 + rz) * g.H + (y0 + ry)) * g.W + (x0 + rx));
    }
    Pv[((long)zz * g.H + yy) * g.W + xx] = r;
  }
}

// 2. unions across tile boundaries: only voxels on a tile face have a backward neighbour in
// another tile (z = 0; y = 0 or TY - 1; x = 0 or TX - 1, the high faces through +1 offsets)
__global__ __launch_bounds__(CC_THREADS) void adell_cc_merge_kernel(CcGeom g, int* P,
                                                                   const int* act) {
  const long vol = blockIdx.y;
  if (act && !act[vol]) return;
  const int tz = blockIdx.x / (g.ty * g.tx), rem = blockIdx.x % (g.ty * g.tx);
  const int z0 = tz * CC_TZ, y0 = (rem / g.tx) * CC_TY, x0 = (rem % g.tx) * CC_TX;
  int* Pv = P + vol * g.V;
  for (int t = threadIdx.x; t < CC_TILE; t += CC_THREADS) {
    const int lx = t % CC_TX, ly = (t / CC_TX) % CC_TY, lz = t / (CC_TX * CC_TY);
    if (lz != 0 && ly != 0 && ly != CC_TY - 1 && lx != 0 && lx != CC_TX - 1) continue;
    const int zz = z0 + lz, yy = y0 + ly, xx = x0 + lx;
    if (zz >= g.D || yy >= g.H || xx >= g.W) continue;
    const int v = (int)(((long)zz * g.H + yy) * g.W + xx);
    if (Pv[v] < 0) continue;
    int last = -1;    // ancestor of the previous neighbour joined: an equal one is in its set already
    for (int k = 0; k < 13; ++k) {
      const int nz = lz + cc_off[k][0], ny = ly + cc_off[k][1], nx = lx + cc_off[k][2];
      if (nz >= 0 && ny >= 0 && ny < CC_TY && nx >= 0 && nx < CC_TX) continue;   // same tile
      const int gz = zz + cc_off[k][0], gy = yy + cc_off[k][1], gx = xx + cc_off[k][2];
      if (gz < 0 || gy < 0 || gy >= g.H || gx < 0 || gx >= g.W) continue;
      const int n = (int)(((long)gz * g.H + gy) * g.W + gx);
      const int pn = __hip_atomic_load(Pv + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (pn < 0 || pn == last) continue;
      cc_union_g(Pv, v, pn);     // pn is an ancestor of n: same set
      last = pn;
    }
  }
}

__device__ __forceinline__ int cc_block_excl_scan(int v, int* total) {
  __shared__ int wsum[CC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < CC_THREADS / 64; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// 3. flatten + roots per chunk (thread: CC_PER consecutive voxels)
__global__ __launch_bounds__(CC_THREADS) void adell_cc_flatten_kernel(CcGeom g, int* P, int* blk,
                                                                     int nb, const int* act) {
  const long vol = blockIdx.y;
  if (act && !act[vol]) return;
  int* Pv = P + vol * g.V;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  int roots = 0;
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= g.V) break;
    const int p = Pv[v];
    if (p < 0) continue;
    if (p == (int)v) {
      ++roots;
      continue;
    }
    Pv[v] = cc_find_g(Pv, p);
  }
  int total;
  cc_block_excl_scan(roots, &total);
  if (threadIdx.x == 0) blk[vol * nb + blockIdx.x] = total;
}

// 4. exclusive scan of the chunk counts of each volume; n[vol] = its component count
__global__ __launch_bounds__(CC_THREADS) void adell_cc_scan_kernel(int* blk, int nb, int* n,
                                                                  const int* act) {
  if (act && !act[blockIdx.x]) return;
  int* b = blk + (long)blockIdx.x * nb;
  int carry = 0;
  for (int base = 0; base < nb; base += CC_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? b[i] : 0;
    int total;
    const int ex = cc_block_excl_scan(v, &total);
    if (i < nb) b[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) n[blockIdx.x] = carry;
}

// 5. roots: label = 1 + rank in raster order
__global__ __launch_bounds__(CC_THREADS) void adell_cc_roots_kernel(CcGeom g, const int* P,
                                                                   const int* blk, int nb, int* L,
                                                                   const int* act) {
  const long vol = blockIdx.y;
  if (act && !act[vol]) return;
  const int* Pv = P + vol * g.V;
  int* Lv = L + vol * g.V;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  int roots = 0;
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v < g.V && Pv[v] == (int)v) ++roots;
  }
  int total;
  int id = 1 + blk[vol * nb + blockIdx.x] + cc_block_excl_scan(roots, &total);
  for (int k = 0; k < CC_PER && roots; ++k) {
    const long v = v0 + k;
    if (v < g.V && Pv[v] == (int)v) {
      Lv[v] = id++;
      --roots;
    }
  }
}

// LDS hash of the aggregating passes: key 0 is empty. Returns false when the table is full (the
// caller then goes to global memory directly).
template <typename K>
__device__ __forceinline__ int cc_lds_slot(K* keys, K key) {
  unsigned s = (unsigned)(key * 0x9E3779B97F4A7C15ull >> 40) & (CC_HS - 1);
  for (int probe = 0; probe < CC_HS; ++probe) {
    const K k = atomicCAS(keys + s, (K)0, key);
    if (k == 0 || k == key) return (int)s;
    s = (s + 1) & (CC_HS - 1);
  }
  return -1;
}

struct CcStats {
  int* cnt;            // [NV][cap] voxel count of component id at [vol][id - 1]; null: none
  unsigned* cmax;      // [NV][cap] ordered detection maximum
  long cap;
};

// 6. every non-root voxel takes its root's label; component counts and maxima (optional)
__global__ __launch_bounds__(CC_THREADS) void adell_cc_relabel_kernel(CcSrc src, CcGeom g,
                                                                     const int* P, int* L,
                                                                     CcStats st) {
  __shared__ unsigned hkey[CC_HS];
  __shared__ int hcnt[CC_HS];
  __shared__ unsigned hmax[CC_HS];
  const long vol = blockIdx.y;
  if (src.act && !src.act[vol]) return;
  const int* Pv = P + vol * g.V;
  int* Lv = L + vol * g.V;
  const bool stats = st.cnt != nullptr;
  const float* x = vol < src.n0 ? src.x0 + vol * g.V : src.x1 + (vol - src.n0) * g.V;
  const int mode = vol < src.n0 ? src.mode0 : src.mode1;
  if (stats) {
    for (int s = threadIdx.x; s < CC_HS; s += CC_THREADS) {
      hkey[s] = 0;
      hcnt[s] = 0;
      hmax[s] = 0;
    }
    __syncthreads();
  }
  int* gcnt = stats ? st.cnt + vol * st.cap : nullptr;
  unsigned* gmax = stats ? st.cmax + vol * st.cap : nullptr;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  int run_id = 0, run_n = 0;
  unsigned run_max = 0;
  auto flush = [&]() {
    if (run_n == 0) return;
    const int s = cc_lds_slot(hkey, (unsigned)run_id);
    if (s >= 0) {
      atomicAdd(hcnt + s, run_n);
      atomicMax(hmax + s, run_max);
    } else {
      atomicAdd(gcnt + run_id - 1, run_n);
      atomicMax(gmax + run_id - 1, run_max);
    }
  };
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= g.V) break;
    const int p = Pv[v];
    int id = 0;
    if (p >= 0) {
      id = Lv[p];               // the root's label (written by the previous kernel)
      if (p != (int)v) Lv[v] = id;
    } else {
      Lv[v] = 0;
    }
    if (!stats || id == 0) continue;
    if (id != run_id) {
      flush();
      run_id = id;
      run_n = 0;
      run_max = 0;
    }
    ++run_n;
    const unsigned o = cc_ord(cc_det(x[v], mode));
    run_max = o > run_max ? o : run_max;
  }
  if (!stats) return;
  flush();
  __syncthreads();
  for (int s = threadIdx.x; s < CC_HS; s += CC_THREADS) {
    const unsigned id = hkey[s];
    if (!id) continue;
    atomicAdd(gcnt + id - 1, hcnt[s]);
    atomicMax(gmax + id - 1, hmax[s]);
  }
}

// ---- host: labelling ----------------------------------------------------------------------
static long cc_nb(long V) { return (V + CC_CHUNK - 1) / CC_CHUNK; }
static long cc_align(long b) { return (b + 255) & ~255L; }
static long cc_label_ws(long NV, long V) { return cc_align(NV * V * 4) + cc_align(NV * cc_nb(V) * 4); }

static CcGeom cc_geom(int D, int H, int W) {
  CcGeom g;
  g.D = D;
  g.H = H;
  g.W = W;
  g.ty = adell_cdiv(H, CC_TY);
  g.tx = adell_cdiv(W, CC_TX);
  g.V = (long)D * H * W;
  return g;
}

// Labels L [NV][V] and counts n [NV] of the volumes of src; P and blk live in ws.
static int cc_run(const CcSrc& src, long NV, const CcGeom& g, int* L, int* n, char* ws,
                  const CcStats& st, hipStream_t s) {
  int* P = reinterpret_cast<int*>(ws);
  int* blk = reinterpret_cast<int*>(ws + cc_align(NV * g.V * 4));
  const long nb = cc_nb(g.V);
  const long tiles = (long)adell_cdiv(g.D, CC_TZ) * g.ty * g.tx;
  ADELL_REQUIRE(tiles < (1L << 31) && nb < (1L << 31) && NV < 65536,
                "cc_label: %ld volumes of %d x %d x %d are too many to grid", NV, g.D, g.H, g.W);
  hipLaunchKernelGGL(adell_cc_local_kernel, dim3((unsigned)tiles, (unsigned)NV), dim3(CC_THREADS), 0,
                     s, src, g, P);
  ADELL_CHECK_HIP(hipGetLastError());
  if (tiles > 1) {
    hipLaunchKernelGGL(adell_cc_merge_kernel, dim3((unsigned)tiles, (unsigned)NV), dim3(CC_THREADS),
                       0, s, g, P, src.act);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(adell_cc_flatten_kernel, dim3((unsigned)nb, (unsigned)NV), dim3(CC_THREADS), 0,
                     s, g, P, blk, (int)nb, src.act);
  ADELL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(adell_cc_scan_kernel, dim3((unsigned)NV), dim3(CC_THREADS), 0, s, blk, (int)nb,
                     n, src.act);
  ADELL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(adell_cc_roots_kernel, dim3((unsigned)nb, (unsigned)NV), dim3(CC_THREADS), 0, s,
                     g, P, blk, (int)nb, L, src.act);
  ADELL_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(adell_cc_relabel_kernel, dim3((unsigned)nb, (unsigned)NV), dim3(CC_THREADS), 0,
                     s, src, g, P, L, st);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

static bool cc_shape_ok(long NV, int D, int H, int W) {
  return NV >= 1 && D >= 1 && H >= 1 && W >= 1 && (long)D * H * W < (1L << 31);
}

extern "C" long adell_cc_workspace(long NV, int D, int H, int W) {
  if (!cc_shape_ok(NV, D, H, W)) return 0;
  return cc_label_ws(NV, (long)D * H * W);
}

extern "C" int adell_cc_label(const float* x, long NV, int D, int H, int W, int use_threshold,
                              float threshold, int* labels, int* counts, void* workspace,
                              long workspace_bytes, void* stream) {
  ADELL_REQUIRE(x && labels && counts && workspace, "cc_label: bad arguments");
  ADELL_REQUIRE(cc_shape_ok(NV, D, H, W), "cc_label: bad shape %ld x %d x %d x %d (at most 2^31 - 1 "
                "voxels per volume)", NV, D, H, W);
  ADELL_REQUIRE(workspace_bytes >= adell_cc_workspace(NV, D, H, W),
                "cc_label: workspace of %ld bytes, %ld needed", workspace_bytes,
                adell_cc_workspace(NV, D, H, W));
  CcSrc src = {x, x, NV, use_threshold ? CC_MODE_GT : CC_MODE_NONZERO, 0, threshold, nullptr, nullptr};
  CcStats st = {nullptr, nullptr, 0};
  return cc_run(src, NV, cc_geom(D, H, W), labels, counts, (char*)workspace, st,
                (hipStream_t)stream);
}

// ---- PI-CAI tables ---------------------------------------------------------------------------
// The most components a 26-connected mask can hold: one per 2 x 2 x 2 block (any two voxels of a
// block touch). It also bounds the distinct (GT, candidate) intersection pairs: each pair holds at
// least one component of the AND mask.
static long pc_lattice(int D, int H, int W) {
  return (long)((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);
}
static long pc_hash_cap(long L) {
  long c = 64;
  while (c < 2 * L) c <<= 1;
  return c;
}

struct PcLayout {
  long L, Hc;
  long off_cnt, off_max, off_hkey, off_hval, off_np, zero_end, off_pairs, off_lab, off_n, off_cc,
      total;
};
static PcLayout pc_layout(long B, int D, int H, int W) {
  PcLayout l;
  const long NV = 2 * B, V = (long)D * H * W;
  l.L = pc_lattice(D, H, W);
  l.Hc = pc_hash_cap(l.L);
  long o = 0;
  l.off_cnt = o;  o += cc_align(NV * l.L * 4);
  l.off_max = o;  o += cc_align(NV * l.L * 4);
  l.off_hkey = o; o += cc_align(B * l.Hc * 8);
  l.off_hval = o; o += cc_align(B * l.Hc * 4);
  l.off_np = o;   o += cc_align(B * 4);
  l.zero_end = o;
  l.off_pairs = o; o += cc_align(B * l.L * 3 * 4);
  l.off_lab = o;  o += cc_align(NV * V * 4);
  l.off_n = o;    o += cc_align(NV * 4);
  l.off_cc = o;   o += cc_label_ws(NV, V);
  l.total = o;
  return l;
}

__device__ __forceinline__ unsigned cc_gh_slot(unsigned long long* keys, unsigned long long mask,
                                               unsigned long long key) {
  unsigned long long s = (key * 0x9E3779B97F4A7C15ull >> 17) & mask;
  while (true) {      // terminates: the table holds at least twice the distinct keys
    const unsigned long long k = atomicCAS(keys + s, 0ull, key);
    if (k == 0 || k == key) return (unsigned)s;
    s = (s + 1) & mask;
  }
}

// 7. (GT lesion, candidate) intersection counts of case b: per-thread runs, LDS hash, global hash
__global__ __launch_bounds__(CC_THREADS) void adell_picai_pairs_kernel(const int* L, long B, long V,
                                                                      unsigned long long* gkeys,
                                                                      int* gvals, long Hc) {
  __shared__ unsigned long long hkey[CC_HS];
  __shared__ int hcnt[CC_HS];
  const long b = blockIdx.y;
  const int* Lp = L + b * V;
  const int* Lg = L + (B + b) * V;
  unsigned long long* gk = gkeys + b * Hc;
  int* gv = gvals + b * Hc;
  const unsigned long long mask = (unsigned long long)Hc - 1;
  for (int s = threadIdx.x; s < CC_HS; s += CC_THREADS) {
    hkey[s] = 0;
    hcnt[s] = 0;
  }
  __syncthreads();
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  unsigned long long run = 0;
  int run_n = 0;
  auto flush = [&]() {
    if (run_n == 0) return;
    const int s = cc_lds_slot(hkey, run);
    if (s >= 0) atomicAdd(hcnt + s, run_n);
    else atomicAdd(gv + cc_gh_slot(gk, mask, run), run_n);
  };
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= V) break;
    const int c = Lp[v], g = Lg[v];
    if (c == 0 || g == 0) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)g << 32) | (unsigned)c;
    if (key != run) {
      flush();
      run = key;
      run_n = 0;
    }
    ++run_n;
  }
  flush();
  __syncthreads();
  for (int s = threadIdx.x; s < CC_HS; s += CC_THREADS)
    if (hkey[s]) atomicAdd(gv + cc_gh_slot(gk, mask, hkey[s]), hcnt[s]);
}

// 8. keep the pairs with 10 * inter >= union (IoU with the reference's 1e-8 terms >= 0.1)
__global__ __launch_bounds__(CC_THREADS) void adell_picai_filter_kernel(
    long B, const unsigned long long* gkeys, const int* gvals, long Hc, const int* cnt, long L,
    int* np, int* pairs) {
  const long b = blockIdx.y;
  for (long s = (long)blockIdx.x * CC_THREADS + threadIdx.x; s < Hc; s += (long)gridDim.x * CC_THREADS) {
    const unsigned long long key = gkeys[b * Hc + s];
    if (!key) continue;
    const int g = (int)(key >> 32), c = (int)(key & 0xffffffffu);
    const long inter = gvals[b * Hc + s];
    const long uni = (long)cnt[(B + b) * L + g - 1] + cnt[b * L + c - 1] - inter;
    if (10 * inter < uni) continue;
    const int i = atomicAdd(np + b, 1);
    if (i >= L) continue;     // cannot happen: distinct pairs <= L
    int* o = pairs + (b * L + i) * 3;
    o[0] = g;
    o[1] = c;
    o[2] = (int)inter;
  }
}

// 9. one packed record per case: [N_cand, N_gt, n_pairs, gt counts[N_gt], cand counts[N_cand],
// cand confidences[N_cand] (fp32 bits), pairs[n_pairs][3] (gt, cand, inter)]; hdr[b] = the first
// three words
__global__ __launch_bounds__(CC_THREADS) void adell_picai_pack_kernel(
    long B, const int* n, const int* cnt, const unsigned* cmax, long L, const int* np,
    const int* pairs, int* hdr, int* out) {
  const long b = blockIdx.y;
  long off = 0;
  for (long k = 0; k < b; ++k) {
    const long nc = n[k], ng = n[B + k], npk = min((long)np[k], L);
    off += 3 + ng + 2 * nc + 3 * npk;
  }
  const long nc = n[b], ng = n[B + b], npb = min((long)np[b], L);
  int* o = out + off;
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int h = threadIdx.x == 0 ? (int)nc : threadIdx.x == 1 ? (int)ng : (int)npb;
    o[threadIdx.x] = h;
    hdr[b * 3 + threadIdx.x] = h;
  }
  const long size = ng + 2 * nc + 3 * npb;
  for (long e = (long)blockIdx.x * CC_THREADS + threadIdx.x; e < size; e += (long)gridDim.x * CC_THREADS) {
    int val;
    if (e < ng) val = cnt[(B + b) * L + e];
    else if (e < ng + nc) val = cnt[b * L + (e - ng)];
    else if (e < ng + 2 * nc) val = __float_as_int(cc_unord(cmax[b * L + (e - ng - nc)]));
    else val = pairs[b * L * 3 + (e - ng - 2 * nc)];
    o[3 + e] = val;
  }
}

extern "C" long adell_picai_tables_workspace(long B, int D, int H, int W) {
  if (!cc_shape_ok(2 * B, D, H, W)) return 0;
  return pc_layout(B, D, H, W).total;
}

extern "C" long adell_picai_tables_capacity(long B, int D, int H, int W) {
  if (!cc_shape_ok(2 * B, D, H, W)) return 0;
  return B * (3 + 6 * pc_lattice(D, H, W));
}

extern "C" int adell_picai_tables(const float* pred, const float* target, long B, int D, int H,
                                  int W, int use_threshold, float threshold, int* hdr, int* out,
                                  long out_capacity, void* workspace, long workspace_bytes,
                                  void* stream) {
  ADELL_REQUIRE(pred && target && hdr && out && workspace, "picai_tables: bad arguments");
  ADELL_REQUIRE(cc_shape_ok(2 * B, D, H, W), "picai_tables: bad shape %ld x %d x %d x %d", B, D, H, W);
  const PcLayout l = pc_layout(B, D, H, W);
  ADELL_REQUIRE(workspace_bytes >= l.total, "picai_tables: workspace of %ld bytes, %ld needed",
                workspace_bytes, l.total);
  ADELL_REQUIRE(out_capacity >= adell_picai_tables_capacity(B, D, H, W),
                "picai_tables: output of %ld words, %ld needed", out_capacity,
                adell_picai_tables_capacity(B, D, H, W));
  ADELL_REQUIRE(l.L < (1L << 31) / 3, "picai_tables: volume too large");
  const hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* cnt = reinterpret_cast<int*>(ws + l.off_cnt);
  unsigned* cmax = reinterpret_cast<unsigned*>(ws + l.off_max);
  unsigned long long* hkey = reinterpret_cast<unsigned long long*>(ws + l.off_hkey);
  int* hval = reinterpret_cast<int*>(ws + l.off_hval);
  int* np = reinterpret_cast<int*>(ws + l.off_np);
  int* pairs = reinterpret_cast<int*>(ws + l.off_pairs);
  int* lab = reinterpret_cast<int*>(ws + l.off_lab);
  int* n = reinterpret_cast<int*>(ws + l.off_n);
  ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, l.zero_end, s));
  CcSrc src = {pred, target, B, use_threshold ? CC_MODE_GT : CC_MODE_NONZERO, CC_MODE_TRUNC, threshold,
               nullptr, nullptr};
  CcStats st = {cnt, cmax, l.L};
  const CcGeom g = cc_geom(D, H, W);
  const int rc = cc_run(src, 2 * B, g, lab, n, ws + l.off_cc, st, s);
  if (rc != ADELL_OK) return rc;
  const long nb = cc_nb(g.V);
  hipLaunchKernelGGL(adell_picai_pairs_kernel, dim3((unsigned)nb, (unsigned)B), dim3(CC_THREADS), 0,
                     s, lab, B, g.V, hkey, hval, l.Hc);
  ADELL_CHECK_HIP(hipGetLastError());
  long fb = l.Hc / CC_THREADS < adell_cu_count() ? l.Hc / CC_THREADS : adell_cu_count();
  if (fb < 1) fb = 1;
  hipLaunchKernelGGL(adell_picai_filter_kernel, dim3((unsigned)fb, (unsigned)B), dim3(CC_THREADS), 0,
                     s, B, hkey, hval, l.Hc, cnt, l.L, np, pairs);
  ADELL_CHECK_HIP(hipGetLastError());
  long pb = (6 * l.L + CC_THREADS - 1) / CC_THREADS;
  if (pb > 4L * adell_cu_count()) pb = 4L * adell_cu_count();
  hipLaunchKernelGGL(adell_picai_pack_kernel, dim3((unsigned)pb, (unsigned)B), dim3(CC_THREADS), 0, s,
                     B, n, cnt, cmax, l.L, np, pairs, hdr, out);
  ADELL_CHECK_HIP(hipGetLastError());
  return ADELL_OK;
}

// ---- lesion candidates -------------------------------------------------------------------------
// The Report-Guided-Annotation post-processing of the reference
// (adell_mri/modules/extract_lesion_candidates.py): a probability map becomes a detection map whose
// components carry their peak probability. Static (:19-55): label x >= thr (and != 0) with the
// sequence above, drop the components of <= min_voxels voxels, paint the others with their
// (optionally rounded) maximum. Dynamic-fast (:198-211): the same with thr = max(x) / factor, taken
// on the device. Dynamic (:58-134): rounds of [label the working copy at max / factor, choose the
// kept component of the largest painted value (ties: the lowest label), reject it if it touches a
// stored one, store it otherwise, remove it from the working copy], all volumes in lockstep; the
// kernels of a finished volume exit at once (act). Per round the host reads back act [NV] and
// nothing else.
enum { LC_STATIC = 0, LC_DYNAMIC_FAST = 1, LC_DYNAMIC = 2 };

// np.round(float64(max), d) as numpy computes it (multiply, rint, divide; for d < 0 divide, rint,
// multiply), then the float32 the reference's `all_hard_blobs += hard_blob` stores
struct LcRound {
  double scale;        // 10^|d|
  int how;             // 0: no rounding; 1: d >= 0; 2: d < 0
};
__device__ __forceinline__ float lc_paint(float m, LcRound r) {
  if (r.how == 0) return m;
  const double d = (double)m;
  return (float)(r.how == 1 ? rint(d * r.scale) / r.scale : rint(d / r.scale) * r.scale);
}

struct LcState {       // per volume, [NV] each
  unsigned* mx;        // ordered maximum of the working copy (0: not taken yet)
  float* thr;
  int* act;
  int* sel;            // the chosen component's label of this round; -1: the whole volume
  float* selconf;
  int* adj;            // the chosen component touches a stored one
  int* pend;           // a choice waits for lc_decide to count it
};

__device__ __forceinline__ unsigned lc_wave_max(unsigned m) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned u = __shfl_xor(m, o, 64);
    m = u > m ? u : m;
  }
  return m;
}

// mx[vol] = max over x[vol] (ordered bits; the caller zeroes mx)
__global__ __launch_bounds__(CC_THREADS) void adell_lc_max_kernel(const float* x, long V,
                                                                 unsigned* mx) {
  const long vol = blockIdx.y;
  const float* xv = x + vol * V;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  unsigned m = 0;
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= V) break;
    const unsigned o = cc_ord(xv[v]);
    m = o > m ? o : m;
  }
  m = lc_wave_max(m);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx + vol, m);
}

// dynamic-fast: thr = max / float32(factor), correctly rounded (:200-201)
__global__ void adell_lc_thr_kernel(long NV, const unsigned* mx, float factor, float* thr) {
  const long vol = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vol < NV) thr[vol] = __fdiv_rn(cc_unord(mx[vol]), factor);
}

// static: the kept components (more than minvox voxels) of every volume in ascending label, and
// cnt / cmax rewritten in place as (kept, painted value bits) for lc_paint_kernel
__global__ __launch_bounds__(CC_THREADS) void adell_lc_table_kernel(
    const int* n, int* cnt, unsigned* cmax, long L, int minvox, LcRound r, int* nout, int* ids,
    float* conf, float* peak, long cap) {
  const long vol = blockIdx.x;
  const int nc = n[vol];
  int* c = cnt + vol * L;
  unsigned* cm = cmax + vol * L;
  int carry = 0;
  for (int base = 0; base < nc; base += CC_THREADS) {
    const int i = base + threadIdx.x;
    const int kept = i < nc && c[i] > minvox;
    int total;
    const int pos = carry + cc_block_excl_scan(kept, &total);
    if (i < nc) {
      const float m = cc_unord(cm[i]);
      const float p = lc_paint(m, r);
      if (kept && pos < cap) {
        ids[vol * cap + pos] = i + 1;
        conf[vol * cap + pos] = p;
        peak[vol * cap + pos] = m;
      }
      c[i] = kept;
      cm[i] = __float_as_uint(p);
    }
    carry += total;
  }
  if (threadIdx.x == 0) nout[vol] = carry < cap ? carry : (int)cap;
}

__global__ __launch_bounds__(CC_THREADS) void adell_lc_paint_kernel(const int* lab, long V,
                                                                   const int* cnt,
                                                                   const unsigned* cmax, long L,
                                                                   float* hard, int* indexed) {
  const long vol = blockIdx.y;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= V) break;
    const int id = lab[vol * V + v];
    const bool kept = id && cnt[vol * L + id - 1];
    hard[vol * V + v] = kept ? __uint_as_float(cmax[vol * L + id - 1]) : 0.0f;
    indexed[vol * V + v] = kept ? id : 0;
  }
}

// dynamic, between the rounds: count the choice of the round before (unless it was rejected), then
// open the next round (:77-87) or finish the volume
__global__ void adell_lc_decide_kernel(long NV, LcState st, float factor, int num, int remove_adj,
                                       int* nout, int* ids, float* conf, float* peak, long cap) {
  const long vol = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vol >= NV) return;
  if (st.pend[vol]) {
    if (!(remove_adj && st.adj[vol])) {
      const int k = nout[vol];
      if (k < cap) {
        ids[vol * cap + k] = k + 1;
        conf[vol * cap + k] = st.selconf[vol];
        peak[vol * cap + k] = st.selconf[vol];
        nout[vol] = k + 1;
      }
    }
    st.pend[vol] = 0;
    st.adj[vol] = 0;
  }
  if (!st.act[vol]) return;
  const float m = cc_unord(st.mx[vol]);
  st.mx[vol] = 0;
  if (nout[vol] >= num || m < 0.01f) st.act[vol] = 0;      // max_prob_failsafe_stopping_threshold
  else st.thr[vol] = __fdiv_rn(m, factor);
}

// dynamic: the kept component with the largest painted value, ties to the lowest label (:101-108:
// the second labelling numbers the components of one first labelling in the same raster order).
// sic: when no component survives the size filter (or the best one is painted 0), all_hard_blobs is
// all zero, `all_hard_blobs == max` is the whole volume, and the reference goes on with that as the
// "lesion", confidence 0. Reproduced: sel = -1.
__global__ __launch_bounds__(CC_THREADS) void adell_lc_select_kernel(const int* n, const int* cnt,
                                                                    const unsigned* cmax, long L,
                                                                    int minvox, LcRound r,
                                                                    LcState st) {
  __shared__ unsigned long long sbest;
  const long vol = blockIdx.x;
  if (!st.act[vol]) return;
  if (threadIdx.x == 0) sbest = 0;
  __syncthreads();
  const int nc = n[vol];
  unsigned long long best = 0;
  for (int i = threadIdx.x; i < nc; i += CC_THREADS) {
    if (cnt[vol * L + i] <= minvox) continue;
    const float p = lc_paint(cc_unord(cmax[vol * L + i]), r);
    const unsigned long long key =
        ((unsigned long long)cc_ord(p) << 32) | (0xffffffffu - (unsigned)(i + 1));
    best = key > best ? key : best;
  }
  if (best) atomicMax(&sbest, best);
  __syncthreads();
  if (threadIdx.x == 0) {
    const float p = sbest ? cc_unord((unsigned)(sbest >> 32)) : 0.0f;
    const bool whole = !(p > 0.0f);
    st.sel[vol] = whole ? -1 : (int)(0xffffffffu - (unsigned)(sbest & 0xffffffffu));
    st.selconf[vol] = whole ? 0.0f : p;
    st.pend[vol] = 1;
  }
}

// dynamic: does the chosen component touch a stored voxel (hard > 0 in its 3x3x3 neighbourhood;
// outside the volume is background) (:114-119)
__global__ __launch_bounds__(CC_THREADS) void adell_lc_adjacent_kernel(const int* lab, CcGeom g,
                                                                      const float* hard,
                                                                      const int* nout, LcState st) {
  const long vol = blockIdx.y;
  if (!st.act[vol] || nout[vol] == 0) return;     // nothing stored: nothing to touch
  const int sel = st.sel[vol];
  const int* lv = lab + vol * g.V;
  const float* hv = hard + vol * g.V;
  const long v0 = (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  bool found = false;
  for (int k = 0; k < CC_PER && !found; ++k) {
    const long v = v0 + k;
    if (v >= g.V) break;
    if (sel >= 0 && lv[v] != sel) continue;
    const int x = (int)(v % g.W), y = (int)((v / g.W) % g.H), z = (int)(v / ((long)g.W * g.H));
    for (int dz = -1; dz <= 1 && !found; ++dz) {
      const int zz = z + dz;
      if (zz < 0 || zz >= g.D) continue;
      for (int dy = -1; dy <= 1 && !found; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= g.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx;
          if (xx < 0 || xx >= g.W) continue;
          if (hv[((long)zz * g.H + yy) * g.W + xx] > 0.0f) {
            found = true;
            break;
          }
        }
      }
    }
  }
  if (found) atomicOr(st.adj + vol, 1);
}

// dynamic: store the chosen component unless it was rejected (:122-129), remove it from the working
// copy either way (:132) and take the maximum of what is left for the next round
__global__ __launch_bounds__(CC_THREADS) void adell_lc_apply_kernel(const int* lab, long V,
                                                                   float* work, float* hard,
                                                                   int* indexed, const int* nout,
                                                                   int remove_adj, LcState st) {
  const long vol = blockIdx.y;
  if (!st.act[vol]) return;
  const int sel = st.sel[vol];
  const bool store = !(remove_adj && st.adj[vol]);
  const float c = st.selconf[vol];
  const int index = nout[vol] + 1;
  const long v0 = vol * V + (long)blockIdx.x * CC_CHUNK + (long)threadIdx.x * CC_PER;
  const long vend = (vol + 1) * V;
  unsigned m = 0;
  for (int k = 0; k < CC_PER; ++k) {
    const long v = v0 + k;
    if (v >= vend) break;
    if (sel < 0 || lab[v] == sel) {
      if (store) {
        hard[v] += c;
        indexed[v] += index;
      }
      work[v] = 0.0f;
      m = m > 0x80000000u ? m : 0x80000000u;      // cc_ord(0.0f)
    } else {
      const unsigned o = cc_ord(work[v]);
      m = o > m ? o : m;
    }
  }
  m = lc_wave_max(m);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(st.mx + vol, m);
}

struct LcLayout {
  long L;
  long off_cnt, off_max, stats_end, off_lab, off_n, off_state, off_work, off_cc, total;
};
static LcLayout lc_layout(long NV, int D, int H, int W, int mode) {
  LcLayout l;
  const long V = (long)D * H * W;
  l.L = pc_lattice(D, H, W);
  long o = 0;
  l.off_cnt = o;   o += cc_align(NV * l.L * 4);
  l.off_max = o;   o += cc_align(NV * l.L * 4);
  l.stats_end = o;
  l.off_lab = o;   o += cc_align(NV * V * 4);
  l.off_n = o;     o += cc_align(NV * 4);
  l.off_state = o; o += 7 * cc_align(NV * 4);
  l.off_work = o;  o += mode == LC_DYNAMIC ? cc_align(NV * V * 4) : 0;
  l.off_cc = o;    o += cc_label_ws(NV, V);
  l.total = o;
  return l;
}

static bool lc_mode_ok(int mode) { return mode >= LC_STATIC && mode <= LC_DYNAMIC; }

extern "C" long adell_lesion_candidates_workspace(long NV, int D, int H, int W, int mode) {
  if (!cc_shape_ok(NV, D, H, W) || !lc_mode_ok(mode)) return 0;
  return lc_layout(NV, D, H, W, mode).total;
}

extern "C" long adell_lesion_candidates_capacity(int D, int H, int W, int mode, int min_voxels,
                                                 int num_lesions) {
  if (!cc_shape_ok(1, D, H, W) || !lc_mode_ok(mode)) return 0;
  if (mode == LC_DYNAMIC) return num_lesions > 1 ? num_lesions : 1;
  // a kept component has more than min_voxels voxels, and no mask holds more than the lattice bound
  const long V = (long)D * H * W, lat = pc_lattice(D, H, W);
  const long by_size = V / ((min_voxels > 0 ? (long)min_voxels : 0) + 1);
  const long c = by_size < lat ? by_size : lat;
  return c > 1 ? c : 1;
}

extern "C" int adell_lesion_candidates(const float* x, long NV, int D, int H, int W, int mode,
                                       float threshold, float factor, int min_voxels,
                                       int num_lesions, int round_decimals, int use_round,
                                       int remove_adjacent, float* hard, int* indexed, int* n_out,
                                       int* ids, float* conf, float* peak, long cap, int* rounds,
                                       void* workspace, long workspace_bytes, void* stream) {
  ADELL_REQUIRE(x && hard && indexed && n_out && ids && conf && peak && workspace,
                "lesion_candidates: bad arguments");
  ADELL_REQUIRE(lc_mode_ok(mode), "lesion_candidates: mode %d (0 static, 1 dynamic-fast, 2 dynamic)",
                mode);
  ADELL_REQUIRE(cc_shape_ok(NV, D, H, W), "lesion_candidates: bad shape %ld x %d x %d x %d", NV, D, H,
                W);
  ADELL_REQUIRE(!use_round || (round_decimals >= -300 && round_decimals <= 300),
                "lesion_candidates: max_prob_round_decimals %d", round_decimals);
  ADELL_REQUIRE(cap >= adell_lesion_candidates_capacity(D, H, W, mode, min_voxels, num_lesions),
                "lesion_candidates: table of %ld entries per volume, %ld needed", cap,
                adell_lesion_candidates_capacity(D, H, W, mode, min_voxels, num_lesions));
  const LcLayout l = lc_layout(NV, D, H, W, mode);
  ADELL_REQUIRE(workspace_bytes >= l.total, "lesion_candidates: workspace of %ld bytes, %ld needed",
                workspace_bytes, l.total);
  const hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* cnt = reinterpret_cast<int*>(ws + l.off_cnt);
  unsigned* cmax = reinterpret_cast<unsigned*>(ws + l.off_max);
  int* lab = reinterpret_cast<int*>(ws + l.off_lab);
  int* n = reinterpret_cast<int*>(ws + l.off_n);
  const long sw = cc_align(NV * 4);
  LcState st;
  st.mx = reinterpret_cast<unsigned*>(ws + l.off_state);
  st.thr = reinterpret_cast<float*>(ws + l.off_state + sw);
  st.act = reinterpret_cast<int*>(ws + l.off_state + 2 * sw);
  st.sel = reinterpret_cast<int*>(ws + l.off_state + 3 * sw);
  st.selconf = reinterpret_cast<float*>(ws + l.off_state + 4 * sw);
  st.adj = reinterpret_cast<int*>(ws + l.off_state + 5 * sw);
  st.pend = reinterpret_cast<int*>(ws + l.off_state + 6 * sw);
  LcRound r = {1.0, 0};
  if (use_round) {
    r.how = round_decimals >= 0 ? 1 : 2;
    for (int k = 0; k < (round_decimals >= 0 ? round_decimals : -round_decimals); ++k) r.scale *= 10.0;
  }
  const CcGeom g = cc_geom(D, H, W);
  const CcStats stats = {cnt, cmax, l.L};
  const long nb = cc_nb(g.V);
  ADELL_REQUIRE(nb < (1L << 31) && NV < 65536, "lesion_candidates: %ld volumes are too many to grid",
                NV);
  const dim3 lin((unsigned)nb, (unsigned)NV), per_vol((unsigned)((NV + 63) / 64));
  if (rounds) *rounds = 0;
  ADELL_CHECK_HIP(hipMemsetAsync(ws + l.off_state, 0, 7 * sw, s));

  if (mode != LC_DYNAMIC) {
    if (mode == LC_DYNAMIC_FAST) {
      hipLaunchKernelGGL(adell_lc_max_kernel, lin, dim3(CC_THREADS), 0, s, x, g.V, st.mx);
      ADELL_CHECK_HIP(hipGetLastError());
      hipLaunchKernelGGL(adell_lc_thr_kernel, per_vol, dim3(64), 0, s, NV, st.mx, factor, st.thr);
      ADELL_CHECK_HIP(hipGetLastError());
    }
    ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, l.stats_end, s));
    const CcSrc src = {x, x, NV, CC_MODE_GE, CC_MODE_GE, threshold,
                       mode == LC_DYNAMIC_FAST ? st.thr : nullptr, nullptr};
    const int rc = cc_run(src, NV, g, lab, n, ws + l.off_cc, stats, s);
    if (rc != ADELL_OK) return rc;
    hipLaunchKernelGGL(adell_lc_table_kernel, dim3((unsigned)NV), dim3(CC_THREADS), 0, s, n, cnt, cmax,
                       l.L, min_voxels, r, n_out, ids, conf, peak, cap);
    ADELL_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(adell_lc_paint_kernel, lin, dim3(CC_THREADS), 0, s, lab, g.V, cnt, cmax, l.L,
                       hard, indexed);
    ADELL_CHECK_HIP(hipGetLastError());
    return ADELL_OK;
  }

  float* work = reinterpret_cast<float*>(ws + l.off_work);
  ADELL_CHECK_HIP(hipMemcpyAsync(work, x, NV * g.V * 4, hipMemcpyDeviceToDevice, s));
  ADELL_CHECK_HIP(hipMemsetAsync(hard, 0, NV * g.V * 4, s));
  ADELL_CHECK_HIP(hipMemsetAsync(indexed, 0, NV * g.V * 4, s));
  ADELL_CHECK_HIP(hipMemsetAsync(n_out, 0, NV * 4, s));
  ADELL_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)st.act, 1, NV, s));
  hipLaunchKernelGGL(adell_lc_max_kernel, lin, dim3(CC_THREADS), 0, s, work, g.V, st.mx);
  ADELL_CHECK_HIP(hipGetLastError());
  std::vector<int> act(NV);
  // a round removes more than min_voxels voxels of a volume, or all of them
  const long max_rounds = g.V / ((min_voxels > 0 ? (long)min_voxels : 0) + 1) + 2;
  for (long round = 0;; ++round) {
    hipLaunchKernelGGL(adell_lc_decide_kernel, per_vol, dim3(64), 0, s, NV, st, factor, num_lesions,
                       remove_adjacent, n_out, ids, conf, peak, cap);
    ADELL_CHECK_HIP(hipGetLastError());
    // the one read-back of the round: which volumes go on
    ADELL_CHECK_HIP(hipMemcpyAsync(act.data(), st.act, NV * 4, hipMemcpyDeviceToHost, s));
    ADELL_CHECK_HIP(hipStreamSynchronize(s));
    bool any = false;
    for (long v = 0; v < NV; ++v) any = any || act[v];
    if (!any) break;
    ADELL_REQUIRE(round < max_rounds, "lesion_candidates: no end after %ld rounds", round);
    if (rounds) *rounds = (int)(round + 1);
    ADELL_CHECK_HIP(hipMemsetAsync(ws, 0, l.stats_end, s));
    const CcSrc src = {work, work, NV, CC_MODE_GE, CC_MODE_GE, 0.0f, st.thr, st.act};
    const int rc = cc_run(src, NV, g, lab, n, ws + l.off_cc, stats, s);
    if (rc != ADELL_OK) return rc;
    hipLaunchKernelGGL(adell_lc_select_kernel, dim3((unsigned)NV), dim3(CC_THREADS), 0, s, n, cnt, cmax,
                       l.L, min_voxels, r, st);
    ADELL_CHECK_HIP(hipGetLastError());
    if (remove_adjacent) {
      hipLaunchKernelGGL(adell_lc_adjacent_kernel, lin, dim3(CC_THREADS), 0, s, lab, g, hard, n_out, st);
      ADELL_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(adell_lc_apply_kernel, lin, dim3(CC_THREADS), 0, s, lab, g.V, work, hard,
                       indexed, n_out, remove_adjacent, st);
    ADELL_CHECK_HIP(hipGetLastError());
  }
  return ADELL_OK;
}
