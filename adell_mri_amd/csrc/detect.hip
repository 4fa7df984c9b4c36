// Kernels of 3-D object detection (adell_mri/modules/object_detection: YOLONet3dPL.step /
// calculate_loss, losses.complete_iou_loss, utils.nms_nd). House rules of mil.hip: fp32 in and out,
// dense inputs, no float atomics, every sum in a fixed order in fp64 -- two runs are bit-identical.
// The heads and the target map are read IN PLACE, in the layout the network produces (channels last,
// [B][S = H W D][k A], or [B][k A][S]: a flag per side): anchor a of a logical [B, k A, H, W, D] tensor is
// channels [k a, k a + k); no split / stack / permute copy is made.
//   * positive-cell table: the cells of the target map whose objectness channel is > threshold, as
//     int32 rows (b, h, w, d, a) in torch.where's order on the stacked [B, H, W, D, A] view (anchor
//     fastest), by a block-scan compaction in three launches: per-block counts, one block's exclusive
//     scan of them (which leaves the total on the device), then each block scans its threads and
//     writes its rows. Nothing is read on the host.
//   * step loss forward, two launches. (1) The first blocks sum -max(log1p(-p), -100) over the whole
//     objectness head (the cross-entropy against a target of 0; one fp64 partial per block); the
//     others take one positive per thread: centre and size of prediction and target gathered, cell
//     index added, scaled by the correction factor, exp(size) anchor / 2, corners, complete IoU
//     (+1 size convention) -> iou, cpd, ar and the cross-entropy's correction iou (log1p(-p) - log p)
//     for a target of iou instead of 0. The dense target is never written. (2) One block adds the
//     partials and the per-positive rows in order: loss = bce_mean + 0.1 (mean(1 - iou) + mean(cpd)
//     + mean(ar)). With no positive the means are 0 / 0: NaN, as the reference's means of empty tensors.
//   * its backward, two launches: the dense pass writes dobjectness for a target of 0 and zeroes
//     dcentre and dsize; then one thread per positive repeats the box arithmetic on dual numbers that
//     carry the six partial derivatives (centre 3, size 3) -- alpha = v / ((1 - iou) + v) is NOT
//     detached -- and overwrites its own cells. The cross-entropy's gradient with respect to its
//     TARGET, (log1p(-p) - log p) / n_cells, flows through iou into centre and size. Every positive
//     is a different cell: plain stores.
//   * non-maximum suppression over score-sorted boxes: a pairwise kernel, one wavefront per 64-bit
//     word (candidate i against candidates 64 w .. 64 w + 63: check_overlap and calculate_iou >
//     threshold, one ballot), then one wavefront sweeps the words in order, 64 candidates at a time.
#include "common.h"

constexpr int DET_NT = 256;                    // threads per block
constexpr int DET_NW = DET_NT / 64;            // waves per block
constexpr int DET_ITEMS = 4;                   // consecutive cells per thread of the table kernels
constexpr int DET_CHUNK = DET_NT * DET_ITEMS;  // cells per block there
constexpr int DET_DENSE_MAX_BLOCKS = 1024;     // dense blocks of the loss forward (grid-stride)
constexpr int DET_POS_MAX_BLOCKS = 512;        // per-positive blocks (grid-stride)
constexpr int DET_NMS_MAX = 16384;             // candidates the sweep keeps in registers (4 words a lane)

struct DetGrid {
  int B, A, H, W, D;
  int Ct, c0, cs;    // channels of the map, channel of anchor 0's objectness, channels per anchor
                     // (7 in the target map, 1 when the map is the objectness head itself)
  int cl_t, cl_h;    // memory layout of the map / of the heads: 0 [B][C][S], 1 channels last [B][S][C]
};

// element (b, c, cell) of a [B][C][S] tensor, or of its channels-last form [B][S][C]
__device__ __forceinline__ size_t det_at(int cl, long b, int c, long cell, int C, long S) {
  return cl ? ((size_t)b * S + cell) * C + c : ((size_t)b * C + c) * S + cell;
}
// distance between channels c and c + 1 of one cell
__device__ __forceinline__ size_t det_cstep(int cl, long S) { return cl ? 1 : (size_t)S; }

// exclusive prefix of v over the block's threads; *tot the block's total. s_w: DET_NW ints of LDS.
__device__ __forceinline__ int det_block_excl_scan(int v, int* s_w, int* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < DET_NW; ++w) {
    const int x = s_w[w];
    if (w < wave) base += x;
    total += x;
  }
  __syncthreads();
  *tot = total;
  return base + inc - v;
}

// flat index m = ((b S + cell) A + a) of the stacked view -> is the cell positive
__device__ __forceinline__ bool det_positive(const float* __restrict__ tgt, const DetGrid g, long S,
                                             long m, float thr) {
  const int a = (int)(m % g.A);
  const long bc = m / g.A;
  const long b = bc / S, cell = bc - b * S;
  return tgt[det_at(g.cl_t, b, g.c0 + g.cs * a, cell, g.Ct, S)] > thr;
}

__global__ __launch_bounds__(DET_NT) void adell_det_table_count_kernel(
    const float* __restrict__ tgt, DetGrid g, long M, float thr, int* __restrict__ block_cnt) {
  __shared__ int s_w[DET_NW];
  const long S = (long)g.H * g.W * g.D;
  const long m0 = (long)blockIdx.x * DET_CHUNK + (long)threadIdx.x * DET_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < DET_ITEMS; ++k)
    if (m0 + k < M && det_positive(tgt, g, S, m0 + k, thr)) ++c;
  int tot;
  det_block_excl_scan(c, s_w, &tot);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = tot;
}

// one block: block_cnt -> its exclusive prefix in place, the total to count[0]
__global__ __launch_bounds__(DET_NT) void adell_det_table_scan_kernel(int* __restrict__ block_cnt,
                                                                      int nblk, int* __restrict__ count) {
  __shared__ int s_w[DET_NW];
  int carry = 0;
  for (int i0 = 0; i0 < nblk; i0 += DET_NT) {
    const int i = i0 + threadIdx.x;
    const int v = i < nblk ? block_cnt[i] : 0;
    int tot;
    const int ex = det_block_excl_scan(v, s_w, &tot);
    if (i < nblk) block_cnt[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(DET_NT) void adell_det_table_write_kernel(
    const float* __restrict__ tgt, DetGrid g, long M, float thr, const int* __restrict__ block_off,
    long cap, int* __restrict__ table) {
  __shared__ int s_w[DET_NW];
  const long S = (long)g.H * g.W * g.D;
  const long m0 = (long)blockIdx.x * DET_CHUNK + (long)threadIdx.x * DET_ITEMS;
  bool f[DET_ITEMS];
  int c = 0;
#pragma unroll
  for (int k = 0; k < DET_ITEMS; ++k) {
    f[k] = m0 + k < M && det_positive(tgt, g, S, m0 + k, thr);
    c += f[k] ? 1 : 0;
  }
  int tot;
  long at = (long)block_off[blockIdx.x] + det_block_excl_scan(c, s_w, &tot);
#pragma unroll
  for (int k = 0; k < DET_ITEMS; ++k) {
    if (!f[k] || at >= cap) continue;
    const long m = m0 + k;
    const int a = (int)(m % g.A);
    long r = m / g.A;
    const int d = (int)(r % g.D);
    r /= g.D;
    const int w = (int)(r % g.W);
    r /= g.W;
    const int h = (int)(r % g.H);
    const int b = (int)(r / g.H);
    int* row = table + at * 5;
    row[0] = b; row[1] = h; row[2] = w; row[3] = d; row[4] = a;
    ++at;
  }
}

static int det_check_grid(const char* what, int B, int A, int H, int W, int D, int Ct, int c0, long* M,
                          int cs = 7) {
  ADELL_REQUIRE(B > 0 && A > 0 && H > 0 && W > 0 && D > 0, "%s: empty grid", what);
  ADELL_REQUIRE((cs == 7 || cs == 1) && c0 >= 0 && c0 + cs * A <= Ct,
                "%s: the map has %d channels, %d anchors need %d each from channel %d", what, Ct, A, cs, c0);
  const double m = (double)B * A * H * W * D;
  ADELL_REQUIRE(m <= (double)(1L << 30) && (double)B * Ct * H * W * D <= (double)(1L << 40),
                "%s: grid too large", what);
  *M = (long)B * A * H * W * D;
  return ADELL_OK;
}

extern "C" long adell_det_table_blocks(long cells) { return (cells + DET_CHUNK - 1) / DET_CHUNK; }

extern "C" int adell_det_positive_table(const float* target, int B, int A, int H, int W, int D, int Ct,
                                        int c0, int cs, int channels_last, float threshold,
                                        int* block_scratch, int* table, int* count, void* stream) {
  long M;
  const int rc = det_check_grid("det_positive_table", B, A, H, W, D, Ct, c0, &M, cs);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(target && block_scratch && table && count, "det_positive_table: null pointer");
  const DetGrid g{B, A, H, W, D, Ct, c0, cs, channels_last ? 1 : 0, 0};
  const int nblk = (int)adell_det_table_blocks(M);
  hipStream_t st = (hipStream_t)stream;
  int e = adell_launch<adell_det_table_count_kernel>(dim3(nblk), dim3(DET_NT), 0, st, target, g, M,
                                                     threshold, block_scratch);
  if (e != ADELL_OK) return e;
  e = adell_launch<adell_det_table_scan_kernel>(dim3(1), dim3(DET_NT), 0, st, block_scratch, nblk, count);
  if (e != ADELL_OK) return e;
  return adell_launch<adell_det_table_write_kernel>(dim3(nblk), dim3(DET_NT), 0, st, target, g, M,
                                                    threshold, (const int*)block_scratch, M, table);
}

// ---- complete IoU on plain floats and on dual numbers --------------------------------------------------
// value and the partial derivatives with respect to (centre 0..2, size 0..2) of the predicted box
struct DetDual {
  float v;
  float d[6];
  __device__ DetDual() {}
  __device__ DetDual(float x) : v(x) {
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = 0.f;
  }
};
#define DET_EACH for (int k = 0; k < 6; ++k)
__device__ __forceinline__ DetDual operator+(const DetDual& a, const DetDual& b) {
  DetDual r; r.v = a.v + b.v;
#pragma unroll
  DET_EACH r.d[k] = a.d[k] + b.d[k];
  return r;
}
__device__ __forceinline__ DetDual operator-(const DetDual& a, const DetDual& b) {
  DetDual r; r.v = a.v - b.v;
#pragma unroll
  DET_EACH r.d[k] = a.d[k] - b.d[k];
  return r;
}
__device__ __forceinline__ DetDual operator*(const DetDual& a, const DetDual& b) {
  DetDual r; r.v = a.v * b.v;
#pragma unroll
  DET_EACH r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
__device__ __forceinline__ DetDual operator/(const DetDual& a, const DetDual& b) {
  DetDual r; r.v = a.v / b.v;
  const float ib = 1.0f / b.v;
#pragma unroll
  DET_EACH r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
  return r;
}
// torch.maximum / minimum: the gradient goes to the larger (smaller) operand, halved on a tie
__device__ __forceinline__ DetDual det_max(const DetDual& a, const DetDual& b) {
  if (a.v == b.v) {
    DetDual r; r.v = a.v;
#pragma unroll
    DET_EACH r.d[k] = 0.5f * (a.d[k] + b.d[k]);
    return r;
  }
  return a.v > b.v ? a : b;
}
__device__ __forceinline__ DetDual det_min(const DetDual& a, const DetDual& b) {
  if (a.v == b.v) {
    DetDual r; r.v = a.v;
#pragma unroll
    DET_EACH r.d[k] = 0.5f * (a.d[k] + b.d[k]);
    return r;
  }
  return a.v < b.v ? a : b;
}
__device__ __forceinline__ DetDual det_atan(const DetDual& a) {
  DetDual r; r.v = atanf(a.v);
  const float s = 1.0f / (1.0f + a.v * a.v);
#pragma unroll
  DET_EACH r.d[k] = a.d[k] * s;
  return r;
}
__device__ __forceinline__ float det_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float det_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float det_atan(float a) { return atanf(a); }
__device__ __forceinline__ float det_val(float a) { return a; }
__device__ __forceinline__ float det_val(const DetDual& a) { return a.v; }

// losses.complete_iou_loss for one box pair: predicted corners pc -+ ps (T: float or DetDual), target
// corners tc -+ ts (constants), the centres handed in as the reference's step does.
template <typename T>
__device__ __forceinline__ void det_ciou(const T pc[3], const T ps[3], const float tc[3],
                                         const float ts[3], T* iou, T* cpd, T* ar) {
  T a_size[3], b_size[3];
  T inter = T(1.0f), va = T(1.0f), vb = T(1.0f), cd = T(0.0f), bd = T(0.0f);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T a_tl = pc[j] - ps[j], a_br = pc[j] + ps[j];
    const T b_tl = T(tc[j] - ts[j]), b_br = T(tc[j] + ts[j]);
    a_size[j] = a_br - a_tl + T(1.0f);
    b_size[j] = b_br - b_tl + T(1.0f);
    inter = inter * (det_min(a_br, b_br) - det_max(a_tl, b_tl) + T(1.0f));
    va = va * a_size[j];
    vb = vb * b_size[j];
    const T dc = pc[j] - T(tc[j]);
    cd = cd + dc * dc;
    const T dg = det_max(a_br, b_br) - det_min(a_tl, b_tl);
    bd = bd + dg * dg;
  }
  const T uni = va + vb - inter;
  *iou = det_val(uni) > 0.0f ? inter / uni : T(0.0f);
  *cpd = cd / bd;
  const float k4 = (float)(4.0 / (3.14159265358979323846 * 3.14159265358979323846));
  T v = T(0.0f);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = i + 1; j < 3; ++j) {
      const T df = det_atan(a_size[i] / a_size[j]) - det_atan(b_size[i] / b_size[j]);
      v = v + T(k4) * (df * df);
    }
  v = v / T(3.0f);
  const T alpha = v / ((T(1.0f) - *iou) + v);
  *ar = v * alpha;
}

struct DetLossArgs {
  const float* centre;   // [B][3 A][S], tanh output
  const float* size;     // [B][3 A][S]
  const float* obj;      // [B][A][S], sigmoid output
  const float* tgt;      // [B][Ct][S]: per anchor objectness, centre 3, size 3 from channel c0
  const float* anchors;  // [A][3]
  const int* table;      // [cap][5]
  const int* count;      // [1]
  float cf[3];           // correction factor
  DetGrid g;
  long cap, n_obj;       // table capacity, B A S
};

// the row's gathers: predicted and target centre (cell added, scaled) and half size; offsets of the
// row's first centre / size channel and of its objectness, *S_out the heads' channel step
template <typename T>
__device__ __forceinline__ void det_gather(const DetLossArgs& q, long i, T pc[3], T ps[3], float tc[3],
                                           float ts[3], size_t* o_box, size_t* o_obj, long* S_out) {
  const int* row = q.table + i * 5;
  const int b = row[0], h = row[1], w = row[2], d = row[3], a = row[4];
  const long S = (long)q.g.H * q.g.W * q.g.D;
  const long cell = ((long)h * q.g.W + w) * q.g.D + d;
  const int idx[3] = {h, w, d};
  *o_box = det_at(q.g.cl_h, b, 3 * a, cell, 3 * q.g.A, S);
  *o_obj = det_at(q.g.cl_h, b, a, cell, q.g.A, S);
  const size_t hs = det_cstep(q.g.cl_h, S), tstep = det_cstep(q.g.cl_t, S);
  *S_out = (long)hs;
  const size_t o_t = det_at(q.g.cl_t, b, q.g.c0 + 7 * a, cell, q.g.Ct, S);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float anc = q.anchors[3 * a + j];
    pc[j] = T((q.centre[*o_box + (size_t)j * hs] + (float)idx[j]) * q.cf[j]);
    ps[j] = T(expf(q.size[*o_box + (size_t)j * hs]) * anc / 2.0f);
    tc[j] = (q.tgt[o_t + (size_t)(1 + j) * tstep] + (float)idx[j]) * q.cf[j];
    ts[j] = expf(q.tgt[o_t + (size_t)(4 + j) * tstep]) * anc / 2.0f;
  }
}

__device__ __forceinline__ double det_block_sum_d(double v, double* s_d) {
  v = adell_wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) s_d[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < DET_NW; ++w) t += s_d[w];
  __syncthreads();
  return t;
}

// blocks [0, nb_dense): partial[blk] = sum over the block's cells of -max(log1p(-p), -100);
// blocks beyond: rows[0 .. 3][i] = iou, cpd, ar, iou (log1p(-p) - log p) of positive i (row stride cap)
__global__ __launch_bounds__(DET_NT) void adell_det_loss_parts_kernel(DetLossArgs q, int nb_dense,
                                                                      double* __restrict__ partial,
                                                                      float* __restrict__ rows) {
  __shared__ double s_d[DET_NW];
  if ((int)blockIdx.x < nb_dense) {
    double acc = 0.0;
    for (long i = (long)blockIdx.x * DET_NT + threadIdx.x; i < q.n_obj; i += (long)nb_dense * DET_NT)
      acc -= (double)fmaxf(log1pf(-q.obj[i]), -100.0f);
    acc = det_block_sum_d(acc, s_d);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
    return;
  }
  const long n = min((long)q.count[0], q.cap);
  const long nb_pos = gridDim.x - nb_dense;
  for (long i = (long)(blockIdx.x - nb_dense) * DET_NT + threadIdx.x; i < n; i += nb_pos * DET_NT) {
    float pc[3], ps[3], tc[3], ts[3], iou, cpd, ar;
    size_t o_box, o_obj;
    long S;
    det_gather<float>(q, i, pc, ps, tc, ts, &o_box, &o_obj, &S);
    det_ciou<float>(pc, ps, tc, ts, &iou, &cpd, &ar);
    const float p = q.obj[o_obj];
    rows[i] = iou;
    rows[q.cap + i] = cpd;
    rows[2 * q.cap + i] = ar;
    rows[3 * q.cap + i] = iou * (fmaxf(log1pf(-p), -100.0f) - fmaxf(logf(p), -100.0f));
  }
}

// one block. out: loss, bce mean, mean(1 - iou), mean(cpd), mean(ar)
__global__ __launch_bounds__(DET_NT) void adell_det_loss_final_kernel(
    const double* __restrict__ partial, int nb_dense, const float* __restrict__ rows, long cap,
    const int* __restrict__ count, long n_obj, float* __restrict__ out) {
  __shared__ double s_d[DET_NW];
  const long n = min((long)count[0], cap);
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb_dense; i += DET_NT) acc += partial[i];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < n; i += DET_NT) {
    s[0] += (double)(1.0f - rows[i]);
    s[1] += (double)rows[cap + i];
    s[2] += (double)rows[2 * cap + i];
    s[3] += (double)rows[3 * cap + i];
  }
  acc = det_block_sum_d(acc, s_d);
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = det_block_sum_d(s[k], s_d);
  if (threadIdx.x == 0) {
    const double bce = (acc + s[3]) / (double)n_obj;
    const double dn = (double)n;             // 0 / 0 -> NaN with no positive, as the reference
    const double m_iou = s[0] / dn, m_cpd = s[1] / dn, m_ar = s[2] / dn;
    out[0] = (float)(bce + 0.1 * (m_iou + m_cpd + m_ar));
    out[1] = (float)bce;
    out[2] = (float)m_iou;
    out[3] = (float)m_cpd;
    out[4] = (float)m_ar;
  }
}

static int det_loss_args(const char* what, DetLossArgs* q, const float* centre, const float* size,
                         const float* obj, const float* target, const float* anchors, const int* table,
                         const int* count, float cf0, float cf1, float cf2, int B, int A, int H, int W,
                         int D, int Ct, int c0, int cl_t, int cl_h) {
  long M;
  const int rc = det_check_grid(what, B, A, H, W, D, Ct, c0, &M);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(centre && size && obj && target && anchors && table && count, "%s: null pointer", what);
  q->centre = centre; q->size = size; q->obj = obj; q->tgt = target; q->anchors = anchors;
  q->table = table; q->count = count;
  q->cf[0] = cf0; q->cf[1] = cf1; q->cf[2] = cf2;
  q->g = DetGrid{B, A, H, W, D, Ct, c0, 7, cl_t ? 1 : 0, cl_h ? 1 : 0};
  q->cap = M;
  q->n_obj = M;
  return ADELL_OK;
}
static int det_dense_blocks(long n) { return (int)min((n + DET_NT - 1) / DET_NT, (long)DET_DENSE_MAX_BLOCKS); }
static int det_pos_blocks(long n) { return (int)min((n + DET_NT - 1) / DET_NT, (long)DET_POS_MAX_BLOCKS); }

extern "C" long adell_det_loss_partials(long cells) { return det_dense_blocks(cells); }

extern "C" int adell_det_loss_fwd(const float* centre, const float* size, const float* obj,
                                  const float* target, const float* anchors, const int* table,
                                  const int* count, float cf0, float cf1, float cf2, int B, int A, int H,
                                  int W, int D, int Ct, int c0, int target_cl, int heads_cl, double* partial,
                                  float* rows, float* out, void* stream) {
  DetLossArgs q;
  const int rc = det_loss_args("det_loss_fwd", &q, centre, size, obj, target, anchors, table, count, cf0,
                               cf1, cf2,
                               B, A, H, W, D, Ct, c0, target_cl, heads_cl);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(partial && rows && out, "det_loss_fwd: null pointer");
  const int nbd = det_dense_blocks(q.n_obj), nbp = det_pos_blocks(q.cap);
  hipStream_t st = (hipStream_t)stream;
  const int e = adell_launch<adell_det_loss_parts_kernel>(dim3(nbd + nbp), dim3(DET_NT), 0, st, q, nbd,
                                                          partial, rows);
  if (e != ADELL_OK) return e;
  return adell_launch<adell_det_loss_final_kernel>(dim3(1), dim3(DET_NT), 0, st, (const double*)partial,
                                                   nbd, (const float*)rows, q.cap, count, q.n_obj, out);
}

// dense pass of the backward: dobj for a target of 0 (torch: (p - t) / max((1 - p) p, 1e-12) / n),
// dcentre and dsize (3 n_obj floats each) zeroed
__global__ __launch_bounds__(DET_NT) void adell_det_loss_bwd_dense_kernel(
    const float* __restrict__ obj, const float* __restrict__ go, long n_obj, float* __restrict__ dcentre,
    float* __restrict__ dsize, float* __restrict__ dobj) {
  const float s = go[0] / (float)n_obj;
  for (long i = (long)blockIdx.x * DET_NT + threadIdx.x; i < n_obj; i += (long)gridDim.x * DET_NT) {
    const float p = obj[i];
    dobj[i] = s * (p / fmaxf((1.0f - p) * p, 1e-12f));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dcentre[i + (size_t)j * n_obj] = 0.f;
      dsize[i + (size_t)j * n_obj] = 0.f;
    }
  }
}

__global__ __launch_bounds__(DET_NT) void adell_det_loss_bwd_pos_kernel(
    DetLossArgs q, const float* __restrict__ go, float* __restrict__ dcentre,
    float* __restrict__ dsize, float* __restrict__ dobj) {
  const long n = min((long)q.count[0], q.cap);
  const float g = go[0];
  const float box_w = 0.1f / (float)n, inv_cells = 1.0f / (float)q.n_obj;
  for (long i = (long)blockIdx.x * DET_NT + threadIdx.x; i < n; i += (long)gridDim.x * DET_NT) {
    DetDual pc[3], ps[3], iou, cpd, ar;
    float tc[3], ts[3];
    size_t o_box, o_obj;
    long S;
    det_gather<DetDual>(q, i, pc, ps, tc, ts, &o_box, &o_obj, &S);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pc[j].d[j] = q.cf[j];          // d (c + idx) cf / dc
      ps[j].d[3 + j] = ps[j].v;      // d exp(s) anchor / 2 / ds
    }
    det_ciou<DetDual>(pc, ps, tc, ts, &iou, &cpd, &ar);
    const float p = q.obj[o_obj];
    // dloss / diou: the cross-entropy's target gradient and the -iou of mean(1 - iou)
    const float g_iou = (fmaxf(log1pf(-p), -100.0f) - fmaxf(logf(p), -100.0f)) * inv_cells - box_w;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dcentre[o_box + (size_t)j * S] = g * (g_iou * iou.d[j] + box_w * (cpd.d[j] + ar.d[j]));
      dsize[o_box + (size_t)j * S] = g * (g_iou * iou.d[3 + j] + box_w * (cpd.d[3 + j] + ar.d[3 + j]));
    }
    dobj[o_obj] = g * inv_cells * ((p - iou.v) / fmaxf((1.0f - p) * p, 1e-12f));
  }
}

extern "C" int adell_det_loss_bwd(const float* centre, const float* size, const float* obj,
                                  const float* target, const float* anchors, const int* table,
                                  const int* count, float cf0, float cf1, float cf2, int B, int A, int H,
                                  int W, int D, int Ct, int c0, int target_cl, int heads_cl,
                                  const float* grad_out, float* dcentre,
                                  float* dsize, float* dobj, void* stream) {
  DetLossArgs q;
  const int rc = det_loss_args("det_loss_bwd", &q, centre, size, obj, target, anchors, table, count, cf0,
                               cf1, cf2,
                               B, A, H, W, D, Ct, c0, target_cl, heads_cl);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(grad_out && dcentre && dsize && dobj, "det_loss_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int e = adell_launch<adell_det_loss_bwd_dense_kernel>(dim3(det_dense_blocks(q.n_obj)), dim3(DET_NT),
                                                              0, st, obj, grad_out, q.n_obj, dcentre,
                                                              dsize, dobj);
  if (e != ADELL_OK) return e;
  return adell_launch<adell_det_loss_bwd_pos_kernel>(dim3(det_pos_blocks(q.cap)), dim3(DET_NT), 0, st, q,
                                                     grad_out, dcentre, dsize, dobj);
}

// ---- non-maximum suppression -------------------------------------------------------------------------
// boxes [n][6] (upper corner, lower corner), sorted by descending score. Word (i, w) of mask [n][nw]:
// bit l set when candidate j = 64 w + l > i overlaps i (utils.check_overlap(i, j)) with
// utils.calculate_iou(i, j) > thr. One wavefront per word.
__global__ __launch_bounds__(DET_NT) void adell_det_nms_mask_kernel(
    const float* __restrict__ boxes, int n, int nw, float thr, unsigned long long* __restrict__ mask) {
  const long word = (long)blockIdx.x * DET_NW + (threadIdx.x >> 6);
  if (word >= (long)n * nw) return;                 // whole waves leave together
  const int i = (int)(word / nw), w = (int)(word - (long)i * nw);
  const int j = w * 64 + (threadIdx.x & 63);
  bool hit = false;
  if (j > i && j < n) {
    const float* a = boxes + (size_t)i * 6;
    const float* b = boxes + (size_t)j * 6;
    bool gt = false, lt = false;
    float inter = 1.f, va = 1.f, vb = 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gt = gt || a[3 + k] > b[k];
      lt = lt || a[k] < b[3 + k];
      inter *= fminf(a[3 + k], b[3 + k]) - fmaxf(a[k], b[k]) + 1.0f;
      va *= a[3 + k] - a[k] + 1.0f;
      vb *= b[3 + k] - b[k] + 1.0f;
    }
    const float uni = va + vb - inter;
    const float iou = uni > 0.0f ? inter / uni : 0.0f;
    hit = gt && lt && iou > thr;
  }
  const unsigned long long bits = __ballot(hit);
  if ((threadIdx.x & 63) == 0) mask[word] = bits;
}

// One wavefront. Lane l owns the removed-words l, l + 64, l + 128, l + 192. For each group of 64
// candidates: the group's removed word, the 64 diagonal words resolved in order in registers, then the
// rows of the kept ones OR-ed into the words behind. keep[i] = 1 for a kept candidate.
__global__ __launch_bounds__(64) void adell_det_nms_sweep_kernel(
    const unsigned long long* __restrict__ mask, int n, int nw, int* __restrict__ keep) {
  const int lane = threadIdx.x;
  unsigned long long rem[DET_NMS_MAX / 64 / 64] = {0ull, 0ull, 0ull, 0ull};
  for (int wb = 0; wb < nw; ++wb) {
    unsigned long long mine = 0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((wb >> 6) == r) mine = rem[r];
    unsigned long long cur = __shfl(mine, wb & 63, 64);
    const int i = wb * 64 + lane;
    const unsigned long long diag = i < n ? mask[(size_t)i * nw + wb] : 0ull;
    for (int k = 0; k < 64; ++k) {
      const unsigned long long dk = __shfl(diag, k, 64);
      if (!((cur >> k) & 1ull)) cur |= dk;
    }
    const int left = n - wb * 64;
    const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const unsigned long long kept = ~cur & valid;
    if (i < n) keep[i] = (int)((kept >> lane) & 1ull);
    unsigned long long rest = kept;
    while (rest) {
      const int k = __ffsll((long long)rest) - 1;
      rest &= rest - 1ull;
      const size_t row = (size_t)(wb * 64 + k) * nw;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int w = lane + 64 * r;
        if (w > wb && w < nw) rem[r] |= mask[row + w];
      }
    }
  }
}

extern "C" int adell_det_nms_max(void) { return DET_NMS_MAX; }

extern "C" int adell_det_nms(const float* boxes, int n, float iou_threshold, unsigned long long* mask,
                             int* keep, void* stream) {
  ADELL_REQUIRE(boxes && mask && keep && n > 0, "det_nms: bad arguments");
  ADELL_REQUIRE(n <= DET_NMS_MAX, "det_nms: %d candidates, at most %d", n, DET_NMS_MAX);
  const int nw = adell_cdiv(n, 64);
  const long words = (long)n * nw;
  hipStream_t st = (hipStream_t)stream;
  const int e = adell_launch<adell_det_nms_mask_kernel>(dim3((unsigned)((words + DET_NW - 1) / DET_NW)),
                                                        dim3(DET_NT), 0, st, boxes, n, nw, iou_threshold,
                                                        mask);
  if (e != ADELL_OK) return e;
  return adell_launch<adell_det_nms_sweep_kernel>(dim3(1), dim3(64), 0, st,
                                                  (const unsigned long long*)mask, n, nw, keep);
}

// ---- box decode (YOLONet3d.recover_boxes for a whole batch) ---------------------------------------------
// table: the cells of the objectness head > 0.5 (adell_det_positive_table with cs = 1), so the rows are in
// torch.where's order image by image. Row i -> boxes[i] = (centre - size / 2, centre + size / 2) with size
// = anchor exp(size head), centre = (centre head + cell index) cf; scores[i] = the objectness; classes[i]
// = the NC class-head values of the cell, or the objectness again when cls is null (n_classes == 2).
// starts[b] = first row of image b, starts[B] = n: the one array the host reads.
__global__ __launch_bounds__(DET_NT) void adell_det_decode_kernel(DetLossArgs q, const float* __restrict__ cls,
                                                                  int NC, float* __restrict__ boxes,
                                                                  float* __restrict__ scores,
                                                                  float* __restrict__ classes,
                                                                  int* __restrict__ starts) {
  const long n = min((long)q.count[0], q.cap);
  const long S = (long)q.g.H * q.g.W * q.g.D;
  if (n == 0 && blockIdx.x == 0)
    for (int b = threadIdx.x; b <= q.g.B; b += DET_NT) starts[b] = 0;
  for (long i = (long)blockIdx.x * DET_NT + threadIdx.x; i < n; i += (long)gridDim.x * DET_NT) {
    const int* row = q.table + i * 5;
    const int b = row[0], h = row[1], w = row[2], d = row[3], a = row[4];
    const int prev = i == 0 ? -1 : row[-5];
    for (int bb = prev + 1; bb <= b; ++bb) starts[bb] = (int)i;
    if (i == n - 1)
      for (int bb = b + 1; bb <= q.g.B; ++bb) starts[bb] = (int)n;
    const long cell = ((long)h * q.g.W + w) * q.g.D + d;
    const int idx[3] = {h, w, d};
    const size_t o_box = det_at(q.g.cl_h, b, 3 * a, cell, 3 * q.g.A, S), hs = det_cstep(q.g.cl_h, S);
    const float p = q.obj[det_at(q.g.cl_h, b, a, cell, q.g.A, S)];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float sz = q.anchors[3 * a + j] * expf(q.size[o_box + (size_t)j * hs]);
      const float c = (q.centre[o_box + (size_t)j * hs] + (float)idx[j]) * q.cf[j];
      boxes[i * 6 + j] = c - sz / 2.0f;
      boxes[i * 6 + 3 + j] = c + sz / 2.0f;
    }
    scores[i] = p;
    if (cls == nullptr) {
      classes[i] = p;
    } else {
      for (int c = 0; c < NC; ++c) classes[i * NC + c] = cls[det_at(q.g.cl_h, b, c, cell, NC, S)];
    }
  }
}

extern "C" int adell_det_decode(const float* centre, const float* size, const float* obj, const float* cls,
                                int NC, const float* anchors, const int* table, const int* count, float cf0,
                                float cf1, float cf2, int B, int A, int H, int W, int D, int heads_cl,
                                float* boxes, float* scores, float* classes, int* starts, void* stream) {
  long M;
  const int rc = det_check_grid("det_decode", B, A, H, W, D, A, 0, &M, 1);
  if (rc != ADELL_OK) return rc;
  ADELL_REQUIRE(centre && size && obj && anchors && table && count && boxes && scores && classes && starts,
                "det_decode: null pointer");
  ADELL_REQUIRE(cls == nullptr || NC > 0, "det_decode: a class head needs its channel count");
  DetLossArgs q;
  q.centre = centre; q.size = size; q.obj = obj; q.tgt = nullptr; q.anchors = anchors;
  q.table = table; q.count = count;
  q.cf[0] = cf0; q.cf[1] = cf1; q.cf[2] = cf2;
  q.g = DetGrid{B, A, H, W, D, A, 0, 1, heads_cl ? 1 : 0, heads_cl ? 1 : 0};
  q.cap = M;
  q.n_obj = M;
  return adell_launch<adell_det_decode_kernel>(dim3(det_pos_blocks(M)), dim3(DET_NT), 0, (hipStream_t)stream,
                                               q, cls, NC, boxes, scores, classes, starts);
}

// ---- box matching for mAP (mAP.compute_image, steps 2 and 3) ----------------------------------------------
// One wavefront per target box t of image img[t]: over that image's predictions [pstart[img], pstart[img
// + 1]) (already filtered by score and sorted as the metric sorts them) the highest calculate_iou among
// those with check_overlap(target, prediction) -- every other entry of the reference's iou_array is 0 --
// and its index within the image, the lowest on a tie (argmax). best_iou 0 and index 0 when nothing
// overlaps (or -1 when the image has no prediction at all).
__global__ __launch_bounds__(DET_NT) void adell_det_match_kernel(
    const float* __restrict__ tgt, const int* __restrict__ img, int T, const float* __restrict__ pred,
    const int* __restrict__ pstart, int* __restrict__ best, float* __restrict__ best_iou) {
  const int t = blockIdx.x * DET_NW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= T) return;
  const float* a = tgt + (size_t)t * 6;
  const int p0 = pstart[img[t]], p1 = pstart[img[t] + 1];
  float bv = -1.0f;
  int bi = 0x7fffffff;
  for (int j = p0 + lane; j < p1; j += 64) {
    const float* b = pred + (size_t)j * 6;
    bool gt = false, lt = false;
    float inter = 1.f, va = 1.f, vb = 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gt = gt || a[3 + k] > b[k];
      lt = lt || a[k] < b[3 + k];
      inter *= fminf(a[3 + k], b[3 + k]) - fmaxf(a[k], b[k]) + 1.0f;
      va *= a[3 + k] - a[k] + 1.0f;
      vb *= b[3 + k] - b[k] + 1.0f;
    }
    const float uni = va + vb - inter;
    const float v = (gt && lt) ? (uni > 0.0f ? inter / uni : 0.0f) : 0.0f;
    if (v > bv) { bv = v; bi = j - p0; }      // ascending j within a lane: the first of equals stays
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
    best[t] = p1 > p0 ? bi : -1;
    best_iou[t] = p1 > p0 ? bv : 0.0f;
  }
}

extern "C" int adell_det_match(const float* targets, const int* target_image, int T, const float* preds,
                               const int* pred_start, int* best, float* best_iou, void* stream) {
  ADELL_REQUIRE(targets && target_image && pred_start && best && best_iou && T > 0, "det_match: bad arguments");
  return adell_launch<adell_det_match_kernel>(dim3(adell_cdiv(T, DET_NW)), dim3(DET_NT), 0,
                                              (hipStream_t)stream, targets, target_image, T, preds, pred_start,
                                              best, best_iou);
}

// ---- anchor-map encoding (utils/monai_transforms/bounding_boxes.py: BBToAdjustedAnchors.__call__) ---------
// One thread per output cell of out [B][1 + 7 A][S] (fp64, zero-filled here). Boxes are the outer loop and
// anchors the inner one, in the reference's order: a cell takes (iou, centre adjustment 3, log size ratio
// 3) of box i for anchor a when the anchor placed at the cell intersects the box, the pair's "iou" (one
// number per box and anchor, as the reference computes it: it can exceed 1) is > thresh, every
// |centre adjustment| < 1 and iou > the value already there (strict: the first box wins a tie); the class
// plane keeps the class of the last successful update. boxes [B][N][6] corner format in input voxels,
// half [A][3] = anchor / rel_sh / 2 in output cells, rel (by value) the boxes' input / output shape ratio.
struct DetEncodeArgs {
  const double* boxes;
  const double* classes;
  const int* counts;
  const double* half;
  double rel[3];
  double thresh;
  int B, N, A, H, W, D;
};
__global__ __launch_bounds__(DET_NT) void adell_det_encode_kernel(DetEncodeArgs q, double* __restrict__ out) {
  const long S = (long)q.H * q.W * q.D;
  const long m = (long)blockIdx.x * DET_NT + threadIdx.x;
  if (m >= (long)q.B * S) return;
  const long b = m / S, cell = m - b * S;
  const int idx[3] = {(int)(cell / ((long)q.W * q.D)), (int)((cell / q.D) % q.W), (int)(cell % q.D)};
  double* o = out + (size_t)b * (1 + 7 * q.A) * S + cell;
  for (int c = 0; c < 1 + 7 * q.A; ++c) o[(size_t)c * S] = 0.0;
  const int nb = min(max(q.counts[b], 0), q.N);
  for (int i = 0; i < nb; ++i) {
    const double* bx = q.boxes + ((size_t)b * q.N + i) * 6;
    double lo[3], hi[3], sz[3], ctr[3], bb_vol = 1.0;
    for (int j = 0; j < 3; ++j) {
      lo[j] = bx[j] / q.rel[j];
      hi[j] = bx[3 + j] / q.rel[j];
      sz[j] = hi[j] - lo[j];
      ctr[j] = (lo[j] + hi[j]) / 2.0;
      bb_vol *= sz[j] + 1.0 / q.rel[j];
    }
    for (int a = 0; a < q.A; ++a) {
      double adim[3], inter_vol = 1.0, anchor_vol = 1.0, adj[3];
      bool ok = true;
      for (int j = 0; j < 3; ++j) {
        const double hf = q.half[3 * a + j];
        adim[j] = (0.0 + hf + 0.5) - (0.0 - hf + 0.5);      // the reference measures the anchor at cell 0
        inter_vol *= fmin(sz[j], adim[j]) + 1.0 / q.rel[j];
        anchor_vol *= adim[j];
        const double alo = (double)idx[j] - hf + 0.5, ahi = (double)idx[j] + hf + 0.5;
        ok = ok && ahi > lo[j] && alo < hi[j];
        adj[j] = ctr[j] - ((double)idx[j] + 0.5);
        ok = ok && fabs(adj[j]) < 1.0;
      }
      const double iou = inter_vol / (anchor_vol + bb_vol - inter_vol);
      double* oa = o + (size_t)(1 + 7 * a) * S;
      if (ok && iou > q.thresh && iou > oa[0]) {
        oa[0] = iou;
        for (int j = 0; j < 3; ++j) {
          oa[(size_t)(1 + j) * S] = adj[j];
          oa[(size_t)(4 + j) * S] = log(sz[j] / adim[j]);
        }
        o[0] = q.classes[(size_t)b * q.N + i];
      }
    }
  }
}

extern "C" int adell_det_encode(const double* boxes, const double* classes, const int* counts,
                                const double* half, double rel0, double rel1, double rel2, double thresh,
                                int B, int N, int A, int H, int W, int D, double* out, void* stream) {
  ADELL_REQUIRE(counts && half && out && B > 0 && N >= 0 && A > 0 && H > 0 && W > 0 && D > 0,
                "det_encode: bad arguments");
  ADELL_REQUIRE(N == 0 || (boxes && classes), "det_encode: null boxes");
  const double cells = (double)B * H * W * D;
  ADELL_REQUIRE(cells * (1 + 7 * A) <= (double)(1L << 40) && cells <= (double)(1L << 30),
                "det_encode: grid too large");
  DetEncodeArgs q;
  q.boxes = boxes; q.classes = classes; q.counts = counts; q.half = half;
  q.rel[0] = rel0; q.rel[1] = rel1; q.rel[2] = rel2;
  q.thresh = thresh;
  q.B = B; q.N = N; q.A = A; q.H = H; q.W = W; q.D = D;
  const long blocks = ((long)cells + DET_NT - 1) / DET_NT;
  return adell_launch<adell_det_encode_kernel>(dim3((unsigned)blocks), dim3(DET_NT), 0, (hipStream_t)stream, q,
                                               out);
}
