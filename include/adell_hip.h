/*
 * adell_hip.h -- C ABI of libadellhip.so, the MI355X (gfx950) kernel library
 * behind the adell_mri U-Net / UNETR forward-backward path.
 *
 * The reference (CCIG-Champalimaud/adell-mri) is pure Python on torch and has
 * no FFI boundary of its own: the operators on its hot path are stock
 * torch.nn calls at the call sites cited on each entry point below (paths are
 * relative to the reference root). This header is the boundary a maintainer
 * binds instead of those calls (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *  - all tensors are fp32, dense, NDHWC ("channels_last_3d": the memory a
 *    torch tensor of logical shape [N,C,D,H,W] has after
 *    .contiguous(memory_format=torch.channels_last_3d));
 *  - pointers are device pointers unless stated; `stream` is a hipStream_t
 *    (NULL = default stream); nothing synchronises the host;
 *  - every function returns ADELL_OK or a negative ADELL_E_* code and never
 *    throws; adell_last_error() gives the message of the calling thread's
 *    last failure.
 */
#ifndef ADELL_HIP_H
#define ADELL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header
 * are exported (their definitions inherit the visibility of these declarations). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define ADELL_OK 0
#define ADELL_E_BADARG (-1)
#define ADELL_E_UNSUPPORTED (-2)
#define ADELL_E_HIP (-3)
#define ADELL_E_NOMEM (-4)

#define ADELL_ABI_VERSION 2

/* activation ids (reference: adell_mri/modules/activations.py:6-31) */
enum {
  ADELL_ACT_IDENTITY = 0,
  ADELL_ACT_SILU = 1, /* "swish" */
  ADELL_ACT_RELU = 2,
  ADELL_ACT_LEAKY_RELU = 3,
  ADELL_ACT_PRELU = 4,
  ADELL_ACT_GELU = 5,
  ADELL_ACT_SIGMOID = 6,
  ADELL_ACT_TANH = 7,
  ADELL_ACT_ELU = 8
};

int adell_abi_version(void);
const char* adell_last_error(void);

/* Launch-plan epoch. Every entry point that writes per-block partial sums (`stat_partials`,
 * `partials`) lays them out as [N][rows][C][2] with `rows` decided by the launch plan, and the
 * plan depends on process-wide switches (adell_set_tuning). ABI version 2: each such entry point
 * takes `partial_rows` = the rows per batch item the caller sized the buffer for (from the matching
 * *_ntiles query) and returns ADELL_E_BADARG -- before anything is launched -- when the plan of the
 * call would write a different number. adell_plan_epoch() changes whenever a switch changes, so a
 * caller may cache an *_ntiles answer per epoch. (Round 3 had a fault here: a row count cached on
 * the host across an adell_set_tuning flip made a kernel write twice the rows it had been given.) */
long adell_plan_epoch(void);

/* ------------------------------------------------------------------------
 * 3D convolution. Replaces torch.nn.Conv3d at unet.py:260-273 (conv_block_3d),
 * res_blocks.py:150-178 (ResidualBlock3d), unet.py:641-655 (final layer); the
 * two sources x0/x1 are the operands of torch.concat at unet.py:817 (never
 * materialised); `residual` is the "+ X" of res_blocks.py:192.
 * ---------------------------------------------------------------------- */
typedef struct adell_conv3d_desc {
  int32_t N, D, H, W; /* input batch / spatial size */
  int32_t C0, C1;     /* channels of source 0 and source 1 (C1 may be 0) */
  int32_t Cout;
  int32_t KD, KH, KW; /* 1..3 */
  int32_t SD, SH, SW; /* 1..2 */
  int32_t PD, PH, PW;
  int32_t Do, Ho, Wo; /* must equal (D + 2P - K) / S + 1 */
} adell_conv3d_desc;

/* Repack weights from the torch layout into the GEMM-B layouts the kernels
 * read. mode 0: conv [Cout=dim0][Cin=dim1][taps] -> [tap][Cin][Cout] (forward);
 * mode 1: same source -> [flipped tap][Cout][Cin] (backward-data);
 * mode 2: convT [Cin=dim0][Cout=dim1][8] -> [Cin][8][Cout] (forward);
 * mode 3: same source -> [tap][Cout][Cin] (backward-data). */
int adell_pack_weight(const float* w, float* out, int mode, int dim0, int dim1,
                      int KD, int KH, int KW, void* stream);

/* Rows of the statistics-partials buffer adell_conv3d_fwd writes per batch
 * item (buffer shape [N][ntiles][Cout][2] floats), or a negative error. */
int adell_conv3d_fwd_ntiles(const adell_conv3d_desc* d);

/* y = conv(concat(x0,x1), w) + bias + residual.  bias, residual, x1 and
 * stat_partials may be NULL. When stat_partials is given, per-block
 * per-channel (sum, sum of squares) of y are written for adell_stats_finalize
 * (InstanceNorm3d / BatchNorm3d statistics without re-reading y). */
int adell_conv3d_fwd(const adell_conv3d_desc* d, const float* x0, const float* x1,
                     const float* w_packed, const float* bias,
                     const float* residual, float* y, float* stat_partials,
                     int partial_rows, void* stream);

/* dX of the convolution above (autograd mirror of the same call sites).
 * dx0 receives channels [0,C0), dx1 channels [C0,C0+C1). */
int adell_conv3d_bwd_data(const adell_conv3d_desc* d, const float* dy,
                          const float* w_packed_bwd, float* dx0, float* dx1,
                          void* stream);

/* The same two operations on the f16 MFMA with error-compensated operand splitting
 * ("f16x3": a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulate, ~2^-22 relative
 * per product; per-chunk / per-layer power-of-two scaling inside the kernel). Tensors
 * stay fp32; only the packed weights differ: adell_pack_weight_f16x3 (mode 0 forward,
 * mode 1 backward-data) writes adell_pack_weight_f16x3_bytes(...) bytes of split fp16
 * tiles plus wscale: one undo factor per GEMM column (mode 0: Cout floats, mode 1: Cin). */
long adell_pack_weight_f16x3_bytes(int mode, int dim0, int dim1, int taps);
int adell_pack_weight_f16x3(const float* w, void* out, float* wscale, int mode, int dim0,
                            int dim1, int KD, int KH, int KW, void* stream);
/* The same for many weights in one launch: `table` is a DEVICE array of `entries` rows of 8
 * int64 {w pointer, out pointer, wscale pointer, mode, dim0, dim1, taps, first block}, rows
 * ordered by first block (= running sum of the GEMM-column counts: dim0 for mode 0, dim1 for
 * mode 1); total_blocks = that sum over all rows. */
int adell_pack_weight_f16x3_multi(const long* table, int entries, long total_blocks, void* stream);
int adell_conv3d_fwd_ntiles_f16x3(const adell_conv3d_desc* d);
/* the same for adell_conv3d_fwd_f16x3_ws (the split-K layers write one row per voxel range of
 * their fold, not per brick) */
int adell_conv3d_fwd_ntiles_f16x3_ws(const adell_conv3d_desc* d);
/* in_absmax / dy_absmax (optional, one zero-initialised uint32 on the device): receive
 * the bit pattern of the absmax of the kernel's input tensor(s) as a by-product;
 * adell_conv3d_bwd_weight_f16x3 takes them as its operand scales. */
int adell_conv3d_fwd_f16x3(const adell_conv3d_desc* d, const float* x0, const float* x1,
                           const void* w_split, const float* wscale, const float* bias,
                           const float* residual, float* y, float* stat_partials,
                           int partial_rows, uint32_t* in_absmax, void* stream);
int adell_conv3d_bwd_data_f16x3(const adell_conv3d_desc* d, const float* dy,
                                const void* w_split_bwd, const float* wscale, float* dx0,
                                float* dx1, uint32_t* dy_absmax, void* stream);

/* adell_conv3d_fwd_f16x3 with split-row sources (see adell_norm_act_fwd_split): xk0 / xk1 non-NULL
 * = that source is rows with exponents xk[N][C / 16], NULL = fp32. 3x3x3 stride-1 layers whose
 * launch plan is a specialised instance: adell_conv3d_f16x3_rows_ok(d) == 1 (else
 * ADELL_E_UNSUPPORTED). stat_partials rows: adell_conv3d_fwd_ntiles_f16x3(d). */
int adell_conv3d_f16x3_rows_ok(const adell_conv3d_desc* d);
int adell_conv3d_fwd_f16x3_rows(const adell_conv3d_desc* d, const void* x0, const int* xk0,
                                const void* x1, const int* xk1, const void* w_split,
                                const float* wscale, const float* bias, const float* residual,
                                float* y, float* stat_partials, int partial_rows,
                                uint32_t* in_absmax, void* stream);

/* Backward-data of a stride-2, k = 3 convolution by parity classes: dX[2i + p], p in {0,1}^3, is a
 * stride-1 convolution of dY with the sub-kernel w[:, :, t0z::2, t0y::2, t0x::2] (t0 = (p + P) mod 2
 * per axis), written onto the stride-2 lattice of dX. w_split[c] / wscale[c] (c = 4 pz + 2 py + px):
 * that sub-kernel packed with adell_pack_weight_f16x3 mode 1. Even input dims, C1 = 0. */
int adell_conv3d_bwd_data_s2_f16x3(const adell_conv3d_desc* d, const float* dy,
                                   const void* const* w_split, const float* const* wscale,
                                   float* dx, uint32_t* dy_absmax, void* stream);
/* ... + add0 ([N, D, H, W, C0] like dx: the gradient another consumer of the same input produced,
 * e.g. the decoder's half of a U-Net skip fork, unet.py:768-822) added in every class launch's
 * epilogue instead of by a separate full-size pass. */
int adell_conv3d_bwd_data_s2_f16x3_add(const adell_conv3d_desc* d, const float* dy,
                                       const void* const* w_split, const float* const* wscale,
                                       const float* add0, float* dx, uint32_t* dy_absmax,
                                       void* stream);

/* The U-Net downsampling layer (32 -> 32 channels, k = 3, stride 2, padding 1, even input dims:
 * unet.py:571-579) in ONE launch: a persistent block keeps the split weight in LDS, stages the dY
 * halo of a brick once and produces all eight parity classes of the dX voxels behind it
 * (csrc/conv_dgrad_s2.hip). w_split_bwd / wscale: adell_pack_weight_f16x3 mode 1 of the full
 * weight; add0: null or as above. _applicable: 1 when the layer qualifies. */
int adell_conv3d_bwd_data_s2_fused_applicable(const adell_conv3d_desc* d);
/* The forward of the same layer in one persistent launch (csrc/conv_fwd_s2.hip): the eight parity
 * sub-lattices of x behind an output brick are staged one after the other (a 51 KB halo each) and
 * accumulate into the same registers; bias, statistics partials ([N][_ntiles][32][2]) and the
 * absmax by-product as adell_conv3d_fwd_f16x3. w_split / wscale: adell_pack_weight_f16x3 mode 0. */
int adell_conv3d_fwd_s2_fused_applicable(const adell_conv3d_desc* d);
int adell_conv3d_fwd_s2_fused_ntiles(const adell_conv3d_desc* d);
int adell_conv3d_fwd_s2_fused(const adell_conv3d_desc* d, const float* x, const void* w_split,
                              const float* wscale, const float* bias, float* y,
                              float* stat_partials, int partial_rows, uint32_t* in_absmax,
                              void* stream);
int adell_conv3d_bwd_data_s2_fused(const adell_conv3d_desc* d, const float* dy,
                                   const void* w_split_bwd, const float* wscale,
                                   const float* add0, float* dx, uint32_t* dy_absmax, void* stream);

/* The same two calls with a caller-provided workspace (adell_conv3d_splitk_workspace bytes; 0 =
 * never needed): layers with too few output bricks to fill the chip (the 8^3 - 16^3 levels)
 * share the channel chunks of a brick out over several blocks (split-K) and fold the partial
 * outputs in fixed order -- bit-reproducible, bias / residual / statistics as in the plain call.
 * Without a workspace (or with one that is too small) they behave like the plain calls. */
long adell_conv3d_splitk_workspace(const adell_conv3d_desc* d, int backward_data);
/* Launch plan of the two _ws calls below (forward: backward_data = 0; backward-data: 1) given the
 * workspace adell_conv3d_splitk_workspace asks for: out[8] = {config (8: the 16-channel z-ring
 * kernel), brick voxels, columns per tile, log2 of the brick's x / y / z extents, K shares (1 = no
 * split), LDS bytes}. ADELL_E_UNSUPPORTED when the f16x3 kernel cannot take the problem. Host
 * only: launches nothing, reads no tensor, needs no GPU. */
int adell_conv3d_f16x3_plan(const adell_conv3d_desc* d, int backward_data, int* out);
int adell_conv3d_fwd_f16x3_ws(const adell_conv3d_desc* d, const float* x0, const float* x1,
                              const void* w_split, const float* wscale, const float* bias,
                              const float* residual, float* y, float* stat_partials,
                              int partial_rows, uint32_t* in_absmax, void* workspace,
                              size_t workspace_bytes, void* stream);
int adell_conv3d_bwd_data_f16x3_ws(const adell_conv3d_desc* d, const float* dy,
                                   const void* w_split_bwd, const float* wscale, float* dx0,
                                   float* dx1, uint32_t* dy_absmax, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* the same with add0 ([N][D][H][W][C0]; C1 must be 0) added to dx0 in the epilogue: the gradient a
 * residual link (res_blocks.py:192, `op(X) + X`) sends straight to the block input */
int adell_conv3d_bwd_data_f16x3_add(const adell_conv3d_desc* d, const float* dy,
                                    const void* w_split_bwd, const float* wscale,
                                    const float* add0, float* dx0, uint32_t* dy_absmax,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Backward-data fused with the backward of the norm -> dropout -> activation site(s) whose OUTPUT
 * the destination(s) are gradients of (reference: the autograd chain Conv3d <- activation <- Dropout
 * <- InstanceNorm3d of adn_fn.py:140-152 feeding unet.py:260-273 / res_blocks.py:150-178). site0 /
 * site1 describe the sites behind dx0 / dx1 (NULL: plain destination); their destinations receive
 *   dt = dout * act'(u) * keep / (1 - p),   u = dropout((y - mean) * rstd)
 * instead of dout, and `partials` ([N][ntiles][C0 + C1][2]) the per-brick sums (sum dt, sum dt xhat)
 * that adell_norm_act_bwd_from_dt folds. ntiles = adell_conv3d_bwd_data_f16x3_adn_ntiles(d); 0 means
 * the problem does not take the fused epilogue (the caller then uses the plain entry points). */
typedef struct adell_adn_site {
  const float* y;         /* the site's input, [N][D][H][W][C] like the destination */
  const float* mean;      /* [N][C] instance statistics of y */
  const float* rstd;
  const void* keep_mask;  /* keep bits written by adell_norm_act_fwd_mask; NULL iff drop_p == 0 */
  float drop_p;
  float act_p;            /* LeakyReLU slope */
  int32_t act;            /* ADELL_ACT_IDENTITY / _SILU / _RELU / _LEAKY_RELU */
} adell_adn_site;
int adell_conv3d_bwd_data_f16x3_adn_ntiles(const adell_conv3d_desc* d);
int adell_conv3d_bwd_data_f16x3_adn(const adell_conv3d_desc* d, const float* dy,
                                    const void* w_split_bwd, const float* wscale,
                                    const float* add0, float* dx0, float* dx1,
                                    uint32_t* dy_absmax, const adell_adn_site* site0,
                                    const adell_adn_site* site1, float* partials,
                                    int partial_rows, void* stream);

/* dW in torch's canonical [Cout][Cin][kD][kH][kW] layout (split-K over voxel
 * bricks, fixed-order reduction: deterministic) and, when db != NULL, the bias
 * gradient db[Cout] = sum over voxels of dy from the same pass. workspace:
 * device scratch of at least adell_conv3d_bwd_weight_workspace(d) bytes. */
long adell_conv3d_bwd_weight_workspace(const adell_conv3d_desc* d);
int adell_conv3d_bwd_weight(const adell_conv3d_desc* d, const float* x0,
                            const float* x1, const float* dy, float* dw, float* db,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The same on the f16 MFMA with error-compensated splitting (f16x3); X and dY get one
 * power-of-two scale per tensor (x_absmax / dy_absmax from the forward and backward-data
 * kernels, or NULL to have them reduced inside the call). */
long adell_conv3d_bwd_weight_f16x3_workspace(const adell_conv3d_desc* d);
int adell_conv3d_bwd_weight_f16x3(const adell_conv3d_desc* d, const float* x0,
                                  const float* x1, const float* dy, float* dw, float* db,
                                  const uint32_t* x_absmax, const uint32_t* dy_absmax,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* The same with split-row sources of X (see adell_norm_act_fwd_split): xk0 / xk1 non-NULL = that
 * source holds rows, ONE exponent per tensor (xk[0]); x_absmax then covers the fp32 source only.
 * _rows_ok(d) == 1: the z-ring kernel serves the problem and no 32-channel tile straddles the two
 * sources. Workspace: adell_conv3d_bwd_weight_f16x3_workspace(d). */
int adell_conv3d_bwd_weight_f16x3_rows_ok(const adell_conv3d_desc* d);
int adell_conv3d_bwd_weight_f16x3_rows(const adell_conv3d_desc* d, const void* x0, const int* xk0,
                                       const void* x1, const int* xk1, const float* dy, float* dw,
                                       float* db, const uint32_t* x_absmax,
                                       const uint32_t* dy_absmax, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* The two calls above with a share hint: what the caller knows about the streams around this one
 * launch (a per-call fact, not an adell_set_tuning switch: no plan, workspace or row count depends on
 * it, the plan epoch does not move, and dw / db are bit-identical under every hint).
 *   ADELL_WGRAD_SHARE_NONE    the plain calls, launch for launch;
 *   ADELL_WGRAD_SHARE_AUTO    other streams have kernels to run beside this launch: the 32 x 32 z-ring
 *                             kernel, whose two blocks per CU otherwise hold every CU until the launch
 *                             ends, requests enough dynamic LDS that ONE block per CU runs and an
 *                             implicit-GEMM block or the norm / activation kernels' waves fit beside
 *                             it. The library refuses the hint (and launches as the plain call) on
 *                             every other route, for the 16 x 16 z-ring form, for launches with no
 *                             more blocks than CUs, and for launches whose blocks march fewer than
 *                             96 planes (beside those it measured no gain or a loss);
 *   ADELL_WGRAD_SHARE_ALWAYS  the same without the two size conditions (tests, measurements).
 * adell_wgrad_zring_share_plan says what a hint does to a problem. */
#define ADELL_WGRAD_SHARE_NONE 0
#define ADELL_WGRAD_SHARE_AUTO 1
#define ADELL_WGRAD_SHARE_ALWAYS 2
int adell_conv3d_bwd_weight_f16x3_share(const adell_conv3d_desc* d, const float* x0,
                                        const float* x1, const float* dy, float* dw, float* db,
                                        const uint32_t* x_absmax, const uint32_t* dy_absmax,
                                        void* workspace, size_t workspace_bytes, void* stream,
                                        int share);
int adell_conv3d_bwd_weight_f16x3_rows_share(const adell_conv3d_desc* d, const void* x0,
                                             const int* xk0, const void* x1, const int* xk1,
                                             const float* dy, float* dw, float* db,
                                             const uint32_t* x_absmax, const uint32_t* dy_absmax,
                                             void* workspace, size_t workspace_bytes, void* stream,
                                             int share);
/* Launch plan of adell_conv3d_bwd_weight_f16x3 (and _rows), host only (no launch, no tensor read, no
 * device needed): what the call would run under the current tuning switches, from the same plan the
 * launch, the workspace query and _rows_ok read. Returns ADELL_OK, or ADELL_E_UNSUPPORTED when no
 * kernel takes the problem. out[25]:
 *   [0] route (ADELL_WGRAD_*); [1] regions = partial slabs the route writes (small: 0);
 *   [2], [3] adell_conv3d_bwd_weight_f16x3_workspace(d) as bytes & 0x7fffffff and bytes >> 31;
 *   [4] adell_conv3d_bwd_weight_f16x3_rows_ok(d);
 *   per-plane route (else 0): [5] MAXJ, [6] PFX, [7] PFY of the kernel instance (jobs per wave,
 *   16-byte prefetch loads per thread of X / dY; 0, 0 = staged in place), [8] log2 of the brick rows,
 *   [9] / [10] input / output channel tile, [11] k-groups of a 32 x 32 tile, [12] LDS bytes,
 *   [13] .. [15] grid extents x, y, z;
 *   z-ring routes (else 0): [16] .. [23] the plan[8] of adell_wgrad_zring_plan;
 *   [24] MAXJ of the instance adell_conv3d_bwd_weight (fp32) runs for d (0: small route or refused). */
#define ADELL_WGRAD_SMALL 0    /* Cin <= 4: vector-ALU kernel, exact fp32 */
#define ADELL_WGRAD_ZRING32 1  /* z-ring kernel, 32 x 32 channel tiles */
#define ADELL_WGRAD_ZRING16 2  /* z-ring kernel, 16 x 16 channel tiles */
#define ADELL_WGRAD_S2 3       /* stride-2 sub-lattice kernel (32 -> 32 downsampling layer) */
#define ADELL_WGRAD_PLANE 4    /* per-plane kernel */
int adell_conv3d_bwd_weight_f16x3_plan(const adell_conv3d_desc* d, int* out);

/* db[c] = sum over rows of dy[rows][C] (torch's bias gradient of Conv3d /
 * ConvTranspose3d). workspace >= adell_bias_grad_workspace(rows, C) bytes. */
long adell_bias_grad_workspace(long rows, int C);
int adell_bias_grad(const float* dy, long rows, int C, float* db, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * ConvTranspose3d(kernel=2, stride=2, padding=0): unet.py:445-458
 * (init_upscale_ops, upscale_type="transpose"), unetr.py:286-308.
 * x [N,D,H,W,Cin] -> y [N,2D,2H,2W,Cout].
 * ---------------------------------------------------------------------- */
/* General form: kernel = stride = (FD,FH,FW), each 1 or 2 (anisotropic upscaling of
 * backbone encoders, e.g. strides [2,2,1]); weights [Cin][Cout][FD][FH][FW]. */
int adell_convtranspose3d_fwd(int N, int D, int H, int W, int Cin, int Cout, int FD, int FH,
                              int FW, const float* x, const float* w_packed, const float* bias,
                              float* y, void* stream);
int adell_convtranspose3d_bwd_data(int N, int D, int H, int W, int Cin, int Cout, int FD,
                                   int FH, int FW, const float* dy, const float* w_packed_bwd,
                                   float* dx, void* stream);
/* The same two on the f16x3 kernels. Forward: w_split / wscale = adell_pack_weight_f16x3(mode 0)
 * of the virtual 1x1x1 conv weight V[(f, co)][ci] = w[ci][co][f] (F*Cout columns);
 * backward-data: mode 0 of the torch weight read as [Cin outputs][Cout inputs][taps]. */
int adell_convtranspose3d_fwd_f16x3(int N, int D, int H, int W, int Cin, int Cout, int FD, int FH,
                                    int FW, const float* x, const void* w_split,
                                    const float* wscale, const float* bias, float* y,
                                    uint32_t* in_absmax, void* stream);
int adell_convtranspose3d_bwd_data_f16x3(int N, int D, int H, int W, int Cin, int Cout, int FD,
                                         int FH, int FW, const float* dy, const void* w_split_bwd,
                                         const float* wscale, float* dx, uint32_t* dy_absmax,
                                         void* stream);
/* Launch plan of adell_convtranspose3d_fwd_f16x3 (out[8] as adell_conv3d_f16x3_plan, host only).
 * Its backward-data is the kernel = stride convolution that adell_conv3d_f16x3_plan describes. */
int adell_convtranspose3d_f16x3_plan(int N, int D, int H, int W, int Cin, int Cout, int FD, int FH,
                                     int FW, int* out);
long adell_convtranspose3d_bwd_weight_workspace(int N, int D, int H, int W, int Cin, int Cout,
                                                int FD, int FH, int FW);
int adell_convtranspose3d_bwd_weight(int N, int D, int H, int W, int Cin, int Cout, int FD,
                                     int FH, int FW, const float* x, const float* dy, float* dw,
                                     void* workspace, size_t workspace_bytes, void* stream);
int adell_convtranspose3d_k2s2_fwd(int N, int D, int H, int W, int Cin, int Cout,
                                   const float* x, const float* w_packed,
                                   const float* bias, float* y, void* stream);
int adell_convtranspose3d_k2s2_bwd_data(int N, int D, int H, int W, int Cin,
                                        int Cout, const float* dy,
                                        const float* w_packed_bwd, float* dx,
                                        void* stream);
/* dw in torch's canonical [Cin][Cout][2][2][2] layout. */
long adell_convtranspose3d_k2s2_bwd_weight_workspace(int N, int D, int H, int W,
                                                     int Cin, int Cout);
int adell_convtranspose3d_k2s2_bwd_weight(int N, int D, int H, int W, int Cin,
                                          int Cout, const float* x, const float* dy,
                                          float* dw, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Normalisation statistics and the fused Norm -> Dropout -> Activation of
 * ActDropNorm with ordering "NDA" (adn_fn.py:56-152; unet.py:697-714).
 * ---------------------------------------------------------------------- */
/* mean / rstd from partials [N][ntiles][C][2]; count = voxels per item; biased
 * variance, rstd = 1/sqrt(var+eps). per_item=1: [N][C] (torch.nn.InstanceNorm3d);
 * per_item=0: [C] over the whole batch (torch.nn.BatchNorm3d in training). */
long adell_stats_finalize_workspace(int N, int ntiles, int C); /* bytes, may be 0 */
int adell_stats_finalize(const float* partials, int N, int ntiles, int C,
                         long count, float eps, int per_item, float* mean,
                         float* rstd, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Running statistics of a BatchNorm site in training, from the batch (mean, rstd) of
 * adell_stats_finalize(per_item = 0) over `count` elements per channel (torch.nn.BatchNorm3d:
 * running = (1 - m) running + m batch, with the unbiased variance; num_batches_tracked (int64, may be
 * NULL) += 1; momentum < 0: the cumulative average m = 1 / num_batches_tracked). One launch. */
int adell_bn_running_update(const float* mean, const float* rstd, float* running_mean,
                            float* running_var, long long* num_batches_tracked, int C, long count,
                            float eps, float momentum, void* stream);
/* Synchronised batch norm (torch.nn.SyncBatchNorm): the statistics split where the sum over
 * data-parallel ranks goes. A site's record is 2C + 1 doubles [sum_c (C) | sum2_c (C) | count]:
 * one all-reduce (SUM) per site and direction between the two halves.
 * adell_bn_stats_sums: the record (sum x, sum x^2 over all N items, count = N * count) of partials
 *   [N][ntiles][C][2] (conv epilogue or adell_channel_partials), in the fixed-order fp64 fold of
 *   adell_stats_finalize; workspace as adell_stats_finalize_workspace.
 * adell_bn_stats_from_sums: mean / rstd [C] from a (reduced) record with adell_stats_finalize's
 *   formula; with running buffers (may be NULL) also adell_bn_running_update with the record's
 *   count. One launch. */
int adell_bn_stats_sums(const float* partials, int N, int ntiles, int C, long count, double* sums,
                        void* workspace, size_t workspace_bytes, void* stream);
int adell_bn_stats_from_sums(const double* sums, int C, float eps, float* mean, float* rstd,
                             float* running_mean, float* running_var,
                             long long* num_batches_tracked, float momentum, void* stream);
/* Partials of an arbitrary tensor x [N][V][C] (same buffer format). */
int adell_channel_partials_ntiles(long V);
int adell_channel_partials(const float* x, int N, long V, int C, float* partials,
                           void* stream);

typedef struct adell_norm_act_desc {
  int64_t N, V;           /* batch items, voxels per item */
  int32_t C;
  int32_t stats_per_item; /* 1: mean/rstd are [N][C] (instance); 0: [C] (batch) */
  int32_t act;            /* ADELL_ACT_* */
  int32_t act_w_n;        /* PReLU weight count (1 or C) when act_w != NULL */
  float act_p;            /* LeakyReLU slope / ELU alpha */
  float drop_p;           /* dropout probability, 0 = off (eval) */
  uint64_t seed;          /* Philox key; mask is a function of (seed, offset, index) */
  uint32_t rng_offset;    /* distinguishes ADN sites sharing one seed */
} adell_norm_act_desc;

/* out = act(dropout((x - mean) * rstd * gamma + beta)); mean/rstd, gamma, beta,
 * act_w may be NULL. */
int adell_norm_act_fwd(const adell_norm_act_desc* d, const float* x,
                       const float* mean, const float* rstd, const float* gamma,
                       const float* beta, const float* act_w, float* out,
                       void* stream);

/* The same, also writing the dropout keep bits (drop_p > 0): element el of batch item n is bit
 * (el >> 2) & 63 of 64-bit word (n * groups + (el >> 8)) * 4 + (el & 3), groups = ceil(V C / 256);
 * adell_norm_act_mask_bytes(d) bytes. All four words of every group are written, the bits past the
 * end of an item as 0. Needs C % 4 == 0 and a power-of-two C <= 1024 (returns
 * ADELL_E_UNSUPPORTED otherwise: the caller then keeps the regenerating backward). */
long adell_norm_act_mask_bytes(const adell_norm_act_desc* d);
int adell_norm_act_fwd_mask(const adell_norm_act_desc* d, const float* x, const float* mean,
                            const float* rstd, const float* gamma, const float* beta,
                            const float* act_w, float* out, void* keep_mask, void* stream);
/* Split rows (round 4): an activation stored as the LDS row image of the f16x3 convolution kernels
 * instead of fp32 values -- per voxel and 16-channel chunk one 64-byte row
 *   [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15]   fp16, hi = fp16(x 2^k), lo = fp16(x 2^k - hi)
 * (same bytes per element; 22 of the 24 mantissa bits, exactly what those kernels keep of an fp32
 * operand), with exponents xk[N][C / 16]. The consumer then stages its halo as a copy: no
 * block-wide absmax, no conversion on the vector ALU. Replaces the fp32 tensor between
 * `ActDropNorm` and the `Conv3d` that is its only reader (unet.py:260-273, res_blocks.py:150-178).
 *
 * adell_norm_act_fwd_split: adell_norm_act_fwd(_mask) writing rows scaled by 2^split_exp (the
 * caller knows a bound: an instance-normalised value is at most sqrt(V) in magnitude, dropout
 * scales by 1 / (1 - p), and |act(u)| <= |u| for the activations it is used with); C a power of two
 * in 16..1024; keep_mask as adell_norm_act_fwd_mask or NULL.
 * adell_split_rows_from_f32 / _to_f32: the conversions for any tensor with known exponents. */
int adell_norm_act_fwd_split(const adell_norm_act_desc* d, const float* x, const float* mean,
                             const float* rstd, const float* gamma, const float* beta,
                             const float* act_w, void* out_rows, int split_exp, void* keep_mask,
                             void* stream);
int adell_split_rows_from_f32(const float* x, int N, long V, int C, const int* xk, void* rows,
                              void* stream);
int adell_split_rows_to_f32(const void* rows, int N, long V, int C, const int* xk, float* x,
                            void* stream);
/* Second half of the site's backward when the producer of dout already applied the activation /
 * dropout derivative (adell_conv3d_bwd_data_f16x3_adn): dx = rstd * (dt - c1 - xhat * c2) with
 * c1 / c2 the means of the partial sums. partials: [N][ntiles][pstride][2], the site's channels
 * at columns [poff, poff + C). dx may alias dt. Instance statistics, no affine parameters.
 * workspace: (2 + 2 * ceil(ntiles / 256)) * N * C floats. */
int adell_norm_act_bwd_from_dt(const adell_norm_act_desc* d, const float* x, const float* dt,
                               const float* mean, const float* rstd, const float* partials,
                               int ntiles, int pstride, int poff, float* dx, void* workspace,
                               size_t workspace_bytes, void* stream);

/* dx (and optionally dgamma / dbeta [C]) of adell_norm_act_fwd; the dropout
 * mask is regenerated from (seed, rng_offset). workspace >=
 * adell_norm_act_bwd_workspace(d) bytes (needed when a norm or affine grad is
 * involved). */
long adell_norm_act_bwd_workspace(const adell_norm_act_desc* d);
int adell_norm_act_bwd(const adell_norm_act_desc* d, const float* x, const float* dout,
                       const float* mean, const float* rstd, const float* gamma,
                       const float* beta, const float* act_w, float* dx, float* dgamma,
                       float* dbeta, void* workspace, size_t workspace_bytes,
                       void* stream);
/* adell_norm_act_bwd of a synchronised batch-norm site (stats_per_item = 0), in two halves around
 * the all-reduce of a 2C + 1 double record [sum dt (C) | sum dt * xhat (C) | count]:
 * adell_norm_act_bwd_sums: the partials kernels of adell_norm_act_bwd, folded into the record;
 *   the local dgamma / dbeta (may be NULL). Workspace: adell_norm_act_bwd_workspace(d) bytes.
 * adell_norm_act_bwd_apply_sums: c1 / c2 from a (reduced) record, then dx with the apply kernels
 *   of adell_norm_act_bwd. Workspace: 2 C floats. */
int adell_norm_act_bwd_sums(const adell_norm_act_desc* d, const float* x, const float* dout,
                            const float* mean, const float* rstd, const float* gamma,
                            const float* beta, const float* act_w, double* sums, float* dgamma,
                            float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int adell_norm_act_bwd_apply_sums(const adell_norm_act_desc* d, const float* x, const float* dout,
                                  const float* mean, const float* rstd, const float* gamma,
                                  const float* beta, const float* act_w, const double* sums,
                                  float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* adell_norm_act_bwd with a LOW-RANK upstream gradient dout[v][c] = sum_o g[v][o] * w[o][c]
 * (g: [N][V][co] channels-last, w: [co][C], 1 <= co <= 4): the site in front of a 1x1x1 conv with
 * few output channels -- the logits head Conv3d -> ADN -> Conv3d(C -> n_classes, k = 1) of
 * lib/modules/segmentation/unet.py:626-655 -- takes that conv's dY and weight, and the conv's
 * backward-data tensor is neither written nor read. Instance statistics without affine
 * parameters; power-of-two C in 4..1024, 16-byte aligned x / dx; workspace as for
 * adell_norm_act_bwd. */
int adell_norm_act_bwd_lowrank(const adell_norm_act_desc* d, const float* x, const float* g,
                               const float* w, int co, const float* mean, const float* rstd,
                               float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* Launch plan of a norm / dropout / activation site, host only (no launch, no tensor read, no
 * device needed): what adell_norm_act_fwd(_mask / _split), adell_norm_act_bwd(_lowrank / _sums /
 * _apply_sums) and adell_norm_act_bwd_from_dt would run, decided by the same function the launches
 * call. Routes:
 *   scalar: any C, any alignment; float4: C % 4 == 0 and 16-byte aligned tensors (both grid-stride
 *   above a grid cap); fast: float4's conditions and a power-of-two C <= 1024 (one grid row per
 *   item, contiguous chunks per block); narrow: the fast kernels at C = 1 or 2 with V C % 4 == 0.
 * The forward looks at x and out, the backward (both passes) at x, dout and dx.
 * aligned: ADELL_NA_ALIGNED_* bits of the tensors that are 16-byte aligned (set the bit of a tensor
 *   the call does not have); want_mask: keep bits are wanted (stored only when drop_p > 0);
 *   split: split-row output; lowrank: factors of a low-rank dout (0: a full dout); norm: the site
 *   has mean / rstd; affine_grads: dgamma or dbeta is wanted. out[10]:
 *   [0] forward route (ADELL_NA_*; REFUSED: keep bits or split rows off the fast route -- what the
 *       entry points answer with ADELL_E_UNSUPPORTED / ADELL_E_BADARG); [1], [2] forward grid x, y;
 *   [3] backward route (REFUSED: a low-rank dout off the fast route; adell_norm_act_bwd_from_dt
 *       needs ADELL_NA_FAST); [4] partial rows per item its reduction pass writes (0: no such
 *       pass); [5], [6] grid x, y of its dx pass;
 *   [7] finalize kernel (ADELL_NA_FIN_*; the record of adell_norm_act_bwd_sums is its own);
 *   [8] workspace bytes adell_norm_act_bwd requires (adell_norm_act_bwd_workspace, or 0 without a
 *       reduction pass); [9] bytes of keep bits the forward stores (0: none).
 * adell_norm_act_stats_plan: how adell_stats_finalize, adell_bn_stats_sums and
 *   adell_norm_act_bwd_from_dt reduce `ntiles` partial rows per item. out[5]: [0] levels (1, or 2
 *   above 512 rows: 256 rows at a time are folded first); [1] rows per item after the first level
 *   (0 with one level); [2] workspace bytes of the folded rows (adell_stats_finalize_workspace;
 *   adell_norm_act_bwd_from_dt adds 2 N C floats); [3] rows from which the all-items finalize and
 *   the record kernel keep eight rows in flight; [4] rows from which the per-item backward
 *   finalize keeps two. */
#define ADELL_NA_SCALAR 0
#define ADELL_NA_FLOAT4 1
#define ADELL_NA_FAST 2
#define ADELL_NA_NARROW 3
#define ADELL_NA_REFUSED 4
#define ADELL_NA_FIN_NONE 0
#define ADELL_NA_FIN_PER_ITEM 1
#define ADELL_NA_FIN_ALL_ITEMS 2
#define ADELL_NA_ALIGNED_X 1
#define ADELL_NA_ALIGNED_OUT 2
#define ADELL_NA_ALIGNED_DOUT 4
#define ADELL_NA_ALIGNED_DX 8
int adell_norm_act_plan(const adell_norm_act_desc* d, int aligned, int want_mask, int split,
                        int lowrank, int norm, int affine_grads, long* out);
int adell_norm_act_stats_plan(int N, int ntiles, int C, long* out);
/* Gradient of the PReLU weight(s) of the same fused op (torch.nn.PReLU is the reference's
 * default activation_fn): dact_w[act_w_n] with act_w_n = 1 or C; operands as above. */
long adell_prelu_wgrad_workspace(const adell_norm_act_desc* d);
int adell_prelu_wgrad(const adell_norm_act_desc* d, const float* x, const float* dout,
                      const float* mean, const float* rstd, const float* gamma, const float* beta,
                      float* dact_w, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Segmentation loss: binary generalised dice + binary focal on probabilities
 * (losses.py:14-54,251-292 with weight=1, scale=1; losses.py:112-164 with
 * alpha=1, threshold=0.5, scale=1, no label smoothing), the CompoundLoss of
 * sample_configs/u-net-3d-resnet.yaml evaluated at segmentation/pl.py:218-222.
 * prob/target are [B][S]; dice/focal are the per-item losses; sums [B][3] is
 * scratch kept for the backward.
 * ---------------------------------------------------------------------- */
long adell_dice_focal_workspace(int B, long S);
int adell_dice_focal_fwd(const float* prob, const float* target, int B, long S,
                         float smooth, float dice_eps, float gamma, float focal_alpha, float focal_eps,
                         float* dice, float* focal, float* sums, void* workspace,
                         size_t workspace_bytes, void* stream);
/* dprob = gdice * d(dice_b)/dprob + gfocal * d(focal_b)/dprob */
int adell_dice_focal_bwd(const float* prob, const float* target, int B, long S,
                         float smooth, float dice_eps, float gamma, float focal_alpha, float focal_eps,
                         const float* sums, float gdice, float gfocal, float* dprob,
                         void* stream);
/* the same with per-item upstream gradients on the device (gdice[B], gfocal[B], NULL = 0) */
int adell_dice_focal_bwd_dev(const float* prob, const float* target, int B, long S, float smooth,
                             float dice_eps, float gamma, float focal_alpha, float focal_eps,
                             const float* sums, const float* gdice, const float* gfocal,
                             float* dprob, void* stream);
/* (focal_alpha: weight of the positive-class term, `alpha` of binary_focal_loss, losses.py:112-164)
 *
 * Per-(item, class) sums (sum p t, sum p, sum t) of probabilities / targets laid out [B][V][C]: the
 * building block of the Tversky-type losses (binary_focal_tversky_loss losses.py:295-337,
 * mc_focal_tversky_loss :656-698 and, through them, hybrid_focal / unified_focal :386-462, 737-808).
 * Backward: dp[b][v][c] = gsums[b][c][0] * t[b][v][c] + gsums[b][c][1]. */
long adell_class_sums_workspace(int B, long V, int C);
int adell_class_sums_fwd(const float* p, const float* t, int B, long V, int C, float* sums,
                         void* workspace, size_t workspace_bytes, void* stream);
int adell_class_sums_bwd(const float* t, const float* gsums, int B, long V, int C, float* dp,
                         void* stream);

/* ------------------------------------------------------------------------
 * Optimiser / EMA updates over flat fp32 buffers (16-byte aligned).
 * adell_sgd_step: torch.optim.SGD(momentum, nesterov, weight_decay), the
 *   default optimiser of UNetBasePL.configure_optimizers (segmentation/pl.py:563-569);
 * adell_adamw_step: torch.optim.AdamW (self_supervised/pl.py:245-250);
 * adell_ema_update: ExponentialMovingAverage.update (utils/utils.py:447-493).
 * grad_scale multiplies the gradient first (1/world_size after a sum
 * all-reduce, 1/accumulate_grad_batches). The betas (and c5 below) are doubles: 1 - beta and
 * the bias corrections are formed from them in double, as torch.optim forms them, and rounded once.
 * ---------------------------------------------------------------------- */
int adell_sgd_step(float* param, const float* grad, float* momentum_buf, long n, float lr,
                   float momentum, float weight_decay, int nesterov, int first_step,
                   float grad_scale, void* stream);
int adell_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     long n, float lr, double beta1, double beta2, float eps,
                     float weight_decay, long step, float grad_scale, void* stream);
/* torch.optim.Adam ("adam" of optimizer_factory.py:5-14): as above with the weight decay added
 * to the gradient instead of decoupled. */
int adell_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                    float lr, double beta1, double beta2, float eps, float weight_decay, long step,
                    float grad_scale, void* stream);

/* The other optimisers of the reference's factory (utils/optimizer_factory.py:5-14), torch.optim
 * single-tensor semantics, L2 weight decay added to the gradient: kind 0 Adamax (state1 exp_avg,
 * state2 exp_inf), 1 Adagrad (sum), 2 NAdam (exp_avg, exp_avg_sq), 3 RAdam (exp_avg, exp_avg_sq),
 * 4 RMSprop (square_avg; momentum 0, not centered). c5: HOST array of the five per-step scalars
 * documented at adell_optim_kernel (csrc/loss_optim.hip). */
int adell_optim_step(int kind, float* param, const float* grad, float* state1, float* state2,
                     long n, float weight_decay, float eps, float grad_scale, const double* c5,
                     void* stream);
int adell_ema_update(float* shadow, const float* param, long n, float decay, void* stream);

/* ------------------------------------------------------------------------
 * Token-sequence kernels of the ViT encoder (UNETR): vit.py:844-1002,
 * linear_blocks.py:358-417. (torch.nn.Linear runs on adell_conv3d_* as a
 * 1x1x1 convolution over the token axis.)
 * ---------------------------------------------------------------------- */
/* torch.nn.LayerNorm over the last dim of x [rows][C]; gamma/beta may be NULL;
 * mean/rstd [rows] are kept for the backward. */
int adell_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                        float* mean, float* rstd, long rows, int C, float eps, void* stream);
long adell_layernorm_bwd_workspace(long rows, int C);
int adell_layernorm_bwd(const float* x, const float* dy, const float* gamma,
                        const float* mean, const float* rstd, float* dx, float* dgamma,
                        float* dbeta, long rows, int C, void* workspace,
                        size_t workspace_bytes, void* stream);
/* out[i] = a[i] + b[i % period] (X + positional_embedding, vit.py:866-867) and the
 * gradient of b: db[j] = sum_k g[k*period + j]. */
int adell_add_bcast(const float* a, const float* b, float* out, long n, long period,
                    void* stream);
int adell_sum_bcast(const float* g, float* db, long n, long period, void* stream);
/* softmax(q k^T * scale + bias) v per sequence, F.scaled_dot_product_attention as called at
 * linear_blocks.py:407-414. adell_attention_desc holds everything of a call that is not one of its
 * tensors; the three entries below take it and their tensors.
 *
 * Contiguous operands (strided = 0): q,k [BH][T][A]; v,out [BH][T][Dv]; lse [BH][T]. Head dims A, Dv
 * up to 256, in the forward and the backward alike, any alignment (adell_attention_plan below).
 * bias [nbias][T][T] or NULL: sequence bh uses bias[bh % nbias].
 * drop_p > 0 drops attention probabilities (dropout_p of the same call): the mask of entry
 * (bh, query, key) is a Philox function of (seed, rng_offset), regenerated by the backward.
 *
 * Region labels: labels int32 [nlab][T] or NULL. Item b (sequences b * H .. b * H + H - 1; contiguous
 * calls take H for this alone) reads row b % nlab, and the score of query i and key j gains -100
 * where labels[i] != labels[j], after scale and bias: the shifted-window mask of SWIN
 * (vit.py:132-207) without its [n_windows][T][T] expansion. NULL labels run the same kernels with the
 * term left out: the results without labels are the same bit for bit whatever nlab and H say.
 *
 * Strided operands (strided != 0): every operand is addressed by element strides, sequence
 * bh = b * H + h (BH a multiple of H), stride[i] = (item b, head h, token row) of operand i in the
 * order q, k, v, out, dout, dq, dk, dv -- the forward reads the first 4, the bias gradient the
 * first 5, the backward all 8. Q / K / V may stay inside the packed [B][T][H][q | k | v] projection
 * output of linear_blocks.py:372-385, O / dO are [B][T][H * Dv] token rows, dV can land inside the
 * packed gradient: the slice / permute copies around F.scaled_dot_product_attention
 * (linear_blocks.py:380-417) are not launches. In the forward and the backward the strides are
 * multiples of 4 elements with rows at least the head width apart, the pointers 16-byte aligned, and
 * the heads MFMA-shaped (A, Dv in {32, 64, 128}, T >= 16: the forward plan with aligned = 1 is an
 * MFMA path); anything else is ADELL_E_BADARG before any launch, and the backward refuses before
 * its first launch whichever of its two passes has no kernel. */
typedef struct adell_attention_desc {
  int32_t BH;           /* sequences */
  int32_t H;            /* sequences per item: label rows, strided addressing */
  int32_t T, A, Dv;     /* tokens, q / k head dim, v / out head dim */
  float scale;          /* of q k^T */
  float drop_p;         /* attention-probability dropout, 0 = off */
  uint32_t rng_offset;  /* distinguishes the calls that share one seed */
  uint64_t seed;        /* Philox key */
  const float* bias;    /* [nbias][T][T] or NULL */
  const int32_t* labels; /* [nlab][T] or NULL */
  int32_t nbias, nlab;
  int32_t strided;      /* 0: contiguous operands, `stride` is not read */
  int64_t stride[8][3]; /* (item, head, row) of q, k, v, out, dout, dq, dk, dv */
} adell_attention_desc;
int adell_attention_fwd(const adell_attention_desc* d, const float* q, const float* k,
                        const float* v, float* out, float* lse, void* stream);
int adell_attention_bwd(const adell_attention_desc* d, const float* q, const float* k,
                        const float* v, const float* out, const float* dout, const float* lse,
                        float* dq, float* dk, float* dv, void* stream);
/* Launch plan of one attention pass, host only (no launch, no tensor read, no device needed): what
 * adell_attention_fwd (pass 0) or the dQ (pass 1) and dK/dV (pass 2) kernels of adell_attention_bwd
 * would run under the current tuning switches, decided by the same function the launches call.
 * aligned: every tensor of the call (forward: q, k, v, out; backward: those and dout, dq, dk, dv) is
 * 16-byte aligned -- the MFMA kernels stage with 16-byte loads, other operands take the vector-ALU
 * kernels (the strided entries refuse them). out[4]:
 *   [0] path (ADELL_ATT_*); [1] dynamic LDS bytes; [2] blocks per sequence (grid x; grid y = BH);
 *   [3] query (pass 2: key) rows per block.
 * MFMA paths: A, Dv in {32, 64, 128} and T >= 16; resident while the sequence, padded to a multiple
 * of 32 rows of A + Dv + 2 (pass 2: + 4) floats, fits 150 KiB of LDS. Vector-ALU: head dims up to
 * 256 in all three passes; the backward kernels work on 8 instead of 16 rows per block where 16
 * would not fit 160 KiB (A + Dv > 507 for dQ, > 502 for dK/dV). Refused: head dims above 256
 * (forward and backward alike, before any launch). */
#define ADELL_ATT_VALU 0
#define ADELL_ATT_MFMA_RESIDENT 1
#define ADELL_ATT_MFMA_STREAMED 2
#define ADELL_ATT_REFUSED 3
int adell_attention_plan(int pass, int T, int A, int Dv, int aligned, int* out);
/* Gradient of the additive bias: dbias[j] = sum over sequences bh % nbias == j of
 * dS[bh] = P o (keep dP / (1 - drop_p) - rowsum(dO o O)), [nbias][T][T], no `scale` factor (the bias
 * is added after it). d->nbias in [1, BH] is the number of result slices whether or not d->bias is
 * NULL: H gives the gradient of a per-head bias, BH the plain dS. Scores, labels and the dropout
 * mask are rebuilt as the backward kernels build them. Operands as in adell_attention_bwd, but
 * strided ones need only rows at least the head width apart and non-negative strides: head dims
 * 32 / 64 / 128 at T >= 16 with 16-byte aligned pointers and strides that are multiples of 4 run on
 * the MFMA, everything else up to head dims of 256 on the vector ALU (the form is the one the dQ pass
 * of the same operands plans). No atomics: the sequences of a slice are summed in ascending order
 * within a chunk, the chunks in order by a second pass through `workspace`, whose size
 * (adell_attention_bias_grad_workspace_floats: at most 16 partial results, and at most 512 tiles of
 * 128 x 128 floats) does not depend on the number of sequences. Nothing of BH * T * T elements
 * is ever written. The slices are the y dimension of the grid: nbias above 65535 is refused with
 * ADELL_E_BADARG (the attention entries above put BH there and fail at the launch beyond it). */
long adell_attention_bias_grad_workspace_floats(int nbias, int T);
int adell_attention_bias_grad(const adell_attention_desc* d, const float* q, const float* k,
                              const float* v, const float* out, const float* dout,
                              const float* lse, float* dbias, float* workspace,
                              long workspace_floats, void* stream);

/* ------------------------------------------------------------------------
 * Data movement for the U-Net++ dense links (standard_blocks.py:365-371):
 * N-way channel concat / split of NDHWC tensors, and nearest-neighbour
 * resampling (F.interpolate's default mode) with its backward.
 * ---------------------------------------------------------------------- */
/* direction 0: full[v][coff + c] = part[v][c]; direction 1: the reverse copy. */
int adell_copy_channels(float* full, float* part, long V, int Cfull, int Cpart, int coff,
                        int direction, void* stream);
int adell_interp_nearest_fwd(const float* x, float* y, int N, int C, int Di, int Hi, int Wi,
                             int Do, int Ho, int Wo, void* stream);
int adell_interp_nearest_bwd(const float* dy, float* dx, int N, int C, int Di, int Hi, int Wi,
                             int Do, int Ho, int Wo, void* stream);
/* torch.nn.Upsample(scale_factor, mode="bilinear" | "trilinear", align_corners=False) of the
 * "upsample" upscaling path (unet.py:419-443): x [N][Di][Hi][Wi][C] -> y [N][Do][Ho][Wo][C] with
 * Do = floor(Di * scale_d) etc.; a 2-D tensor is Di = Do = 1, scale_d = 1. align_corners != 0:
 * F.interpolate(size=(Do,Ho,Wo), align_corners=True) (the deep-supervision targets of
 * pl.py:305-309; the scale arguments are then ignored). The backward gathers (deterministic). */
int adell_interp_linear_fwd(const float* x, float* y, int N, int C, int Di, int Hi, int Wi,
                            int Do, int Ho, int Wo, float scale_d, float scale_h, float scale_w,
                            int align_corners, void* stream);
int adell_interp_linear_bwd(const float* dy, float* dx, int N, int C, int Di, int Hi, int Wi,
                            int Do, int Ho, int Wo, float scale_d, float scale_h, float scale_w,
                            int align_corners, void* stream);

/* y[n][v][c] = x[n][v][c] * s[n][c] on NDHWC activations (x, y: [N][V][C]; s: [N][C]): the tabular
 * feature gates of the decoder (unet.py:803-810) and U-out (regularization.py:48-55). The
 * backward is the same call on dy (dx = dy * s) plus ds[n][c] = sum_v dy * x
 * (adell_scale_bc_dscale; workspace of adell_scale_bc_dscale_workspace_floats floats). */
/* out[n][z][y][ox][kx * Cin + ci] = x[n][z][y][ox - P + kx][ci] (zeros outside the row and in the
 * slots >= K * Cin), x [N][D][H][W][Cin], out [N][D][H][W + 2P - K + 1][Cp]: the x taps of a
 * small-Cin convolution folded into a 16-channel chunk, so that a Kd x Kh x K conv over Cin <= 4
 * channels runs as a Kd x Kh x 1 conv over Cp channels (first layers: unet.py:260-273,
 * res_net.py:60-130). */
int adell_fold_x_taps(const float* x, float* out, int N, int D, int H, int W, int Cin, int K,
                      int P, int Cp, void* stream);
int adell_scale_bc(const float* x, const float* s, float* y, int N, long V, int C, void* stream);
long adell_scale_bc_dscale_workspace_floats(int N, long V, int C);
int adell_scale_bc_dscale(const float* x, const float* dy, float* ds, int N, long V, int C,
                          float* workspace, void* stream);

/* Concurrent squeeze-and-excite gate used where the multi-branch U-Net merges its encoders
 * (reference adell_mri/modules/layers/self_attention.py:21-150 ConcurrentSqueezeAndExcite{2,3}d,
 * called at adell_mri/modules/segmentation/unet.py:1186-1207): y = acc + x * (s[n][v] + c[n][ch]) *
 * inv[n]. x, acc, y: [N][V][C] (NDHWC); s: [N][V] spatial gate; c: [N][C] channel gate; inv: [N] or
 * null (1); acc null = 0. Backward: dx, ds [N][V], dc [N][C] (C <= 512; workspace of
 * adell_cse_apply_bwd_workspace_floats floats). */
int adell_cse_apply(const float* x, const float* s, const float* c, const float* inv,
                    const float* acc, float* y, int N, long V, int C, void* stream);
long adell_cse_apply_bwd_workspace_floats(int N, long V, int C);
int adell_cse_apply_bwd(const float* x, const float* dy, const float* s, const float* c,
                        const float* inv, float* dx, float* ds, float* dc, int N, long V, int C,
                        float* workspace, void* stream);
/* out[n][v][ch] = g[n][ch] * scale: gradient of the per-channel spatial mean the channel gate is
 * computed from (self_attention.py:95-96, torch.flatten(X, 2).mean(-1)). */
int adell_bcast_nc(const float* g, float* out, int N, long V, int C, float scale, void* stream);

/* torch.nn.MaxPool3d (ceil_mode False, dilation 1, -inf padding): unet.py:335,368,
 * 595-603, res_net.py:180,209. Geometry in an adell_conv3d_desc (C0 = channels, C1 and
 * Cout ignored); argmax [N][Do][Ho][Wo][C] holds the winner's (z*H+y)*W+x. */
int adell_maxpool3d_fwd(const adell_conv3d_desc* d, const float* x, float* y,
                        int32_t* argmax, void* stream);
int adell_maxpool3d_bwd(const adell_conv3d_desc* d, const float* dy, const int32_t* argmax,
                        float* dx, void* stream);

/* ------------------------------------------------------------------------
 * ConvNeXt / VICReg self-supervised path (BASELINE config 4).
 * Depthwise Conv3d(groups=C, stride 1, "same" padding, odd kernels):
 * res_blocks.py:552-558. w / dw in torch's [C][1][KD][KH][KW] layout.
 * ---------------------------------------------------------------------- */
int adell_dwconv3d_fwd(int N, int C, int D, int H, int W, int KD, int KH, int KW,
                       const float* x, const float* w, const float* bias, float* y,
                       void* stream);
int adell_dwconv3d_bwd_data(int N, int C, int D, int H, int W, int KD, int KH, int KW,
                            const float* dy, const float* w, float* dx, void* stream);
/* workspace: adell_dwconv3d_bwd_weight_workspace_floats(...) floats (split partial sums of
 * the tiled kernel; may be NULL when that returns 0) */
long adell_dwconv3d_bwd_weight_workspace_floats(int N, int C, int D, int H, int W, int KD, int KH,
                                                int KW);
int adell_dwconv3d_bwd_weight(int N, int C, int D, int H, int W, int KD, int KH, int KW,
                              const float* x, const float* dy, float* dw, float* db,
                              float* workspace, void* stream);
/* VICReg terms of two [B][D] embeddings (self_supervised/losses/vicreg.py:60-140):
 * out3 = (invariance, variance, covariance), unweighted; scratch of
 * adell_vicreg_scratch_floats(B, D) floats is kept for the backward, which returns
 * g3[0]*d(inv) + g3[1]*d(var) + g3[2]*d(cov) (g3: 3 floats on the device) w.r.t. x1 (dx1) and x2 (dx2, may be NULL). */
long adell_vicreg_scratch_floats(int B, int D);
int adell_vicreg_fwd(const float* x1, const float* x2, int B, int D, float min_var, float eps,
                     float* scratch, float* out3, void* stream);
int adell_vicreg_bwd(const float* x1, const float* x2, int B, int D, float min_var, float eps,
                     const float* scratch, const float* g3, float* dx1, float* dx2,
                     void* stream);

/* Local VICReg loss (VICRegLocalLoss, self_supervised/losses/vicreg.py:168-404; csrc/vicregl.hip).
 * adell_top_pairs: per item the gamma pairs (i, j) of token rows a[b][i][:], b[b][j][:] (both
 * [B][T][C], channels innermost) with the LARGEST Euclidean distance, ordered by (distance
 * descending, flat index i T + j ascending): pairs is int32 [B][gamma][2], dist2 (may be NULL) the
 * squared distances [B][gamma], fp32 sums of (a - b)^2 over the channels in order. The T x T matrix
 * is never written. workspace: adell_top_pairs_workspace_words(B, T, gamma) 8-byte words, 8-byte
 * aligned. 1 <= gamma <= 64, gamma <= T^2, T <= 65535, else ADELL_E_UNSUPPORTED.
 * adell_top_pairs_boxes: the same ranking of the distances between the token grid (dims[0 .. ndim),
 * row-major, ndim 2 or 3; dims on the host) mapped into each view's box, grid * (hi - lo) + lo with
 * box = (lo..., hi...) as [B][2 ndim]; T = prod(dims).
 * adell_gather_rows_fwd: out[b gamma + k][:] = x[b][pairs[b][k][col]][:] (x [B][T][C], col 0 or 1);
 * adell_gather_rows_bwd: dx = 0, then dx[b][pairs[b][k][col]][:] += dout[b gamma + k][:] for k in
 * order, one thread per (item, channel): no float atomics, duplicates welcome, bit-reproducible. */
long adell_top_pairs_workspace_words(int B, int T, int gamma);
int adell_top_pairs(const float* a, const float* b, int B, int T, int C, int gamma, void* workspace,
                    long workspace_words, int* pairs, float* dist2, void* stream);
int adell_top_pairs_boxes(const float* box1, const float* box2, int B, int ndim, const int* dims,
                          int gamma, void* workspace, long workspace_words, int* pairs,
                          float* dist2, void* stream);
int adell_gather_rows_fwd(const float* x, const int* pairs, int col, int B, int T, int C, int gamma,
                          float* out, void* stream);
int adell_gather_rows_bwd(const float* dout, const int* pairs, int col, int B, int T, int C,
                          int gamma, float* dx, void* stream);

/* DINO (self_supervised/dino.py, losses/dino.py; csrc/dino.hip). All tensors fp32 and dense, rows of
 * K floats at any 4-byte address; no float atomics, results repeat bit for bit.
 * adell_dino_loss_plan: out = {chunks per row, chunk length}: how adell_dino_loss_fwd / _bwd split a
 * row over workgroups (host only; the launches call this same function).
 * adell_dino_loss_fwd: loss_rows[r] = -sum_k p_t[r][k] log_softmax(a / t1)[r][k], p_t =
 * softmax((b - centers) / t2) (centers [K] or NULL = zeros) or, with teacher_is_scores, b itself
 * (its row sum is accumulated, not assumed 1). stats [R][4] = (lse of a / t1, lse of (b - centers) / t2
 * | sum_k b, loss_r, sum_k p_t a | 0) is all the backward needs. workspace: adell_dino_loss_workspace_floats(R, K).
 * loss_mean (may be NULL): 1 float, the mean of loss_rows in a fixed order.
 * adell_dino_loss_bwd: da = g_r (softmax_s sum_k p_t - p_t) / t1, db = -g_r p_t
 * (log_softmax_s - sum_k p_t log_softmax_s) / t2 (centre mode only); either may be NULL. g_r =
 * g_rows[r], or with g_rows NULL g_all[0] * g_scale (the gradient of the mean: g_scale = 1 / R). R <= 65535.
 * adell_dino_scores: out = x / t - stats[r][slot] (mode 0) or exp((x - centers) / t - stats[r][slot])
 * (mode 1): the log-softmax / softmax of a row whose lse a forward left in stats. */
int adell_dino_loss_plan(int R, int K, int* out);
long adell_dino_loss_workspace_floats(int R, int K);
int adell_dino_loss_fwd(const float* a, const float* b, const float* centers, int R, int K, float t1,
                        float t2, int teacher_is_scores, float* workspace, long workspace_floats,
                        float* loss_rows, float* stats, float* loss_mean, void* stream);
int adell_dino_loss_bwd(const float* a, const float* b, const float* centers, const float* stats,
                        const float* g_rows, const float* g_all, float g_scale, int R, int K, float t1,
                        float t2, int teacher_is_scores, float* da, float* db, void* stream);
int adell_dino_scores(const float* x, const float* centers, const float* stats, int slot, int mode,
                      int R, int K, float t, float* out, void* stream);
/* Centres: out[k] = sum_r x[r][k] (rows in order); centers = centers m + (batch_sum / denom) rest with
 * rest = 1 - m formed by the caller in double. */
int adell_dino_center_sum(const float* x, int R, int K, float* out, void* stream);
int adell_dino_center_apply(float* centers, const float* batch_sum, int K, float m, float rest,
                            float denom, void* stream);
/* Sinkhorn-Knopp teacher scores in factored form Q[k][r] = u_k exp(x[r][k] / t2) v_r:
 * proto_sums: t[k] = sum_r exp(x[r][k] / t2) v[r] (the caller all-reduces t over the ranks);
 * sample_weights: v[r] = 1 / (samples sum_k exp(x[r][k] / t2) / (K t[k]));
 * final: out[r][k] = exp(x[r][k] / t2) / (K t[k]) v[r] samples. samples = R x world size. */
int adell_dino_sk_proto_sums(const float* x, const float* v, int R, int K, float t2, float* t,
                             void* stream);
int adell_dino_sk_sample_weights(const float* x, const float* t, int R, int K, float t2, float samples,
                                 float* v, void* stream);
int adell_dino_sk_final(const float* x, const float* t, const float* v, int R, int K, float t2,
                        float samples, float* out, void* stream);
/* Head. l2_normalize_rows: y = x / max(||x||, eps) per row of C floats, inv[row] = 1 / max(||x||, eps)
 * kept for the backward (which takes y). row_inv_norm: s[row] = g[row] / ||v[row]|| for v [rows][C]
 * (weight norm over dim 0); its backward is the gradient to v alone. row_mean: the mean of each row.
 * col_scale: y[r][k] = x[r][k] s[k]; col_scale_dscale: ds[k] = sum_r dy[r][k] y0[r][k]. */
int adell_l2_normalize_rows_fwd(const float* x, int rows, int C, float eps, float* y, float* inv,
                                void* stream);
int adell_l2_normalize_rows_bwd(const float* y, const float* dy, const float* inv, int rows, int C,
                                float eps, float* dx, void* stream);
int adell_row_inv_norm_fwd(const float* v, const float* g, int rows, int C, float* s, void* stream);
int adell_row_inv_norm_bwd(const float* v, const float* g, const float* ds, int rows, int C, float* dv,
                           void* stream);
int adell_row_mean_fwd(const float* x, int rows, int C, float* out, void* stream);
int adell_row_mean_bwd(const float* dout, int rows, int C, float* dx, void* stream);
int adell_col_scale(const float* x, const float* s, int R, int K, float* y, void* stream);
int adell_col_scale_dscale(const float* dy, const float* y0, int R, int K, float* ds, void* stream);

/* iBOT (self_supervised/ibot.py, iBOTPL; csrc/ibot.hip): the masked-token objective on the prototype
 * logits of every token. fp32, dense, no float atomics, results repeat bit for bit. Index tables are
 * int32 on the device and are NOT range-checked here: the caller checks them on the host.
 * adell_ibot_mask_tokens_fwd: y [B][N][E] = x with the rows idx[0..M) (sorted, unique, < N) of every
 * item replaced by token [E]. _bwd: dx = dy with those rows zeroed, dtoken[e] = sum_b sum_j
 * dy[b][idx[j]][e] in a fixed order; either may be NULL.
 * adell_ibot_token_sums: out[b][k] = scale sum_{t >= first} x[b][t][k] for x [B][Tt][K], accumulated
 * in fp64; raw [B][K] (may be NULL) the same sums unscaled and kept in fp64; one read of x.
 * adell_ibot_token_sums_plan(B, T = Tt - first, K): out = {splits of the token axis, tokens per
 * split} (host only); with more than one split the launch needs
 * adell_ibot_token_sums_workspace_doubles(B, T, K) doubles. adell_ibot_center_sum: out[k] = the sum
 * over the R rows of such fp64 sums [R][K] (the items of every view), rounded to fp32 once.
 * adell_ibot_loss_fwd: adell_dino_loss_fwd over the R = B M rows r = b M + j: the student row is
 * s[b][rows[j]][:] of s [B][Tt][K], the teacher row y[b][rows[j]][:] of y [B][Tt][K] or, with
 * teacher_is_scores, row r of the dense scores y [R][K]. Plan and workspace: adell_dino_loss_plan(R, K),
 * adell_dino_loss_workspace_floats(R, K); stats [R][4] as there. R <= 65535.
 * adell_ibot_bwd: one launch writes every element of ds [B][Tt][K] once:
 *   ds[b][t][:] = (reduce_cls and t == 0 ? d_red[b][:] : 0)
 *               + (not reduce_cls and t >= class_token ? d_red[b][:] / (Tt - class_token) : 0)
 *               + (inv[t] = j >= 0 ? g_loss[0] / (B M) (softmax(s / t1) sum p_t - p_t) / t1 : 0)
 * with the probabilities recomputed from stats; inv [Tt] maps a token to its j or -1. d_red [B][K]
 * and g_loss (1 float) may each be NULL (no such term; without g_loss s, y, stats, inv are unused). */
int adell_ibot_mask_tokens_fwd(const float* x, const int* idx, const float* token, int B, int N, int E,
                               int M, float* y, void* stream);
int adell_ibot_mask_tokens_bwd(const float* dy, const int* idx, int B, int N, int E, int M, float* dx,
                               float* dtoken, void* stream);
int adell_ibot_token_sums_plan(int B, int T, int K, int* out);
long adell_ibot_token_sums_workspace_doubles(int B, int T, int K);
int adell_ibot_token_sums(const float* x, int B, int Tt, int K, int first, float scale,
                          double* workspace, long workspace_doubles, float* out, double* raw,
                          void* stream);
int adell_ibot_center_sum(const double* sums, int R, int K, float* out, void* stream);
int adell_ibot_loss_fwd(const float* s, const float* y, const float* centers, const int* rows, int B,
                        int Tt, int K, int M, float t1, float t2, int teacher_is_scores,
                        float* workspace, long workspace_floats, float* loss_rows, float* stats,
                        float* loss_mean, void* stream);
int adell_ibot_bwd(const float* s, const float* y, const float* centers, const float* stats,
                   const int* inv, const float* d_red, const float* g_loss, int B, int Tt, int K, int M,
                   int class_token, int reduce_cls, float t1, float t2, int teacher_is_scores,
                   float* ds, void* stream);

/* I-JEPA (self_supervised/jepa.py, IJEPAPL; csrc/ijepa.hip): token plumbing and loss. fp32, dense, one
 * wave per row, no float atomics, results repeat bit for bit. Index tables are int32 on the device,
 * sorted and unique, and are NOT range-checked here: the caller checks them on the host.
 * adell_ijepa_gather_fwd: y [B][M][E], y[b][j] = x[b][rows[j]] of x [B][N][E]. _bwd: every row of
 * dx [B][N][E] written once: dx[b][n] = dy[b][inv[n]], zeros where inv[n] < 0 (inv [N]: token -> j).
 * adell_ijepa_predictor_fwd: out [B][nc + nt][P]; out[b][j] = e[b][j] + pos[ctx[j]] for j < nc (e
 * [B][nc][P], pos [T][P]), out[b][nc + j] = mask[:] + pos[tgt[j]] (mask [P]); ctx and tgt disjoint.
 * _bwd: de [B][nc][P] = dout[:, :nc]; dpos [T][P] whole: row t = sum_b dout[b][inv_ctx[t]] or sum_b
 * dout[b][nc + inv_tgt[t]] (b in order) or zeros; dmask [P] = sum_j dpos[tgt[j]] (j in order, fp64),
 * a second launch. de, dpos, dmask may each be NULL (dmask needs dpos).
 * adell_ijepa_loss_fwd: loss[0] = mean over B nt E of smooth_l1(pred - t), beta 1, with t[b][j] the
 * layer norm (no affine, eps 1e-5, biased variance) of h[b][rows[j]][:]; pred [B][nt][E], h
 * [B][N][E]. stats [B nt][2] takes (mean, rstd) per row, part [B nt] the row sums, which a one-wave
 * second launch adds in a fixed order in fp64. _bwd: dpred = g[0] clamp(pred - t, -1, 1) / (B nt E)
 * from the saved stats; h takes no gradient. */
int adell_ijepa_gather_fwd(const float* x, const int* rows, int B, int N, int E, int M, float* y,
                           void* stream);
int adell_ijepa_gather_bwd(const float* dy, const int* inv, int B, int N, int E, int M, float* dx,
                           void* stream);
int adell_ijepa_predictor_fwd(const float* e, const float* pos, const float* mask, const int* ctx,
                              const int* tgt, int B, int nc, int nt, int T, int P, float* out,
                              void* stream);
int adell_ijepa_predictor_bwd(const float* dout, const int* tgt, const int* inv_ctx, const int* inv_tgt,
                              int B, int nc, int nt, int T, int P, float* de, float* dpos, float* dmask,
                              void* stream);
int adell_ijepa_loss_fwd(const float* pred, const float* h, const int* rows, int B, int nt, int N, int E,
                         float* stats, float* part, float* loss, void* stream);
int adell_ijepa_loss_bwd(const float* pred, const float* h, const int* rows, const float* stats,
                         const float* g, int B, int nt, int N, int E, float* dpred, void* stream);

/* ViT masked autoencoder (self_supervised/autoencoders.py: random_masking, ViTMaskedAutoEncoder.forward;
 * ViTMaskedAutoEncoderPL, pl.py:1434-1611; csrc/mae.hip). fp32, dense, one wave per row, no float
 * atomics, results repeat bit for bit. Index tables are int32 on the device, one row PER ITEM, not
 * sorted, and are NOT range-checked here: the caller checks them on the host.
 * adell_mae_gather_rows: out [B][No][E], out[b][o] = in[b][tab[b][o]] of in [B][Ni][E], zeros where
 * tab[b][o] < 0 (tab [B][No]). torch.gather(x, 1, ids_keep) with tab = ids_keep [B][K]; its gradient,
 * written whole, with the inverse table [B][L] (token -> kept position or -1).
 * adell_mae_restore_fwd: out [B][L][E]; out[b][l] = (r = restore[b][l]) < K ? enc[b][r] :
 * scale[0] mask_token[:], plus pos[l] (enc [B][K][E], mask_token [E], pos [L][E]; scale on the device).
 * The cat of mask tokens, the gather by ids_restore and the second positional embedding in one launch.
 * _bwd, at most three launches: denc [B][K][E] = dout[b][keep[b][j]] and dpos [L][E] = sum_b dout[b][l]
 * (b in order) in one; S[e] = the sum of dout over the masked rows (restore >= K) in fp64, per chunk of
 * rows into part [chunks][E] (doubles; chunks = adell_mae_restore_bwd_chunks(B, L), passed back as
 * part_rows and checked), then the chunks in order; dmask [E] = scale S, dscale [1] = sum_e
 * mask_token[e] S[e]. denc, dpos, dmask, dscale may each be NULL (part only with dmask or dscale).
 * adell_mae_loss_fwd: loss[0] = mean over B C L P of (pred[b][l][p C + c] - x[b][c][l P + p])^2:
 * MSELoss()(pred.view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).view(B, C, H, W), x) with P = ph pw and
 * L P = H W, the permuted tensor never written. part [B L] takes the row sums, which a one-wave second
 * launch adds in a fixed order in fp64. _bwd: dpred = g[0] 2 (pred - x_at) / (B C L P).
 * adell_mae_to_image: image[b][c][l P + p] = tokens[b][l][p C + c]; _from_image: the inverse copy. */
int adell_mae_gather_rows(const float* in, const int* tab, int B, int No, int Ni, int E, float* out,
                          void* stream);
int adell_mae_restore_fwd(const float* enc, const float* mask_token, const float* scale,
                          const float* pos, const int* restore, int B, int L, int K, int E, float* out,
                          void* stream);
int adell_mae_restore_bwd_chunks(int B, int L);
int adell_mae_restore_bwd(const float* dout, const float* mask_token, const float* scale,
                          const int* keep, const int* restore, int B, int L, int K, int E, float* denc,
                          float* dpos, float* dmask, float* dscale, double* part, int part_rows,
                          void* stream);
int adell_mae_loss_fwd(const float* pred, const float* x, int B, int C, int L, int P, float* part,
                       float* loss, void* stream);
int adell_mae_loss_bwd(const float* pred, const float* x, const float* g, int B, int C, int L, int P,
                       float* dpred, void* stream);
int adell_mae_to_image(const float* tokens, int B, int C, int L, int P, float* image, void* stream);
int adell_mae_from_image(const float* image, int B, int C, int L, int P, float* tokens, void* stream);

/* Classification (modules/classification/losses.py, pl.py; utils/batch_preprocessing.py;
 * csrc/classify.hip). fp32, dense, one wave per row, floating-point sums in a fixed order in fp64, no
 * float atomics: results repeat bit for bit. The counts are int64 and use integer atomics.
 * adell_cls_loss_fwd, one launch: kind 0 BCE with logits (x [B][1], float targets tf [B], soft targets
 * allowed, l = max(x, 0) - x t + log1p(exp(-|x|)); w: NULL, or 1 or B item weights), kind 1 cross
 * entropy (x [B][K], int64 labels ti [B], w: NULL or [K] class weights), kind 2 the ordinal sigmoidal
 * (CORAL) loss (x [B][K - 1], t_j = [y >= j], l = -sum_j (logsig(x_j) t_j + (logsig(x_j) - x_j)
 * (1 - t_j)), w: NULL or [K]). item [B] = weight * l; red [1] = sum(item) / aux[0] with aux[0] (a double,
 * kept for the backward) = sum of w[y] for kind 1 and B otherwise. A label outside [0, K) is never used
 * as an index: that row's item and gradient are NaN. _bwd, one launch: dx = c_b dl_b/dx with
 * c_b = g[0] weight_b / aux[0] (per_item = 0) or g[b] weight_b (per_item = 1; aux may be NULL).
 * adell_cls_roc_fwd (relative_order_consistency): over the M ordered pairs i != j with y_i != y_j the
 * mean of BCE-with-logits(p_i - p_j, [y_i > y_j]); rows [B] doubles take the row sums, aux[0] = M;
 * M = 0 gives NaN. _bwd: dp [B] in one launch, row i collecting its (i, .) and (., i) terms.
 * adell_cls_mixup: out[b][:] = factor[b] x[b][:] + (1 - factor[b]) x[partner[b]][:] over [B][V], the two
 * products and the sum rounded one by one; a row with partner[b] == b is copied. partner in [0, B) is
 * the caller's to check. Any alignment, any V.
 * adell_cls_confusion_update: counts [C][C] (row: label, column: prediction) += the samples, and
 * counts[C C] += those whose label or integer prediction lies outside [0, C). mode 0: pf [N][C], argmax
 * (first maximal index, a NaN wins); mode 1: pf [N], class [p > 0.5], C = 2; mode 2: pi [N] classes.
 * adell_cls_auroc_pairs: out[0] += 2 #{s_pos > s_neg} + #{s_pos == s_neg} over the pairs of a positive
 * (y = 1) and a negative (y = 0), out[1] += positives, out[2] += negatives; exact, O(P Nneg). */
int adell_cls_loss_fwd(int kind, const float* x, const float* tf, const long long* ti, const float* w,
                       int nw, int B, int K, float* item, float* red, double* aux, void* stream);
int adell_cls_loss_bwd(int kind, const float* x, const float* tf, const long long* ti, const float* w,
                       int nw, const float* g, int per_item, const double* aux, int B, int K, float* dx,
                       void* stream);
int adell_cls_roc_fwd(const float* p, const long long* y, int B, double* rows, float* loss, double* aux,
                      void* stream);
int adell_cls_roc_bwd(const float* p, const long long* y, const float* g, const double* aux, int B,
                      float* dp, void* stream);
int adell_cls_mixup(const float* x, const float* factor, const int* partner, int B, long V, float* out,
                    void* stream);
int adell_cls_confusion_update(int mode, const float* pf, const long long* pi, const long long* y, long N,
                               int C, long long* counts, void* stream);
int adell_cls_auroc_pairs(const float* scores, const long long* y, int N, long long* out, void* stream);

/* Multiple-instance classification (modules/classification/classification/multiple_instance_learning.py;
 * csrc/mil.hip). fp32, dense, floating-point sums in a fixed order, no float atomics: results repeat bit
 * for bit.
 * adell_mil_volume_to_slices: "b c h w s -> (b s) c h w" with P = H W: slices[(b S + s) C + c][p] =
 * vol[b C + c][p][s], a tiled transpose through LDS, both global sides contiguous. _slices_to_volume is
 * the inverse copy (its gradient).
 * adell_mil_pool_fwd, one launch, a block per item and 64 features: score[b][s] = sum_n w[n] tanh(hv[b][s][n])
 * sigmoid(hu[b][s][n]) + bias[0], A [B][S] = softmax over s (max-subtracted); hv == NULL: A = 1 / S and
 * hu, w, bias are not read. pooled [B][F] by mode: ADELL_MIL_MEAN sum_s feat[b][s][f] A[b][s];
 * ADELL_MIL_MAX the maximum over s of the same products, arg [B][F] its slice (the lowest on a tie; a NaN
 * wins); ADELL_MIL_VOCABULARY sum_s softmax_F(feat[b][s])[f] A[b][s] with rowstat [B][S][2] = (row max,
 * log of the row's sum of exponentials). F = 0: only A (feat, pooled, arg, rowstat unused). S <= 8192.
 * adell_mil_pool_bwd: g [B][F] the gradient of pooled, gA [B][S] (or NULL) the one that arrived on A;
 * writes dfeat [B][S][F] and, with hv, dhv, dhu [B][S][N], dw [N], db [1] (the fixed-order sum of
 * dscore: zero up to rounding); part: B (N + 1) doubles of workspace. Two launches, one without hv.
 * adell_mil_slice_tokens_fwd: out [B][S + ct][E], row 0 = class_token [E] (ct = 1; NULL: ct = 0), row
 * ct + s = x[b][s] + pos[s] (pos [S], one scalar per slice; NULL: a copy); one launch. _bwd, one launch:
 * dx [B][S][E] copied whole, dpos[s] = sum_b sum_e and dclass_token[e] = sum_b in fp64, b in order; a
 * NULL output is not computed. */
enum { ADELL_MIL_MEAN = 0, ADELL_MIL_MAX = 1, ADELL_MIL_VOCABULARY = 2 };
int adell_mil_volume_to_slices(const float* vol, int B, int C, int P, int S, float* slices, void* stream);
int adell_mil_slices_to_volume(const float* slices, int B, int C, int P, int S, float* vol, void* stream);
int adell_mil_pool_fwd(int mode, const float* hv, const float* hu, const float* w, const float* bias,
                       const float* feat, int B, int S, int N, int F, float* A, float* pooled, int* arg,
                       float* rowstat, void* stream);
int adell_mil_pool_bwd(int mode, const float* hv, const float* hu, const float* w, const float* feat,
                       const float* A, const int* arg, const float* rowstat, const float* g,
                       const float* gA, int B, int S, int N, int F, float* dfeat, float* dhv, float* dhu,
                       float* dw, float* db, double* part, void* stream);
int adell_mil_slice_tokens_fwd(const float* x, const float* pos, const float* class_token, int B, int S,
                               int E, float* out, void* stream);
int adell_mil_slice_tokens_bwd(const float* dout, int B, int S, int E, int has_class_token, float* dx,
                               float* dpos, float* dclass_token, void* stream);

/* 3-D object detection (csrc/detect.hip; adell_mri/modules/object_detection). Heads and target map are
 * read in place, [B][C][H W D] or channels last [B][H W D][C] (the *_cl / channels_last flags; the three
 * heads and the class head share one): anchor a of a logical [B, k A, ...] tensor is channels [k a, k a + k). target [B][Ct][H W D]
 * holds, from channel c0 on, 7 channels per anchor: objectness, centre 3, size 3.
 * adell_det_positive_table: int32 rows (b, h, w, d, a) of the cells with target objectness > threshold in
 *   torch.where's order on the stacked [B, H, W, D, A] view, capacity B A H W D rows; count [1] stays on
 *   the device; block_scratch: adell_det_table_blocks(B A H W D) ints. cs: channels per anchor of the
 *   map, 7 for the target map, 1 when the map is the objectness head itself (box decoding, c0 = 0).
 * adell_det_loss_fwd: out[5] = loss, bce mean, mean(1 - iou), mean(cpd), mean(ar) of YOLONet3dPL's step
 *   with complete_iou_loss and binary_cross_entropy (NaN with no positive); rows [4][B A H W D] = iou,
 *   cpd, ar and the cross-entropy correction per positive; partial: adell_det_loss_partials(B A H W D)
 *   doubles. cf0..2: the correction factor. adell_det_loss_bwd: grad_out[1] on the device; dcentre,
 *   dsize, dobj written whole.
 * adell_det_nms: boxes [n][6] sorted by descending score, n <= adell_det_nms_max(); mask: n ceil(n / 64)
 *   64-bit words; keep[n] = 1 for a candidate that survives the greedy sweep. */
long adell_det_table_blocks(long cells);
int adell_det_positive_table(const float* target, int B, int A, int H, int W, int D, int Ct, int c0,
                             int cs, int channels_last, float threshold, int* block_scratch, int* table,
                             int* count, void* stream);
long adell_det_loss_partials(long cells);
int adell_det_loss_fwd(const float* centre, const float* size, const float* obj, const float* target,
                       const float* anchors, const int* table, const int* count, float cf0, float cf1,
                       float cf2, int B, int A, int H, int W, int D, int Ct, int c0, int target_cl,
                       int heads_cl, double* partial, float* rows, float* out, void* stream);
int adell_det_loss_bwd(const float* centre, const float* size, const float* obj, const float* target,
                       const float* anchors, const int* table, const int* count, float cf0, float cf1,
                       float cf2, int B, int A, int H, int W, int D, int Ct, int c0, int target_cl,
                       int heads_cl, const float* grad_out, float* dcentre, float* dsize, float* dobj,
                       void* stream);
int adell_det_nms_max(void);
int adell_det_nms(const float* boxes, int n, float iou_threshold, unsigned long long* mask, int* keep,
                  void* stream);
/* adell_det_decode: YOLONet3d.recover_boxes for a batch from the table of objectness > 0.5 (cs = 1):
 *   boxes [n][6], scores [n], classes [n][NC] (cls [B][NC][H W D]; NULL: classes [n] = the objectness),
 *   starts [B + 1] = first row of every image and n.
 * adell_det_match: per target box t of image target_image[t] the prediction of that image
 *   (preds[pred_start[img] .. pred_start[img + 1])) with the highest IoU among the overlapping ones, the
 *   lowest index on a tie (0 and IoU 0 when none overlaps, -1 when the image has no prediction).
 * adell_det_encode: BBToAdjustedAnchors for a batch in fp64: boxes [B][N][6], classes [B][N],
 *   counts [B], half [A][3] = anchor / rel_sh / 2, rel0..2 the boxes' input / output shape ratio ->
 *   out [B][1 + 7 A][H W D]. */
int adell_det_decode(const float* centre, const float* size, const float* obj, const float* cls, int NC,
                     const float* anchors, const int* table, const int* count, float cf0, float cf1,
                     float cf2, int B, int A, int H, int W, int D, int heads_cl, float* boxes,
                     float* scores, float* classes, int* starts, void* stream);
int adell_det_match(const float* targets, const int* target_image, int T, const float* preds,
                    const int* pred_start, int* best, float* best_iou, void* stream);
int adell_det_encode(const double* boxes, const double* classes, const int* counts, const double* half,
                     double rel0, double rel1, double rel2, double thresh, int B, int N, int A, int H,
                     int W, int D, double* out, void* stream);
/* torch.optim.AdamW(amsgrad=True): adell_adamw_step with max_exp_avg_sq kept and used in the denominator. */
int adell_adamw_amsgrad_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                             float* max_exp_avg_sq, long n, float lr, double beta1, double beta2, float eps,
                             float weight_decay, long step, float grad_scale, void* stream);

/* DDPM diffusion (modules/diffusion/unet.py, diffusion_process.py, modules/layers/class_attention.py;
 * csrc/diffusion.hip). fp32, dense, floating-point sums in a fixed order with fp64 accumulation, no
 * float atomics: results repeat bit for bit.
 * adell_eca_gates_fwd, ONE launch for n_sites <= 32 gate blocks (op_type="linear") that read the same
 * embedding. table (HOST memory), 11 words per site: C (1..1024), the eight parameters
 * class_to_channels.weight [C][T], .bias, op.1.weight [C][C], op.1.bias, op.2.weight, op.2.bias,
 * op.4.weight [C][C], op.4.bias, the logits z [Ng][C] (output) and the site's record of Ng (8 C + 4)
 * floats (output, the backward's input). Row g of the embedding emb [Ng][T] (output): the sinusoidal
 * embedding of t[Gt == 1 ? 0 : g] (cos half, sin half, zero pad for odd T, T <= 1024; evaluated in
 * fp64; t NULL: zeros) plus cls[g] (cls [Ng][T] or NULL). z = Linear(SiLU(LayerNorm(Linear(SiLU(Linear(emb))))))
 * before the sigmoid; eps: LayerNorm's.
 * adell_eca_gates_bwd, TWO launches: table of 19 words per site: C, the eight parameters, gz [Ng][C]
 * (NULL: zeros), the forward's record, the eight parameter gradients (outputs, summed over the Ng rows
 * in order). de [Ng][T] (NULL: not computed): the gradient of cls, summed over the sites in order.
 * adell_eca_apply_fwd: y = x sigmoid(z[Ng == 1 ? 0 : n][c]) for x, y [N][V][C] (NDHWC), z [Ng][C], Ng in
 * {1, N}, C <= 16384; one launch. adell_eca_apply_bwd: dx = dy s (NULL: skipped) in the one pass over x
 * and dy that also leaves fp64 partial sums of dy x in part (adell_eca_apply_bwd_workspace_doubles(N,
 * V, C) doubles), then dz [Ng][C] = s (1 - s) sum (over the items too when Ng == 1) by a small second
 * kernel; dz and part NULL together: dx alone.
 * adell_diffusion_noise: y = sqrt(ab[t[n]]) x + sqrt(1 - ab[t[n]]) eps for N items of M elements;
 * alpha_bar [S] and t [N] (int64) on the device; an item whose t is outside [0, S) is NaN.
 * adell_diffusion_reverse_step: e = eps_uncond + scale (eps - eps_uncond) (eps_uncond NULL: e = eps);
 * out = c_x x + c_e e [+ c_x0 x0 with ADELL_DIFFUSION_X0: x0 = (x - sb e) / sa, clamped to [-1, 1] with
 * ADELL_DIFFUSION_CLIP] [+ c_n noise, noise NULL: none]; n elements, one launch.
 * adell_mse_fwd: loss[0] = mean((pred - target)^2), one launch; ws: adell_mse_workspace_bytes() bytes,
 * 16-byte aligned. adell_mse_bwd: dpred = g[0] 2 (pred - target) / n, g on the device. */
enum { ADELL_DIFFUSION_X0 = 1, ADELL_DIFFUSION_CLIP = 2 };
int adell_eca_gates_fwd(const long long* table, int n_sites, const float* t, int Gt, const float* cls,
                        int Ng, int T, float eps, float* emb, void* stream);
int adell_eca_gates_bwd(const long long* table, int n_sites, const float* emb, float* de, int Ng, int T,
                        void* stream);
int adell_eca_apply_fwd(const float* x, const float* z, int Ng, float* y, int N, long V, int C,
                        void* stream);
long adell_eca_apply_bwd_workspace_doubles(int N, long V, int C);
int adell_eca_apply_bwd(const float* x, const float* dy, const float* z, int Ng, float* dx, float* dz,
                        double* part, int N, long V, int C, void* stream);
int adell_diffusion_noise(const float* x, const float* eps, const float* alpha_bar, int S,
                          const long long* t, float* y, int N, long M, void* stream);
int adell_diffusion_reverse_step(const float* x, const float* eps, const float* eps_uncond,
                                 const float* noise, float* out, long n, float sb, float sa, float c_x0,
                                 float c_x, float c_e, float c_n, float scale, int flags, void* stream);
long adell_mse_workspace_bytes(void);
int adell_mse_fwd(const float* pred, const float* target, long n, void* ws, float* loss, void* stream);
int adell_mse_bwd(const float* pred, const float* target, const float* g, long n, float* dpred,
                  void* stream);

/* Cosine-similarity losses between two [B][D] embedding batches, the non-VICReg choices of
 * SelfSLBasePL.init_loss (self_supervised/pl.py:202-212): kind 0 simsiam_loss, kind 1 byol_loss
 * (self_supervised/losses/functional.py:138-164), kind 2 NTXentLoss (losses/ntxent.py:11-46;
 * temperature, apply_relu). loss: 1 float on the device. scratch of
 * adell_pair_loss_scratch_floats(B, D) floats is kept for the backward, which returns
 * g[0] * dloss/dx1 (dx1) and / or dx2 (either may be NULL). 2 B <= 256. */
long adell_pair_loss_scratch_floats(int B, int D);
int adell_pair_loss_fwd(const float* x1, const float* x2, int B, int D, int kind,
                        float temperature, int apply_relu, float* scratch, float* loss,
                        void* stream);
int adell_pair_loss_bwd(const float* x1, const float* x2, int B, int D, int kind,
                        float temperature, int apply_relu, const float* scratch, const float* g,
                        float* dx1, float* dx2, void* stream);

/* Local contrastive loss of the semi-supervised U-Net (LocalContrastiveLoss.forward,
 * semi_supervised_segmentation/losses.py:498-526; called by UNetContrastiveSemiSL.step_semi_sl_loco,
 * semi_supervised_segmentation/pl.py:244-281): f1 / f2 = decoder features of the two views, NDHWC
 * [B][S][C] (B <= 8, C % 4 == 0). loss[i] = mean_s -log(max(softmax_j(cos(f2[i,s], f1[j,s]) / T)[i],
 * eps)). Backward: gloss[B] (device) = dL/dloss; df1 / df2 [B][S][C], either may be NULL.
 * Workspace of the forward: adell_loco_loss_workspace(B, S, C) bytes (per-block partial sums,
 * folded in fixed order). */
long adell_loco_loss_workspace(int B, long S, int C);
int adell_loco_loss_fwd(const float* f1, const float* f2, int B, long S, int C, float temperature,
                        float eps, float* loss, void* workspace, size_t workspace_bytes,
                        void* stream);
int adell_loco_loss_bwd(const float* f1, const float* f2, const float* gloss, int B, long S, int C,
                        float temperature, float eps, float* df1, float* df2, void* stream);

/* ConvTranspose3d with kernel = stride = 2 on all three axes and 32 / 64 channels on both sides
 * (unet.py:445-458, the upscaling of the high-resolution decoder levels) as streaming GEMMs on the
 * fp32 MFMA: every input voxel feeds exactly its 8 output voxels, so nothing needs a halo or a
 * packed weight. w / dw: torch's canonical [Cin][Cout][2][2][2]. `applicable`: factors 2x2x2,
 * 32 / 64 input and 16 / 32 / 64 output channels, at least 32 768 input voxels (below that the
 * implicit-GEMM entry points above stay in use). x / dy 16-byte aligned.
 * adell_convt_k221_*: the same for factors (2, 2, 1) -- depth and height doubled, width kept
 * (SWIN-UNet's anisotropic upscaling, unetr.py:902-925); w / dw [Cin][Cout][2][2][1], 32 / 64
 * channels on both sides. */
int adell_convt_k2_applicable(int N, int D, int H, int W, int Cin, int Cout);
int adell_convt_k2_fwd(int N, int D, int H, int W, int Cin, int Cout, const float* x,
                       const float* w, const float* bias, float* y, void* stream);
int adell_convt_k2_bwd_data(int N, int D, int H, int W, int Cin, int Cout, const float* dy,
                            const float* w, float* dx, void* stream);
long adell_convt_k2_wgrad_workspace(int N, int D, int H, int W, int Cin, int Cout);
/* db (optional, [Cout]): the bias gradient, a by-product of the same pass over dy */
int adell_convt_k2_bwd_weight(int N, int D, int H, int W, int Cin, int Cout, const float* x,
                              const float* dy, float* dw, float* db, void* workspace,
                              size_t workspace_bytes, void* stream);
int adell_convt_k221_applicable(int N, int D, int H, int W, int Cin, int Cout);
int adell_convt_k221_fwd(int N, int D, int H, int W, int Cin, int Cout, const float* x,
                         const float* w, const float* bias, float* y, void* stream);
int adell_convt_k221_bwd_data(int N, int D, int H, int W, int Cin, int Cout, const float* dy,
                              const float* w, float* dx, void* stream);
long adell_convt_k221_wgrad_workspace(int N, int D, int H, int W, int Cin, int Cout);
int adell_convt_k221_bwd_weight(int N, int D, int H, int W, int Cin, int Cout, const float* x,
                                const float* dy, float* dw, float* db, void* workspace,
                                size_t workspace_bytes, void* stream);

/* 3x3x3 stride-1 convolution with 1..4 input channels and a wide output (the 2 -> 32 conv of the
 * U-Net input block, unet.py:260-273; UNETR's first encoder, unetr.py:225-237) as one small GEMM per
 * brick over K = 27 Cin on the fp32 MFMA (exact fp32 products): forward (+ bias, + the statistics
 * partials [N][adell_conv_cinfold_ntiles][Cout][2] of the fused norm) and weight / bias gradient.
 * x [N][D][H][W][Cin], w / dw canonical [Cout][Cin][3][3][3]. `applicable` tells whether a
 * descriptor takes this path. */
int adell_conv_cinfold_applicable(const adell_conv3d_desc* d);
int adell_conv_cinfold_ntiles(const adell_conv3d_desc* d);
int adell_conv_cinfold_fwd(const adell_conv3d_desc* d, const float* x, const float* w,
                           const float* bias, float* y, float* stat_partials, int partial_rows,
                           void* stream);
/* the same arithmetic on the f16 MFMA with error-compensated operand splits (two input channels;
 * other channel counts run the exact kernel above) */
int adell_conv_cinfold_fwd_f16x3(const adell_conv3d_desc* d, const float* x, const float* w,
                                 const float* bias, float* y, float* stat_partials, int partial_rows,
                           void* stream);
long adell_conv_cinfold_wgrad_workspace(const adell_conv3d_desc* d);
int adell_conv_cinfold_bwd_weight(const adell_conv3d_desc* d, const float* x, const float* dy,
                                  float* dw, float* db, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* the same on the f16 MFMA with error-compensated operand splits (every channel count 1..4; same
 * workspace): bound by the one pass over dy instead of by the fp32 MFMA */
int adell_conv_cinfold_bwd_weight_f16x3(const adell_conv3d_desc* d, const float* x, const float* dy,
                                        float* dw, float* db, void* workspace,
                                        size_t workspace_bytes, void* stream);
/* backward-data of the same convs (dx has 1..4 channels): one GEMM per dY voxel over K = Cout
 * (Cout <= 64, multiple of 4) into the 27 Cin (tap, channel) columns, gathered into dx along a
 * z march. dy 16-byte aligned. */
int adell_conv_cinfold_dx_applicable(const adell_conv3d_desc* d);
int adell_conv_cinfold_bwd_data(const adell_conv3d_desc* d, const float* dy, const float* w,
                                float* dx, void* stream);
/* the same with the per-voxel GEMM on the f16 MFMA with error-compensated operand splits */
int adell_conv_cinfold_bwd_data_f16x3(const adell_conv3d_desc* d, const float* dy, const float* w,
                                      float* dx, void* stream);

/* 1x1x1 convolution with Cout <= 4 (the logits head, unet.py:712-731) on canonical weights
 * w [Cout][C0+C1]: one HBM-bound pass each way. `applicable` tells whether a descriptor takes
 * this path (k = 1, stride 1, no padding, Cout <= 4, Cin <= 512). */
int adell_conv1_small_applicable(const adell_conv3d_desc* d);
int adell_conv1_small_fwd(const adell_conv3d_desc* d, const float* x0, const float* x1,
                          const float* w, const float* bias, float* y, void* stream);
int adell_conv1_small_bwd_data(const adell_conv3d_desc* d, const float* dy, const float* w,
                               float* dx0, float* dx1, void* stream);
long adell_conv1_small_wgrad_workspace(const adell_conv3d_desc* d);
int adell_conv1_small_bwd_weight(const adell_conv3d_desc* d, const float* x0, const float* x1,
                                 const float* dy, float* dw, float* db, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Convolutions with Cin <= 4 (the 2-channel input block, unet.py:260-273), k = 3 in H and W,
 * 1 or 3 in D, stride 1, one source, canonical weights w [Cout][Cin][KD][3][3]: exact fp32 on
 * the vector ALU instead of an MFMA tile padded to 16 input channels. The forward writes the
 * same (sum, sum of squares) partials as adell_conv3d_fwd, [N][ntiles][Cout][2]. The
 * backward-data produces dX [N][D][H][W][Cin] from dY (Cout a multiple of 4). */
int adell_conv_cin_small_applicable(const adell_conv3d_desc* d);
int adell_conv_cin_small_ntiles(const adell_conv3d_desc* d);
int adell_conv_cin_small_fwd(const adell_conv3d_desc* d, const float* x, const float* w,
                             const float* bias, float* y, float* stat_partials, int partial_rows,
                           void* stream);
int adell_conv_cin_small_bwd_data(const adell_conv3d_desc* d, const float* dy, const float* w,
                                  float* dx, void* stream);

/* dst[off_r + i] = src_r[i] for rows r of a DEVICE table of `rows` triples (source pointer,
 * destination offset in elements, element count <= 16384 per row): gathers the parameter
 * gradients autograd produced into the flat gradient buffer of the fused optimisers. */
int adell_multi_copy(const long* table, int rows, float* dst, void* stream);

/* Gradient-norm clipping over the flat gradient buffers, torch.nn.utils.clip_grad_norm_ (norm 2 or
 * inf) as Lightning's Trainer(gradient_clip_val) calls it (entrypoints/segmentation/train.py:807,
 * ssl/train_3d.py:354; flag: assemble_args.py:386-392). No host synchronisation, no allocation:
 *   adell_grad_norm_workspace(runs): bytes of the fp64 partials of `runs` runs (one per contiguous
 *     run of parameters that have a gradient, over every parameter group);
 *   adell_grad_norm_partials: run `run` (16-byte aligned, any length) -> its slots of `partials`;
 *   adell_grad_norm_finalize: out[0] = ||scale g|| over every run, out[1] = the clip coefficient
 *     min(max_norm / (out[0] + 1e-6), 1) (fp32; NaN stays NaN). `scale` is the factor between the
 *     buffer and the gradient the optimiser applies (grad_scale / accumulate_grad_batches);
 *   adell_grad_scale_by: g *= *coef_dev (returns at once, no traffic, when it is 1).
 * Fixed grids and fixed-order fp64 sums: the same buffer gives the same bits. */
long adell_grad_norm_workspace(int runs);
int adell_grad_norm_partials(const float* g, long n, int norm_inf, double* partials, int run,
                             void* stream);
int adell_grad_norm_finalize(const double* partials, int runs, int norm_inf, float scale,
                             float max_norm, float* out, void* stream);
int adell_grad_scale_by(float* g, long n, const float* coef_dev, void* stream);
/* adell_multi_copy with dst += src: folds a micro-batch's parameter gradients into the flat buffer
 * under Trainer(accumulate_grad_batches) (train.py:811, ssl/train_3d.py:355). */
int adell_multi_accumulate(const long* table, int rows, float* dst, void* stream);

/* Segmentation metrics (csrc/seg_metrics.hip): the confusion counts behind the reference's
 * torchmetrics dicts (modules/segmentation/pl.py:100-187, setup_metrics :655-671; updated from
 * training_step / validation_step / test_step :403, :467, :513; reported by
 * entrypoints/segmentation/test.py:337-392). A metric state is int64 [3 C + 1]: (tp, fp, fn) per
 * class, then the bad-target flag.
 *   adell_seg_confusion_workspace(n, C): bytes of the int32 partial rows for n = B * S voxels;
 *   adell_seg_confusion_update: pred fp32 [B][C][S] (channels_last: [B][S][C]; C <= 32), target
 *     [B][S] of target_type 0 fp32 (rounded half-to-even), 1 uint8 / bool, 2 int64. Two launches
 *     (partial rows, one-block finalize) that ADD the counts of this update into each of the
 *     nstates <= 8 states (host array of device pointers). C = 1: mask p > 0.5, or sigmoid(p) > 0.5
 *     when any p of this update lies outside [0, 1] (NaN included). C > 1: argmax over the
 *     channels. A target outside {0, 1} / [0, C) sets the flag. No host synchronisation;
 *   adell_seg_metric_compute: out[0] (fp32) = kind of the state, fp64 arithmetic, averaged over the
 *     classes with tp + fp + fn > 0 (0 when none; a zero denominator gives 0). */
enum { ADELL_SEG_IOU = 0, ADELL_SEG_PRECISION = 1, ADELL_SEG_FBETA = 2, ADELL_SEG_DICE = 3 };
long adell_seg_confusion_workspace(long n, int C);
int adell_seg_confusion_update(const float* pred, const void* target, int target_type, long B, int C,
                               long S, int channels_last, int* workspace, long workspace_bytes,
                               long long* const* states, int nstates, void* stream);
int adell_seg_metric_compute(const long long* state, int C, int kind, float beta, float* out,
                             void* stream);

/* Connected components and PI-CAI lesion tables (csrc/components.hip).
 *   adell_cc_label: labels int32 [NV][D][H][W] and component counts [NV] of fp32 volumes x
 *     [NV][D][H][W], bit-identical to scipy.ndimage.label(x_i, np.ones((3, 3, 3))) (26-connected,
 *     components numbered in the raster order of their first voxel); foreground is x > threshold
 *     (use_threshold) or x != 0. Replaces the labelling of the reference's picai_eval
 *     (picai_eval/analysis_utils.py:38, eval.py:163; reached from modules/segmentation/pl.py:609-652).
 *     adell_cc_workspace gives the workspace bytes. No host synchronisation;
 *   adell_picai_tables: the lesion tables of picai_eval.evaluate_case (eval.py:51-251) for B cases,
 *     fed by the reference's all_pred / all_true lists (pl.py:446-452, 503-509): candidates are the
 *     components of pred > threshold (get_lesions, pl.py:75-97; or pred != 0 without use_threshold,
 *     confidence = the maximum of pred over each), GT lesions those of target.astype(int32) != 0.
 *     hdr int32 [B][3] = (N_cand, N_gt, n_pairs); out holds one record per case, back to back:
 *     [N_cand, N_gt, n_pairs, gt voxel counts, candidate voxel counts, candidate confidences (fp32
 *     bits), (gt, cand, intersection) x n_pairs], the pairs (any order) being those with
 *     10 * intersection >= union. out_capacity >= adell_picai_tables_capacity words. No host
 *     synchronisation. */
long adell_cc_workspace(long NV, int D, int H, int W);
int adell_cc_label(const float* x, long NV, int D, int H, int W, int use_threshold, float threshold,
                   int* labels, int* counts, void* workspace, long workspace_bytes, void* stream);
long adell_picai_tables_workspace(long B, int D, int H, int W);
long adell_picai_tables_capacity(long B, int D, int H, int W);
int adell_picai_tables(const float* pred, const float* target, long B, int D, int H, int W,
                       int use_threshold, float threshold, int* hdr, int* out, long out_capacity,
                       void* workspace, long workspace_bytes, void* stream);

/* Lesion-candidate extraction (csrc/components.hip): the reference's
 * adell_mri/modules/extract_lesion_candidates.py (Report-Guided-Annotation), reached from
 * get_lesions(extract_lesions=True) (modules/segmentation/pl.py:76-97) and from the test entry point
 * (entrypoints/segmentation/test.py:361-399), on fp32 volumes x [NV][D][H][W] of finite,
 * non-negative values. mode 0, static (:19-55): foreground x >= threshold and x != 0, 26-connected
 * labelling as adell_cc_label, components of <= min_voxels voxels dropped, every other one painted
 * with its maximum in hard [NV][D][H][W] and with its scipy label in indexed (int32). use_round:
 * the painted value is float32(np.round(float64(max), round_decimals)). mode 1, dynamic-fast
 * (:198-211): static with threshold = max(x_i) / factor per volume, a correctly rounded fp32
 * division on the device. mode 2, dynamic (:58-134): up to num_lesions rounds per volume of
 * [threshold = max(working) / factor, stop below 0.01; static extraction; choose the kept component
 * of the largest painted value, ties to the lowest label; reject it when remove_adjacent and a stored
 * voxel > 0 lies in the 3x3x3 neighbourhood of one of its voxels, else store it with index 1 + the
 * number stored; remove it from the working copy], including the reference's whole-volume
 * "candidate" of confidence 0 when no component survives the size filter.
 * n_out [NV], ids / conf / peak [NV][cap]: the kept components in ascending index, their painted
 * value and their unrounded maximum; cap >= adell_lesion_candidates_capacity. rounds (host, may be
 * null): the rounds the dynamic mode ran. Modes 0 and 1 never synchronise with the host; mode 2
 * synchronises rounds + 1 times, reading back one int per volume each time. */
long adell_lesion_candidates_workspace(long NV, int D, int H, int W, int mode);
long adell_lesion_candidates_capacity(int D, int H, int W, int mode, int min_voxels, int num_lesions);
int adell_lesion_candidates(const float* x, long NV, int D, int H, int W, int mode, float threshold,
                            float factor, int min_voxels, int num_lesions, int round_decimals,
                            int use_round, int remove_adjacent, float* hard, int* indexed, int* n_out,
                            int* ids, float* conf, float* peak, long cap, int* rounds,
                            void* workspace, long workspace_bytes, void* stream);

/* ---- shifted-window (SWIN) token path: vit.py:33-45,95-129,1005-1256; linear_blocks.py:358-417 */
/* out (contiguous over sizes[0..nd)) = gather of `in`: out dim d adds coord*mult[d] to input
 * axis axis[d]; input axis a has extent / stride (elements) / cyclic shift:
 * in_coord[a] = (sum + shift[a]) mod extent[a]. One kernel for every einops rearrange and
 * torch.roll of the path (window partition + cyclic shift, its inverse, einops_rescale). */
int adell_gather_nd(const float* in, float* out, int nd, const int* sizes, const int* axis,
                    const long* mult, int na, const long* extent, const long* stride,
                    const long* shift, void* stream);
/* LayerNorm over rows of C <= 512 values; input row r starts at (r/inner)*so + (r%inner)*si
 * (contiguous rows: inner = 1, so = C); y, dy, mean, rstd are contiguous; dx is strided by
 * (dso, dsi) the same way, so q / k slices of a QKV buffer are normalised in place. */
int adell_layernorm_rows_fwd(const float* x, long rows, int C, int inner, long so, long si,
                             const float* gamma, const float* beta, float eps, float* y,
                             float* mean, float* rstd, void* stream);
long adell_layernorm_rows_bwd_workspace(long rows, int C);
int adell_layernorm_rows_bwd(const float* x, const float* dy, const float* gamma,
                             const float* mean, const float* rstd, long rows, int C, int inner,
                             long so, long si, float* dx, long dso, long dsi, float* dgamma,
                             float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* Attention inside windows of T <= 64 tokens (token row = w*T + i). q, k, out: [tokens][H][A|Dv]
 * contiguous; v (and dv) element (t,h,d) at v[t*v_ts + h*v_hs + d] (inside a QKV buffer).
 * S = scale*q k^T + rel[H][T][T] + mask[w % n_mask][T][T]; O = dropout(softmax(S)) v (Philox
 * mask from (seed, rng_offset), regenerated in the backward); lse [W][H][T] is kept for the
 * backward; ds (optional [W][H][T][T]) receives dS, the gradient of the additive bias. */
int adell_winattn_fwd(const float* q, const float* k, const float* v, long v_ts, long v_hs,
                      const float* rel, const float* mask, int n_mask, long W, int H, int T, int A,
                      int Dv, float scale, float drop_p, unsigned long seed, unsigned rng_offset,
                      float* out, float* lse, void* stream);
int adell_winattn_bwd(const float* q, const float* k, const float* v, long v_ts, long v_hs,
                      const float* rel, const float* mask, int n_mask, const float* o,
                      const float* dout, const float* lse, long W, int H, int T, int A, int Dv,
                      float scale, float drop_p, unsigned long seed, unsigned rng_offset,
                      float* dq, float* dk, float* dv, float* ds, void* stream);

/* Row-major fp32 GEMM (fp32 MFMA) behind torch.nn.Linear (layers/linear_blocks.py,
 * res_blocks.py:559-566, res_net.py:278-324): C[M][N] = A x B (+ bias[N]) (+ residual).
 * a_kc != 0: A(m,k) = A[m*lda + k], else A[k*lda + m]; b_kc != 0: B(k,n) = B[n*ldb + k], else
 * B[k*ldb + n]. Forward X W^T: (1,1); backward-data dY W: (1,0); backward-weight dY^T X: (0,0).
 * workspace: adell_gemm_f32_workspace_floats(M, N, K) floats of split-k slabs (NULL if 0). */
long adell_gemm_f32_workspace_floats(int M, int N, int K);
int adell_gemm_f32(int M, int N, int K, const float* A, long lda, int a_kc, const float* B,
                   long ldb, int b_kc, float* C, long ldc, const float* bias,
                   const float* residual, long ldr, float* workspace, void* stream);

/* The same GEMM on the f16 MFMA by error-compensated splitting (3 MFMAs per product, fp32-class
 * accuracy: csrc/gemm_f16x3.hip) -- torch.nn.Linear forward / dX / dW of the ConvNeXt point-wise
 * MLPs (res_blocks.py:559-566), the ViT / SWIN projections (linear_blocks.py) and the projection
 * heads (res_net.py:278-324). a_absmax / b_absmax: both NULL (operand scales chosen inside the
 * kernel per block and 64-k stage), or device words with the float bits of the absmax of the A / B
 * tensors (adell_absmax_f32 into a zero-initialised word): one scale per tensor. Operands that do
 * not qualify (route ADELL_GEMM_H_REFUSED of adell_gemm_plan below) make the call return
 * ADELL_E_UNSUPPORTED; the caller asks the plan first and uses adell_gemm_f32.
 * workspace: adell_gemm_f16x3_workspace_floats(M, N, K) floats (NULL when that is 0). */
int adell_absmax_f32(const float* x, long n, uint32_t* out, void* stream);
long adell_gemm_f16x3_workspace_floats(int M, int N, int K);
int adell_gemm_f16x3(int M, int N, int K, const float* A, long lda, int a_kc, const float* B,
                     long ldb, int b_kc, float* C, long ldc, const float* bias,
                     const float* residual, long ldr, const uint32_t* a_absmax,
                     const uint32_t* b_absmax, float* workspace, void* stream);
/* The same GEMM with an activation (ADELL_ACT_*) in its epilogue: a Linear -> activation pair
 * without an element-wise pass over the 4 C-wide intermediate (res_blocks.py:559-566: pwconv1 ->
 * GELU -> pwconv2; linear_blocks.py MLP). act_out != NULL: C = A B^T + bias (+ residual) and
 * act_out = act(C), both [M][ldc] (the backward needs the pre-activation, the next layer the
 * activation: one GEMM writes both). dact_in != NULL: C = (A B^T + ...) * act'(dact_in), with
 * dact_in [M][ldc] the saved pre-activation -- the gradient through the activation, applied by the
 * GEMM that produces the gradient of the activation's output. A must be K-contiguous (a_kc = 1). */
int adell_gemm_f16x3_act(int M, int N, int K, const float* A, long lda, int a_kc, const float* B,
                         long ldb, int b_kc, float* C, long ldc, const float* bias,
                         const float* residual, long ldr, const uint32_t* a_absmax,
                         const uint32_t* b_absmax, float* workspace, int act, float act_p,
                         float* act_out, const float* dact_in, void* stream);
/* Launch plan of a GEMM, host only (no launch, no tensor read, no device needed): what adell_gemm_f32
 * (family ADELL_GEMM_F32) or adell_gemm_f16x3 / adell_gemm_f16x3_act (ADELL_GEMM_F16X3) would run
 * under the current tuning switches, decided by the same function the launchers and the two
 * *_workspace_floats queries call (those take the largest workspace over the layouts, alignments and
 * epilogues a shape can arrive in).
 * aligned: ADELL_GEMM_ALIGNED_* bits; set the bit of a tensor the call does not have. A, B, BIAS,
 *   WORKSPACE: the pointer is 16-byte aligned; C, RESIDUAL: that and a leading dimension that is a
 *   multiple of 4. The fp32 family looks at A and B only.
 * epilogue (f16x3 family): ADELL_GEMM_EPI_NONE (adell_gemm_f16x3), _ACT_GELU / _ACT (act_out of
 *   adell_gemm_f16x3_act with GELU / any other activation), _DACT (dact_in).
 * fp32 routes, in the order they are tried:
 *   ROWS_SMALL   a_kc, K <= 64, N <= 64, N K <= 512, M >= 65536: a thread per output (four when N
 *                allows), weights in LDS: adell_gemm_rows_small_kernel<b_kc>. No workspace.
 *   TALL_LDS     both operands outer-contiguous, K >= 16384 and K % 4 == 0, M and N powers of two up to
 *                64 with 8 <= M N <= 512, lda == M, ldb == N, A and B 16-byte aligned: chunks of both
 *                operands staged in LDS, one partial per block: adell_gemm_tall_lds_kernel +
 *                adell_gemm_reduce_kernel.
 *   TALL_SMALL   both operands outer-contiguous, K >= 16384, M <= 32, N <= 32 (whatever TALL_LDS left):
 *                adell_gemm_tall_small_kernel + adell_gemm_reduce_kernel.
 *   TILE_SKINNY  M <= 32: 32 x 128 MFMA tiles; TILE_SQUARE: 128 x 128 tiles
 *                (adell_gemm_f32_kernel<.., a_kc, b_kc>). Split along k while there are fewer than 512
 *                tiles (at least 4 k-steps of 16 per split, at most 256 k-steps, slabs up to 64 MB);
 *                2 .. 8 splits are summed by adell_gemm_reduce_flat_kernel (REDUCE_FLAT), more by
 *                adell_gemm_reduce_kernel (REDUCE_TREE).
 *   out[8]: [0] route; [1] splits (tall routes: partials = blocks); [2] k-steps per split; [3]
 *   ADELL_GEMM_REDUCE_*; [4] chunk rows, [5] outputs per thread (TALL_LDS); [6] blocks of the first
 *   kernel; [7] workspace floats of this route.
 * f16x3 routes, in the order they are tried:
 *   REFUSED      A or B not 16-byte aligned, lda, ldb or K not a multiple of 4, an outer-contiguous
 *                operand whose outer extent (M, N) is not; or an activation epilogue without the wide
 *                epilogue's conditions. The fields are those of TILE: what the shape would launch.
 *   ROWS         a_kc, K % 32 == 0, K <= 8192, N >= 32, M >= 2048, K N <= 4 Mi, a 16-byte aligned
 *                workspace, epilogue NONE or ACT_GELU (never DACT: measured slower than the tiles), not
 *                under the tuning switch "gemm_norows", and at least one (256-row tile, 128-column
 *                slice) pair per CU: adell_gemm_rows_pack_kernel + adell_gemm_rows_f16x3_kernel.
 *   TILE         everything else: 128 x 128 tiles, adell_gemm_f16x3_kernel<a_kc, b_kc, wide>. wide: N % 4
 *                == 0 and C, bias, residual, workspace aligned (required by an activation epilogue).
 *                Split along K while there are fewer than 512 tiles (at least 4 stages of 64 per
 *                split, slabs up to 64 MB) and folded by adell_gemm_f16x3_fold_kernel<V, S>: V = 4 when
 *                N % 4 == 0 and the workspace is aligned, else 1; S = 1, 4 (>= 8 splits), 16 (>= 32).
 *   out[14]: [0] route; [1] epilogue; ROWS: [2] column slices, [3] pack rows per block, [4] blocks,
 *   [5] tiles per block; TILE: [4] blocks, [6] wide, [7] splits, [8] stages per split, [9] fold V,
 *   [10] fold S (0 without a fold); [11] workspace floats of this route; [12] the streaming regime
 *   (min(M, N) >= 32 and max(M, K) >= 65536: this family pays off below the callers' size rule too);
 *   [13] the CU count ROWS compares its tile count against. */
#define ADELL_GEMM_F32 0
#define ADELL_GEMM_F16X3 1
#define ADELL_GEMM_ROWS_SMALL 0
#define ADELL_GEMM_TALL_LDS 1
#define ADELL_GEMM_TALL_SMALL 2
#define ADELL_GEMM_TILE_SKINNY 3
#define ADELL_GEMM_TILE_SQUARE 4
#define ADELL_GEMM_REDUCE_NONE 0
#define ADELL_GEMM_REDUCE_FLAT 1
#define ADELL_GEMM_REDUCE_TREE 2
#define ADELL_GEMM_H_REFUSED 0
#define ADELL_GEMM_H_ROWS 1
#define ADELL_GEMM_H_TILE 2
#define ADELL_GEMM_EPI_NONE 0
#define ADELL_GEMM_EPI_ACT_GELU 1
#define ADELL_GEMM_EPI_ACT 2
#define ADELL_GEMM_EPI_DACT 3
#define ADELL_GEMM_ALIGNED_A 1
#define ADELL_GEMM_ALIGNED_B 2
#define ADELL_GEMM_ALIGNED_C 4
#define ADELL_GEMM_ALIGNED_BIAS 8
#define ADELL_GEMM_ALIGNED_RESIDUAL 16
#define ADELL_GEMM_ALIGNED_WORKSPACE 32
#define ADELL_GEMM_ALIGNED_ALL 63
int adell_gemm_plan(int family, int M, int N, int K, int a_kc, int b_kc, long lda, long ldb,
                    int aligned, int epilogue, long* out);

/* Element-wise segmentation losses beyond the fused binary dice + focal pair, on probabilities
 * p[B][V][C] (NDHWC; C = 1 for the binary family) against targets of the same layout:
 * kind 0 binary_cross_entropy (losses.py:79-109), 1 cat_cross_entropy (:528-562), 2 mc_focal_loss
 * (:565-607), 3 mc_generalized_dice_loss (:610-653). cw[C] = class weights / alpha (not used by
 * kind 0, which takes w_pos). loss[B]; sums[B][C][2] is kept for the backward, which writes
 * dp = gout[b] * d loss[b] / d p. workspace: adell_seg_loss_workspace(B, V, C) bytes. */
long adell_seg_loss_workspace(int B, long V, int C);
int adell_seg_loss_fwd(int kind, const float* p, const float* t, const float* cw, int B, long V,
                       int C, float eps, float scale, float label_smoothing, float gamma,
                       float smooth, float w_pos, float* loss, float* sums, void* workspace,
                       size_t workspace_bytes, void* stream);
int adell_seg_loss_bwd(int kind, const float* p, const float* t, const float* cw, int B, long V,
                       int C, float eps, float scale, float label_smoothing, float gamma,
                       float smooth, float w_pos, const float* sums, const float* gout, float* dp,
                       void* stream);

/* Softmax over the channel axis of an NDHWC tensor (rows = N * voxels, C <= 32 contiguous
 * class values per row): the n_classes > 2 head, torch.nn.Softmax(dim=1) at unet.py:641-655.
 * backward: dx = y * (dy - sum_c dy * y). */
int adell_channel_softmax_fwd(const float* x, float* y, long rows, int C, void* stream);
int adell_channel_softmax_bwd(const float* y, const float* dy, float* dx, long rows, int C,
                              void* stream);

/* out[n][c] = max over the V voxels of NDHWC x[n][v][c], arg = the first voxel attaining it
 * (torch.max semantics): X.flatten(2).max(-1).values in front of the bottleneck classifier
 * (unet.py:826-828). backward: dx = 0 except dx[n][arg[n][c]][c] = dout[n][c]. */
int adell_channel_max_fwd(const float* x, float* out, int* arg, int N, long V, int C,
                          void* stream);
int adell_channel_max_bwd(const float* dout, const int* arg, float* dx, int N, long V, int C,
                          void* stream);

/* test hook: force one conv tile configuration (0..3), -1 = heuristic */
void adell_debug_force_conv_cfg(int cfg);

/* Launch-plan switches (ten): each selects another BUILT path that the parity tests compare with
 * the default -- "igemm_nospec" (3^3 convs on the generic f16x3 instance), "igemm_no8" (no 8x8x8
 * bricks), "no_splitk", "wgrad_nozring", "wgrad_no16", "igemm_no16" (16-channel layers off their
 * 16-column kernels), "attn_nomfma", "dw_nomfma", "dw_wgrad_nomfma" (depthwise 7^3 on the
 * vector-ALU kernels), "gemm_norows" (Linear layers never on the streaming GEMM). Initialised once
 * at load from the environment variables of the same names (ADELL_ prefix, upper case); the launch
 * path itself never reads the environment. The kernel timing experiments ("igemm_dbg", "zr_dbg":
 * results become WRONG) exist only in -DADELL_DEBUG builds of the library. adell_set_tuning
 * returns ADELL_E_BADARG for an unknown name; adell_get_tuning -1. */
int adell_set_tuning(const char* name, int value);
/* Replay counter of the dropout offsets: a device word (0 after load) that every dropout kernel of
 * the library ADDS to its `rng_offset` argument. Eager callers never touch it. A caller that
 * captures a training step in a HIP graph enqueues adell_rng_advance(K, 0, stream) as the LAST
 * node, K = the number of offsets the step draws: replay r then uses offsets c + r K .. where the
 * capture drew c .., i.e. the masks eager step r would have drawn. set != 0: the word is set to
 * `delta` instead (0 when the caller goes back to eager launches). Stream-ordered. */
int adell_rng_advance(uint32_t delta, int set, void* stream);
int adell_get_tuning(const char* name);

/* ------------------------------------------------------------------------
 * Device-side batch augmentation (csrc/augment.hip): the arithmetic of the MONAI transforms the
 * reference composes in transform_factory/augmentations.py:19-178 (get_augmentations_unet) on
 * volumes resident in HBM. The random draws are the caller's; these are the per-element passes.
 * ---------------------------------------------------------------------- */
/* out[N][4] = (min, max, mean, population std) of each item of per_item contiguous floats
 * (what RandAdjustContrast / RandStdShiftIntensity need of an image) */
long adell_item_stats_workspace(int N, long per_item);
int adell_item_stats(const float* x, int N, long per_item, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* One pass: gamma contrast -> std shift -> Rician noise. params[N][8] per item:
 * {min, max - min, gamma (<= 0: skip), shift, noise std (<= 0: skip), unused x 3}:
 *   v = ((x - min) / (range + 1e-7))^gamma * range + min;  v += shift;
 *   v = sqrt((v + n1)^2 + n2^2), n1, n2 ~ N(0, std) from Philox(seed, rng_offset, element). */
int adell_aug_intensity(const float* x, float* out, int N, long per_item, const float* params,
                        uint64_t seed, uint32_t rng_offset, void* stream);
/* Affine resampling of NDHWC volumes: out[n][v] = sample(x[n], theta[n] (v - centre) + centre) in
 * voxel coordinates (theta[N][12]: rows of a 3 x 4 matrix over (z, y, x)); linear: 1 trilinear,
 * 0 nearest; pad_mode: 0 zeros, 1 border, 2 reflection (about -0.5 / size - 0.5). */
int adell_affine_sample(const float* x, float* out, int N, int D, int H, int W, int C,
                        const float* theta, int linear, int pad_mode, void* stream);
/* Round 4, the rest of get_augmentations_unet (augmentations.py:52-127). All on NDHWC volumes.
 * adell_axis_filter: 1-D filter along spatial axis 0 / 1 / 2 with zero padding, taps[N][2 R + 1]
 *   per item (three calls = the separable Gaussian of RandGaussianSmoothd, "blur").
 * adell_bias_field: out = x * exp(sum c[i][j][k] P_i(z) P_j(y) P_k(x)), Legendre polynomials over
 *   linspace(-1, 1, size), coef[N][64] = dense 4 x 4 x 4 cube (RandBiasFieldd degree 3, "rbf").
 * adell_axis_lut_sample: resampling through per-axis coordinate tables lut[N][D + H + W] (input
 *   voxel coordinate per output index), trilinear / nearest, border padding (RandGridDistortiond,
 *   "distort").
 * adell_gibbs_lowpass: per item the spectrum (three-axis DFT, any axis length <= 1024) is zeroed
 *   outside the sphere of radius[n] about the centre of the SHIFTED spectrum and transformed back
 *   (RandGibbsNoised, the k-space half of "noise"); workspace adell_gibbs_workspace bytes. */
int adell_axis_filter(const float* x, float* out, int N, int D, int H, int W, int C, int axis,
                      const float* taps, int radius, void* stream);
int adell_bias_field(const float* x, float* out, int N, int D, int H, int W, int C,
                     const float* coef, void* stream);
int adell_axis_lut_sample(const float* x, float* out, int N, int D, int H, int W, int C,
                          const float* lut, int linear, void* stream);
/* ------------------------------------------------------------------------
 * Dispatch queries of the depthwise 7^3 kernels (csrc/dw_mfma.hip, dw_dense.hip, dw_wgrad_mfma.hip):
 * 1 when adell_dwconv3d_fwd / _bwd_data / _bwd_weight run this problem on the f16x3 MFMA forms
 * (planes of 9 .. 16 rows and columns, channels in fours, 16-byte aligned tensors, the "dw_nomfma" /
 * "dw_wgrad_nomfma" switches off), resp. on the dense small-volume form (volumes of <= 4^3 voxels).
 * x / y: the two tensors of the launch (alignment is part of the answer). */
int adell_dw_mfma_ok(int N, int C, int D, int H, int W, int KD, int KH, int KW, const float* x,
                     const float* y);
int adell_dw_dense_ok(int N, int C, int D, int H, int W, int KD, int KH, int KW, const float* x,
                      const float* y);
int adell_dw_wgrad_mfma_ok(int N, int C, int D, int H, int W, int KD, int KH, int KW, const float* x,
                           const float* dy);

/* Launch plan of a depthwise convolution, host only (no launch, no tensor read, no device needed):
 * what adell_dwconv3d_fwd / adell_dwconv3d_bwd_data (pass 0: one dispatch for both) or
 * adell_dwconv3d_bwd_weight (pass 1) would run under the current tuning switches, decided by the same
 * functions the launch calls. a_aligned / b_aligned: the launch's two tensors (x, y / dy, dx / x, dy)
 * are 16-byte aligned. out[10]:
 *   [0] form (ADELL_DW_*); [1] K, [2] WT of a tile instantiation <K, WT> (ring: 7, 16; else 0);
 *   [3] x segments of a tile row / z segments of the ring; [4] outputs per x segment / planes per z
 *   segment; [5] 1 when 16-byte channel loads are used; [6] blocks of the main kernel;
 *   [7] the most work items one block loops over: rounds of the resident MFMA kernel, items per chunk
 *   (MFMA weight gradient), tiles per split (tile weight gradient), items of a dense block's M tile,
 *   grid-stride rounds (generic), voxels per lane (generic weight gradient), 1 otherwise;
 *   [8] chunks / splits of the weight gradient (generic: rows of 64 channels; forward MFMA: work
 *   items; dense: item blocks); [9] workspace floats this form needs. */
#define ADELL_DW_GENERIC 0
#define ADELL_DW_DENSE 1
#define ADELL_DW_MFMA 2         /* resident: persistent blocks, D <= 16 */
#define ADELL_DW_MFMA_STREAM 3  /* streamed column, D > 16 */
#define ADELL_DW_ZRING 4
#define ADELL_DW_TILE 5
#define ADELL_DW_WGRAD_MFMA 6
int adell_dwconv3d_plan(int pass, int N, int C, int D, int H, int W, int KD, int KH, int KW,
                        int a_aligned, int b_aligned, long* out);

/* Launch plan of the z-ring weight-gradient kernel (csrc/conv_wgrad_zring.hip) for a conv of these
 * extents: returns 1 and fills plan[8] = {column tiles x, y, z segments, planes per segment, input /
 * output channel tiles, resident blocks, 1 when the 16 x 16 tile form (16-channel layers) runs}, or 0
 * when adell_conv3d_bwd_weight_f16x3 runs the layer on the per-plane kernel instead. */
int adell_wgrad_zring_plan(int N, int D, int H, int W, int C0, int C1, int Cout, int KD, int KH,
                           int KW, int SD, int SH, int SW, int Do, int Ho, int Wo, int* plan);
/* The same for a descriptor under a share hint (ADELL_WGRAD_SHARE_*), host only: returns 1 and fills
 * out[11] = {the plan[8] above -- no hint changes it --, [8] resident blocks per CU the launch is sized
 * for (1: the hint is accepted; else 2, or 3 for the 16 x 16 form), [9] dynamic LDS bytes it requests,
 * [10] LDS bytes of a CU those blocks leave to another kernel's}, or 0 when the z-ring kernel does not
 * serve d. An accepted request is the smallest LDS allocation of which two exceed a CU's LDS; it is
 * accepted only while the largest specialised implicit-GEMM block (78 400 B) fits in [10]. */
int adell_wgrad_zring_share_plan(const adell_conv3d_desc* d, int share, int* out);
/* Blocks per CU the runtime's occupancy calculator gives that launch (needs a device, runs no kernel);
 * a negative ADELL_E_* when the z-ring kernel does not serve d. */
int adell_wgrad_zring_occupancy(const adell_conv3d_desc* d, int share);

/* Layer scale folded into a Linear layer's parameters (ConvNeXtBlock3d, res_blocks.py:588-604:
 * gamma * (h W^T + b) = h (gamma W)^T + gamma b): W2[c][k] = gamma[c] W[c][k], b2[c] = gamma[c] b[c]
 * (b / b2 may be NULL), and the backward of that algebra: dW = gamma dW2, db = gamma db2,
 * dgamma[c] = sum_k dW2[c][k] W[c][k] + db2[c] b[c]. W, W2, dW2, dW: [C][K] row-major. */
int adell_rowscale_fwd(const float* gamma, const float* W, const float* b, float* W2, float* b2, int C,
                       int K, void* stream);
int adell_rowscale_bwd(const float* gamma, const float* W, const float* b, const float* dW2,
                       const float* db2, float* dgamma, float* dW, float* db, int C, int K,
                       void* stream);

/* Spatial window of a dense channels-last volume: out[n][d][h][w][:] = in[n][d + od][h + oh][w + ow][:]
 * where that voxel exists, zeros elsewhere (in [N][Di][Hi][Wi][C], out [N][Do][Ho][Wo][C]). Positive
 * offsets and a smaller output: crop_to_size (adell_mri/modules/layers/utils.py:30-52); negative
 * offsets and a larger output: its gradient (a zero frame around dY). */
int adell_window_ndhwc(const float* in, float* out, int N, int C, int Di, int Hi, int Wi, int Do, int Ho,
                       int Wo, int od, int oh, int ow, void* stream);

long adell_gibbs_workspace(int N, int D, int H, int W, int C);
int adell_gibbs_lowpass(const float* x, float* out, int N, int D, int H, int W, int C,
                        const float* radius, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Ensemble classifiers and the Gaussian-process (SNGP) head (csrc/ensemble.hip; the reference's
 * modules/classification/classification/ensemble.py and modules/layers/gaussian_process.py). fp32,
 * dense row-major tensors, every sum in a fixed order in fp64, no atomics: bit-reproducible.
 * ---------------------------------------------------------------------- */
#define ADELL_GP_FUSED 0     /* adell_gp_phi_fwd / _bwd */
#define ADELL_GP_COMPOSED 1  /* layer norm, GEMM and adell_gp_cos */
#define ADELL_ENSEMBLE_MAX 8 /* members of one adell_ensemble_* launch */
/* Host only: the route of a Gaussian-process layer over n rows of i inputs with r random features
 * (the fused kernels keep i + r floats in LDS: i <= 1024 and r <= 4096), or ADELL_E_BADARG. */
int adell_gp_route(int n, int i, int r);
/* One launch: x^ = LayerNorm(x) over the row (gamma, beta [i]; both NULL: x^ = x), z = b - W x^
 * (W [r][i], b [r]), phi [N][r] = scale cos(z), logits [N][o] = phi weights^T (weights [o][r];
 * logits NULL: phi only). mean, rstd [N]: the row statistics, written with the norm. */
int adell_gp_phi_fwd(const float* x, const float* gamma, const float* beta, const float* W,
                     const float* b, const float* weights, int N, int I, int R, int O, float scale,
                     float eps, float* phi, float* logits, float* mean, float* rstd, void* stream);
/* At most two launches: from dlogits [N][o] and / or dphi [N][r] (either may be NULL) dx [N][i], and
 * dgamma, dbeta [i], dweights [o][r] summed over the rows in order (each may be NULL). dxhat [N][i]:
 * the gradient of x^, needed with dgamma (without the norm it is dx itself and may be NULL). */
int adell_gp_phi_bwd(const float* x, const float* gamma, const float* beta, const float* W,
                     const float* b, const float* weights, const float* phi, const float* mean,
                     const float* rstd, const float* dlogits, const float* dphi, int N, int I, int R,
                     int O, float scale, float eps, float* dx, float* dxhat, float* dgamma,
                     float* dbeta, float* dweights, void* stream);
/* The epilogue of the composed route over t = x^ W^T [rows][r]: dphi NULL: out = scale cos(b - t);
 * else the gradient of t, out = scale sin(b - t) dphi. */
int adell_gp_cos(const float* t, const float* b, const float* dphi, long rows, int R, float scale,
                 float* out, void* stream);
/* One launch, in place on P [r][r]: U = sum_n c_n phi_n phi_n^T (n in order), c_n = sum over the row
 * of prob [N][Cp] of p (1 - p); P += U, or P = m P + (1 - m) U with use_momentum. The upper triangle
 * is computed and mirrored: P comes out exactly symmetric. */
int adell_gp_precision_update(const float* phi, const float* prob, int N, int R, int Cp,
                              int use_momentum, float m, float* P, void* stream);
/* var[n] = phi_n^T cov phi_n (cov [r][r]). */
int adell_gp_variance(const float* phi, const float* cov, int N, int R, float* var, void* stream);
/* samples [S][N][o] = mean [N][o] + sqrt(max(var[n], 0)) eps [S][N][o]; smean, sstd [N][o]: their
 * mean and unbiased standard deviation over S (S = 1: NaN). */
int adell_gp_sample(const float* mean, const float* var, const float* eps, int S, int N, int O,
                    float* samples, float* smean, float* sstd, void* stream);
/* K <= ADELL_ENSEMBLE_MAX members x[k] [B][V[k]][C[k]] (channels last; V = 1: a vector) max-pooled over
 * their voxels into out [B][sum C] at their channel offset; arg: the int32 voxel index, the lowest on
 * a tie, the first NaN wins. x, C, V (and dx) are HOST arrays of K entries: the device pointers
 * travel in the launch's arguments. Backward: dx[k] (NULL: not wanted) = g scattered to the arg-max. */
int adell_ensemble_pool_fwd(const float* const* x, const int* C, const long* V, int K, int B,
                            float* out, int* arg, void* stream);
int adell_ensemble_pool_bwd(const float* g, const int* arg, const int* C, const long* V, int K, int B,
                            float* const* dx, void* stream);
/* y [B][C] = sigmoid (C = 1) or softmax over C of the mean of the K <= ADELL_ENSEMBLE_MAX logit
 * tensors x[k] [B][C] (host array of device pointers); backward: every dx[k] (NULL: not wanted) = the
 * gradient of the mean / K. */
int adell_ensemble_average_fwd(const float* const* x, int K, int B, int C, float* y, void* stream);
int adell_ensemble_average_bwd(const float* y, const float* dy, int K, int B, int C, float* const* dx,
                               void* stream);

/* ------------------------------------------------------------------------
 * Batch-ensemble layers (csrc/batch_ensemble.hip; the reference's modules/layers/batch_ensemble.py,
 * arXiv:2002.06715). Activations [B][V][C] (NDHWC memory; V = 1: rows [B][C]), tables [n][C]. fp32,
 * every sum in a fixed order in fp64, no atomics: bit-reproducible. B K <= 65535 rows per launch.
 * ---------------------------------------------------------------------- */
/* One launch: out[k B + b] = x[b] * table[row] * scale for k < K; x is read once. idx (int32 [B] on the
 * device, K = 1): row = idx[b], the training scale; idx NULL: row = m0 + k, the members [m0, m0 + K)
 * side by side. table NULL: all ones. An index outside [0, n) makes its item NaN and is never read
 * through. */
int adell_be_expand(const float* x, const float* table, const int* idx, int m0, int K, int n, float scale,
                    float* out, int B, long V, int C, void* stream);
/* One launch: out[b] = acc[b] (NULL: 0) + sum over k < K of table[m0 + k] y[k B + b], one fma chain in
 * member order; with `scaled` the chain's end is multiplied by scale. Cutting the members into several
 * calls (acc = the previous out) gives the same bits as one call. */
int adell_be_members_sum(const float* y, const float* table, const float* acc, int m0, int K, int n,
                         float scale, int scaled, float* out, int B, long V, int C, void* stream);
/* Doubles of the partial-sum workspace of adell_be_tgrad (K = 0 counts as one copy). */
long adell_be_tgrad_workspace_doubles(int B, long V, int C, int K);
/* At most two launches. One pass over p [max(K, 1) B rows] and q [B rows] leaves fp64 partial sums of
 * p[k B + b] q[b] over tiles of voxels in part; the fold writes all n rows of dtable.
 *   K = 0, the training scale's backward (p = dy, q = x): dx[b] = p[b] table[idx[b]] in the same pass
 *     (NULL: skipped) and dtable[m] = scale * the sum over the items with idx[b] == m in ascending
 *     order (idx NULL: every item is member 0's); a member nobody drew gets an exact 0.
 *   K > 0, members side by side: dtable[m0 + k] = scale * the sum over b; other rows 0. dx must be NULL.
 * dtable NULL (with part NULL): dx alone, one launch. */
int adell_be_tgrad(const float* p, const float* q, const float* table, const int* idx, int m0, int K,
                   int n, float scale, float* dx, float* dtable, double* part, int B, long V, int C,
                   void* stream);

/* ------------------------------------------------------------------------
 * Deconfounded classification (csrc/deconfound.hip; the reference's DeconfoundedNetPL,
 * modules/classification/pl.py). The pooled features x [B][F] are read in place: columns [0, n) are
 * the confounded ones, [n, F) the others, 0 < n < F. fp32, every sum in a fixed order in fp64, no float
 * atomics: bit-reproducible.
 * ---------------------------------------------------------------------- */
/* One launch each: a [B][n] and b [B][F - n] from x; dx [B][F] from da and db (NULL: zeros). */
int adell_deconf_split_fwd(const float* x, float* a, float* b, int B, int F, int n, void* stream);
int adell_deconf_split_bwd(const float* da, const float* db, float* dx, int B, int F, int n, void* stream);
/* Doubles of the forward's workspace (16 bytes of ticket counter and a partial per block) and of what it
 * keeps for the backward: mean [F], centred norm [F], the ratio before the clamp [n][F - n]. */
long adell_deconf_corr_workspace_doubles(int B, int F, int n);
long adell_deconf_corr_saved_doubles(int B, int F, int n);
/* One launch (and the counter's memset): loss[0] = the mean over the n (F - n) pairs of
 * clamp(<a', b'> / max(|a'| |b'|, 1e-8), -1, 1)^2, a' and b' the columns centred over the batch. */
int adell_deconf_corr_fwd(const float* x, int B, int F, int n, double* ws, double* saved, float* loss,
                          void* stream);
/* One launch: dx [B][F] = g[0] * the gradient, clamp gradients passed on their closed intervals; the
 * gradient of sqrt at an exactly zero centred norm is 0 (such a column gets an exact 0). */
int adell_deconf_corr_bwd(const float* x, const double* saved, const float* g, int B, int F, int n,
                          float* dx, void* stream);
#define ADELL_DECONF_MAX_HEADS 8    /* categorical heads of one launch */
#define ADELL_DECONF_MAX_CLASSES 64 /* classes of one head */
#define ADELL_DECONF_MAX_CONT 64    /* outputs of the regression head */
#define ADELL_DECONF_MAX_CONF 1024  /* confounded columns (kept in LDS) */
#define ADELL_DECONF_FUSED 0
#define ADELL_DECONF_COMPOSED 1
/* The linear confounder heads: W[h] [K[h]][n] and b[h] [K[h]] per categorical head, Wc [n_cont][n] and
 * bc [n_cont] of the regression head (device pointers, the struct itself on the host). */
typedef struct adell_deconf_heads {
  int32_t n_heads, n_cont;
  int32_t K[ADELL_DECONF_MAX_HEADS];
  const float* W[ADELL_DECONF_MAX_HEADS];
  const float* b[ADELL_DECONF_MAX_HEADS];
  const float* Wc;
  const float* bc;
} adell_deconf_heads;
typedef struct adell_deconf_head_grads { /* NULL: not wanted */
  float* dW[ADELL_DECONF_MAX_HEADS];
  float* db[ADELL_DECONF_MAX_HEADS];
  float* dWc;
  float* dbc;
} adell_deconf_head_grads;
/* Host only: ADELL_DECONF_FUSED when the kernels below take n confounded columns, n_heads heads of K[h]
 * classes and n_cont regression outputs, ADELL_DECONF_COMPOSED beyond a limit above, or ADELL_E_BADARG. */
int adell_deconf_route(int n, int n_heads, const int* K, int n_cont);
long adell_deconf_heads_workspace_doubles(int B);
/* One launch (and the counter's memset): out[0] = conf_mult * sum_h mean_b CE(x[b][:n] W[h]^T + b[h],
 * cat_t[h][b]) / n_heads, out[1] = conf_mult * the mean squared error of the regression head against
 * cont_t [B][n_cont]; 0 for a kind without heads. cat_t: int64 [n_heads][B]; a label outside [0, K[h])
 * is never used as an index and makes the loss NaN. */
int adell_deconf_heads_fwd(const adell_deconf_heads* hd, const float* x, const long long* cat_t,
                           const float* cont_t, int B, int F, int n, float conf_mult, double* ws,
                           float* out, void* stream);
/* Two launches: dz [B][sum K + n_cont] doubles (workspace) and dx [B][F] (zeros past n; NULL: skipped)
 * per item, then every dW and db of gr (NULL: one launch) over the items in order. g_cat / g_cont: the
 * one-element gradients of out[0] / out[1] (NULL: none). */
int adell_deconf_heads_bwd(const adell_deconf_heads* hd, const adell_deconf_head_grads* gr, const float* x,
                           const long long* cat_t, const float* cont_t, const float* g_cat,
                           const float* g_cont, int B, int F, int n, float conf_mult, double* dz,
                           float* dx, void* stream);

/* ------------------------------------------------------------------------
 * Evaluation with uncertainty (csrc/bootstrap.hip; the reference's utils/bootstrap_metrics.py and
 * modules/conformal_prediction/conformal.py). Integer or fixed-order fp64 arithmetic: bit-reproducible.
 * ---------------------------------------------------------------------- */
#define ADELL_BOOT_MAX_N 196608 /* samples of the bitmask route: 72 KiB of LDS, two blocks per CU */
#define ADELL_BOOT_BITMASK 0
#define ADELL_BOOT_LOOP 1
/* Host only: ADELL_BOOT_BITMASK when adell_boot_auroc_pairs takes n samples, ADELL_BOOT_LOOP beyond
 * ADELL_BOOT_MAX_N (the caller loops over adell_cls_auroc_pairs), or ADELL_E_BADARG. */
int adell_boot_auroc_route(int n);
/* One launch, a block per resample: out[r] = (2 #{pos > neg} + #{pos == neg}, positives, negatives, bad
 * indices) over the samples idx[r][0 .. m) (int32 [R][m], distinct values in [0, n)), every element
 * written. The caller sorts the n scores once, stable and ascending: pos[i] is the sorted position of
 * sample i, [gstart[p], gend[p]) the run of equal scores around sorted position p, lab[p] the label at p
 * (1 positive, 0 negative, anything else skipped). Bad indices: a value outside [0, n), or one that a row
 * holds twice (of a sample that is not skipped); a row with any has unspecified counts. LDS: 3 n / 8
 * bytes, n <= ADELL_BOOT_MAX_N. */
int adell_boot_auroc_pairs(const int* idx, int R, int m, const int* pos, const int* gstart, const int* gend,
                           const int* lab, int n, long long* out, void* stream);
#define ADELL_APS_MAX_CLASSES 64
/* One launch: cum[i][c] = the cumulative probability of row i of p [N][C] at the rank of class c in the
 * stable descending order (of equal probabilities the lower index first), every prefix summed in fp64 in
 * rank order and rounded to fp32. With y (int64 [N]) and score [N]: score[i] = cum[i][y[i]], NaN for a
 * label outside [0, C), which is never used as an index; both NULL: skipped. C <= ADELL_APS_MAX_CLASSES. */
int adell_aps_cumulative(const float* p, const long long* y, int N, int C, float* cum, float* score,
                         void* stream);

/* ------------------------------------------------------------------------
 * Losses of the semi-supervised U-Net beyond LocalContrastiveLoss (csrc/semisl.hip; the reference's
 * LocalContrastiveLossWithAnchors, NearestNeighbourLoss and PseudoLabelCrossEntropy,
 * semi_supervised_segmentation/losses.py). fp32 data, fixed-order fp64 sums, no float atomics:
 * bit-reproducible. Feature rows are NDHWC, [B][V][C]; label and logit planes channel-major, [B][K][V].
 * ---------------------------------------------------------------------- */
#define ADELL_SEMISL_ANCHOR 0
#define ADELL_SEMISL_NN 1
#define ADELL_SEMISL_PSEUDO_LABEL 2
#define ADELL_SEMISL_FUSED 0
#define ADELL_SEMISL_COMPOSED 1
#define ADELL_SEMISL_ANCHOR_MAX_C 1024 /* the anchor kernels loop over channel quads: no register limit */
#define ADELL_SEMISL_NN_MAX_C 64       /* two blocks of the nearest-neighbour kernels per CU's LDS */
#define ADELL_SEMISL_MAX_CLASSES 64
#define ADELL_SEMISL_PUT_CHUNK 4096    /* voxels per entry of the adell_nn_queue_count table */
/* Host only: ADELL_SEMISL_FUSED when the kernels of `kind` take C channels (anchor, nn: C % 4 == 0 and
 * C <= the kind's maximum) and K classes (nn, pseudo-label: K <= ADELL_SEMISL_MAX_CLASSES),
 * ADELL_SEMISL_COMPOSED beyond, or ADELL_E_BADARG. An argument the kind does not use is ignored. */
int adell_semisl_route(int kind, int C, int K);
/* loss[b] = sum_v (xlogy(q_v, q_v) - q_v p_v), p = softmax_v(cos(x, a1) / T), q = softmax_v(cos(x, a2) / T),
 * the softmax over the V voxels of item b: F.kl_div(p, q, reduction="none").sum(-1) with a probability
 * (not a log-probability) as its input. Four launches. Kept for the backward: sim1, sim2 [B][V] (the
 * cosines / T) and stats [B][6] = (max_1, log sum_1, max_2, log sum_2, sum q log q, sum p q).
 * Workspace: adell_loco_anchor_workspace_doubles(B, V, C) doubles. */
long adell_loco_anchor_workspace_doubles(int B, long V, int C);
int adell_loco_anchor_fwd(const float* x, const float* a1, const float* a2, int B, long V, int C,
                          float temperature, float* sim1, float* sim2, double* stats, float* loss,
                          double* workspace, long workspace_doubles, void* stream);
/* One launch: dx (always), da1 and da2 (NULL: not wanted) for the loss gradient gloss [B]. */
int adell_loco_anchor_bwd(const float* x, const float* a1, const float* a2, const float* sim1,
                          const float* sim2, const double* stats, const float* gloss, int B, long V, int C,
                          float temperature, float* dx, float* da1, float* da2, void* stream);
/* out[q] = past[q] / max(|past[q]|, 1e-8), [Q][C]; one launch. */
int adell_nn_queue_normalize(const float* past, int Q, int C, float* out, void* stream);
/* loss = the mean over the voxels whose ratio is not NaN of S / O, S = sum_q exp(-d_q m_q / T),
 * O = sum_q exp(-d_q (1 - m_q) / T), d_q = 1 - cos(x[b][v], past_q), m_q = y[b][past_class[q]][v] (0 for a
 * class outside [0, K), which is never used as an index); a NaN term counts 0. pastn: the rows of
 * adell_nn_queue_normalize. Two launches. Kept for the backward: S, O [B V] and stats = (sum, count).
 * Workspace: adell_nn_queue_workspace_doubles(B, V) doubles. The [B][V][Q] products are never written. */
long adell_nn_queue_workspace_doubles(int B, long V);
int adell_nn_queue_loss_fwd(const float* x, const float* y, const float* pastn, const int* past_class, int B,
                            long V, int C, int K, int Q, float temperature, float* S, float* O,
                            double* stats, float* loss, double* workspace, long workspace_doubles,
                            void* stream);
/* One launch: dx [B][V][C] for the gradient g [1]; an exact 0 at a voxel whose ratio is NaN. */
int adell_nn_queue_loss_bwd(const float* x, const float* y, const float* pastn, const int* past_class,
                            const float* S, const float* O, const double* stats, const float* g, int B,
                            long V, int C, int K, int Q, float temperature, float* dx, void* stream);
/* cc[b][k][chunk] = #{v in the chunk of ADELL_SEMISL_PUT_CHUNK voxels: y[b][k][v] > 0}, int32, every
 * entry written; one launch. */
int adell_nn_queue_count(const float* y, int B, int K, long V, int* cc, void* stream);
/* out[r] = the row x[b][:][v] of the sel_rank[r]-th positive (y > 0; item-major, then voxel) of class
 * sel_class[r]; incl [K][B chunks] int64: the inclusive scan of cc over (item, chunk) per class. x is
 * read through the element strides (sb, sc, sv) of its [B][C][V] view, channel-major or channels-last.
 * A rank beyond the positives of its class writes zeros. One launch, a wave per row. */
int adell_nn_queue_gather(const float* x, const float* y, const long long* incl, const int* sel_class,
                          const long long* sel_rank, int n_sel, int B, int K, long V, int C, long sb, long sc,
                          long sv, float* out, void* stream);
/* Cross entropy of the logits pred [B][K][V] against the probability targets
 * t_k = (proba_k > threshold) (1 - label_smoothing) + label_smoothing / K, weighted per class (weight
 * NULL: ones): the sum over voxels and classes of -w_k t_k log_softmax_k, divided by B V when `mean`.
 * One launch each way. workspace: adell_pseudo_label_ce_workspace_doubles(B, V) doubles whose first
 * word is zero on entry (and left zero). */
long adell_pseudo_label_ce_workspace_doubles(int B, long V);
int adell_pseudo_label_ce_fwd(const float* pred, const float* proba, const float* weight, int B, int K,
                              long V, float threshold, float label_smoothing, int mean, float* loss,
                              double* workspace, long workspace_doubles, void* stream);
int adell_pseudo_label_ce_bwd(const float* pred, const float* proba, const float* weight, const float* g,
                              int B, int K, long V, float threshold, float label_smoothing, int mean,
                              float* dpred, void* stream);

/* ------------------------------------------------------------------------
 * Spectral normalisation of a weight (csrc/spectral_norm.hip; torch's _SpectralNorm parametrization,
 * which the reference's utils/pl_callbacks.SpectralNorm applies). fp32 data, fixed-order fp64 sums, no
 * float atomics: bit-reproducible. The weight is read in place as the matrix [h][w], w = outer * inner,
 * element (r, c = o * inner + t) at (o * h + r) * inner + t: dim = 0 is outer = 1, a transposed-conv
 * weight [Cin][Cout][k...] is outer = Cin, h = Cout, inner = prod(k).
 * ---------------------------------------------------------------------- */
#define ADELL_SN_BLOCK 0
#define ADELL_SN_GRID 1
#define ADELL_SN_COMPOSED 2
#define ADELL_SN_MAX_DIM 32768 /* rows and columns of the grid route */
/* Host only: ADELL_SN_BLOCK when one workgroup keeps the matrix, both vectors and the fp64 products in
 * LDS (4 (h w + h + w) + 8 (max(h, w) + 1040) <= 158 KiB), ADELL_SN_GRID up to ADELL_SN_MAX_DIM rows and
 * columns, ADELL_SN_COMPOSED beyond (the caller composes torch operators), or ADELL_E_BADARG. */
int adell_spectral_norm_route(long h, long w);
/* Doubles of workspace of both directions (the ticket counter's 16 bytes first), or ADELL_E_BADARG. */
long adell_spectral_norm_workspace_doubles(long h, long w);
/* n_iter times u <- normalize(W v), v <- normalize(W^T u) IN PLACE in u [h] and v [w] (normalize(x) =
 * x / max(|x|, eps), rounded to fp32), then sigma[0] = u^T W v (fp64; with n_iter > 0 taken as
 * (W^T u) . v of the last half-iteration), out = W / sigma in the weight's layout, and u_used / v_used =
 * the vectors sigma was taken with. n_iter = 0 (eval mode): u and v are only read. A zero weight gives
 * sigma = 0 and NaN in out. Block route: one launch; grid route: 2 n_iter + 1 launches (2 for n_iter = 0)
 * and the counter's memset. */
int adell_spectral_norm_fwd(const float* W, float* u, float* v, int outer, int h, int inner, int n_iter,
                            double eps, double* ws, long ws_doubles, float* u_used, float* v_used,
                            double* sigma, float* out, void* stream);
/* dW = (G - <G, Wsn> u v^T) / sigma in the weight's layout, u and v constants (the forward's u_used /
 * v_used). Block route: one launch; grid route: two and the counter's memset. */
int adell_spectral_norm_bwd(const float* G, const float* Wsn, const float* u, const float* v,
                            const double* sigma, int outer, int h, int inner, double* ws, long ws_doubles,
                            float* dW, void* stream);

/* ------------------------------------------------------------------------
 * Elastic-weight-consolidation penalty (csrc/ewc.hip): sum_k ||p_k - p0_k||_p over any number of
 * parameter tensors, the reference's ElasticWeightConsolidation.__call__
 * (continuous_learning/regularization.py:38-45), value and gradient in three launches. fp32 data (the
 * difference is taken in fp32 as the reference takes it), fp64 sums in a fixed order, no float
 * atomics: bit-reproducible. p is any finite number >= 1; 1 and 2 have instances without pow.
 * `table` is a DEVICE array of `chunks` rows of 5 longs: parameter pointer, anchor pointer, element
 * count (1 .. adell_ewc_chunk()), tensor index, destination offset in elements (read by
 * adell_ewc_grad only). The chunks of a tensor are consecutive rows; `tensor_first` is a DEVICE array of
 * tensors + 1 longs, the rows of tensor k being tensor_first[k] .. tensor_first[k + 1] - 1. Null
 * pointers, counts < 1 and a p that is not a finite number >= 1 are refused before any HIP call.
 * ---------------------------------------------------------------------- */
/* continuous_learning/regularization.py:38-45: elements per chunk (a compile-time constant). */
int adell_ewc_chunk(void);
/* continuous_learning/regularization.py:38-45: doubles of workspace of the partials and finalize
 * passes (0: bad arguments). */
long adell_ewc_workspace_doubles(int chunks, int tensors);
/* continuous_learning/regularization.py:38-45: workspace[r] = sum |p - p0|^p over chunk r. */
int adell_ewc_partials(const long* table, int chunks, double p, double* workspace, void* stream);
/* continuous_learning/regularization.py:38-45: norms[k] = (sum of tensor k's partials)^(1/p) in fp32
 * (kept for adell_ewc_grad), total[0] = sum_k norm_k (fp64, stored as fp32). */
int adell_ewc_finalize(const long* tensor_first, int tensors, int chunks, double p, double* workspace,
                       float* norms, float* total, void* stream);
/* continuous_learning/regularization.py:38-45 (its gradient): g = C sgn(d) |d|^(p-1) / norm_k^(p-1),
 * d = p - p0 in fp32, C = c * c_dev[0] (c_dev may be NULL: C = c), exactly 0 where d == 0 or
 * norm_k == 0 (torch's masked forms). add == 0: base[offset + i] = g; add != 0: base[offset + i] += g. */
int adell_ewc_grad(const long* table, int chunks, double p, const float* norms, float c,
                   const float* c_dev, int add, float* base, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ADELL_HIP_H */
