// Host side of the conv weight gradient: the plan structs and the prototypes that cross the four
// translation units (conv_wgrad.hip, conv_wgrad_f16.hip, conv_wgrad_zring.hip, conv_wgrad_s2.hip)
// and conv_small.hip, each written once. Every internal function takes the conv descriptor and its
// plan; none of them is exported.
#pragma once
#include "common.h"

// z-ring kernel for 3^3 stride-1 convolutions (conv_wgrad_zring.hip). The field order is the
// plan[8] of the exported adell_wgrad_zring_plan (include/adell_hip.h).
struct WgradZrPlan {
  int ntx, nty, nseg, seglen, nci, nco, R, t16;
};
// true + plan when the z-ring kernel serves the problem
bool adell_wgrad_zring_plan_desc(const adell_conv3d_desc& d, WgradZrPlan& p);
// Residency of a z-ring launch under a share hint (ADELL_WGRAD_SHARE_*, include/adell_hip.h): the
// blocks per CU it is sized for, the dynamic LDS it requests, the LDS of a CU it leaves to others.
struct WgradZrShare {
  int per_cu;
  size_t lds, room;
};
WgradZrShare adell_wgrad_zring_share(const adell_conv3d_desc& d, const WgradZrPlan& p, int share);
// the most LDS a specialised 3x3x3 stride-1 implicit-GEMM block asks for (conv3d.hip)
size_t adell_conv_f16_spec_lds_max();
// slabs: [R][27][Cin][Cout], wsdb: [R][Cout] or null; xk0 / xk1 non-null = that source holds split
// rows; share: the caller's hint (the launch is the same grid and the same bits either way)
int adell_wgrad_zring_launch(const adell_conv3d_desc& d, const WgradZrPlan& p, const float* x0,
                             const float* x1, const float* dy, float* slabs, float* wsdb,
                             const unsigned* xmax, const unsigned* ymax, hipStream_t st,
                             const int* xk0, const int* xk1, int share);

// the 32 -> 32 stride-2 downsampling layer (conv_wgrad_s2.hip)
struct WgradS2Plan {
  int ntx, nty, ntz, nbricks, blocks, R;
};
bool adell_wgrad_s2_plan(const adell_conv3d_desc& d, WgradS2Plan& p);
int adell_wgrad_s2_launch(const adell_conv3d_desc& d, const WgradS2Plan& p, const float* x,
                          const float* dy, float* slabs, float* wsdb, const unsigned* xmax,
                          const unsigned* ymax, hipStream_t st);

// per-plane f16x3 kernel (conv_wgrad_f16.hip)
struct WgradF16Plan {
  int lTY, HX, HY, TCI, TCO, nci, nco, maxj, R, ntx, nty, GKH, NGY, ksplit;
  size_t lds;
};

// fp32 kernel (conv_wgrad.hip); maxj_inst: the MAXJ of the instance that runs the plan
struct WgradPlan {
  int lTX, lTY, lTZ, HX, HY, HZ, TCI, TCO, nci, nco, KDg, ngrp, R, maxj, maxj_inst;
  size_t lds;
  long ntiles;
};
int adell_wgrad_plan(const adell_conv3d_desc& d, WgradPlan* p);

// fixed-order fold of the R slabs into torch's [Cout][Cin][taps] layout, and of wsdb into db
// (conv_wgrad.hip)
extern "C" int adell_wgrad_reduce_launch(const float* ws, float* out, int R, int ntap, int Cin,
                                         int Cout, const float* wsdb, float* db, void* stream);

// small-channel paths (conv_small.hip): workspace > 0 when the vector-ALU kernel takes the problem
extern "C" long adell_wgrad_small_workspace(const adell_conv3d_desc* d);
extern "C" int adell_wgrad_small(const adell_conv3d_desc* d, const float* x0, const float* x1,
                                 const float* dy, float* dw, float* db, void* workspace,
                                 size_t workspace_bytes, void* stream);
