// Which kernel a vps_conv2d launch gets, decided in ONE host-only function (conv_plan.cpp, plain C++: no HIP header, no HIP call,
// testable without a GPU - tests/test_conv_plan.py). vps_conv2d (conv_mfma.hip) asks for the plan and switches over its kernel id;
// the vpsi_launch_* functions of the conv_*.hip files launch what was planned and decide nothing.
#pragma once
#include <stddef.h>
#include "../../include/vps_hip.h"

#ifndef VPS_EARG
#define VPS_EARG(x) (-1000 - (x))
#endif

// in the order of precedence of the planner
enum conv_kernel {
    CONV_K_NONE = 0,        // no launch: conv_plan.err says why
    CONV_K_SMALL3X3V,       // conv_small.hip: narrow outputs in exact fp32, sliding-window 3x3
    CONV_K_SMALL_BATCHED,   //                 eight loads per lane in flight
    CONV_K_SMALL,           //                 one load per step
    CONV_K_THIN,            // conv_thin.hip:  thin-input layers at full resolution
    CONV_K_DCN256,          // conv_mfma.hip:  256-column deformable block
    CONV_K_N16T,            // conv_n16.hip:   <= 16 channels, the four classes of a transposed layer in one block
    CONV_K_N32,             //                 17 .. 32 channels
    CONV_K_N16,             //                 5 .. 16 channels
    CONV_K_H8S2,            // conv_h8.hip:    stride-2 phase-split 8-wave halo kernel
    CONV_K_H8P,             // conv_h8p.hip:   pipelined 8-wave halo kernel
    CONV_K_H8,              // conv_h8.hip:    8-wave halo kernel
    CONV_K_HALO,            // conv_mfma.hip:  4-wave halo kernel
    CONV_K_PW,              // conv_pw.hip:    persistent pointwise kernel
    CONV_K_Q,               // conv_q.hip:     uniform-lead kernel
    CONV_K_F32,             // conv_mfma.hip:  exact fp32 MFMA
    CONV_K_BF16P,           // conv_mfma.hip:  pipelined split-operand kernel
};

struct conv_plan {
    int kernel;             // conv_kernel
    int err;                // 0, or the VPS_EARG value vps_conv2d returns
    int M;                  // N * Qh * Qw
    int tiles_m, tiles_n;   // tiles of the PLANNED kernel (128 rows | 8x16 | 8x32 patches; the thin kernel's 32-wide patches)
    int per_split;          // k-steps of a split-K range (pipelined kernels)
    int chunks_per_split;   // 32-channel chunks of a range (halo kernels)
    unsigned grid, block;
    size_t smem;            // dynamic LDS (small kernels)
    int nk, nit;            // pw: k-steps per tile, tiles per block
    int G, logG, nslot;     // small / small_batched: lanes per pixel, channel slots per lane
    int runs_per_row, total_runs;   // small3x3v
    int thin;               // thin: instance 0 .. 3 (conv_thin_shapes), tiles_m x tiles_n = tiles_y x tiles_x there
    int ntiles;
    bool needs_reduce;      // split-K partials are summed by conv_splitk_reduce_kernel<reduce_v4 ? 4 : 1>
    bool reduce_v4;
};

// what the planner has to know about the device: filled once by the .hip side (occupancy queries of the persistent kernels)
struct conv_limits {
    int cus;                // compute units
    int pw_per_cu[2];       // resident blocks per CU of conv_pw_kernel<TN = 1 | 2>
    int thin_per_cu[4];     // ... of the four conv_thin_kernel instances (conv_thin_shapes order)
};

// environment switches (A/B runs), read by conv_switches_now() in conv_mfma.hip and nowhere else
struct conv_switches {
    bool pw;        // VPS_PW=0: no persistent pointwise kernel
    bool h8p;       // VPS_H8P=0: conv_mfma_h8_kernel instead of the pipelined instance
    bool n16t;      // VPS_N16T=0: transposed <= 16-channel layers as four class launches
    bool n32;       // VPS_N32=0: layers with 17 .. 32 output channels stay on the 32-column halo kernel
    bool s2_halo;   // VPS_S2_HALO=0: stride-2 layers on the pipelined kernels
    bool thin;      // VPS_THIN=0: no thin-input kernel
    bool debug_occ; // VPS_DEBUG_OCC: print the occupancy numbers of conv_limits once
};

// <C4 = cin_pad, KS, S = stride, PH = patch height> of the thin-input instances
struct conv_thin_shape { int c4, ks, s, ph; };
extern const conv_thin_shape conv_thin_shapes[4];

int vpsi_conv_check(const vps_conv_desc& d);   // the argument checks: 0 or a VPS_EARG value; touches nothing but the descriptor
conv_plan vpsi_conv_plan(const vps_conv_desc& d, const conv_limits& lim, const conv_switches& sw);   // of a CHECKED descriptor
const char* vpsi_conv_kernel_name(int kernel);

#ifdef __HIPCC__
// the launchers: each enqueues the planned kernel, unconditionally
void vpsi_launch_conv_small(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_thin(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_n16(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_h8(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_h8p(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_h8s2(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_pw(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
void vpsi_launch_conv_q(const vps_conv_desc& d, const conv_plan& p, hipStream_t s);
// occupancy of the persistent kernels for conv_limits (and the VPS_DEBUG_OCC lines)
void vpsi_conv_pw_limits(conv_limits& lim, bool debug);
void vpsi_conv_thin_limits(conv_limits& lim, bool debug);
void vpsi_conv_q_debug_occ();
#endif
