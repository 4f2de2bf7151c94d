/*
 * vps_hip.h — C-ABI of libvpship.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * VPSNet FuseTrack inference hot path (PanopticFuseTrack.simple_test).
 *
 * Conventions
 *   - Every entry point returns 0 on success, a negative hipError_t otherwise, -1000-x for argument
 *     errors. Nothing throws, nothing allocates, nothing synchronises: the caller owns all device
 *     memory (including workspaces) and passes the hipStream_t (as void*) to launch on.
 *   - All tensors are fp32 device pointers unless stated. The internal activation layout is NHWC
 *     with an explicit per-pixel channel stride `ld` (floats) and channel offset `coff`, so that
 *     producers write straight into slices of concat buffers (no torch.cat on the path).
 *   - "ref:" lines cite the interface in mcahny/vps (relative to the reference root) that the
 *     symbol replaces.
 */
#ifndef VPS_HIP_H
#define VPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------------------------------------
 * Library info
 * -------------------------------------------------------------------------------------------- */
/* returns the ABI version of the library (bumped on any signature change) */
int vps_abi_version(void);
/* human readable build string: arch, kernels */
const char* vps_build_info(void);

/* ----------------------------------------------------------------------------------------------
 * Dense contraction: conv / transposed conv / linear / deformable conv as implicit GEMM on MFMA
 *   ref: every torch.nn.Conv2d / ConvTranspose2d / Linear + BatchNorm2d(eval) + ReLU/LeakyReLU on the
 *        path (SURVEY §8a a2,a7,a8,a11-a15,a17,a19,a20), mmdet/ops/dcn/src/deform_conv_cuda.cpp:151-250
 *        (deform_conv_forward_cuda) + deform_conv_cuda_kernel.cu:189-241 (deformable_im2col).
 * GEMM view: out[m][co] = act( scale[co] * sum_k A[m][k] * Wp[co][k] + shift[co] + res[m][co] )
 *   m  = (n, qy, qx) output-grid pixel,  k = (ky*KW + kx)*cin_pad + ci
 *   A[m][k] = in[n][qy*stride - pad_y + ky][qx*stride - pad_x + kx][ci]   (0 outside the image)
 *   deformable: A sampled bilinearly at (.. + dh, .. + dw) from `offset` (per-corner zeroing).
 * Transposed convs are `nclass` = s*s independent convs (one per output parity class); class c
 * (py = c / os_x, px = c % os_x) uses weight block c, pads pad_y[py], pad_x[px] and writes output pixel
 * (qy*os_y + py, qx*os_x + px).
 * -------------------------------------------------------------------------------------------- */
enum { VPS_ACT_NONE = 0, VPS_ACT_RELU = 1, VPS_ACT_LEAKY = 2 };
/* arithmetic of the contraction (accumulation is always fp32):
 *   VPS_PREC_F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32), needs `w`
 *   VPS_PREC_BF16   operands rounded to bf16 (RNE) when staged, 1 bf16 MFMA per product (~2^-8 relative): the plain
 *                   "bf16 in, fp32 accumulate" arithmetic of BASELINE config 5; activations stay fp32 in HBM; needs `w_split`
 *   VPS_PREC_BF16X3 fp32 operands split into 2 bf16 terms, 3 bf16 MFMAs per product (~2^-16 relative), needs `w_split`
 *   VPS_PREC_BF16X6 3 bf16 terms, 6 bf16 MFMAs per product (~2^-23 relative, fp32-grade), needs `w_split`
 *   VPS_PREC_F16X3  fp32 operands split into 2 fp16 terms with a scaled residual, 3 fp16 MFMAs per product, needs `w_split`:
 *                     x = h0 + 2^-11*h1,  h0 = fp16(x), h1 = fp16((x - h0) * 2^11)        (22 significand bits)
 *                     w = g0 + g1,        g0 = fp16(w), g1 = fp16(w - g0),  g2 = 2^-11*g0 (exact for |g0| >= 2^-3, i.e. weights less than 2^14 below their channel's maximum; fp16-rounded below), w pre-scaled per output channel
 *                     x*w ~ h0*g0 + h0*g1 + h1*g2   (dropped: 2^-11*h1*g1 and the two residual roundings, <= 3*2^-22 relative)
 *                   full precision for 2^-14 <= |x| <= 65504 (below: absolute error <= 2^-36; above: fp16 overflow, reported
 *                   through `status`); weights within 2^-15 of their channel's largest keep 22 bits. */
enum { VPS_PREC_F32 = 0, VPS_PREC_BF16 = 1, VPS_PREC_BF16X3 = 2, VPS_PREC_BF16X6 = 3, VPS_PREC_F16X3 = 4 };

typedef struct vps_conv_desc {
    /* input activation, NHWC */
    const float* in;
    int32_t N, H, W;
    int32_t in_ld;      /* floats per pixel (multiple of 4) */
    int32_t in_coff;    /* first channel used (multiple of 4) */
    int32_t cin_pad;    /* channels contracted, multiple of 4; weights are zero for the pad */
    /* packed weights [nclass][cout_pad][kpad], k contiguous; kpad multiple of 32, cout_pad of tile_n */
    const float* w;
    int32_t cout, cout_pad, kpad;
    int32_t KH, KW, stride;
    int32_t pad_y[2], pad_x[2];
    /* output */
    float* out;
    int32_t Ho, Wo;     /* full output spatial size */
    int32_t out_ld, out_coff;
    int32_t Qh, Qw;     /* GEMM pixel grid per class (== Ho,Wo for a conv) */
    int32_t os_y, os_x; /* 1 for conv, s for a stride-s transposed conv */
    int32_t nclass;     /* os_y*os_x */
    /* epilogue */
    const float* scale; /* [cout] or NULL (=1) */
    const float* shift; /* [cout] or NULL (=0) */
    const float* res;   /* residual NHWC or NULL; read at (oy>>res_shift, ox>>res_shift) */
    int32_t res_ld, res_coff, res_shift;
    int32_t act;        /* VPS_ACT_* */
    float slope;        /* LeakyReLU negative slope */
    /* deformable sampling (NULL = plain conv): NHWC [N][Ho][Wo][off_ld], ch 2*(ky*KW+kx) = dh, +1 = dw */
    const float* offset;
    int32_t off_ld;
    /* tiling */
    int32_t tile_n;     /* 32, 64 or 128; 256 for a deformable layer (offset set) in VPS_PREC_F16X3 with korder 1 and 256 | cout_pad */
    int32_t ksplit;     /* >=1; >1 needs ws of ksplit*M*cout_pad floats (M = nclass*N*Qh*Qw) */
    float* ws;
    /* split modes: 16-bit weight planes, no `w`. P planes: bf16 1, bf16x3 2, bf16x6 3 (plane p = bf16 RNE of the residual after p
     * terms), f16x3 3 (g0, g1, 2^-11*g0 of the per-channel pre-scaled weight; the scale's inverse is folded into `scale`).
     *   with `offset` (deformable) AND korder 0:  [P][nclass][cout_pad][kpad] (two-barrier kernel, weights through LDS)
     *   otherwise - deformable layers in the chunk-major order included - MFMA-fragment order (weights go straight to registers, one coalesced 1 KB load per fragment):
     *                               [P][nclass][cout_pad/32][kpad/16][lane 0..63][8], lane = 32*((k/8)%2) + cout%32 */
    int32_t prec;       /* VPS_PREC_* */
    const void* w_split;
    /* k ordering of the packed weights: 0 = tap-major k = (ky*KW+kx)*cin_pad + ci;
     * 1 = chunk-major k = ((ci/32)*KH*KW + ky*KW+kx)*32 + ci%32, kpad = KH*KW*ceil(cin_pad/32)*32 (L2-friendly) */
    int32_t korder;
    /* VPS_PREC_F16X3: device word that gets bit 0 OR-ed in when an activation beyond the fp16 range (|x| > 65504) was staged
     * (the result of that launch is then not fp32-grade); NULL = not reported. Never written in the other modes. */
    int32_t* status;
    /* GroupNorm sums of the OUTPUT taken by the epilogue (the deformable conv + GroupNorm towers, upsnetFPN.py:39-52): when non-NULL,
     * the sum and the sum of squares of the stored values of every group of gn_cpg consecutive output channels (4, or a multiple
     * of 8) are ADDED to gn_stats[r][2 g], gn_stats[r][2 g + 1] (doubles; the caller zeroes all gn_rep copies; a block adds to
     * copy r = block index % gn_rep, gn_rep a power of two, so that the atomics of ~1000 blocks spread over gn_rep * 4 cache lines)
     * - the statistics pass of vps_groupnorm_relu without re-reading the tensor; finish with vps_groupnorm_apply, which adds the
     * copies up. Deformable launches (offset != NULL) of the split-operand modes only, ksplit == 1, no residual, N == 1 (the sums
     * have no image dimension: GroupNorm normalises per image), cout/out_ld/out_coff multiples of 4; VPS_EARG otherwise. */
    double* gn_stats;
    int32_t gn_cpg, gn_rep;
    /* ksplit > 1: int32 [nclass * tiles] tickets, ZERO on entry (the launch leaves them zero). Non-NULL: the block that finishes a
     * tile's last split sums the partials (in split order) and applies the epilogue itself; NULL: a separate reduce launch does.
     * tiles = ceil(M/128) * cout_pad/tile_n for the pipelined kernels; the halo kernels tile in 8x16 / 8x32 patches:
     * N * ceil(Qh/8) * ceil(Qw/16) * cout_pad/tile_n is an upper bound for all of them. */
    int32_t* tile_counter;
    /* VPS_PREC_F16X3, optional: the weights of a thin-input layer (cin_pad 4 / 8 / 12, cout_pad 64, KH == KW, korder 0) in the packing
     * of the thin-input kernel (csrc/conv_thin.hip): fp16 [KH][plane 0..1][ceil(KW*cin_pad/16)][cout/32][lane = 32*(k/8 % 2) + cout % 32][8],
     * k = position within one kernel ROW's KW*cin_pad values (tap-major, zero-padded to a multiple of 16), same per-channel scaling
     * as w_split. NULL, or a shape the kernel has no instance for: the launch uses w_split. */
    const void* w_thin;
} vps_conv_desc;

int vps_conv2d(const vps_conv_desc* d, void* stream);

/* ----------------------------------------------------------------------------------------------
 * FlowNet2 gather / scan ops (HBM bound)
 * All take explicit element strides (sn, sc, sh, sw) so the same kernel serves the reference's NCHW
 * operator API and the NHWC pipeline.
 * -------------------------------------------------------------------------------------------- */
typedef struct vps_tensor4 {
    float* p;
    int64_t sn, sc, sh, sw; /* element strides */
} vps_tensor4;

/* ref: resample2d_package/resample2d.py:40-49, resample2d_kernel.cu:15-72 (kernel_size=1, bilinear,
 * border clamp of the four tap indices). out[b,c,y,x] = bilinear(in[b,c], x+flow[b,0,y,x], y+flow[b,1,y,x]) */
int vps_resample2d(vps_tensor4 in, vps_tensor4 flow, vps_tensor4 out,
                   int B, int C, int H, int W, void* stream);

/* ref: channelnorm_package/channelnorm.py:31-38, channelnorm_kernel.cu:18-60. out[b,0,y,x] = sqrt(sum_c in^2) */
int vps_channelnorm(vps_tensor4 in, vps_tensor4 out, int B, int C, int H, int W, void* stream);

/* ref: correlation_package/correlation.py:47-61, correlation_cuda.cc:10-87,
 * correlation_cuda_kernel.cu:46-147 (kernel_size=1, stride1=1). Inputs NHWC (ld/coff), output channel
 * tc = (tj+r)*(2r+1)+(ti+r), r = max_disp/stride2, written to out[.., out_coff+tc] with optional LeakyReLU.
 * out = (1/C) * sum_c in1[y,x,c] * in2[y+tj*s2, x+ti*s2, c], zero outside. */
int vps_correlation(const float* in1, int ld1, int coff1, const float* in2, int ld2, int coff2,
                    float* out, int out_ld, int out_coff,
                    int N, int H, int W, int C, int max_disp, int stride2,
                    int act, float slope, void* stream);
/* the same operator in SPLIT fp16 on the matrix cores (round 5; the two configurations of the path with C = 256: max_disp 20 / stride2 2
 * and max_disp 4 / stride2 1; every other shape runs the exact kernels): operands as fp16 pairs with a scaled residual (22 significand
 * bits), a*b ~ h0 k0 + 2^-11 (h0 k1 + h1 k0), fp32 accumulate - fp32-grade like VPS_PREC_F16X3 for 2^-14 <= |x| <= 65504. status: device
 * word that receives bit 0 when an operand lies beyond the fp16 range: the caller then repeats the call with vps_correlation. */
int vps_correlation_f16(const float* in1, int ld1, int coff1, const float* in2, int ld2, int coff2,
                        float* out, int out_ld, int out_coff, int N, int H, int W, int C,
                        int max_disp, int stride2, int act, float slope, int32_t* status, void* stream);

/* ref: flow_modules/flow_modules.py:126-148 (WarpingLayer): grid = linspace(-1,1) + flow/((W-1)/2),
 * F.grid_sample(bilinear, zeros padding, align_corners=False). NHWC in/out, flow NHWC [N,H,W,flow_ld] (ch0=x,1=y) */
int vps_flow_warp(const float* in, int in_ld, int in_coff, const float* flow, int flow_ld, int flow_coff,
                  float* out, int out_ld, int out_coff, int N, int H, int W, int C, void* stream);

/* layout transposes: NCHW (contiguous) <-> NHWC (ld/coff); pad channels [C, Cpad) are written as zero */
int vps_nchw_to_nhwc(const float* in, float* out, int out_ld, int out_coff, int N, int C, int H, int W,
                     int Cpad, void* stream);
int vps_nhwc_to_nchw(const float* in, int in_ld, int in_coff, float* out, int N, int C, int H, int W, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Resize / pool / elementwise (NHWC)
 * -------------------------------------------------------------------------------------------- */
/* F.interpolate(mode=bilinear, align_corners=False) (mode 0) or nearest (mode 1); out = alpha * resized.
 * ref: flownet2.py:143,155 (upsample1/2 bilinear x4), :167,180 (nearest x4), panoptic_fusetrack.py:140-142,
 * upsnetFPN.py:73-80, tcea_modules.py:72 */
int vps_resize(const float* in, int in_ld, int in_coff, int Hi, int Wi,
               float* out, int out_ld, int out_coff, int Ho, int Wo,
               int N, int C, int mode, float alpha, void* stream);
/* 3x3 stride-2 pad-1 max (mode 0, -inf pad; ref resnet.py:465, tcea_modules.py:27) or avg pool
 * (mode 1, count_include_pad=True; ref tcea_modules.py:28) */
int vps_pool3x3s2(const float* in, int in_ld, int in_coff, int Hi, int Wi,
                  float* out, int out_ld, int out_coff, int N, int C, int mode, void* stream);
/* BFP gather: out = (sum_l nearest_resize(level_l)) / L at level-0 resolution; ratio[l] = H0 / H_l.
 * ref: extra_necks/bfp_tcea.py:96-109 (refine_level = 0) */
int vps_bfp_gather(const float* const* levels, const int* ld, const int* ratio, int nlevels,
                   float* out, int out_ld, int out_coff, int N, int H0, int W0, int C, void* stream);
/* BFP scatter: out = adaptive_max_pool2d(bsf, (H0/ratio, W0/ratio)) + level. ref: bfp_tcea.py:139-147 */
int vps_bfp_scatter(const float* bsf, int bsf_ld, const float* level, int lvl_ld, float* out, int out_ld,
                    int N, int H0, int W0, int C, int ratio, void* stream);
/* the same for ALL levels in one pass over bsf (round 6): level l = adaptive_max_pool2d(bsf, (H0 >> l, W0 >> l)) + levels[l], l < nlevels
 * (2..5; ratio 2^l), H0 and W0 multiples of 2^(nlevels-1), C a multiple of 32. Bitwise vps_bfp_scatter per level; bsf is read once. */
int vps_bfp_scatter_all(const float* bsf, int bsf_ld, const float* const* levels, const int* lvl_ld, float* const* outs,
                        const int* out_ld, int nlevels, int N, int H0, int W0, int C, void* stream);
/* y = x*a + b elementwise over a slice (used for flow scaling) */
int vps_axpb(const float* in, int in_ld, int in_coff, float* out, int out_ld, int out_coff,
             int64_t npix, int C, float a, float b, void* stream);

/* FlowNet2 input prep. ref: utils/flow_utils.py:5-10 (denormalize), flownet2.py:135-139 (rgb_mean over both
 * frames, (x-mean)/rgb_max, cat). img/ref NCHW [1,3,H,W] normalised; out NHWC [H*W][out_ld] ch0-2 img, 3-5 ref.
 * `partial` is a caller workspace of 3*nblk doubles, `mean3` 3 floats. */
int vps_flow_prep(const float* img, const float* ref, const float* mean3, const float* std3,
                  float* out, int out_ld, int H, int W, double* partial, int nblk, float* rgb_mean_out,
                  void* stream);
/* the same with the pair zero-padded (in 0..255 RGB space, bottom / right) to [Hp][Wp] before the mean is taken and x6 is
 * written — ref: panoptic_fusetrack.py:125-128 (800x1600 -> 832x1664, 200x400 -> 256x448; FlowNet2 needs multiples of 64). */
int vps_flow_prep_pad(const float* img, const float* ref, const float* mean3, const float* std3,
                      float* out, int out_ld, int H, int W, int Hp, int Wp, double* partial, int nblk, float* rgb_mean_out,
                      void* stream);
/* FlowNet2 inter-stage tensor build (ref flownet2.py:142-151,154-163,166-174,179-187): given a 1/4-res
 * 2-channel flow (NHWC, ld/coff) compute flow_full = up4(div_mode ? flow/mul : flow*mul) (up_mode 0
 * bilinear / 1 nearest), warped = resample2d(x[3:6], flow_full), diff = x[0:3]-warped, and write any of:
 *   x[0:3] -> out[img_off..+3], flow_full (/flow_out_div if >0) -> out[flow_off..+2],
 *   warped -> out[warp_off..+3], ||diff||2 -> out[diffnorm_off], ||flow_full||2 -> out[flownorm_off]
 * (offset < 0 = skip). H, W multiples of 4. */
int vps_flow_stage(const float* x6, int x_ld, const float* flow_lo, int flo_ld, int flo_coff,
                   int H, int W, int up_mode, float mul, int div_mode,
                   float* out, int out_ld, int flow_off, float flow_out_div, int warp_off,
                   int diffnorm_off, int flownorm_off, int img_off, void* stream);

/* The same stage writing WHOLE 12-float pixels (three 16-byte stores; x6 with x_ld == 8, out with out_ld == 12, both 16-byte
 * aligned), same formulas as vps_flow_stage (+ vps_axpb for the image channels):
 *   mode 0, FlowNetS input (flownet2.py:142-163): out = [x6[0..5] | warp(img2, f) | f / mul | ||img1 - warp||], f = bilinear x4 of
 *           flow_a * mul (flow_b unused);
 *   mode 1, FlowNetFusion input (flownet2.py:166-187): out = [img1 | f_b | f_a | |f_b| | |f_a| | ||img1 - warp(img2, f_b)|| |
 *           ||img1 - warp(img2, f_a)|| | 0], f_a = nearest x4 of flow_a * mul (FlowNetS_2), f_b = nearest x4 of flow_b / mul (FlowNetSD). */
int vps_flow_stage_full(const float* x6, int x_ld, const float* flow_a, int a_ld, int a_coff,
                        const float* flow_b, int b_ld, int b_coff, int H, int W, int mode, float mul,
                        float* out, int out_ld, void* stream);

/* GroupNorm(G) + ReLU over NHWC (N=1): stats pass then apply pass. ref: upsnetFPN.py:39-52 (GroupNorm(32)).
 * in is a coff-0 buffer, the result goes to out[.., out_coff + c]. `stats` workspace: 2*G doubles (zeroed by the call). */
int vps_groupnorm_relu(const float* in, int in_ld, float* out, int out_ld, int out_coff, int64_t npix, int C, int G,
                       const float* gamma, const float* beta, float eps, int relu,
                       double* stats, void* stream);
/* The apply pass alone: `stats` already holds nrep copies [nrep][2*G] of partial sums (vps_conv_desc.gn_stats / gn_rep of the
 * conv that produced `in`); 2*G <= 512. */
int vps_groupnorm_apply(const float* in, int in_ld, float* out, int out_ld, int out_coff, int64_t npix, int C, int G,
                        const float* gamma, const float* beta, float eps, int relu,
                        const double* stats, int nrep, void* stream);

/* TCEA temporal attention, N=2 frames, center 0. ref: utils/tcea_modules.py:50-65.
 * emb [npix][>=2C] holds tAtt_1(frame0) in channels [0,C) and tAtt_1(frame1) in [C,2C); emb_ref = tAtt_2(frame0);
 * fea0/fea1 are the two aligned frames (pointers already offset to their first channel, 16B aligned).
 * out[npix][2C] = [fea0 * sigmoid(<emb0,emb_ref>) | fea1 * sigmoid(<emb1,emb_ref>)] (frame-major channels). */
int vps_tcea_temporal(const float* emb, int emb_ld, const float* emb_ref, int ref_ld,
                      const float* fea0, int f0_ld, const float* fea1, int f1_ld,
                      float* out, int out_ld, int64_t npix, int C, void* stream);
/* out = fea * sigmoid(att) * 2 + att_add. ref: tcea_modules.py:74-77 */
int vps_tcea_modulate(const float* fea, const float* att, const float* att_add, float* out,
                      int64_t n, void* stream);
/* the same on channel windows: pointers at the first channel of each window, leading dimensions in floats, C channels (4 | C, ld) */
int vps_tcea_modulate_ld(const float* fea, int fea_ld, const float* att, int att_ld, const float* att_add, int add_ld,
                         float* out, int out_ld, int64_t npix, int C, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Detection ops
 * -------------------------------------------------------------------------------------------- */
/* ref: mmdet/ops/roi_align/roi_align.py:59-87, src/roi_align_kernel.cu:16-124 + roi_extractors/
 * single_level.py:54-107 (level mapping lvl = floor(log2(sqrt(w*h)/56 + 1e-6)) clamped to [0,nlvl-1]).
 * feats: NHWC levels (ld each), spatial_scale 1/stride; rois [R][5] (b,x1,y1,x2,y2); out NHWC [R][P][P][C] */
int vps_roi_align(const float* const* feats, const int* ld, const int* Hs, const int* Ws, const float* scales,
                  int nlevels, float finest_scale, const float* rois, int R, int C, int P, int sample_num,
                  float* out, void* stream);

/* ref: mmdet/ops/nms/src/nms_kernel.cu:13-130 and utils/upsnet/nms/nms_kernel.cu:40-150.
 * Batched: boxes [nbatch][nmax][5] each sorted by descending score, counts_dev[nbatch] valid boxes (device),
 * IoU with the +1 convention, suppress if IoU > thr. mask_ws: nbatch*nmax*ceil(nmax/64) uint64.
 * keep [nbatch][nmax] int32 (indices into the sorted list, ascending), nkeep[nbatch] (device).
 * The greedy reduce (a host loop in the reference) runs on the device, one wavefront per batch entry. */
int vps_nms_batched(const float* boxes, int nbatch, int nmax, const int32_t* counts_dev, float thr,
                    uint64_t* mask_ws, int32_t* keep, int32_t* nkeep, void* stream);

/* ref: core/bbox/transforms.py:34-68 (delta2bbox, means 0, stds given, clamp to img, wh_ratio_clip 16/1000).
 * anchors [n][4], deltas [n][4] -> boxes5 [n][5] (x1,y1,x2,y2,score) */
int vps_delta2bbox(const float* anchors, const float* deltas, const float* scores, float* boxes5, int n,
                   float std_x, float std_y, float std_w, float std_h, float img_h, float img_w, void* stream);

/* ref: core/bbox/geometry.py:4-63 (bbox_overlaps, +1 convention). a [m][4/5] lda, b [n][ldb] -> out [m][n] */
int vps_bbox_overlaps(const float* a, int lda, int m, const float* b, int ldb, int n, float* out, void* stream);

/* row softmax / log-softmax for small matrices: in [rows][cols] -> out. mode 0 softmax, 1 log_softmax */
int vps_row_softmax(const float* in, float* out, int rows, int cols, int mode, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Panoptic head
 * -------------------------------------------------------------------------------------------- */
/* ref: utils/mask_removal.py:29-92, body of the per-box loop (boxes visited in descending cls_prob order by
 * the host): resize the SxS (28x28) mask logits to the int32-truncated box (cv2.resize INTER_LINEAR on float32),
 * binarise > 0, compare with the class occupancy plane (uint8 [H][W]).
 *   vps_mask_count : counts[0] = #mask pixels in the clipped box, counts[1] = #mask pixels already occupied
 *   vps_mask_commit: keep = counts[0] != 0 && !(counts[1]/counts[0] > thr) decided ON THE DEVICE;
 *                    *flag = keep; kept masks are added to the occupancy plane. No host sync between boxes. */
int vps_mask_count(const float* logit, int S, int bx1, int by1, int bx2, int by2, int H, int W,
                   const uint8_t* occ, int32_t* counts, void* stream);
int vps_mask_commit(const float* logit, int S, int bx1, int by1, int bx2, int by2, int H, int W,
                    uint8_t* occ, const int32_t* counts, double thr, int32_t* flag, void* stream);

/* the whole MaskRemoval box loop in ONE launch (one workgroup per class walks the score-sorted boxes; masks of different
 * classes never interact). boxes [n][4] int32-truncated (x1,y1,x2,y2), cls0[n] 0-based class, mask_idx[n] row of logits,
 * all in descending-score order and on the device; occ: ncls*H*W uint8 workspace (zeroed by the call); flags[n] = kept. */
int vps_mask_removal(const float* logits, int S, const int32_t* boxes, const int32_t* cls0, const int32_t* mask_idx,
                     int n, int ncls, int H, int W, uint8_t* occ, double thr, int32_t* flags, void* stream);

/* the same loop in ONE launch with one workgroup PER BOX of the score-sorted walk (round 5): a box finds the earlier same-class boxes
 * whose rectangles intersect its own, waits (bounded) until each has published its decision, then counts, decides (flags[i]) and
 * commits - independent boxes run side by side, dependent ones back to back without a launch in between. Arguments as above
 * (n <= 256, 2 <= S <= 32, W % 4 == 0, occ 4-byte aligned; occ and `done` [n] are zeroed by the call). status: bit 2 (value 4) is OR-ed in
 * when a wait expired (boxes wait for lower workgroup indices only, but HIP promises neither dispatch order nor progress): the flags of
 * that call are not valid - the caller repeats the walk with vps_mask_level (vps_amd/detector.py does, counted in
 * panoptic_ops.MR_RECOVERIES). VPS_MR_SPIN_LIMIT in the environment overrides the number of polls per dependency (tests). */
int vps_mask_removal_dep(const float* logits, int S, const int32_t* boxes, const int32_t* cls0, const int32_t* mask_idx,
                         int n, int ncls, int H, int W, uint8_t* occ, double thr, int32_t* flags, int32_t* done,
                         int32_t* status, void* stream);

/* the same decisions WITHOUT a dependency chain (round 6, the detector's default): rank[n] = position of box i among the boxes of its
 * class in the score-sorted walk, max_rank = its largest value (<= 126: at most 127 boxes per class; ncls <= 32, n <= 256). One pass over
 * the frame gives every pixel its per-class pattern of covering boxes (per-box pixel counts by wavefront ballots, patterns with >= 2
 * bits counted in a per-class hash table), then one wavefront per class walks its boxes over the distinct patterns: overlap_i = sum of
 * count(P) over the patterns P with bit i and a kept earlier bit (mask_removal.py:75-88). A class with more than 64 boxes takes a second
 * pass for its ranks 64..126 (key = their pattern + "covered by a kept box of ranks 0..63"). scratch: 8-byte aligned,
 * (n rounded up to 2) int32 + (ncls + groups * ncls * 4096) 64-bit words with groups = 1 + (max_rank >= 64), zeroed by the call.
 * status: bit 2 (value 4) is OR-ed in when a hash table (2048 distinct overlap patterns per class and group) is full: the flags of that
 * call are not valid - the caller repeats the walk with vps_mask_level, as for vps_mask_removal_dep. No occupancy plane, no
 * cross-workgroup wait. */
int vps_mask_removal_hist(const float* logits, int S, const int32_t* boxes, const int32_t* cls0, const int32_t* mask_idx,
                          const int32_t* rank, int max_rank, int n, int ncls, int H, int W, int32_t* scratch, size_t scratch_bytes,
                          double thr, int32_t* flags, int32_t* status, void* stream);

/* one dependency LEVEL of the MaskRemoval loop (count launch + commit launch): `level` = nlevel indices (device) into the
 * score-sorted box arrays whose boxes are mutually independent (no earlier same-class box of the same level intersects
 * them); counts [n][2] and occ must have been zeroed by the caller before the first level; max_area = largest clipped
 * box area of the level (grid sizing). Keep decision on the device, flags[i] written. */
int vps_mask_level(const float* logits, int S, const int32_t* boxes, const int32_t* cls0, const int32_t* mask_idx,
                   const int32_t* level, int nlevel, int max_area, int H, int W, uint8_t* occ, int32_t* counts,
                   double thr, int32_t* flags, void* stream);

/* one kept instance of the panoptic combine */
typedef struct vps_pan_inst {
    int32_t sx0, sy0, sx1, sy1;     /* SegTerm crop [x0,x1) x [y0,y1): int(b), int(round(b)+1) (unary_logits.py:102-105) */
    int32_t seg_ch;                 /* class_mapping[cls] channel of fcn_output */
    int32_t bx1, by1, bx2, by2;     /* MaskRemoval int32-truncated box (mask_removal.py:56-62) */
    int32_t mask_idx;               /* row of mask_logits [*][S][S] */
} vps_pan_inst;

/* ref: upsnetFPN.py:81 (bilinear x4 of fcn_score), utils/unary_logits.py:81-108 (SegTerm),
 * mask_removal.py:88 (paste), panoptic_fusetrack.py:588-597 (cat, softmax, argmax; argmax of fcn_output).
 * fcn_score NHWC [Hs][Ws][score_ld]; fcn_output (x H/Hs bilinear) is recomputed per pixel, never stored.
 * pan/sem: uint8 [H][W] (ids 0..nstuff-1 stuff, nstuff+j = j-th instance; k <= 255-nstuff). */
int vps_panoptic_combine(const float* fcn_score, int score_ld, int Hs, int Ws, int nclass, int nstuff,
                         const vps_pan_inst* inst, int k, const float* mask_logits, int S,
                         uint8_t* pan, uint8_t* sem, int H, int W, void* stream);

/* same, with the instance count read from DEVICE memory (k_dev[0] <= kmax; k_dev[0] > 255 - nstuff raises status bit 0 of
 * k_dev[2] and writes nothing): the table comes from vps_pan_instances, the host never sees the kept list before the launch */
int vps_panoptic_combine_dev(const float* fcn_score, int score_ld, int Hs, int Ws, int nclass, int nstuff,
                             const vps_pan_inst* inst, const int32_t* k_dev, const float* mask_logits, int S,
                             uint8_t* pan, uint8_t* sem, int H, int W, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Device-resident detection post-processing (csrc/head_ops.hip): the order-defining HOST code of the reference's heads as
 * single-workgroup kernels, so that a frame needs ONE mid-frame D2H (the detection list) and one at its end (kept list + ids).
 * -------------------------------------------------------------------------------------------- */
/* HOST functions (no device work, no stream): PNG decode for the input pipeline - `mmcv.imread` in datasets/pipelines/loading.py:43-68
 * (cv2.imread(IMREAD_COLOR): BGR uint8). Called through the C-ABI they run without the Python interpreter lock, so a pool of plain
 * threads scales. `file` = the file's bytes. vps_png_info: size / channel count of an 8-bit non-interlaced RGB, RGBA or grey PNG;
 * any other PNG flavour (16-bit, palette, interlaced) returns an argument error and the caller uses its general decoder.
 * vps_png_decode_bgr8: out [H][W][3] BGR (alpha dropped, grey replicated), out_capacity >= H*W*3 bytes. */
int vps_png_info(const uint8_t* file, int64_t nbytes, int32_t* H, int32_t* W, int32_t* channels);
int vps_png_decode_bgr8(const uint8_t* file, int64_t nbytes, uint8_t* out, int64_t out_capacity);

/* PNG input with the un-filter on the DEVICE (opt-in: `ClipFeeder(png='device')`; csrc/png_in_ops.hip). The zlib stream is inflated on the
 * HOST (one function, no device work, no stream, no interpreter lock, no allocation); the five scanline filters and the RGB -> BGR copy
 * run on the device and give vps_png_decode_bgr8's bytes.
 * vps_png_inflate: takes the files vps_png_decode_bgr8 takes, makes its checks and returns its error codes; scan receives the FILTERED
 * scanlines as zlib delivers them, H rows of 1 + W*channels bytes, tightly packed, each led by its filter byte; scan_capacity in bytes
 * >= H * (1 + W*channels). The stream is inflated straight into scan (a pinned staging slot). Every filter byte is checked to be 0..4
 * here - the device never sees another value.
 * vps_png_reconstruct_ws (HOST arithmetic only): the workspace bytes of vps_png_reconstruct.
 * vps_png_reconstruct: every pointer is a DEVICE pointer (scan and out_bgr at any byte address, ws 4-byte aligned); launches on
 * `stream`, no sync, no hidden allocation. scan is READ in aligned 4-byte words: where scan or scan + H*(1 + W*channels) is not a
 * multiple of 4, up to 3 bytes in front of the first row and behind the last row are loaded (and ignored) - they share an aligned word
 * with a byte of the buffer, so the read cannot leave its page, but it is outside the caller's H*(1 + W*channels) bytes. scan as vps_png_inflate wrote it, H / W / channels (1, 3 or 4) as vps_png_info reported
 * them; out_bgr = uint8 [H][W][3] BGR (alpha dropped, grey replicated), out_capacity >= H*W*3 bytes. A row of type None or Sub
 * (and row 0) starts a group of rows that reads nothing above it; one workgroup rebuilds one group as a skewed wavefront, in bands of
 * vps_png_reconstruct_block_rows() rows (a constant of the build; HOST, no device work), and no workgroup waits for another. */
int vps_png_inflate(const uint8_t* file, int64_t nbytes, uint8_t* scan, int64_t scan_capacity);
int vps_png_reconstruct_ws(int H, int W, int channels, int64_t* ws_bytes);
int vps_png_reconstruct(const uint8_t* scan, int H, int W, int channels, uint8_t* out_bgr, int64_t out_capacity,
                        void* ws, int64_t ws_bytes, void* stream);
int vps_png_reconstruct_block_rows(void);

/* KITTI flow files (csrc/png_host.cpp, csrc/png_in_ops.hip, csrc/kitti_flow_ops.hip; vps_amd/kittiflow.py): optical
 * flow as a 16-bit RGB PNG. The coding is restated from memory of the KITTI devkit's io_flow.h; tests/kitti_flow_restate.py pins it.
 *   file    non-interlaced PNG, colour type 2, bit depth 16; samples big-endian in the order R, G, B: 6 bytes per pixel
 *   read    a pixel is valid iff B > 0 (the 16-bit value); then u = (R - 32768) / 64, v = (G - 32768) / 64, exact in fp32; an invalid
 *           pixel reads as u = v = 0
 *   write   R = (uint16) max(min(u * 64.0f + 32768.0f, 65535.0f), 0.0f) in fp32, the cast truncating behind the clamp; G likewise from
 *           v; B = 1 where valid, 0 otherwise. This library's own rule: a pixel whose u or v is NaN or +-inf is written R = G = B = 0
 * vps_png16_info, vps_png16_inflate (HOST, no device work, no stream, no interpreter lock, no allocation): vps_png_info / vps_png_inflate
 * for exactly this flavour - depth 16, colour type 2, not interlaced; every other file is refused with their codes (-1001 signature,
 * IHDR or its CRC, -1002 size, -1003 flavour, -1004 scan NULL or scan_capacity too small, -1007 stream incomplete or a chunk cut,
 * -1008 a filter byte above 4, -1009 more than 1 GiB of scanlines), and the IEND chunk must be there (-1007). channels = 3. scan
 * receives H rows of 1 + 6 W bytes; nothing is written behind scan_capacity. vps_png_info keeps refusing these files.
 * vps_kitti_flow_reconstruct_ws (HOST arithmetic only): the workspace bytes of vps_kitti_flow_reconstruct.
 * vps_kitti_flow_reconstruct: every pointer is a DEVICE pointer; two launches on `stream`, no sync, no allocation. Un-filters the scan
 * at 6 bytes per pixel with vps_png_reconstruct's wavefront (one lane per row, groups cut by None / Sub rows, bands of
 * vps_png_reconstruct_block_rows() rows) and decodes in the same launch.
 *   scan        as vps_png16_inflate wrote it, at any byte address; read as aligned dwords (up to 3 bytes in front of and behind it
 *               are loaded and ignored, as vps_png_reconstruct)
 *   noc_valid   NULL, or uint8 [H][W], any byte alignment: non-zero = the pixel is valid in the pair's flow_noc file
 *   flow        fp32 [H][W][2] dense, 16-byte aligned; flow_capacity in BYTES >= 8 H W
 *   mask        uint8 [H][W], any byte alignment, in vps_flow_error's codes. noc_valid NULL: 1 valid, 0 invalid. noc_valid given: 1 valid
 *               here and in noc, 2 valid here but not in noc (occluded), 0 invalid here
 *   ws          4-byte aligned, at least vps_kitti_flow_reconstruct_ws bytes: the group table and, for every band that another follows,
 *               its last rebuilt raw row (the decoded flow no longer holds B, so the next band cannot read it back from the output)
 * Errors before any launch: -1001 a null pointer or H, W outside 1..65535, -1003 ws or flow misaligned, -1004 flow_capacity,
 * -1006 ws_bytes.
 * vps_kitti_flow_encode: flow = DEVICE fp32 NHWC map in any layout vps_flow_colour takes (pixel p at flow[p * ld + coff] (u) and
 * [.. + 1] (v), coff + 2 <= ld, 4-byte aligned); valid = NULL (every pixel valid) or DEVICE uint8 [H][W]; img16 = DEVICE uint8
 * [H][6 W], dense, 4-byte aligned: the big-endian RGB16 image by the write rule. One launch on `stream`, no sync, no allocation. Errors
 * before the launch: -1001 flow or img16 NULL, -1002 H, W outside 1..65535, -1003 ld / coff, -1004 alignment. */
int vps_png16_info(const uint8_t* file, int64_t nbytes, int32_t* H, int32_t* W, int32_t* channels);
int vps_png16_inflate(const uint8_t* file, int64_t nbytes, uint8_t* scan, int64_t scan_capacity);
int vps_kitti_flow_reconstruct_ws(int H, int W, int64_t* ws_bytes);
int vps_kitti_flow_reconstruct(const uint8_t* scan, int H, int W, const uint8_t* noc_valid, float* flow, int64_t flow_capacity,
                               uint8_t* mask, void* ws, int64_t ws_bytes, void* stream);
int vps_kitti_flow_encode(const float* flow, int ld, int coff, const uint8_t* valid, int H, int W, uint8_t* img16, void* stream);

/* JPEG input (the VIPER frames). The Huffman bit stream is decoded on the HOST (two functions, no device work, no stream, no
 * interpreter lock, no allocation); dequantisation, the 8x8 inverse DCT, chroma upsampling and YCbCr -> BGR run on the DEVICE and are
 * bit-exact with libjpeg's default decode (slow-integer IDCT, fancy upsampling, 16-bit fixed-point colour) - what cv2.imread and PIL
 * compute.
 * vps_jpeg_info: geometry of an 8-bit Huffman-coded sequential JPEG (SOF0 / SOF1, one interleaved scan) with 1 component or 3 YCbCr
 * components sampled 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2). samp [3][2] = (h, v) sampling factors, grid [3][2] = (block rows, block
 * columns) of each component padded to whole MCUs, qt [3][64] = each component's quantisation table in natural (row-major) order,
 * coef_bytes = what vps_jpeg_decode_coef writes; a grey file repeats its component in entries 1 and 2. Every output pointer may be
 * NULL. Progressive / lossless / arithmetic / 12-bit files, other component counts or colour spaces (Adobe APP14), other sampling,
 * an EXIF orientation other than 1 (cv2.imread rotates such files, PIL does not) and a scan that does not end in EOI return an
 * argument error: the caller uses its general decoder.
 * vps_jpeg_decode_coef: quantised coefficients, int16 [component][block row][block column][64] in natural order, DC prediction
 * undone, NOT dequantised; capacity in bytes >= coef_bytes. A damaged bit stream returns an argument error.
 * vps_jpeg_reconstruct (device; launches on `stream`, no sync, no hidden allocation): coef and qt are DEVICE pointers (16-byte
 * aligned), H / W / ncomp / samp / grid (host arrays) as vps_jpeg_info reported them, ws = device workspace for the sample planes,
 * ws_bytes >= coef_bytes / 2; out = uint8 [H][W][3] BGR cropped to the true size (a grey file replicated, like IMREAD_COLOR). */
int vps_jpeg_info(const uint8_t* file, int64_t nbytes, int32_t* H, int32_t* W, int32_t* ncomp, int32_t* samp, int32_t* grid,
                  uint16_t* qt, int64_t* coef_bytes);
int vps_jpeg_decode_coef(const uint8_t* file, int64_t nbytes, int16_t* coef, int64_t capacity);
int vps_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, int H, int W, int ncomp, const int32_t* samp, const int32_t* grid,
                         uint8_t* ws, int64_t ws_bytes, uint8_t* out, void* stream);

/* JPEG output (overlay images; csrc/jpeg_enc_ops.hip + csrc/jpeg_enc_host.cpp): the input path above in the other direction.
 * Blending, RGB -> YCbCr, chroma down-sampling, the 8x8 forward DCT and quantisation run on the DEVICE and are bit-exact with
 * libjpeg's default compressor (16-bit fixed-point colour, h2v2 box filter with the bias alternating 1, 2, slow-integer DCT, rounded
 * division); the Huffman coding and the container are written on the HOST (no device work, no stream, no interpreter lock, no
 * allocation, thread-safe). `subsampling` is 0 (4:4:4) or 2 (4:2:0), three components always; anything else is an argument error.
 * Both directions share one description of a file: the coefficient layout and the block grids are those of vps_jpeg_decode_coef /
 * vps_jpeg_info.
 * vps_overlay_render (device; launches on `stream`, no sync, no hidden allocation): frame_bgr uint8 [H][W][3] BGR, colour_rgb uint8
 * [H][W][3] RGB (the painted panoptic map; 0, 0, 0 = void), alpha 0..256 -> out_rgb uint8 [H][W][3] RGB, all dense DEVICE arrays.
 * A pixel whose right or lower neighbour has another colour triple is white (the last column has no right, the last row no lower
 * neighbour); otherwise a void pixel keeps the frame and every other one is (frame * (256 - alpha) + colour * alpha + 128) >> 8.
 * vps_jpeg_quant_tables (HOST): qt uint16 [2][64] (luma, chroma; natural order) = the Annex K tables scaled by libjpeg's quality
 * rule (quality 1..100), entries limited to 1..255 (baseline).
 * vps_jpeg_encode_bound (HOST arithmetic only): grid [3][2] = (block rows, block columns) per component padded to whole MCUs and
 * coef_bytes, the size of the coefficient array - the only buffer vps_jpeg_encode_coef needs. Either output may be NULL.
 * vps_jpeg_encode_coef (device; launches on `stream`, no sync, no hidden allocation, no workspace): rgb uint8 [H][W][3] with
 * row_stride >= 3 * W bytes between rows, qt as vps_jpeg_quant_tables wrote it but in DEVICE memory, coef (DEVICE, 16-byte aligned,
 * coef_capacity >= coef_bytes) = int16 [component][block row][block column][64] in natural order, every block written: pixels are
 * replicated to a whole block / iMCU row, the blocks that only fill the last MCU are zero but for the DC of the block before them.
 * vps_jpeg_write_bound (HOST arithmetic only): capacity that holds the file of ANY coefficients of that size.
 * vps_jpeg_write (HOST): coef (host memory) + qt [2][64] -> a baseline JFIF file in out: SOI, APP0, two DQT, SOF0, the four Annex K
 * DHT, SOS, one interleaved scan, EOI; nbytes[0] = its size. A capacity that does not hold it (a smaller one than the bound is fine
 * when the file fits) or a coefficient outside the range of 8-bit baseline data returns an argument error; no byte beyond
 * out + capacity is ever stored. */
int vps_overlay_render(const uint8_t* frame_bgr, const uint8_t* colour_rgb, int H, int W, int alpha, uint8_t* out_rgb, void* stream);
int vps_jpeg_quant_tables(int quality, uint16_t* qt);
int vps_jpeg_encode_bound(int H, int W, int subsampling, int32_t* grid, int64_t* coef_bytes);
int vps_jpeg_encode_coef(const uint8_t* rgb, int H, int W, int64_t row_stride, int subsampling, const uint16_t* qt, int16_t* coef,
                         int64_t coef_capacity, void* stream);
int vps_jpeg_write_bound(int H, int W, int subsampling, int64_t* capacity);
int vps_jpeg_write(const int16_t* coef, int H, int W, int subsampling, const uint16_t* qt, uint8_t* out, int64_t capacity,
                   int64_t* nbytes);

/* JPEG output with the entropy coding on the DEVICE (opt-in: `entropy='device'`; csrc/jpeg_scan_ops.hip). The coefficients stay where
 * vps_jpeg_encode_coef wrote them; the device writes the entropy-coded segment - the bytes vps_jpeg_write puts between the SOS header
 * and EOI for the same coefficients, byte for byte - and the host copies that (about the size of the file) and puts the container
 * round it.
 * vps_jpeg_scan_bound (HOST arithmetic only): ws_bytes = the workspace of vps_jpeg_encode_scan, scan_bytes = the longest scan of that
 * size = vps_jpeg_write_bound less the header and EOI. Either output may be NULL. Bit offsets on the device are 32-bit: a size whose
 * worst-case scan has 2^32 bits or more (about 1.29 million blocks: 27 Mpixel at 4:4:4, 55 Mpixel at 4:2:0) returns an argument error
 * here and in vps_jpeg_encode_scan.
 * vps_jpeg_encode_scan (device; 5 launches on `stream`, no sync, no hidden allocation): coef = DEVICE int16 array of
 * vps_jpeg_encode_coef, out = DEVICE buffer of `capacity` bytes (any capacity >= 0; may be NULL at 0), result = DEVICE int64 [2]
 * (8-byte aligned), ws = DEVICE workspace (16-byte aligned, ws_bytes >= the bound; needs no initialisation). result[1] is the status:
 *   0  out[0 : result[0]) is the scan
 *   1  the scan has result[0] bytes and capacity is smaller: out holds its first `capacity` bytes; call again with result[0]
 *   2  a DC difference of category > 11 or an AC coefficient of category > 10 (what vps_jpeg_write refuses): result[0] = 0, out untouched
 * Nothing is stored at or beyond out + capacity or outside ws, whatever the coefficients are. The same input gives the same bytes on
 * every call.
 * vps_jpeg_wrap (HOST): header (SOI .. SOS, as vps_jpeg_write writes it) + scan[0 : scan_bytes) + EOI -> out, nbytes[0] = its size.
 * The scan is copied, not parsed. A capacity below header + scan_bytes + 2, or a scan longer than vps_jpeg_scan_bound allows, is an
 * argument error and nothing is stored. */
int vps_jpeg_scan_bound(int H, int W, int subsampling, int64_t* ws_bytes, int64_t* scan_bytes);
int vps_jpeg_encode_scan(const int16_t* coef, int H, int W, int subsampling, uint8_t* out, int64_t capacity, int64_t* result, void* ws,
                         int64_t ws_bytes, void* stream);
int vps_jpeg_wrap(const uint8_t* scan, int64_t scan_bytes, int H, int W, int subsampling, const uint16_t* qt, uint8_t* out,
                  int64_t capacity, int64_t* nbytes);

/* Y4M video in and out (vps_amd/y4m.py; csrc/y4m_host.cpp + csrc/yuv_ops.hip): the uncompressed YUV4MPEG2 container, 8-bit planar
 * frames. The host only parses the two kinds of header line; chroma resampling and the colour matrix run on the device.
 * A stream is `YUV4MPEG2 W.. H.. [F..:..] [I.] [A..:..] [C..] [X..]\n` followed by frames of `FRAME[ params]\n` + Y, Cb, Cr planes.
 * vps_y4m_info (HOST; untrusted bytes: never reads past nbytes, allocates nothing): parses the stream header. W and H are required,
 * positive and W*H < 2^31; F and A are reported (0:0 when absent); I may be p or ? (t, b, m refused); C is 420jpeg, 420mpeg2, 420
 * (= 420jpeg, also when absent), 422, 444 or mono; XCOLORRANGE=FULL|LIMITED is honoured (absent: limited), other X tags are ignored.
 * The line is at most 256 bytes with its newline. Refusals, each -1000-x: 1 null / negative argument, 2 not the magic, 3 no newline
 * within nbytes / 256 bytes, 4 malformed number or ratio, 5 W or H missing, 6 size not positive, 7 size too large, 8 interlaced,
 * 9 420paldv, 10 more than 8 bits per sample, 11 444alpha, 12 unknown C, 13 unknown XCOLORRANGE, 14 unknown I.
 * vps_y4m_frame_header (HOST): buf starts a frame: `FRAME`, then a newline or a blank and parameters (skipped) up to the newline,
 * at most 80 bytes in all; len[0] = bytes of the line. 20 = not a FRAME line, 21 = no newline within nbytes / 80 bytes.
 * vps_y4m_write_header (HOST): the header line of `info` (W, H, F unless 0:0, Ip when interlace is 1, A, C, XCOLORRANGE), which
 * vps_y4m_info parses back to the same struct; len[0] = its bytes. 30 = a field out of range, 31 = capacity too small (nothing stored). */
enum { VPS_Y4M_420JPEG = 0, VPS_Y4M_420MPEG2 = 1, VPS_Y4M_422 = 2, VPS_Y4M_444 = 3, VPS_Y4M_MONO = 4 };
enum { VPS_YUV_LIMITED = 0, VPS_YUV_FULL = 1 };
enum { VPS_YUV_BT601 = 0, VPS_YUV_BT709 = 1 };
typedef struct vps_y4m_desc {
    int32_t W, H;                 /* luma size */
    int32_t CW, CH;               /* chroma plane size, rounded up for odd W / H; 0, 0 for mono */
    int32_t sampling;             /* VPS_Y4M_* : sub-sampling and chroma siting */
    int32_t range;                /* VPS_YUV_LIMITED / VPS_YUV_FULL */
    int32_t fps_num, fps_den;     /* F tag; 0:0 = absent */
    int32_t aspect_num, aspect_den;   /* A tag; 0:0 = unknown or absent */
    int32_t interlace;            /* 1 = Ip, 0 = I? or absent */
    int32_t header_bytes;         /* the header line with its newline */
    int64_t frame_bytes;          /* payload of one frame: W*H + 2*CW*CH */
} vps_y4m_desc;
int vps_y4m_info(const uint8_t* buf, int64_t nbytes, vps_y4m_desc* info);
int vps_y4m_frame_header(const uint8_t* buf, int64_t nbytes, int32_t* len);
int vps_y4m_write_header(const vps_y4m_desc* info, uint8_t* out, int64_t capacity, int32_t* len);

/* Colour conversion and chroma resampling of such frames (csrc/yuv_ops.hip; device, launch on `stream`, no sync, no allocation).
 * Integer arithmetic throughout (csrc/yuv_tables.h): every coefficient is round(65536 * c) with c from (Kr, Kb) = (0.299, 0.114) for
 * VPS_YUV_BT601, (0.2126, 0.0722) for VPS_YUV_BT709 and the range's offsets / scales (16 / 219 / 224 limited, 0 / 255 / 255 full);
 * every output is (sum + 32768) >> 16, clamped to 0..255 (decode, full-range encode) or 16..235 / 16..240 (limited-range encode).
 * tests/y4m_restate.py is the NumPy twin; results are equal byte for byte.
 * vps_yuv_to_bgr: frame = DEVICE planar frame (4-byte aligned; Y [H][W], then Cb, Cr [CH][CW] as vps_y4m_info sizes them for
 * `sampling`, tightly packed, frame_bytes >= that) -> out = BGR uint8 [H][W][3] dense, out_capacity >= 3*H*W bytes. Chroma is
 * up-sampled bilinearly at the declared siting with weights of denominator 4 per axis, (sum wy*wx*s + 8) >> 4 over the 2x2
 * neighbourhood with replicated borders: a centre-sited axis (420jpeg both, 420mpeg2 vertical) weights the nearer / farther sample
 * 3, 1; a co-sited axis (420mpeg2 and 422 horizontal) 4, 0 on even and 2, 2 on odd positions; mono uses Cb = Cr = 128.
 * vps_bgr_to_yuv: bgr = DEVICE uint8 [H][W][3] with row_stride >= 3*W bytes between rows, bytes B, G, R (rgb_order 0: a decoded
 * frame) or R, G, B (rgb_order 1: what vps_overlay_render writes) -> out = planar frame of `sampling`
 * (VPS_Y4M_444, VPS_Y4M_420JPEG or VPS_Y4M_420MPEG2), out_capacity >= its frame_bytes. Chroma is converted per pixel, then
 * reduced: 420jpeg by a 2x2 box, (sum + 2) >> 2; 420mpeg2 by (1, 2, 1) horizontally centred on the even column times the row pair,
 * (sum + 4) >> 3; source indices are clamped to the image. One launch, no intermediate plane.
 * Refusals: 1 null pointer or size not positive / W*H >= 2^31, 2 sampling, 3 range or matrix, 4 capacity / frame_bytes / stride too
 * small, 5 frame not 4-byte aligned. Nothing is launched and nothing is written on a refusal. */
int vps_yuv_to_bgr(const uint8_t* frame, int64_t frame_bytes, int H, int W, int sampling, int range, int matrix, uint8_t* out,
                   int64_t out_capacity, void* stream);
int vps_bgr_to_yuv(const uint8_t* bgr, int H, int W, int64_t row_stride, int rgb_order, int sampling, int range, int matrix,
                   uint8_t* out, int64_t out_capacity, void* stream);
/* the pixels one workgroup of each kernel covers, rows then columns (HOST; constants of the build, for tests that cross a tile) */
int vps_yuv_tile(int32_t* to_bgr_rows_cols, int32_t* to_yuv_rows_cols);

/* ref: models/anchor_heads/rpn_head.py:62-91 (sigmoid objectness, `scores.topk(nms_pre)`, gathers) + core/anchor/anchor_generator.py:55-72
 * (grid anchors) + core/bbox/transforms.py:34-68 (delta2bbox, means 0, clipped to the image) for ALL levels: one chip-wide scoring
 * launch + one select / sort / decode launch with one workgroup per level. cls[l] / reg[l]: NHWC maps [H_l][W_l][ld] of level l
 * (device pointers in host arrays; channels [0, A) / [0, 4A) used), base_anchors: device [nlv][A][4] (the rounded base anchors of
 * gen_base_anchors), strides / stds [4]: host arrays. Scratch: keys [sum_l H_l*W_l*A] uint32, hist [nlv * 4096] int32 ZERO on entry
 * (the launch leaves it zero). boxes [nlv][nms_pre][5]: the min(H_l*W_l*A, nms_pre) best positions of level l in DESCENDING score
 * order (equal scores: ascending position), rows beyond that count zeroed. nlv <= 8, nms_pre <= 8192. */
int vps_rpn_select(const float* const* cls, const int32_t* cls_ld, const float* const* reg, const int32_t* reg_ld,
                   const int32_t* Hs, const int32_t* Ws, const float* strides, int nlv, int A, const float* base_anchors,
                   int nms_pre, const float* stds, float img_h, float img_w, uint32_t* keys, int32_t* hist, float* boxes, void* stream);

/* ref: models/anchor_heads/rpn_head.py:94-104 (`mlvl_proposals` cat, `[:nms_post]` per level, top `max_num` by score).
 * boxes [nlv][nmax][5] per level in descending score order, keep [nlv][nmax] / nkeep [nlv] as written by vps_nms_batched.
 * out [max_num][5] (rows >= n_out[0] zeroed), n_out[0] = min(max_num, sum_l min(nkeep[l], nms_post)). nlv*nms_post <= 8192. */
int vps_rpn_collect(const float* boxes, const int32_t* keep, const int32_t* nkeep, int nlv, int nmax, int nms_post, int max_num,
                    float* out, int32_t* n_out, void* stream);

/* ref: models/utils/mask_roi.py:43-95 (class_agnostic=True, clip_boxes=True) + utils/upsnet/bbox/bbox_transform.py:45-60,290-330
 * + utils/upsnet/nms/gpu_nms.pyx:23-38 (`order = scores.argsort()[::-1]`).
 * rois [n][5], bbox_delta [n][4*nc], cls_prob [n][nc]; n_valid (device, may be NULL): rows >= n_valid[0] are ignored.
 * Candidates q = roi*(nc-1) + cls-1 with prob > score_thresh, sorted by descending score (equal scores: larger q first),
 * refined + clipped boxes in fp32 in the reference's operation order -> dets [<= 8192][5] (x1,y1,x2,y2,score), cand [<= 8192] = q,
 * m_out[0] = count, m_out[1] = 1 if more than 8192 candidates passed (the list is then truncated), m_out[2] = rois considered.
 * reg_weights: host float[4]. */
int vps_maskroi_select(const float* rois, const float* bbox_delta, const float* cls_prob, int n, const int32_t* n_valid,
                       int num_classes, float score_thresh, const float* reg_weights, float im_h, float im_w, float* dets,
                       int32_t* cand, int32_t* m_out, void* stream);

/* ref: models/utils/mask_roi.py:96-147 (post-NMS list, `max_det` cap by VALUE: `>= image_thresh` keeps ties; dummy row).
 * keep / nkeep: output of vps_nms_batched on `dets`. res: float [8 + 8*kcap]: res[0] = K, res[1] = candidates, res[2] = post-NMS
 * count, res[3] = status (bit 0: candidate overflow, bit 1: more than kcap detections), res[4] = rois considered, then K rows
 * (0, x1, y1, x2, y2, score, class, candidate index). */
int vps_maskroi_finish(const float* dets, const int32_t* cand, const int32_t* m_in, const int32_t* keep, const int32_t* nkeep,
                       int num_classes, int max_det, int kcap, float* res, void* stream);

/* ref: models/detectors/panoptic_fusetrack.py:424-469 (arg-max of comp_scores, greedy assignment with undo, new ids, memory
 * update). comp [K][M+1]; emb [K][E], box [K][ldb], label [K]; prev_emb [>= M+K][E], prev_box [>= M+K][4], prev_label [>= M+K]
 * are updated in place; scratch int32 [M + 3K + 1]; ids [K]; m_out[0] = new memory size. */
int vps_track_assign(const float* comp, int K, int M, const float* emb, int E, const float* box, int ldb, const int64_t* label,
                     float* prev_emb, float* prev_box, int64_t* prev_label, int32_t* scratch, int32_t* ids, int32_t* m_out,
                     void* stream);

/* the end-of-frame record a host reads once per frame, gathered in one launch: tail int32 [8 + 2*kcap] =
 * [kinfo[0..3] (k, masks valid, status, -), mem_count[0] or 0, max over f16_status[0..nslots) or 0, -, -, keep[0..K), ids[0..K) at 8 + kcap]
 * (ids, mem_count, f16_status may be NULL / nslots 0) */
int vps_frame_tail(const int32_t* kinfo, const int32_t* keep, const int32_t* ids, const int32_t* mem_count, const int32_t* f16_status,
                   int nslots, int K, int kcap, int32_t* tail, void* stream);

/* ref: models/utils/mask_removal.py:81-91 (kept list; nothing kept -> [0] with zero logits) + utils/unary_logits.py:96-106
 * (SegTerm crop of boxes*4*0.25). order [n] / flags [n] / tbox [n][4]: MaskRemoval's walk (vps_mask_level), rows [n][8]:
 * vps_maskroi_finish. class_mapping: host int32 [num_classes]. -> inst [n], keep_out [n], k_out[0] = k, k_out[1] = masks valid. */
int vps_pan_instances(const int32_t* order, const int32_t* flags, const float* rows, const int32_t* tbox, int n,
                      const int32_t* class_mapping, int num_classes, vps_pan_inst* inst, int32_t* keep_out, int32_t* k_out,
                      void* stream);

/* ----------------------------------------------------------------------------------------------
 * Panoptic post-processing. Replaces the per-frame body of
 * tools/dataset/cityscapes_vps.py:183-224 (CityscapesVPS.get_unified_pan_result): ~250 boolean masks + np.unique over
 * 2 M pixels per frame on the host become three passes over the uint8 maps on the device. All integer, bit-exact.
 *   pan, seg  uint8 [npix] (pan ids <= id_last_stuff are stuff classes, id_last_stuff+1+j = j-th instance, 255 = void)
 *   hist      int32 [256][256] (instance rows only), pan_count int32 [256]; both zeroed by vps_unify_hist
 *   cls_ind   int32 [k] (panoptic_cls_inds), obj_id int32 [nobj] or NULL (de-duplicated object ids, host side)
 *   tables    uint8 [3][256]: output values of the three channels per pan id
 *   status    int32 [1]: 0 ok, 1 = instance id without cls_ind entry, 2 = without obj_id entry (reference: IndexError)
 *   out       uint8 [npix][3] = (pan_seg, pan_ins, pan_obj) */
int vps_unify_hist(const uint8_t* pan, const uint8_t* seg, int64_t npix, int id_last_stuff, int32_t* hist, int32_t* pan_count,
                   void* stream);
int vps_unify_tables(const int32_t* hist, const int32_t* pan_count, const int32_t* cls_ind, int k, const int32_t* obj_id, int nobj,
                     int id_last_stuff, int64_t stuff_area_limit, uint8_t* tables, int32_t* status, void* stream);
int vps_unify_write(const uint8_t* pan, int64_t npix, const uint8_t* tables, uint8_t* out, void* stream);

/* Second half of the output path: tools/dataset/cityscapes_vps.py:97-159 (converter_2ch_track_core) without its per-segment
 * boolean masks. pan_2ch uint8 [H][W][3] = (pan_seg, pan_ins, pan_obj); a segment is a (pan_seg, pan_obj) pair, key =
 * seg*256 + obj (the reference's 1000*seg + obj).
 *   stats  int32 [65536][5] = (pixel count, xmin, ymin, xmax, ymax), initialised by the call (count 0 = absent)
 *   lut    uint8 [65536][3] colour per key (chosen on the host), out uint8 [npix][3] */
int vps_segment_stats(const uint8_t* pan_2ch, int H, int W, int32_t* stats, void* stream);
int vps_segment_paint(const uint8_t* pan_2ch, int64_t npix, const uint8_t* lut, uint8_t* out, void* stream);

/* VPQ evaluation: confusion counts of tools/eval_vpq.py:150-157 for ONE frame.
 *   gt_rgb, pred_rgb  uint8 [npix][3] panoptic PNGs (segment id = R + 256 G + 65536 B)
 *   gt_ids, pred_ids  sorted unique uint32 ids (device), typically the ids of the frame's segments_info plus 0 (VOID)
 *   counts            int32 [ngt+1][npred+1], zeroed by the call; row / column n collects the ids that are not listed */
int vps_pair_count(const uint8_t* gt_rgb, const uint8_t* pred_rgb, int64_t npix, const uint32_t* gt_ids, int ngt,
                   const uint32_t* pred_ids, int npred, int32_t* counts, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Image-level evaluation (csrc/ipq_ops.hip): the device passes behind tools/test_eval_ipq.py.
 *
 * vps_unify_tables_image: vps_unify_tables for tools/dataset/base_dataset.py:239-267 (BaseDataset.get_unified_pan_result): the same
 * decisions, no object ids, channel 2 of the table is 0. Between vps_unify_hist and vps_unify_write, which are shared.
 *
 * vps_segment_stats_ch / vps_segment_paint_ch: vps_segment_stats / vps_segment_paint with the segment id read from channel
 * id_channel (1 or 2): key = pan_2ch[.., 0] * 256 + pan_2ch[.., id_channel]. Channel 1 is the key of _converter_2ch_single_core
 * (base_dataset.py:296, 1000 * pan_seg + pan_ins). Same `stats` and `lut` layouts.
 *
 * vps_sseg_confusion: one image of Cityscapes.evaluate_ssegs (tools/dataset/cityscapes.py:120-135) with get_confusion_matrix
 * (base_dataset.py:449-467).
 *   gt      uint8 [Hg][Wg] label map (255 = ignored), pred uint8 [Hp][Wp] prediction
 *   ytab    int32 [Hg], xtab int32 [Wg]: source row / column of every label row / column (Pillow's NEAREST resize of pred to the
 *           label's size; values are clamped to the prediction). Both NULL = identity, sizes must then be equal.
 *   counts  int64 [class_num][class_num], DEVICE, caller-owned: the call ADDS to it and never zeroes it, so a whole validation set
 *           accumulates without a synchronisation. For gt != 255: idx = gt * class_num + pred, counted when idx < class_num^2
 *           (a prediction >= class_num lands in a later cell, as the reference's bincount puts it).
 *   class_num 1..32, otherwise -1001 and nothing is launched; Hg * Wg < 2^31. */
int vps_unify_tables_image(const int32_t* hist, const int32_t* pan_count, const int32_t* cls_ind, int k, int id_last_stuff,
                           int64_t stuff_area_limit, uint8_t* tables, int32_t* status, void* stream);
int vps_segment_stats_ch(const uint8_t* pan_2ch, int H, int W, int id_channel, int32_t* stats, void* stream);
int vps_segment_paint_ch(const uint8_t* pan_2ch, int64_t npix, int id_channel, const uint8_t* lut, uint8_t* out, void* stream);
int vps_sseg_confusion(const uint8_t* gt, int Hg, int Wg, const uint8_t* pred, int Hp, int Wp, const int32_t* ytab,
                       const int32_t* xtab, int class_num, int64_t* counts, void* stream);

/* STQ video evaluation (csrc/stq_ops.hip, vps_amd/stq.py): the counting pass of Segmentation and Tracking Quality
 * (Weber et al., "STEP", 2021) for ONE frame of a video. The definition the counts follow is restated in vps_amd/stq.py.
 *   gt_rgb, pred_rgb   DEVICE uint8 [npix][3] panoptic maps (segment id = R + 256 G + 65536 B); any byte alignment, read as aligned dwords,
 *                      nothing outside the 3 * npix bytes of each is read
 *   gt_ids, pred_ids   DEVICE sorted unique uint32 ids of the VIDEO's segments; gt_info, pred_info uint8 per id: bits 0-5 class index
 *                      (>= num_classes counts as void), bit 6 thing, bit 7 crowd (ground truth only)
 *   conf [C][C+1], gt_size [ngt], pred_size [npred+1], inter [ngt][npred]: DEVICE int64, 8-byte aligned, caller-owned. The call ADDS to
 *                      them and never zeroes them (as vps_sseg_confusion), launches on `stream`, does not synchronise or allocate.
 * Per pixel (G, P): cg = class of G, void (= C) when G is 0 or unlisted; cp = class of P, void when P is 0 or unlisted; a non-zero
 * unlisted P also adds 1 to pred_size[npred]. crowd = cg thing and G crowd; gt_track = cg thing and not crowd; pred_track = cp thing and
 * not crowd. cg != void: conf[cg][cp] += 1; gt_track: gt_size[G] += 1; pred_track: pred_size[P] += 1; both: inter[G][P] += 1.
 * Tables of at most vps_stq_lds_cells() = 12288 cells in all (C (C+1) + ngt + npred + 1 + ngt npred) are counted in a workgroup-private
 * LDS image and added with one 64-bit atomic per non-zero cell and workgroup; larger ones take 64-bit global atomics per run of equal
 * pairs. Both give the same tables. Errors before any launch: -1001 null pointer, -1002 npix outside 1 .. 2^31-1, -1003 num_classes
 * outside 1..63, -1004 negative count, -1005 more than 2^26 cells in all, -1006 a table that is not 8-byte aligned. */
int vps_stq_accumulate(const uint8_t* gt_rgb, const uint8_t* pred_rgb, int64_t npix, const uint32_t* gt_ids, const uint8_t* gt_info, int ngt,
                       const uint32_t* pred_ids, const uint8_t* pred_info, int npred, int num_classes, int64_t* conf, int64_t* gt_size,
                       int64_t* pred_size, int64_t* inter, void* stream);
int vps_stq_lds_cells(void);

/* Temporal consistency without ground truth (csrc/tc_ops.hip, vps_amd/tc.py): the counting pass of the flow-warped map
 * agreement for ONE (prev, cur, flow) pair of a video, in one launch on `stream`; does not synchronise or allocate. The definition the
 * counts follow is restated in vps_amd/tc.py.
 *   prev, cur    DEVICE uint8 [H][W][3] unified maps (pan_seg, pan_ins, pan_obj); any byte alignment, nothing outside their 3 H W bytes is
 *                read
 *   flow         DEVICE fp32 NHWC map, pixel p at flow[p * flow_ld + flow_coff] (x) and [.. + 1] (y), as vps_flow_colour; it points from cur
 *                to prev: warped(p) = prev(p + flow(p)), the convention of vps_resample2d. Read as 16-byte loads when it is the dense
 *                [h,w,2] copy on a 16-byte boundary, as 8-byte loads when flow_ld is even and flow + flow_coff is 8-byte aligned
 *   id_channel   1 or 2: key = map[.., 0] * 256 + map[.., id_channel] (as vps_segment_stats_ch)
 *   seg_class    HOST uint8 [256], copied into the launch: class index of every pan_seg value; a value >= num_classes is void (= index C)
 *   keys         DEVICE sorted unique uint16 [nkeys] keys of the video's tracks (NULL when nkeys == 0)
 *   conf [C+1][C+1], prev_size [nkeys], cur_size [nkeys], same [nkeys], misc [2] = {in view, outside}: DEVICE int64, 8-byte aligned,
 *                caller-owned; the call ADDS to them and never zeroes them (as vps_stq_accumulate)
 *   flicker      NULL, or DEVICE uint8 [H][W], every byte written: 0 agrees, 1 class differs, 2 same class and both keys listed and
 *                different, 3 not in view
 * The warp rule below, and its corners, weights and sample further down (vps_flow_occlusion), are implemented once: csrc/warp_rule.h.
 * Per pixel p = (x, y) of cur, fp32: sx = float(x) + u, sy = float(y) + v, qx = floorf(sx + 0.5f), qy = floorf(sy + 0.5f); in view iff
 * 0 <= qx <= W-1 and 0 <= qy <= H-1 as floats (NaN, inf fall out), else misc[1] += 1 and nothing else. In view, a = cur[p], b = prev[q]:
 * misc[0] += 1, conf[c(b)][c(a)] += 1, cur_size[k] += 1 when a's key is listed, prev_size[k] += 1 when b's is, same[k] += 1 when both are
 * and equal. Tables of at most vps_stq_lds_cells() cells in all ((C+1)^2 + 3 nkeys + 2) are counted in a workgroup-private LDS image and
 * added with one 64-bit atomic per non-zero cell and workgroup; larger ones take 64-bit global atomics per run of equal pairs. Both give
 * the same tables. Errors before any launch: -1001 null pointer, -1002 H or W < 1 or H W >= 2^31, -1003 num_classes outside 1..63,
 * -1004 nkeys outside 0..65536, -1005 id_channel not 1 or 2, -1006 a table that is not 8-byte aligned, -1007 flow_coff < 0 or
 * flow_ld < flow_coff + 2. */
int vps_tc_accumulate(const uint8_t* prev, const uint8_t* cur, int H, int W, const float* flow, int flow_ld, int flow_coff, int id_channel,
                      const uint8_t* seg_class, int num_classes, const uint16_t* keys, int nkeys, int64_t* conf, int64_t* prev_size,
                      int64_t* cur_size, int64_t* same, int64_t* misc, uint8_t* flicker, void* stream);

/* Occlusion-aware temporal consistency (csrc/flow_occ_ops.hip, csrc/tc_ops.hip, vps_amd/tc.py): the forward-backward
 * flow check (restated from memory of Sundaram et al., ECCV 2010, as used by UnFlow, Meister et al., AAAI 2018; alpha = 0.01, beta = 0.5
 * there) and the counting pass that honours its mask. One launch each on `stream`; neither synchronises, allocates or zeroes.
 * vps_flow_occlusion:
 *   fwd          DEVICE fp32 NHWC flow on the grid of cur, pointing into prev (vps_tc_accumulate's `flow`): pixel p at
 *                fwd[p * fwd_ld + fwd_coff] (x) and [.. + 1] (y)
 *   back         DEVICE fp32 NHWC flow on the grid of prev, pointing into cur (FlowNet2 run with the two images swapped), its own
 *                back_ld and back_coff. Both flows: any 4-byte aligned base; fwd is read as 16-byte loads when it is the dense [h,w,2]
 *                copy on a 16-byte boundary, either flow as 8-byte loads when its ld is even and base + coff is 8-byte aligned
 *   occ          NULL, or DEVICE uint8 [H][W], any byte alignment, every byte written: 0 visible, 1 occluded, 2 not in view
 *   counts       NULL, or DEVICE int64 [3], 8-byte aligned: the call ADDS the number of pixels of each code. Not both NULL.
 * Per pixel p = (x, y), everything fp32 and every operation rounded on its own (no contraction), in this order:
 *   u, v = fwd(p); sx = float(x) + u, sy = float(y) + v
 *   in view: vps_tc_accumulate's rule - qx = floorf(sx + 0.5f), qy likewise, 0 <= qx <= W-1 and 0 <= qy <= H-1 compared as floats before
 *   any conversion to int (NaN, +-inf, 1e30 fall out). Not in view: code 2, counts[2] += 1, back is not read
 *   x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1; x0 and x1 are clamped to [0, W-1] after conversion to int; the same for y
 *   b00 at (y0, x0), b01 at (y0, x1), b10 at (y1, x0), b11 at (y1, x1), per channel: top = b00 + wx*(b01 - b00),
 *   bot = b10 + wx*(b11 - b10), bt = top + wy*(bot - top)
 *   dx = u + bt_u, dy = v + bt_v; d2 = dx*dx + dy*dy; m = (u*u + v*v) + (bt_u*bt_u + bt_v*bt_v); thr = alpha*m + beta
 *   visible (code 0, counts[0]) iff d2 <= thr is true, otherwise occluded (code 1, counts[1]): a NaN anywhere gives occluded
 * No index is formed from a float before the in-view test has passed and every address of back is clamped, so no flow value makes the
 * call read outside the two maps. Errors before any launch: -1001 fwd or back NULL, or occ and counts both NULL; -1002 H or W < 1 or
 * H W >= 2^31; -1003 coff < 0 or ld < coff + 2 for either flow; -1004 counts not 8-byte aligned; -1005 alpha or beta negative or NaN.
 * vps_tc_accumulate_masked: vps_tc_accumulate with
 *   mask         DEVICE uint8 [H][W], any byte alignment (vps_flow_occlusion's occ: 0 = count the pixel)
 *   masked       DEVICE int64 [1], 8-byte aligned, ADDED to
 * A pixel that is not in view counts as outside (misc[1], flicker 3) whatever its mask byte says; an in-view pixel with mask[p] != 0 adds 1
 * to masked[0] and to nothing else (flicker 4); an in-view pixel with mask[p] == 0 is counted as vps_tc_accumulate counts it. So
 * misc[0] + misc[1] + masked[0] grows by H W per call. The table path is chosen by (C+1)^2 + 3 nkeys + 3 cells against
 * vps_stq_lds_cells(). Errors: those of vps_tc_accumulate; -1001 also for mask or masked NULL, -1006 also for masked. */
int vps_flow_occlusion(const float* fwd, int fwd_ld, int fwd_coff, const float* back, int back_ld, int back_coff, int H, int W, float alpha,
                       float beta, uint8_t* occ, int64_t* counts, void* stream);
int vps_tc_accumulate_masked(const uint8_t* prev, const uint8_t* cur, int H, int W, const float* flow, int flow_ld, int flow_coff, int id_channel,
                             const uint8_t* seg_class, int num_classes, const uint16_t* keys, int nkeys, int64_t* conf, int64_t* prev_size,
                             int64_t* cur_size, int64_t* same, int64_t* misc, uint8_t* flicker, const uint8_t* mask, int64_t* masked,
                             void* stream);

/* Optical-flow accuracy against ground truth (csrc/flow_err_ops.hip, vps_amd/floweval.py): end-point error, outlier
 * and speed-bin counts and the error image of ONE (pred, gt) pair of flows. The rules are restated from memory of the KITTI, Sintel and
 * Middlebury kits (vps_amd/floweval.py). Two launches on `stream` (the counting pass, then one workgroup that adds the partial sums); the
 * call does not synchronise, allocate or zero.
 *   pred, gt     DEVICE fp32 NHWC flows, pixel p at f[p * ld + coff] (x) and [.. + 1] (y) as vps_flow_colour / vps_tc_accumulate, each with
 *                its own ld and coff; any 4-byte aligned base. Either is read as 16-byte loads when it is the dense [h,w,2] copy on a
 *                16-byte boundary, as 8-byte loads when its ld is even and base + coff is 8-byte aligned, as 4-byte loads otherwise
 *   mask         NULL, or DEVICE uint8 [H][W], any byte alignment (read as aligned dwords, bytewise at the edges): 1 = valid and not
 *                occluded (group noc = 0), 2 = valid and occluded in the ground truth (group occ = 1), 0 and >= 3 = invalid.
 *                NULL: every pixel is in group noc
 *   occ_pred     NULL, or DEVICE uint8 [H][W], any byte alignment: the codes of vps_flow_occlusion (0 visible, 1 occluded, 2 not in view)
 *   counts       DEVICE int64 [25], 8-byte aligned, ADDED to: [g * 12 + k] for the groups g = 0 (noc), 1 (occ) and cell 24 = invalid pixels.
 *                k: 0 n (valid, not bad), 1 bad, 2 Fl outliers, 3 / 4 / 5 epe > 1 / 3 / 5, 6 / 7 / 8 n with mag < 10 / 10 <= mag < 40 /
 *                mag >= 40, 9 / 10 / 11 valid pixels (bad ones too) whose occ_pred code is 0 / 1 / 2 (a code >= 3 is counted in none;
 *                untouched when occ_pred is NULL). Cells 0 and 1 of both groups and cell 24 together grow by H W per call
 *   sums         DEVICE double [2][4], 8-byte aligned, ADDED to: per group the sum of epe over n and over each of the three speed bins
 *   err_rgb      NULL, or DEVICE uint8 [H][W][3], any byte alignment, every byte written in the counting launch
 *   ws           DEVICE workspace, 8-byte aligned, at least vps_flow_error_ws_bytes(H, W) bytes (HOST arithmetic; -1002 for a bad size):
 *                eight doubles per workgroup of the counting launch
 * Per pixel, fp64 from the fp32 inputs, every operation rounded on its own (no contraction):
 *   invalid      the mask says so, or a gt component is NaN or |.| > 1e9 (unknown flow): counts[24] += 1, nothing else; black
 *   bad          valid, but a pred component is NaN, +-inf or |.| > 1e9: cell 1 and the occ_pred cell; no sum; (255, 0, 255)
 *   otherwise    du = u - ug, dv = v - vg, epe = sqrt(du*du + dv*dv), mag = sqrt(ug*ug + vg*vg); outlier iff epe > 3.0 and
 *                epe > 0.05 * mag (KITTI, strict, a product); colour: n_err = min(epe / 3.0, epe / (0.05 * mag)), epe / 3.0 when
 *                mag == 0; the first row with n_err < hi of hi = 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48, inf ->
 *                (49,54,149) (69,117,180) (116,173,209) (171,217,233) (224,243,248) (254,224,144) (253,174,97) (244,109,67) (215,48,39)
 *                (165,0,38)
 * Determinism: the counts leave a workgroup as one 64-bit integer atomic per non-zero cell; the sums are reduced in a fixed tree inside
 * the workgroup, written to the workgroup's own slot of ws, and the second launch adds the slots in a fixed order (lane by lane in
 * ascending slot order, then a fixed tree) before it adds the totals to `sums`: no floating-point atomics, the same bytes on every call.
 * No address is formed from a flow value. Errors before any launch: -1001 pred, gt, counts, sums or ws NULL; -1002 H or W < 1 or
 * H W >= 2^31; -1003 coff < 0 or ld < coff + 2 for either flow; -1004 counts or sums not 8-byte aligned, or a flow base not 4-byte
 * aligned; -1005 ws not 8-byte aligned or ws_bytes too small. */
int64_t vps_flow_error_ws_bytes(int H, int W);
int vps_flow_error(const float* pred, int pred_ld, int pred_coff, const float* gt, int gt_ld, int gt_coff, const uint8_t* mask,
                   const uint8_t* occ_pred, int H, int W, int64_t* counts, double* sums, uint8_t* err_rgb, void* ws, int64_t ws_bytes,
                   void* stream);

/* Flow quality without ground truth (csrc/flow_photo_ops.hip, vps_amd/flowphoto.py): the photometric warp error of ONE
 * (cur, prev, flow) triple - prev sampled at p + flow(p) against cur - beside the static error of prev(p) against cur(p). It is the warp /
 * interpolation error that Middlebury reports beside EPE, restated from memory (vps_amd/flowphoto.py). Two launches on `stream` (the
 * counting pass, then one workgroup that adds the partial sums); the call does not synchronise, allocate or zero.
 *   cur_bgr, prev_bgr  DEVICE uint8 [H][W][3] frames, any byte alignment; nothing outside their 3 H W bytes is read
 *   flow         DEVICE fp32 NHWC map on the grid of cur, pointing into prev, pixel p at flow[p * flow_ld + flow_coff] (x) and [.. + 1] (y)
 *                as vps_tc_accumulate's; any 4-byte aligned base. Read as 16-byte loads when it is the dense [h,w,2] copy on a 16-byte
 *                boundary, as 8-byte loads when flow_ld is even and flow + flow_coff is 8-byte aligned, as 4-byte loads otherwise
 *   mask_in      NULL, or DEVICE uint8 [H][W], any byte alignment, vps_flow_occlusion's codes: 0 puts a pixel into group 0, any other
 *                byte into group 1. NULL: every pixel is in group 0
 *   thr          the flag threshold in grey levels; negative or NaN is refused
 *   counts       DEVICE int64 [21], 8-byte aligned, ADDED to: [g * 10 + k] for the groups g = 0, 1 and cell 20 = pixels not in view.
 *                k: 0 n, 1 flagged, 2 sum of as, 3 sum of qs, 4 / 5 / 6 / 7 pixels with e > 4 / 8 / 16 / 32, 8 pixels with
 *                aw < double(as) (the flow helps), 9 pixels with aw > double(as). Cells 0 of both groups and cell 20 together grow by
 *                H W per call
 *   sums         DEVICE double [2][2], 8-byte aligned, ADDED to: per group the sum of aw and the sum of qw
 *   mask_out     NULL, or DEVICE uint8 [H][W], any byte alignment, every byte written. It MAY BE THE SAME BUFFER as mask_in: a lane reads
 *                its own four bytes before it writes them
 *   residual     NULL, or DEVICE uint8 [H][W], any byte alignment, every byte written
 *   ws           DEVICE workspace, 8-byte aligned, at least vps_flow_photo_ws_bytes(H, W) bytes (HOST arithmetic; -1002 for a bad size):
 *                four doubles per workgroup of the counting launch
 * Per pixel p = (x, y) of cur, in this order, every operation rounded on its own (no contraction):
 *   1. in view, fp32: u, v = flow(p); sx = float(x) + u, sy = float(y) + v; in view iff floorf(sx + 0.5f) and floorf(sy + 0.5f) lie in
 *      [0, W-1] and [0, H-1], compared as floats (vps_tc_accumulate's rule: NaN, +-inf, 1e30 fall out; no index is formed from a float
 *      before this test has passed). Not in view: counts[20] += 1, mask_out = 2, residual = 0, nothing else
 *   2. group: g = 0 when mask_in is NULL or mask_in[p] == 0, otherwise 1
 *   3. bilinear sample, fp32, corners and weights as vps_flow_occlusion forms them: x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1, both
 *      clamped to [0, W-1] after conversion to int; the same for y. Per channel c, the corner bytes of prev converted to float:
 *      top = b00 + wx*(b01 - b00), bot = b10 + wx*(b11 - b10), s_c = top + wy*(bot - top)
 *   4. errors, fp64: dw_c = double(s_c) - double(cur_c); aw = (|dw_0| + |dw_1|) + |dw_2|; qw = (dw_0*dw_0 + dw_1*dw_1) + dw_2*dw_2;
 *      e = aw / 3.0. The static twin from prev(p) itself, exact integers: as = sum |prev_c(p) - cur_c(p)|, qs = sum (prev_c(p) - cur_c(p))^2
 *   5. flagged iff e > double(thr), strictly
 *   6. the cells of counts[g * 10 + k] above; sums[g][0] += aw, sums[g][1] += qw
 *   7. mask_out[p] = mask_in[p] when that is non-zero, else 3 when flagged, else 0
 *   8. residual[p] = min(255, (int)floor(e + 0.5))
 * Determinism: as vps_flow_error - one 64-bit integer atomic per non-zero cell and workgroup; the sums are reduced in a fixed tree inside
 * the workgroup, written to the workgroup's own slot of ws, and the second launch adds the slots in a fixed order before it adds the
 * totals to `sums`: no floating-point atomics, the same bytes on every call, twice without zeroing is exactly double. Every corner
 * address of prev is clamped to the map. Errors before any launch: -1001 cur_bgr, prev_bgr, flow, counts, sums or ws NULL; -1002 H or
 * W < 1 or H W >= 2^31; -1003 flow_coff < 0 or flow_ld < flow_coff + 2; -1004 counts or sums not 8-byte aligned, or the flow base not
 * 4-byte aligned; -1005 ws not 8-byte aligned or ws_bytes too small; -1006 thr negative or NaN. */
int64_t vps_flow_photo_ws_bytes(int H, int W);
int vps_flow_photo(const uint8_t* cur_bgr, const uint8_t* prev_bgr, int H, int W, const float* flow, int flow_ld, int flow_coff,
                   const uint8_t* mask_in, float thr, int64_t* counts, double* sums, uint8_t* mask_out, uint8_t* residual, void* ws,
                   int64_t ws_bytes, void* stream);

/* Illumination-robust flow residual (csrc/flow_census_ops.hip, vps_amd/flowphoto.py): the ternary census warp error of
 * ONE (cur, prev, flow) triple. The hard ternary census (Stein 2004) as UnFlow (Meister et al. 2018) uses it, RESTATED FROM MEMORY;
 * UnFlow's soft, differentiable form is not built. Two launches on `stream` (the warp pass, then the census pass on tiles of
 * vps_flow_census_tile rows x columns); the call does not synchronise, allocate or zero, and no workgroup waits for or reads from another.
 *   cur_bgr, prev_bgr, flow, flow_ld, flow_coff, mask_in, mask_out, residual   as vps_flow_photo's: any byte alignment of the five byte maps,
 *                the three flow layouts, mask_out MAY BE THE SAME BUFFER as mask_in, nothing outside the maps is read
 *   thr          the flag threshold, an integer percent in 0 .. 100 (default of the Python side 25)
 *   eps          the dead zone of the ternary code in units of g, finite and not negative (default of the Python side 2000.0 = two grey
 *                levels). Both defaults are parameter defaults with no real footage behind them
 *   table        DEVICE int64 [2][13], 8-byte aligned, ADDED to: row g for the mask groups g = 0, 1 of vps_flow_photo
 *   ws           DEVICE workspace, 16-byte aligned, at least vps_flow_census_ws_bytes(H, W) bytes (HOST arithmetic; -1002 for a bad size):
 *                three fp32 planes (Wg, the grey of cur, the grey of prev), each (H W rounded up to a multiple of 4) floats: 12 bytes
 *                per pixel
 * The rule, every fp32 operation rounded on its own (no contraction):
 *   1. grey: g = 299 R + 587 G + 114 B (byte 0 of a pixel is B, byte 2 is R), an integer in 0 .. 255 000, held as fp32 (exact)
 *   2. warped grey Wg(p): the in-view rule (step 1) and the corners and weights (step 3) of vps_flow_photo verbatim; the bilinear sample
 *      of the four corners' greys in fp32: top = g00 + wx*(g01 - g00), bot = g10 + wx*(g11 - g10), Wg = top + wy*(bot - top). A pixel
 *      that is not in view has no Wg (-1.0f in the workspace)
 *   3. window: the neighbours q = p + (dx, dy), dx, dy in -3 .. 3, not both zero: 48
 *   4. code of an image A: code_A(p, q) = +1 if A(q) - A(p) > eps, -1 if it is < -eps, else 0: one fp32 subtraction, two comparisons
 *   5. warped count: a neighbour counts when q lies in the image and Wg(q) exists; n_w(p) of them, d_w(p) of those with
 *      code_cur != code_Wg
 *   6. static count: prev unwarped in the place of Wg; n_s counts every neighbour in the image, d_s as in 5
 *   7. p is scored when it is in view and n_w(p) >= 1
 *   8. a scored pixel is flagged when 100 d_w > thr n_w, strictly, in integers
 *   9. helped when d_w n_s < d_s n_w, hurt when >
 *  10. table[g][k]: 0 scored pixels; 1, 2 the sums of d_w, n_w; 3, 4 the sums of d_s, n_s over scored pixels; 5, 6, 7 scored pixels with
 *      100 d_w > 10, 25, 50 n_w; 8 helped; 9 hurt; 10 flagged; 11 not in view; 12 in view with n_w = 0. Cells 0, 11, 12 of both rows
 *      together grow by H W per call
 *  11. mask_out[p] = 2 when p is not in view, else mask_in[p] when that is non-zero, else 3 when flagged, else 0
 *  12. residual[p] = (255 d_w + n_w / 2) / n_w in integer division; 0 for a pixel that is not scored
 * Determinism: every decision after the codes is an integer one and the table grows by one 64-bit integer atomic per non-zero cell and
 * workgroup: the same bytes on every call, twice without zeroing is exactly double; there are no floating-point sums and no finishing
 * launch. Every corner address of prev is clamped to the map and no index is formed from a float before the in-view test has passed.
 * vps_flow_census_tile (HOST): rows_cols[0], rows_cols[1] = rows and columns of a tile of the census pass (constants of the build, for
 * tests that put edges on the seams).
 * Errors before any launch: -1001 cur_bgr, prev_bgr, flow, table or ws NULL; -1002 H or W < 1 or H W >= 2^31; -1003 flow_coff < 0 or
 * flow_ld < flow_coff + 2; -1004 table not 8-byte aligned, or the flow base not 4-byte aligned; -1005 ws not 16-byte aligned or ws_bytes
 * too small; -1006 thr outside 0 .. 100; -1007 eps negative, NaN or infinite. */
int64_t vps_flow_census_ws_bytes(int H, int W);
int vps_flow_census_tile(int32_t* rows_cols);
int vps_flow_census(const uint8_t* cur_bgr, const uint8_t* prev_bgr, int H, int W, const float* flow, int flow_ld, int flow_coff,
                    const uint8_t* mask_in, int thr, float eps, int64_t* table, uint8_t* mask_out, uint8_t* residual, void* ws,
                    int64_t ws_bytes, void* stream);

/* Boundary PQ / boundary VPQ (csrc/boundary_ops.hip, vps_amd/boundary.py): the boundary band of EVERY segment of a
 * panoptic map in one call, the device form of Boundary IoU's mask_to_boundary (Cheng et al., CVPR 2021) applied per segment.
 *   pan_rgb   DEVICE uint8 [H][W][3] panoptic map (segment id = R + 256 G + 65536 B, the maps vps_pair_count reads); any byte alignment,
 *             nothing outside its 3 * H * W bytes is read
 *   out_rgb   DEVICE uint8 [H][W][3], every byte written. For a pixel of id s: s == 0 (VOID) -> 0. Otherwise the pixel is INTERIOR when
 *             the whole (2d+1) x (2d+1) window centred on it lies inside the image and every pixel of the window has id s; an interior
 *             pixel -> 0xFFFFFF (the reserved fill id), every other pixel is a band pixel -> s. (Padding the mask with a ring of zeros
 *             and eroding it d times with a 3 x 3 kernel removes exactly the pixels that are not interior.)
 *   ws        DEVICE workspace, 4-byte aligned, at least vps_boundary_band_ws(H, W, d) = 4 * H * W bytes: one dword per pixel, the id and
 *             the flag "the row window [x-d, x+d] is inside the image and uniform"
 * Two launches on `stream` (row pass, column pass), no sync, no allocation, no atomics; the bytes do not depend on the launch geometry
 * or on the workspace's size. The work per pixel does not grow with d: the row pass takes a prefix sum of the id changes over
 * 512 columns plus a halo of d, the column pass walks 32 rows plus a halo of d per lane and keeps the last row that changed.
 * vps_boundary_tile (HOST): rows_cols[0] = rows of a column-pass tile, rows_cols[1] = columns of a row-pass tile (constants of the build,
 * for tests that put edges on the seams).
 * Errors before any launch: -1001 null pointer, -1002 H or W < 1 or H * W >= 2^31, -1003 d outside 1..255, -1004 workspace too small
 * or not 4-byte aligned. */
int vps_boundary_band(const uint8_t* pan_rgb, int H, int W, int d, uint8_t* out_rgb, void* ws, int64_t ws_bytes, void* stream);
int vps_boundary_band_ws(int H, int W, int d, int64_t* ws_bytes);
int vps_boundary_tile(int32_t* rows_cols);

/* PNG output without a match search (csrc/png_ops.hip): a uint8 [H][W][C] DEVICE image, C = 1 or 3 in stored
 * order, row stride in bytes -> one zlib stream for the IDAT chunk of an 8-bit grey / RGB PNG. The format is fixed:
 *   filter   per row None (0), Sub (1) or Up (2) by the smallest sum of |int8(residual)|, a tie to the lower number; S = the rows in
 *            order, each its filter byte + W*C residuals; N = H * (1 + W*C)
 *   segments S in pieces of 8192 bytes, each coded alone: maximal runs of equal bytes; the first byte of a run is a literal, the other
 *            R-1 are distance-1 matches of 258 while >= 258 remain, then one match of the rest if it is >= 3, else literals
 *   bits     per segment a fixed-Huffman block (BFINAL 0) with those tokens and end-of-block, then an empty stored block
 *            (pads to the byte, 00 00 FF FF): at most ceil(9*8192/8) + 7 bytes
 *   stream   78 01, the segments, 03 00 (empty final fixed block), Adler-32 of S big-endian
 * vps_png_encode_bound (HOST arithmetic only): worst-case stream bytes and the workspace bytes of vps_png_deflate.
 * vps_png_deflate: every pointer is a DEVICE pointer (ws 16-byte, out_nbytes 8-byte aligned); launches on `stream`, no sync, no
 * hidden allocation. out_nbytes[0] = bytes written, or -1 when out_capacity is too small (then nothing is stored to out). */
int vps_png_encode_bound(int H, int W, int channels, int64_t* out_capacity, int64_t* ws_bytes);
int vps_png_deflate(const uint8_t* img, int H, int W, int channels, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                    int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream);
/* The same chain for a row given in bytes and a pixel of bpp bytes: H rows of rowbytes bytes (a multiple of bpp, at most 65535 pixels),
 * bpp = 1 (grey), 3 (RGB) or 6 (RGB with 16-bit samples, the KITTI flow files). S = the rows in order, each its filter byte + rowbytes
 * residuals, N = H * (1 + rowbytes); Sub takes the byte bpp to the left; filter choice, segments, bits and stream are the ones above,
 * and for bpp 1 / 3 the bytes are vps_png_deflate's. -1002 for another bpp, -1001 for a bad H or rowbytes; the other codes, pointers,
 * alignments and out_nbytes as vps_png_deflate. */
int vps_png_encode_bound_bpp(int H, int64_t rowbytes, int bpp, int64_t* out_capacity, int64_t* ws_bytes);
int vps_png_deflate_bpp(const uint8_t* img, int H, int64_t rowbytes, int bpp, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                        int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream);
/* The two calls above with the Huffman code as an argument, for dense images (flow files, colour images, error maps).
 * huffman 0: the fixed code, byte for byte vps_png_deflate / vps_png_deflate_bpp. huffman 1: "dynamic", below. Any other value: -1007
 * before any launch. Filter, segments, tokens, stream framing, bounds (vps_png_encode_bound*), workspace, pointers, alignments,
 * out_nbytes and the other error codes are the same for both. The dynamic stream, per segment:
 *   symbols  the segment's tokens as RFC 1951 literal/length symbols: a literal is its byte, a match its length symbol (3.2.5) with
 *            its extra bits; every match has distance 1. count[s] = uses of symbol s in the segment, count[256] (end of block) = 1
 *   lengths  LIMITED(count[0..285], 15). LIMITED(count, L) is package-merge: the n symbols with count > 0 are the leaves, in ascending
 *            order of (count, symbol). List 1 = the leaves. List j (2..L) = the leaves merged by weight with the packages of list j-1
 *            (item 2k + item 2k+1 for k = 0 .., an odd last item dropped); of a leaf and a package of equal weight the leaf comes
 *            first; the list is cut to its first 2n-2 items. Start with k = 2n-2 at list L; at each list from L down to 1, if a of
 *            its first k items are leaves, the a first leaves gain one bit and k becomes 2 (k - a). n = 1: that symbol gets length 1.
 *            The lengths are optimal under the limit, so they cost what a Huffman tree costs wherever that tree is at most L deep
 *   codes    canonical codes of the lengths (RFC 1951 3.2.2)
 *   distance HDIST = 2: distance symbols 0 and 1 with length 1 each (a complete code); a match's distance is the single bit 0
 *   header   BFINAL 0, BTYPE 10, HLIT = max(257, last symbol with a length + 1), HDIST, HCLEN. The HLIT + 2 lengths are ONE sequence,
 *            coded per maximal run of equal values. R zeros: symbol 18 with min(R, 138) while R >= 11, then 17 if R >= 3, else R
 *            times 0. R times v > 0: v once, then with R-1 left: 16 with min(left, 6) while left >= 3, then v for each one left.
 *            cl_count[0..18] = uses of those symbols; their lengths = LIMITED(cl_count, 7), canonical codes; HCLEN = max(4, last
 *            nonzero length in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, + 1)
 *   block    header, the tokens (code, extra bits, distance bit), end of block; D = its bits. F = the bits of the fixed block
 *            (3 + tokens + 7)
 *   choice   the segment is this block if F >= 512 and D < F, else the fixed block of vps_png_deflate, the same bytes. (A segment
 *            under 512 bits is almost all runs, a label map's: a code of its own could save less than 64 bytes of 8192 there and is
 *            not built. An all-zero segment, F = 439, stays fixed.) Either is
 *            followed by the empty stored block, so a stream is never longer than the fixed one and the bounds do not change. */
int vps_png_deflate_h(const uint8_t* img, int H, int W, int channels, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                      int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream, int huffman);
int vps_png_deflate_bpp_h(const uint8_t* img, int H, int64_t rowbytes, int bpp, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                          int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream, int huffman);

/* Optical-flow output (csrc/flow_vis_ops.hip; vps_amd/flowvis.py): the colour coding of the reference's flow_utils.py (vis_flow) on the
 * device. Both launch on `stream`, no sync, no hidden allocation. flow: DEVICE fp32 NHWC map of H x W pixels, pixel p at
 * flow[p * ld + coff] (u) and [p * ld + coff + 1] (v); coff + 2 <= ld. A pixel with u > 1e9 or v > 1e9 (unknown flow) counts as (0, 0).
 *   vps_flow_max_radius  out (DEVICE double [1], 8-byte aligned) = max sqrt(u*u + v*v) over the frame in fp64; the call itself sets it
 *                        to 0 on the stream first
 *   vps_flow_colour      rgb (DEVICE uint8 [H][W][3], dense, 4-byte aligned) = vis_flow(flow.astype(float64)) with the normaliser
 *                        max_rad[0] (DEVICE double [1]): u, v /= max_rad + DBL_EPSILON; hue from atan2(-v, -u) over the 55-entry colour
 *                        wheel; radius <= 1: col = 1 - radius * (1 - col), else col * 0.75; floor(255 * col). fp64, no contraction.
 *                        The frame's own vps_flow_max_radius result is the reference's behaviour; a fixed value keeps a clip's colours
 *                        steady. NaN flow is not handled. */
int vps_flow_max_radius(const float* flow, int ld, int coff, int H, int W, double* out, void* stream);
int vps_flow_colour(const float* flow, int ld, int coff, int H, int W, const double* max_rad, uint8_t* rgb, void* stream);

/* Track tubes (csrc/rle_ops.hip, csrc/rle_host.cpp; vps_amd/tubes.py): the COCO run-length encoding of every
 * segment of a panoptic map. The device lists the runs of the map, the host turns the list into one `counts` string per segment.
 *
 * vps_rle_runs: pan_2ch DEVICE uint8 [H][W][3]; key = pan_2ch[.., 0] * 256 + pan_2ch[.., id_channel], id_channel 1 or 2 (as
 * vps_segment_stats_ch). Position q = x * H + y (column-major, the order of COCO's rleEncode). A run starts at q = 0 and wherever
 * key(q) != key(q - 1); a run that leaves a column at its bottom and goes on at the top of the next one is ONE run.
 *   run_start  DEVICE uint32 [cap] (4-byte aligned), run_key DEVICE uint16 [cap]: the first min(nruns, cap) runs in ascending q;
 *              nothing is stored at or behind index cap
 *   nruns      DEVICE int32 [1]: the TRUE number of runs, also when it exceeds cap (the caller then calls again with that capacity)
 *   ws         DEVICE workspace, 16-byte aligned, at least vps_rle_runs_ws(H, W) bytes (0 for sizes that are rejected)
 * Three launches on `stream`, no sync, no hidden allocation, no atomics: the list is the same on every call. Rejected before any
 * launch (<= -1000): a null pointer, H or W < 1, H * W >= 2^31, id_channel not 1 or 2, cap < 0, a short or misaligned workspace.
 * vps_rle_band_rows: rows of one band of the kernel's sweeps (its launch constant; for tests that put a run across a band edge).
 *
 * vps_rle_strings (HOST arithmetic only, no allocation, thread-safe): run list -> compressed COCO `counts` strings.
 *   run_start, run_key, nruns  HOST copies of the list (all nruns runs), npix = H * W
 *   keys       sorted ascending, unique, nkeys of them; a key that is absent gets the single count npix
 *   out        the strings one behind the other, no terminator: key i at out + offset[i], length[i] characters (offset, length
 *              int64 [nkeys]); vps_rle_strings_bound(nruns, nkeys) characters always suffice
 *   scratch    int64 [4 * nkeys]
 * The counts of a key alternate zero-runs and one-runs, starting with a zero-run that may be 0; a trailing zero-run is written only
 * when it is not empty. Coding: COCO's rleToString (count i >= 3 as the difference to count i - 2; 5 bits and a continuation bit per
 * character, + 48). Too small an out_capacity: -1008, offset / length hold what is needed, nothing is stored to out. A list that does
 * not start at 0, does not ascend, reaches npix or repeats a key in neighbouring runs, and unsorted keys, are rejected too. */
int vps_rle_runs(const uint8_t* pan_2ch, int H, int W, int id_channel, uint32_t* run_start, uint16_t* run_key, int cap, int32_t* nruns,
                 void* ws, size_t ws_bytes, void* stream);
int64_t vps_rle_runs_ws(int H, int W);
int vps_rle_band_rows(void);
int vps_rle_strings(const uint32_t* run_start, const uint16_t* run_key, int nruns, int64_t npix, const uint16_t* keys, int nkeys, char* out,
                    int64_t out_capacity, int64_t* offset, int64_t* length, int64_t* scratch);
int64_t vps_rle_strings_bound(int nruns, int nkeys);

/* ----------------------------------------------------------------------------------------------
 * Input preparation: Normalize -> Pad(size_divisor) -> ImageToTensor of the test pipeline in one pass.
 * Replaces mmdet/datasets/pipelines/transforms.py:258-269, :310-318 and formating.py:52-67 (mmcv 0.2.14 imnormalize,
 * impad_to_multiple) for a decoded uint8 [H][W][3] image already on the device.
 *   mean, std  HOST pointers to 3 floats (channel order of the OUTPUT, i.e. RGB when to_rgb)
 *   out        fp32 [3][Hp][Wp], (c - mean) / std in fp32, bottom/right padding = pad_val. Bit-exact with NumPy. */
/* Resize of the same pipeline (transforms.py:107-122 -> mmcv.imrescale -> cv2.resize, INTER_LINEAR) on the decoded uint8 image:
 * OpenCV's 8-bit fixed-point bilinear (11-bit coefficients), or the area average when the size is halved exactly.
 *   xtab / ytab  DEVICE int32 [W][3] / [H][3]: source index, weight of it, weight of its successor (weights sum to 2048);
 *                unused (may be NULL) for the exact 2x shrink
 *   src / dst    uint8 [H0][W0][C] -> [H][W][C], C <= 4 */
int vps_resize_u8(const uint8_t* src, int H0, int W0, uint8_t* dst, int H, int W, int C, const int32_t* xtab,
                  const int32_t* ytab, void* stream);

int vps_image_prep(const uint8_t* img, int H, int W, int Hp, int Wp, const float* mean, const float* std, int to_rgb,
                   float pad_val, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VPS_HIP_H */
