// Optical-flow accuracy against ground truth (vps_amd/floweval.py): the counting pass of end-point error, outlier rate
// and speed bins, and the error image.
//   vps_flow_error_ws_bytes  host arithmetic: eight doubles per workgroup of the counting launch
//   vps_flow_error           one (pred, gt) pair: every pixel is ADDED to the caller's int64 [25] counts and double [2][4] sums; optionally
//                            the KITTI-coloured error image is written in the same launch. Nothing is zeroed, downloaded or synchronised.
// Arithmetic: fp32 widened to fp64, the operations of the definition (include/vps_hip.h) in its order, every one rounded on its own - the
// whole file is compiled without contraction, so that every decision (outlier, threshold, speed bin, colour row) equals the NumPy float64
// restatement (tests/flow_err_restate.py): epe == 3.0 and epe == 0.05 * mag sit on the boundary for whole-number differences, where a
// fused multiply-add under the root decides differently. sqrt and / of doubles are correctly rounded on the device.
// Determinism: integer atomics for the counts; the sums never meet a floating-point atomic - fixed trees and one slot per workgroup.
// No address is formed from a flow value: NaN, inf and 1e30 read and write nothing outside the buffers.
#include "px4.h"

#pragma clang fp contract(off)

namespace {

constexpr int FE_THREADS = PX4_WG;
constexpr int FE_CELLS = 25, FE_SUMS = 8;
constexpr double FE_UNKNOWN = 1e9;                    // the Middlebury convention of vps_flow_max_radius

// the row of the error-colour table, R | G << 8 | B << 16
__device__ __forceinline__ uint32_t fe_colour(double n_err) {
#define FE_RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
    uint32_t c = FE_RGB(165, 0, 38);
    if (n_err < 48.0) c = FE_RGB(215, 48, 39);
    if (n_err < 24.0) c = FE_RGB(244, 109, 67);
    if (n_err < 12.0) c = FE_RGB(253, 174, 97);
    if (n_err < 6.0) c = FE_RGB(254, 224, 144);
    if (n_err < 3.0) c = FE_RGB(224, 243, 248);
    if (n_err < 1.5) c = FE_RGB(171, 217, 233);
    if (n_err < 0.75) c = FE_RGB(116, 173, 209);
    if (n_err < 0.375) c = FE_RGB(69, 117, 180);
    if (n_err < 0.1875) c = FE_RGB(49, 54, 149);
    return c;
#undef FE_RGB
}

// A lane owns 4 consecutive pixels (linear index) per step; a workgroup strides over the chunks. The 25 counters (uint32: H W < 2^31) and the
// 8 sums of a lane stay in registers under constant indices; they leave in the order of the tables through Part C of px4.h: the counts
// as one 64-bit atomic per non-zero cell, the sums as the workgroup's own slot of `slots` (always written, zeros too: the finishing
// launch reads every slot). No workgroup reads what another one writes.
__global__ __launch_bounds__(FE_THREADS)
void flow_error_kernel(const float* __restrict__ pred, int pld, int pcoff, int pmode, const float* __restrict__ gt, int gld, int gcoff, int gmode,
                       const uint8_t* __restrict__ mask, const uint8_t* __restrict__ occ_pred, long npix, unsigned long long* __restrict__ counts,
                       double* __restrict__ slots, uint8_t* __restrict__ rgb) {
    __shared__ uint32_t red_c[FE_THREADS / 64][FE_CELLS];
    __shared__ double red_s[FE_THREADS / 64][FE_SUMS];
    const long nchunk = (npix + PX4 - 1) / PX4;
    const bool rgb4 = rgb && ((uintptr_t)rgb & 3) == 0;
    uint32_t cnt[2][12], n_inv = 0;
    double sum[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int k = 0; k < 12; ++k) cnt[g][k] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[g][k] = 0.0;
    }
    for (long ch = (long)blockIdx.x * FE_THREADS + threadIdx.x; ch < nchunk; ch += (long)gridDim.x * FE_THREADS) {
        const long p0 = PX4 * ch;
        const int n = (int)min((long)PX4, npix - p0);
        float u[PX4], v[PX4], ug[PX4], vg[PX4];
        px4_load_flow(pred, pld, pcoff, pmode, p0, n, u, v);
        px4_load_flow(gt, gld, gcoff, gmode, p0, n, ug, vg);
        const uint32_t M = mask ? px4_load_bytes(mask, npix, p0, n) : 0x01010101u;
        const uint32_t O = occ_pred ? px4_load_bytes(occ_pred, npix, p0, n) : 0xffffffffu;
        uint32_t col[PX4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            if (i >= n) break;
            // ---- the definition, in its order
            const double dug = (double)ug[i], dvg = (double)vg[i], du0 = (double)u[i], dv0 = (double)v[i];
            const uint32_t m = (M >> (8 * i)) & 0xffu, oc = (O >> (8 * i)) & 0xffu;
            const bool known = fabs(dug) <= FE_UNKNOWN && fabs(dvg) <= FE_UNKNOWN;           // false for NaN
            if (!((m == 1 || m == 2) && known)) { ++n_inv; continue; }                       // black
            const bool occ = m == 2;
            const bool good = fabs(du0) <= FE_UNKNOWN && fabs(dv0) <= FE_UNKNOWN;             // false for NaN, +-inf, 1e30
            bool out = false, e1 = false, e3 = false, e5 = false, b0 = false, b1 = false, b2 = false;
            double epe = 0.0;
            if (good) {
                const double du = du0 - dug, dv = dv0 - dvg;
                epe = sqrt(du * du + dv * dv);
                const double mag = sqrt(dug * dug + dvg * dvg);
                const double rel = 0.05 * mag;
                out = epe > 3.0 && epe > rel;
                e1 = epe > 1.0; e3 = epe > 3.0; e5 = epe > 5.0;
                b0 = mag < 10.0; b1 = !b0 && mag < 40.0; b2 = !b0 && !b1;
                double n_err = epe / 3.0;
                if (mag != 0.0) {
                    const double r = epe / rel;
                    if (r < n_err) n_err = r;
                }
                col[i] = fe_colour(n_err);
            } else {
                col[i] = 255u | (255u << 16);
            }
#pragma unroll
            for (int g = 0; g < 2; ++g) {             // constant indices: the tables stay in registers
                const bool mine = occ == (g == 1);
                cnt[g][0] += mine && good;  cnt[g][1] += mine && !good;  cnt[g][2] += mine && out;
                cnt[g][3] += mine && e1;    cnt[g][4] += mine && e3;     cnt[g][5] += mine && e5;
                cnt[g][6] += mine && b0;    cnt[g][7] += mine && b1;     cnt[g][8] += mine && b2;
                cnt[g][9] += mine && oc == 0; cnt[g][10] += mine && oc == 1; cnt[g][11] += mine && oc == 2;
                sum[g][0] += mine ? epe : 0.0;        // epe is 0 for a bad pixel
                sum[g][1] += mine && b0 ? epe : 0.0;
                sum[g][2] += mine && b1 ? epe : 0.0;
                sum[g][3] += mine && b2 ? epe : 0.0;
            }
        }
        if (rgb) px4_store_px3(rgb, rgb4, p0, n, col);
    }
    uint32_t cell[FE_CELLS];                          // the tables' order (flat arrays through the loop cost 5 VGPRs and a wave of occupancy)
    double tot[FE_SUMS];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int k = 0; k < 12; ++k) cell[g * 12 + k] = cnt[g][k];
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[g * 4 + k] = sum[g][k];
    }
    cell[24] = n_inv;
    wg_counts_to_table(cell, red_c, counts);
    wg_sums_to_slot(tot, red_s, slots);
}

}  // namespace

extern "C" int64_t vps_flow_error_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    return px4_slot_bytes(px4_groups((long)H * W), FE_SUMS);
}

extern "C" int vps_flow_error(const float* pred, int pred_ld, int pred_coff, const float* gt, int gt_ld, int gt_coff, const uint8_t* mask,
                              const uint8_t* occ_pred, int H, int W, int64_t* counts, double* sums, uint8_t* err_rgb, void* ws, int64_t ws_bytes,
                              void* stream) {
    if (!pred || !gt || !counts || !sums || !ws) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);           // a lane's uint32 counts cannot wrap
    if (pred_coff < 0 || pred_ld < pred_coff + 2 || gt_coff < 0 || gt_ld < gt_coff + 2) return VPS_EARG(3);
    if ((((uintptr_t)counts | (uintptr_t)sums) & 7) || (((uintptr_t)pred | (uintptr_t)gt) & 3)) return VPS_EARG(4);
    const long npix = (long)H * W, g = px4_groups(npix);
    if (((uintptr_t)ws & 7) || ws_bytes < px4_slot_bytes(g, FE_SUMS)) return VPS_EARG(5);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_error_kernel, dim3((unsigned)g), dim3(FE_THREADS), 0, s, pred, pred_ld, pred_coff, px4_flow_mode(pred, pred_ld, pred_coff), gt,
                       gt_ld, gt_coff, px4_flow_mode(gt, gt_ld, gt_coff), mask, occ_pred, npix, reinterpret_cast<unsigned long long*>(counts),
                       static_cast<double*>(ws), err_rgb);
    int st = vps_launch_status();
    if (st) return st;
    hipLaunchKernelGGL(slot_finish_kernel<FE_SUMS>, dim3(1), dim3(PX4_WG), 0, s, static_cast<const double*>(ws), (int)g, sums);
    return vps_launch_status();
}
