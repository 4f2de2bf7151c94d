// Flow quality without ground truth (vps_amd/flowphoto.py): the photometric warp error of a flow between the two
// frames it was computed from - the previous frame sampled at p + flow(p) against the current frame, beside the "static" error of not
// warping at all.
//   vps_flow_photo_ws_bytes  host arithmetic: four doubles per workgroup of the counting launch
//   vps_flow_photo           one (cur, prev, flow) triple: every pixel is ADDED to the caller's int64 [21] counts and double [2][2] sums;
//                            optionally the mask with the flagged pixels (code 3) and the residual image are written in the same launch.
//                            Nothing is zeroed, downloaded or synchronised.
// Arithmetic: the in-view rule and the bilinear sample in fp32, the errors in fp64, the operations of the definition (include/vps_hip.h)
// in its order, every one rounded on its own - the whole file is compiled without contraction, so that every decision (flagged, the four
// thresholds, helped / hurt, the rounded residual) equals the NumPy restatement (tests/flow_photo_restate.py). The static error is exact
// integer arithmetic on the bytes.
// Determinism: integer atomics for the counts; the sums never meet a floating-point atomic - fixed trees and one slot per workgroup.
// The in-view test, the corners and the sample are warp_rule.h, the one implementation: NaN, inf and 1e30 flows read nothing outside `prev`.
// The gather: the four corners of a pixel are 3 bytes each at addresses that are 0..3 bytes off a dword boundary (3 bytes per pixel),
// and the corner pairs of the lanes of a wavefront overlap each other wherever the flow is smooth, so they come from the cache lines
// the neighbouring lanes have just touched. They are read as byte loads: a dword (or the 6 contiguous bytes of a corner pair) would
// need a condition per corner for the map's last bytes and a per-lane shift, for loads that hit the vector cache either way. The
// streamed operands (cur, prev(p), flow, the mask bytes) go through px4.h as dwords.
#include "px4.h"
#include "warp_rule.h"

#pragma clang fp contract(off)

namespace {

constexpr int FP_THREADS = PX4_WG;
constexpr int FP_CELLS = 21, FP_SUMS = 4;

// the three bytes of pixel (iy, ix) of a [H][W][3] byte map as floats; iy and ix are inside the map
__device__ __forceinline__ void fp_corner(const uint8_t* __restrict__ prev, int W, int iy, int ix, float (&b)[3]) {
    const uint8_t* a = prev + 3 * ((long)iy * W + ix);
    b[0] = (float)a[0]; b[1] = (float)a[1]; b[2] = (float)a[2];
}

__device__ __forceinline__ int fp_absdiff(uint32_t a, uint32_t b) {
    const int d = (int)a - (int)b;
    return d < 0 ? -d : d;
}

// A lane owns 4 consecutive pixels of cur (linear index, a chunk may run over the end of a row) per step; a workgroup strides over the
// chunks. The counters and the four sums of a lane stay in registers under constant indices. Pixel counters are uint32 (H W < 2^31);
// the two integer sums of the static error are 64-bit in every lane and through the reduction (one pixel adds up to 3 * 255^2 to the
// squares: a lane's share of 2^31 pixels would still fit 32 bits, the sum over a wavefront would not). They leave through Part C of
// px4.h, with 64-bit LDS rows for the counts: one 64-bit atomic per non-zero cell, the sums as the workgroup's own slot of `slots`.
// mask_in and mask_out may be the same buffer: a lane reads its own four bytes before it writes them, and no lane reads what another
// one writes.
__global__ __launch_bounds__(FP_THREADS)
void flow_photo_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int H, int W, const float* __restrict__ flow, int fld, int fcoff,
                       int fmode, const uint8_t* mask_in, double thr, unsigned long long* __restrict__ counts, double* __restrict__ slots,
                       uint8_t* mask_out, uint8_t* __restrict__ residual) {
    __shared__ unsigned long long red_c[FP_THREADS / 64][FP_CELLS];
    __shared__ double red_s[FP_THREADS / 64][FP_SUMS];
    const long npix = (long)H * W, nchunk = (npix + PX4 - 1) / PX4;
    const bool mout4 = mask_out && ((uintptr_t)mask_out & 3) == 0, res4 = residual && ((uintptr_t)residual & 3) == 0;
    uint32_t cnt[2][8], n_out = 0;                    // n, flagged, e > 4 / 8 / 16 / 32, helped, hurt
    unsigned long long stat[2][2];                    // sum of as, sum of qs
    double sum[FP_SUMS];                              // per group: sum of aw, sum of qw
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt[g][k] = 0;
        stat[g][0] = stat[g][1] = 0;
        sum[2 * g] = sum[2 * g + 1] = 0.0;
    }
    for (long ch = (long)blockIdx.x * FP_THREADS + threadIdx.x; ch < nchunk; ch += (long)gridDim.x * FP_THREADS) {
        const long p0 = PX4 * ch;
        const int n = (int)min((long)PX4, npix - p0);
        float u[PX4], v[PX4];
        uint32_t c4[PX4], s4[PX4];
        px4_load_flow(flow, fld, fcoff, fmode, p0, n, u, v);
        px4_load_px3(cur, 3 * npix, ch, n, c4);
        px4_load_px3(prev, 3 * npix, ch, n, s4);
        const uint32_t M = mask_in ? px4_load_bytes(mask_in, npix, p0, n) : 0u;
        int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
        uint32_t codes = 0, resid = 0;
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            if (i >= n) break;
            // ---- the definition, in its order (warp_rule.h: in view, corners, sample)
            const float sx = warp_pos(x, u[i]), sy = warp_pos(y, v[i]);
            const uint32_t m = (M >> (8 * i)) & 0xffu;
            uint32_t code = 2, res = 0;
            if (warp_in_view(sx, sy, W, H)) {
                const WarpCorners k = warp_corners(sx, sy, W, H);
                float b00[3], b01[3], b10[3], b11[3];
                fp_corner(prev, W, k.y0, k.x0, b00); fp_corner(prev, W, k.y0, k.x1, b01);
                fp_corner(prev, W, k.y1, k.x0, b10); fp_corner(prev, W, k.y1, k.x1, b11);
                double aw = 0.0, qw = 0.0;
                int as = 0, qs = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float s = warp_lerp2(b00[c], b01[c], b10[c], b11[c], k.wx, k.wy);
                    const uint32_t cc = (c4[i] >> (8 * c)) & 0xffu, pc = (s4[i] >> (8 * c)) & 0xffu;
                    const double dw = (double)s - (double)cc;
                    // (|dw_0| + |dw_1|) + |dw_2| and (dw_0^2 + dw_1^2) + dw_2^2: 0.0 + a is a for the non-negative first term
                    aw = c ? aw + fabs(dw) : fabs(dw);
                    qw = c ? qw + dw * dw : dw * dw;
                    const int d = fp_absdiff(pc, cc);
                    as += d; qs += d * d;
                }
                const double e = aw / 3.0;
                const bool flagged = e > thr;
                const bool helped = aw < (double)as, hurt = aw > (double)as;
                code = m ? m : (flagged ? 3u : 0u);
                res = (uint32_t)min(255, (int)floor(e + 0.5));
#pragma unroll
                for (int g = 0; g < 2; ++g) {         // constant indices: the tables stay in registers
                    const bool mine = (m != 0) == (g == 1);
                    cnt[g][0] += mine;             cnt[g][1] += mine && flagged;
                    cnt[g][2] += mine && e > 4.0;  cnt[g][3] += mine && e > 8.0;  cnt[g][4] += mine && e > 16.0;  cnt[g][5] += mine && e > 32.0;
                    cnt[g][6] += mine && helped;   cnt[g][7] += mine && hurt;
                    stat[g][0] += mine ? (unsigned long long)as : 0ull;
                    stat[g][1] += mine ? (unsigned long long)qs : 0ull;
                    sum[2 * g] += mine ? aw : 0.0;
                    sum[2 * g + 1] += mine ? qw : 0.0;
                }
            } else {
                ++n_out;
            }
            codes |= code << (8 * i);
            resid |= res << (8 * i);
            if (++x == W) { x = 0; ++y; }
        }
        if (mask_out) px4_store_bytes(mask_out, mout4, p0, n, codes);
        if (residual) px4_store_bytes(residual, res4, p0, n, resid);
    }
    // the cells in the order of the table: per group n, flagged, sum as, sum qs, the four thresholds, helped, hurt; then outside
    const unsigned long long cell[FP_CELLS] = {
        cnt[0][0], cnt[0][1], stat[0][0], stat[0][1], cnt[0][2], cnt[0][3], cnt[0][4], cnt[0][5], cnt[0][6], cnt[0][7],
        cnt[1][0], cnt[1][1], stat[1][0], stat[1][1], cnt[1][2], cnt[1][3], cnt[1][4], cnt[1][5], cnt[1][6], cnt[1][7], n_out};
    wg_counts_to_table(cell, red_c, counts);
    wg_sums_to_slot(sum, red_s, slots);
}

}  // namespace

extern "C" int64_t vps_flow_photo_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    return px4_slot_bytes(px4_groups((long)H * W), FP_SUMS);
}

extern "C" int vps_flow_photo(const uint8_t* cur_bgr, const uint8_t* prev_bgr, int H, int W, const float* flow, int flow_ld, int flow_coff,
                              const uint8_t* mask_in, float thr, int64_t* counts, double* sums, uint8_t* mask_out, uint8_t* residual, void* ws,
                              int64_t ws_bytes, void* stream) {
    if (!cur_bgr || !prev_bgr || !flow || !counts || !sums || !ws) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);           // a lane's uint32 counts cannot wrap
    if (flow_coff < 0 || flow_ld < flow_coff + 2) return VPS_EARG(3);
    if ((((uintptr_t)counts | (uintptr_t)sums) & 7) || ((uintptr_t)flow & 3)) return VPS_EARG(4);
    const long npix = (long)H * W, g = px4_groups(npix);
    if (((uintptr_t)ws & 7) || ws_bytes < px4_slot_bytes(g, FP_SUMS)) return VPS_EARG(5);
    if (!(thr >= 0.f)) return VPS_EARG(6);                                          // negative or NaN
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_photo_kernel, dim3((unsigned)g), dim3(FP_THREADS), 0, s, cur_bgr, prev_bgr, H, W, flow, flow_ld, flow_coff,
                       px4_flow_mode(flow, flow_ld, flow_coff), mask_in, (double)thr, reinterpret_cast<unsigned long long*>(counts),
                       static_cast<double*>(ws), mask_out, residual);
    int st = vps_launch_status();
    if (st) return st;
    hipLaunchKernelGGL(slot_finish_kernel<FP_SUMS>, dim3(1), dim3(PX4_WG), 0, s, static_cast<const double*>(ws), (int)g, sums);
    return vps_launch_status();
}
