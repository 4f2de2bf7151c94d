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
// No index is formed from a float before the in-view test has passed, and every corner address of `prev` is clamped to the map: NaN,
// inf and 1e30 flows read nothing outside it.
// The gather: the four corners of a pixel are 3 bytes each at addresses that are 0..3 bytes off a dword boundary (3 bytes per pixel),
// and the corner pairs of the lanes of a wavefront overlap each other wherever the flow is smooth, so they come from the cache lines
// the neighbouring lanes have just touched. They are read as byte loads: a dword (or the 6 contiguous bytes of a corner pair) would
// need a condition per corner for the map's last bytes and a per-lane shift, for loads that hit the vector cache either way. The
// streamed operands (cur, prev(p), flow, the mask bytes) go through px4.h as dwords.
#include "px4.h"

#pragma clang fp contract(off)

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_MAX_GROUPS = 1024;                   // workgroups of the counting launch = slots of the workspace (4 per CU, then grid-stride)
constexpr int FP_CELLS = 21, FP_SUMS = 4;

long fp_groups(long npix) {
    const long nchunk = (npix + PX4 - 1) / PX4;
    long g = (nchunk + FP_THREADS - 1) / FP_THREADS;
    return g > FP_MAX_GROUPS ? FP_MAX_GROUPS : g;
}

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
// squares: a lane's share of 2^31 pixels would still fit 32 bits, the sum over a wavefront would not). At the end they are summed
// across the wavefront by xor shuffles (a fixed tree) and across the four wavefronts in LDS in a fixed order. The counts leave as one 64-bit atomic per non-zero cell, the sums as the
// workgroup's own slot of `slots` (always written, zeros too: the finishing launch reads every slot). mask_in and mask_out may be the
// same buffer: a lane reads its own four bytes before it writes them, and no lane reads what another one writes.
__global__ __launch_bounds__(FP_THREADS)
void flow_photo_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int H, int W, const float* __restrict__ flow, int fld, int fcoff,
                       int fmode, const uint8_t* mask_in, double thr, unsigned long long* __restrict__ counts, double* __restrict__ slots,
                       uint8_t* mask_out, uint8_t* __restrict__ residual) {
    __shared__ unsigned long long red_c[FP_THREADS / 64][FP_CELLS];
    __shared__ double red_s[FP_THREADS / 64][FP_SUMS];
    const long npix = (long)H * W, nchunk = (npix + PX4 - 1) / PX4;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const bool mout4 = mask_out && ((uintptr_t)mask_out & 3) == 0, res4 = residual && ((uintptr_t)residual & 3) == 0;
    uint32_t cnt[2][8], n_out = 0;                    // n, flagged, e > 4 / 8 / 16 / 32, helped, hurt
    unsigned long long stat[2][2];                    // sum of as, sum of qs
    double sum[2][2];                                 // sum of aw, sum of qw
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cnt[g][k] = 0;
        stat[g][0] = stat[g][1] = 0;
        sum[g][0] = sum[g][1] = 0.0;
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
            // ---- the definition, in its order
            const float sx = (float)x + u[i], sy = (float)y + v[i];
            const float qx = floorf(sx + 0.5f), qy = floorf(sy + 0.5f);
            const bool in = qx >= 0.f && qx <= xmax && qy >= 0.f && qy <= ymax;    // as floats: NaN, +-inf, 1e30 fall out here
            const uint32_t m = (M >> (8 * i)) & 0xffu;
            uint32_t code = 2, res = 0;
            if (in) {
                const float x0 = floorf(sx), y0 = floorf(sy);                      // -1 .. W-1 resp. -1 .. H-1 once in view
                const float wx = sx - x0, wy = sy - y0;
                const float x1 = x0 + 1.f, y1 = y0 + 1.f;
                const int ix0 = min(max((int)x0, 0), W - 1), ix1 = min(max((int)x1, 0), W - 1);
                const int iy0 = min(max((int)y0, 0), H - 1), iy1 = min(max((int)y1, 0), H - 1);
                float b00[3], b01[3], b10[3], b11[3];
                fp_corner(prev, W, iy0, ix0, b00); fp_corner(prev, W, iy0, ix1, b01);
                fp_corner(prev, W, iy1, ix0, b10); fp_corner(prev, W, iy1, ix1, b11);
                double aw = 0.0, qw = 0.0;
                int as = 0, qs = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = b00[c] + wx * (b01[c] - b00[c]), bot = b10[c] + wx * (b11[c] - b10[c]);
                    const float s = top + wy * (bot - top);
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
                    sum[g][0] += mine ? aw : 0.0;
                    sum[g][1] += mine ? qw : 0.0;
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        // the cells of group g in the order of the table: n, flagged, sum as, sum qs, the four thresholds, helped, hurt
        unsigned long long cell[10] = {cnt[g][0], cnt[g][1], stat[g][0], stat[g][1], cnt[g][2], cnt[g][3], cnt[g][4], cnt[g][5], cnt[g][6], cnt[g][7]};
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const unsigned long long c = wave_sum(cell[k]);
            if (lane == 0) red_c[wave][g * 10 + k] = c;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double s = wave_sum(sum[g][k]);                                     // s(l) + s(l ^ off): the same tree in every lane
            if (lane == 0) red_s[wave][g * 2 + k] = s;
        }
    }
    n_out = wave_sum(n_out);
    if (lane == 0) red_c[wave][20] = n_out;
    __syncthreads();
    if (threadIdx.x < FP_CELLS) {
        unsigned long long c = 0;
        for (int w = 0; w < FP_THREADS / 64; ++w) c += red_c[w][threadIdx.x];
        if (c) atomicAdd(&counts[threadIdx.x], c);
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + FP_SUMS) {
        const int k = threadIdx.x - 64;
        slots[(long)blockIdx.x * FP_SUMS + k] = (red_s[0][k] + red_s[1][k]) + (red_s[2][k] + red_s[3][k]);
    }
}

// ONE workgroup: lane t owns cell t & 3 and adds the slots t >> 2, t >> 2 + 64, ... in ascending order; the 64 lanes of a cell are then
// summed in a fixed tree (xor shuffles over 4, 8, 16, 32, then the four wavefronts in order) and the four totals are added to `sums`.
__global__ __launch_bounds__(FP_THREADS)
void flow_photo_finish_kernel(const double* __restrict__ slots, int nslots, double* __restrict__ sums) {
    __shared__ double part[FP_THREADS / 64][FP_SUMS];
    const int k = threadIdx.x & 3;
    double s = 0.0;
    for (int j = threadIdx.x >> 2; j < nslots; j += FP_THREADS / FP_SUMS) s += slots[(long)j * FP_SUMS + k];
    for (int off = 4; off <= 32; off <<= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) < FP_SUMS) part[threadIdx.x >> 6][k] = s;
    __syncthreads();
    if (threadIdx.x < FP_SUMS) sums[k] = sums[k] + ((part[0][k] + part[1][k]) + (part[2][k] + part[3][k]));
}

}  // namespace

extern "C" int64_t vps_flow_photo_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    return (int64_t)(fp_groups((long)H * W) * FP_SUMS * sizeof(double));
}

extern "C" int vps_flow_photo(const uint8_t* cur_bgr, const uint8_t* prev_bgr, int H, int W, const float* flow, int flow_ld, int flow_coff,
                              const uint8_t* mask_in, float thr, int64_t* counts, double* sums, uint8_t* mask_out, uint8_t* residual, void* ws,
                              int64_t ws_bytes, void* stream) {
    if (!cur_bgr || !prev_bgr || !flow || !counts || !sums || !ws) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);           // a lane's uint32 counts cannot wrap
    if (flow_coff < 0 || flow_ld < flow_coff + 2) return VPS_EARG(3);
    if ((((uintptr_t)counts | (uintptr_t)sums) & 7) || ((uintptr_t)flow & 3)) return VPS_EARG(4);
    const long npix = (long)H * W, g = fp_groups(npix);
    if (((uintptr_t)ws & 7) || ws_bytes < (int64_t)(g * FP_SUMS * sizeof(double))) return VPS_EARG(5);
    if (!(thr >= 0.f)) return VPS_EARG(6);                                          // negative or NaN
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(flow_photo_kernel, dim3((unsigned)g), dim3(FP_THREADS), 0, s, cur_bgr, prev_bgr, H, W, flow, flow_ld, flow_coff,
                       px4_flow_mode(flow, flow_ld, flow_coff), mask_in, (double)thr, reinterpret_cast<unsigned long long*>(counts),
                       static_cast<double*>(ws), mask_out, residual);
    int st = vps_launch_status();
    if (st) return st;
    hipLaunchKernelGGL(flow_photo_finish_kernel, dim3(1), dim3(FP_THREADS), 0, s, static_cast<const double*>(ws), (int)g, sums);
    return vps_launch_status();
}
