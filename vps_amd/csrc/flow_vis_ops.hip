// Optical-flow output (vps_amd/flowvis.py): the Middlebury colour coding of a flow field on the device.
//   vps_flow_max_radius  max over the frame of sqrt(u*u + v*v) -> device double [1] (the normaliser of the colour coding)
//   vps_flow_colour      flow + normaliser -> RGB uint8 [H][W][3], the image vis_flow(flow.astype(float64)) of the reference's
//                        flow_utils.py gives, level for level
// The flow is an NHWC map: pixel p has its two floats at flow[p * ld + coff]. FlowNet2's result has ld 4.
// Arithmetic: fp32 widened to fp64, then the reference's operations in the reference's order, every one rounded on its own. The whole
// file is compiled without contraction: floor(255 * col) sits on exact integers for zero flow, v = +-0 and radius 1, and a fused
// multiply-add moves those by an ulp to the wrong side. sqrt and / of doubles are correctly rounded on the
// device as in NumPy; atan2 may differ by an ulp or two, which moves no level (tests/flow_vis_restate.py with a perturbed arctan2).
// tests/flow_vis_restate.py is the NumPy twin.
#include "common.h"

#include <float.h>

#pragma clang fp contract(off)

namespace {

constexpr int NCOLS = 55;                     // RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
constexpr double UNKNOWN_FLOW_THRESH = 1e9;
constexpr double PI = 3.141592653589793;      // np.pi

// entry k of the colour wheel, 0..255 per channel: six linear ramps of floor(255 * j / N)
__device__ __forceinline__ void wheel_entry(int k, int& r, int& g, int& b) {
    if (k < 15) { r = 255; g = 255 * k / 15; b = 0; return; }
    k -= 15;
    if (k < 6) { r = 255 - 255 * k / 6; g = 255; b = 0; return; }
    k -= 6;
    if (k < 4) { r = 0; g = 255; b = 255 * k / 4; return; }
    k -= 4;
    if (k < 11) { r = 0; g = 255 - 255 * k / 11; b = 255; return; }
    k -= 11;
    if (k < 13) { r = 255 * k / 13; g = 0; b = 255; return; }
    k -= 13;
    r = 255; g = 0; b = 255 - 255 * k / 6;
}

__device__ __forceinline__ void load_uv(const float* __restrict__ flow, int ld, int coff, long p, double& u, double& v) {
    const float* q = flow + p * ld + coff;
    u = (double)q[0];
    v = (double)q[1];
    if (u > UNKNOWN_FLOW_THRESH || v > UNKNOWN_FLOW_THRESH) u = v = 0.0;
}

// Non-negative doubles order like their bit patterns: the blocks combine with one 64-bit unsigned atomic max. max sqrt(s) = sqrt(max s)
// (a correctly rounded sqrt is monotone), so threads keep the largest u*u + v*v and one lane per block takes the root.
__global__ __launch_bounds__(256)
void flow_max_radius_kernel(const float* __restrict__ flow, int ld, int coff, long npix, unsigned long long* __restrict__ out) {
    __shared__ double part[4];
    double m = 0.0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
        double u, v;
        load_uv(flow, ld, coff, p, u, v);
        m = fmax(m, u * u + v * v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
        atomicMax(out, (unsigned long long)__double_as_longlong(sqrt(m)));
    }
}

// A block colours 1024 consecutive pixels: in each of four steps lane l takes pixel (step * 256 + l) - adjacent lanes, adjacent pixels -
// and leaves its three bytes in LDS; then the 3072 bytes go out as 768 dwords, three per lane, adjacent lanes adjacent dwords. The
// image is dense, so a block's first byte, 3072 * blockIdx, is dword-aligned whenever the image is.
constexpr int PIX_PER_BLOCK = 1024;

__global__ __launch_bounds__(256)
void flow_colour_kernel(const float* __restrict__ flow, int ld, int coff, long npix, const double* __restrict__ max_rad,
                        uint8_t* __restrict__ rgb) {
    __shared__ double cw[NCOLS * 3];                                             // colorwheel / 255
    __shared__ __attribute__((aligned(16))) uint8_t px[PIX_PER_BLOCK * 3];
    if (threadIdx.x < NCOLS) {
        int c[3];
        wheel_entry(threadIdx.x, c[0], c[1], c[2]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) cw[threadIdx.x * 3 + ch] = (double)c[ch] / 255.0;
    }
    __syncthreads();
    const double den = max_rad[0] + DBL_EPSILON;
    const long base = (long)blockIdx.x * PIX_PER_BLOCK;
#pragma unroll 1
    for (int step = 0; step < PIX_PER_BLOCK / 256; ++step) {
        const int lp = step * 256 + threadIdx.x;
        const long p = base + lp;
        if (p >= npix) break;
        double u, v;
        load_uv(flow, ld, coff, p, u, v);
        u = u / den;
        v = v / den;
        const double radius = sqrt(u * u + v * v);
        const double a = atan2(-v, -u) / PI;
        const double fk = (a + 1.0) / 2.0 * (double)(NCOLS - 1);
        const int k0 = min(max((int)fk, 0), NCOLS - 1);                          // 0..54 (the clamp only matters for NaN flow)
        const int k1 = k0 + 1 == NCOLS ? 0 : k0 + 1;
        const double f = fk - (double)k0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double col = (1.0 - f) * cw[k0 * 3 + ch] + f * cw[k1 * 3 + ch];
            if (radius <= 1.0) col = 1.0 - radius * (1.0 - col);                 // saturation grows with the radius
            else col = col * 0.75;                                               // out of range
            px[lp * 3 + ch] = (uint8_t)(int)floor(255.0 * col);
        }
    }
    __syncthreads();
    const long left = npix - base;
    const int nbytes = (int)(left < PIX_PER_BLOCK ? left : PIX_PER_BLOCK) * 3;
    uint8_t* q = rgb + base * 3;
    const uint32_t* px4 = reinterpret_cast<const uint32_t*>(px);
#pragma unroll
    for (int j = 0; j < PIX_PER_BLOCK * 3 / 4 / 256; ++j) {
        const int w = j * 256 + threadIdx.x;
        if (w * 4 + 4 <= nbytes) {
            reinterpret_cast<uint32_t*>(q)[w] = px4[w];
        } else {
            for (int k = w * 4; k < nbytes; ++k) q[k] = px[k];                   // the last one to three bytes of the image
        }
    }
}

int check_flow(const float* flow, int ld, int coff, int H, int W) {
    if (!flow || H <= 0 || W <= 0) return VPS_EARG(1);
    if (ld < 2 || coff < 0 || coff + 2 > ld) return VPS_EARG(2);
    return 0;
}

}  // namespace

extern "C" int vps_flow_max_radius(const float* flow, int ld, int coff, int H, int W, double* out, void* stream) {
    const int st = check_flow(flow, ld, coff, H, W);
    if (st) return st;
    if (!out || ((uintptr_t)out & 7)) return VPS_EARG(3);
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return -(int)e;
    const long npix = (long)H * W;
    hipLaunchKernelGGL(flow_max_radius_kernel, dim3(stream_grid(npix, 256 * 4)), dim3(256), 0, (hipStream_t)stream, flow, ld, coff, npix,
                       reinterpret_cast<unsigned long long*>(out));
    return vps_launch_status();
}

extern "C" int vps_flow_colour(const float* flow, int ld, int coff, int H, int W, const double* max_rad, uint8_t* rgb, void* stream) {
    const int st = check_flow(flow, ld, coff, H, W);
    if (st) return st;
    if (!max_rad || ((uintptr_t)max_rad & 7)) return VPS_EARG(3);
    if (!rgb || ((uintptr_t)rgb & 3)) return VPS_EARG(4);
    const long npix = (long)H * W;
    hipLaunchKernelGGL(flow_colour_kernel, dim3(cdiv(npix, PIX_PER_BLOCK)), dim3(256), 0, (hipStream_t)stream, flow, ld, coff, npix, max_rad, rgb);
    return vps_launch_status();
}
