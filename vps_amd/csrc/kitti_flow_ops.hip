// KITTI flow files, output half (include/vps_hip.h, vps_kitti_flow_encode; the input half is kitti_wave_kernel in png_in_ops.hip): an
// fp32 NHWC flow -> the bytes of the 16-bit RGB image that vps_png_deflate_bpp (bpp 6) filters and deflates. The coding is restated from
// memory of the KITTI devkit's io_flow.h:
//   R = (uint16) max(min(u * 64.0f + 32768.0f, 65535.0f), 0.0f), G likewise from v (fp32, the cast truncates behind the clamp),
//   B = 1 where valid, 0 otherwise; samples big-endian in the order R, G, B.
// This repository's own rule: a pixel whose u or v is NaN or +-inf is written invalid, R = G = B = 0.
// The image is dense, so pixel p owns bytes 6p .. 6p + 5 whatever the row: a thread codes two neighbouring pixels into three aligned dwords.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t kitti_code(float f) {
    const float q = __fadd_rn(__fmul_rn(f, 64.0f), 32768.0f);           // (no contraction: the product is exact anyway)
    return (uint32_t)fmaxf(fminf(q, 65535.0f), 0.0f);
}

// -> the six bytes of a pixel in file order, byte k at bits 8k
__device__ __forceinline__ uint64_t kitti_pixel(const float* __restrict__ flow, int ld, int coff, const uint8_t* __restrict__ valid, int64_t p,
                                                bool pair) {
    float u, v;
    const float* f = flow + p * ld + coff;
    if (pair) {
        const float2 t = *reinterpret_cast<const float2*>(f);
        u = t.x; v = t.y;
    } else {
        u = f[0]; v = f[1];
    }
    const bool finite = fabsf(u) <= 3.402823466e+38f && fabsf(v) <= 3.402823466e+38f;     // false for NaN and +-inf
    if (!finite) return 0ull;
    const uint32_t R = kitti_code(u), G = kitti_code(v), B = (!valid || valid[p]) ? 1u : 0u;
    return (uint64_t)(R >> 8) | ((uint64_t)(R & 255u) << 8) | ((uint64_t)(G >> 8) << 16) | ((uint64_t)(G & 255u) << 24) | ((uint64_t)B << 40);
}

__global__ __launch_bounds__(256) void kitti_encode_kernel(const float* __restrict__ flow, int ld, int coff, const uint8_t* __restrict__ valid,
                                                           int64_t npix, int pair, uint8_t* __restrict__ img16) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = 2 * t;
    if (p >= npix) return;
    const uint64_t a = kitti_pixel(flow, ld, coff, valid, p, pair != 0);
    uint32_t* o = reinterpret_cast<uint32_t*>(img16 + 6 * p);            // 12 t bytes behind a 4-byte aligned base
    if (p + 1 < npix) {
        const uint64_t b = kitti_pixel(flow, ld, coff, valid, p + 1, pair != 0);
        o[0] = (uint32_t)a;
        o[1] = (uint32_t)(a >> 32) | ((uint32_t)b << 16);
        o[2] = (uint32_t)(b >> 16);
    } else {                                                             // the last pixel of an odd count: six bytes, no more
        o[0] = (uint32_t)a;
        reinterpret_cast<uint16_t*>(o + 1)[0] = (uint16_t)(a >> 32);
    }
}

}  // namespace

extern "C" int vps_kitti_flow_encode(const float* flow, int ld, int coff, const uint8_t* valid, int H, int W, uint8_t* img16, void* stream) {
    if (!flow || !img16) return VPS_EARG(1);
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535) return VPS_EARG(2);
    if (ld < 2 || coff < 0 || coff + 2 > ld) return VPS_EARG(3);
    if (((uintptr_t)flow & 3) || ((uintptr_t)img16 & 3)) return VPS_EARG(4);
    const int64_t npix = (int64_t)H * W;
    const int pair = (ld % 2 == 0 && ((uintptr_t)(flow + coff) & 7) == 0) ? 1 : 0;       // (u, v) of a pixel as one 8-byte load
    const int64_t blocks = ((npix + 1) / 2 + 255) / 256;
    hipLaunchKernelGGL(kitti_encode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flow, ld, coff, valid, npix, pair, img16);
    return vps_launch_status();
}
