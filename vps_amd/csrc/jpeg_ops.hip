// Device half of the JPEG input path: quantised coefficients (jpeg_host.cpp) -> BGR uint8 [H][W][3], the frame
// `cv2.imread` / PIL deliver. Every step is the integer arithmetic libjpeg's default decode defines, restated from the published
// algorithms of jidctint.c (slow-integer IDCT), jdsample.c (fancy upsampling) and jdcolor.c (fixed-point YCbCr -> RGB), so the result
// is bit-exact with it:
//   kernel 1  dequantise + 8x8 IDCT of every block of every component -> sample planes (uint8, padded to whole MCUs) in the workspace
//   kernel 2  chroma upsampling (edges replicated at the TRUE down-sampled size, not at the MCU padding) + colour + interleaved store
// Both are HBM-bound streaming kernels (12.5 MB of algorithmic traffic at 1080x1920 4:2:0); the planes add one 3 MB round trip that
// stays in the Infinity Cache. Nothing here is on the model's critical path.
#include "common.h"

namespace {

struct JpegGeom {
    int H, W, nc;
    int hs, vs;                   // luma sampling factors (chroma is 1x1)
    int brows[3], bcols[3];       // block grid per component
    int nblk[3];                  // blocks per component
    long plane[3];                // byte offset of a component's sample plane in the workspace
};

constexpr int CB = 13, P1 = 2;    // CONST_BITS, PASS1_BITS
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

// one 8-point pass of jpeg_idct_islow: in[0..7] -> out[0..7] descaled by `shift` (DESCALE rounds half up on an arithmetic shift)
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * F_0_541196100;
    int tmp2 = z1 + z3 * (-F_1_847759065);
    int tmp3 = z1 + z2 * F_0_765366865;
    z2 = in[0]; z3 = in[4];
    int tmp0 = (z2 + z3) * (1 << CB);
    int tmp1 = (z2 - z3) * (1 << CB);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int r = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + r) >> shift; out[7] = (tmp10 - tmp3 + r) >> shift;
    out[1] = (tmp11 + tmp2 + r) >> shift; out[6] = (tmp11 - tmp2 + r) >> shift;
    out[2] = (tmp12 + tmp1 + r) >> shift; out[5] = (tmp12 - tmp1 + r) >> shift;
    out[3] = (tmp13 + tmp0 + r) >> shift; out[4] = (tmp13 - tmp0 + r) >> shift;
}

// the IDCT's range limit: the table libjpeg indexes with `x & 1023` holds x + 128 clamped to 0..255 for the 10-bit two's complement
// value of x, i.e. values beyond +-512 wrap before they are clamped
__device__ __forceinline__ int range_limit(int x) {
    const int s = ((x + 512) & 1023) - 512 + 128;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// Eight lanes hold one block (a wavefront works on 8 blocks, a workgroup on 32). Lane j loads row j of the coefficients (one 16-byte
// load; the wave reads 1 KiB contiguous), dequantises it into LDS; pass 1 reads COLUMN j, pass 2 reads ROW j of its results. A block is
// 64 words + 8 of padding: the column reads of the four blocks of a 32-lane group then fall on four different 8-bank groups.
constexpr int BLK_LD = 72;

__global__ __launch_bounds__(256)
void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, JpegGeom g, int total, uint8_t* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) int lds[32 * BLK_LD];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int blk = blockIdx.x * 32 + lb;
    const bool live = blk < total;
    int* t = lds + lb * BLK_LD;
    int c = 0, local = blk;
    if (live) {
        if (local >= g.nblk[0]) { local -= g.nblk[0]; c = 1; }
        if (c == 1 && local >= g.nblk[1]) { local -= g.nblk[1]; c = 2; }
        const int4 cv = *reinterpret_cast<const int4*>(coef + (size_t)blk * 64 + j * 8);
        const int4 qv = *reinterpret_cast<const int4*>(qt + c * 64 + j * 8);
        const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
        int d[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[2 * k] = (int)(int16_t)(cw[k] & 0xFFFF) * (qw[k] & 0xFFFF);
            d[2 * k + 1] = (cw[k] >> 16) * (int)((unsigned)qw[k] >> 16);
        }
        *reinterpret_cast<int4*>(t + j * 8) = make_int4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<int4*>(t + j * 8 + 4) = make_int4(d[4], d[5], d[6], d[7]);
    }
    __syncthreads();
    if (live) {
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = t[r * 8 + j];
        idct8(in, out, CB - P1);
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r * 8 + j] = out[r];                       // its own column: no other lane touches it in this pass
    }
    __syncthreads();
    if (live) {
        const int4 a = *reinterpret_cast<const int4*>(t + j * 8), b = *reinterpret_cast<const int4*>(t + j * 8 + 4);
        const int in[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        int out[8];
        idct8(in, out, CB + P1 + 3);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)range_limit(out[k]) << (8 * k);
            hi |= (uint32_t)range_limit(out[4 + k]) << (8 * k);
        }
        const int by = local / g.bcols[c], bx = local - by * g.bcols[c];
        const size_t pitch = (size_t)g.bcols[c] * 8;
        *reinterpret_cast<uint2*>(ws + g.plane[c] + ((size_t)by * 8 + j) * pitch + (size_t)bx * 8) = make_uint2(lo, hi);
    }
}

constexpr int SCALEBITS = 16, ONE_HALF = 1 << 15;
constexpr int FIX_1_40200 = 91881, FIX_1_77200 = 116130, FIX_0_34414 = 22554, FIX_0_71414 = 46802;

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one thread = four horizontally adjacent pixels of a row (x0 a multiple of 4): 12 output bytes
__global__ __launch_bounds__(256)
void jpeg_colour_kernel(const uint8_t* __restrict__ ws, JpegGeom g, int quads_per_row, long total, uint8_t* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int y = (int)(idx / quads_per_row), x0 = (int)(idx - (long)y * quads_per_row) * 4;
    const int H = g.H, W = g.W;
    const int py = g.bcols[0] * 8;
    const uint8_t* yrow = ws + g.plane[0] + (size_t)y * py;
    const uint32_t yv = *reinterpret_cast<const uint32_t*>(yrow + x0);           // the padded plane is a multiple of 8 wide
    int cb[4], cr[4];
    if (g.nc == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cb[k] = cr[k] = 128;
    } else {
        const int pc = g.bcols[1] * 8;
        const uint8_t* p1 = ws + g.plane[1];
        const uint8_t* p2 = ws + g.plane[2];
        if (g.hs == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = min(x0 + k, W - 1);
                cb[k] = p1[(size_t)y * pc + x]; cr[k] = p2[(size_t)y * pc + x];
            }
        } else {
            const int cw = (W + 1) >> 1, ch = g.vs == 2 ? (H + 1) >> 1 : H;
            // libjpeg picks the triangle filter only for a down-sampled width above 2; narrower planes are replicated (box filter),
            // in both directions
            const bool fancy = cw > 2;
            const int i0 = x0 >> 1;                                              // chroma columns i0 - 1 .. i0 + 2 serve the four pixels
            const int xs[4] = {max(i0 - 1, 0), min(i0, cw - 1), min(i0 + 1, cw - 1), min(i0 + 2, cw - 1)};
            int sb[4], sr[4];                                                    // column sums: 3 * near + far row (h2v2), or the sample (h2v1)
            if (g.vs == 2) {
                const int r = y >> 1;
                const int fr = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int nb = p1[(size_t)r * pc + xs[k]], nr = p2[(size_t)r * pc + xs[k]];
                    if (fancy) {
                        sb[k] = 3 * nb + p1[(size_t)fr * pc + xs[k]];
                        sr[k] = 3 * nr + p2[(size_t)fr * pc + xs[k]];
                    } else {
                        sb[k] = nb; sr[k] = nr;
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { sb[k] = p1[(size_t)y * pc + xs[k]]; sr[k] = p2[(size_t)y * pc + xs[k]]; }
            }
            if (!fancy) {
                cb[0] = cb[1] = sb[1]; cb[2] = cb[3] = sb[2];
                cr[0] = cr[1] = sr[1]; cr[2] = cr[3] = sr[2];
            } else if (g.vs == 2) {                                              // h2v2: (3 * this + neighbour + 8 | 7) >> 4
                cb[0] = (3 * sb[1] + sb[0] + 8) >> 4; cb[1] = (3 * sb[1] + sb[2] + 7) >> 4;
                cb[2] = (3 * sb[2] + sb[1] + 8) >> 4; cb[3] = (3 * sb[2] + sb[3] + 7) >> 4;
                cr[0] = (3 * sr[1] + sr[0] + 8) >> 4; cr[1] = (3 * sr[1] + sr[2] + 7) >> 4;
                cr[2] = (3 * sr[2] + sr[1] + 8) >> 4; cr[3] = (3 * sr[2] + sr[3] + 7) >> 4;
            } else {                                                             // h2v1: (3 * this + neighbour + 1 | 2) >> 2
                cb[0] = (3 * sb[1] + sb[0] + 1) >> 2; cb[1] = (3 * sb[1] + sb[2] + 2) >> 2;
                cb[2] = (3 * sb[2] + sb[1] + 1) >> 2; cb[3] = (3 * sb[2] + sb[3] + 2) >> 2;
                cr[0] = (3 * sr[1] + sr[0] + 1) >> 2; cr[1] = (3 * sr[1] + sr[2] + 2) >> 2;
                cr[2] = (3 * sr[2] + sr[1] + 1) >> 2; cr[3] = (3 * sr[2] + sr[3] + 2) >> 2;
            }
        }
    }
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int Y = (int)((yv >> (8 * k)) & 255);
        if (g.nc == 1) {
            px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (uint8_t)Y;
        } else {
            const int u = cb[k] - 128, v = cr[k] - 128;
            px[3 * k + 0] = (uint8_t)clamp8(Y + ((FIX_1_77200 * u + ONE_HALF) >> SCALEBITS));
            px[3 * k + 1] = (uint8_t)clamp8(Y + ((-FIX_0_34414 * u - FIX_0_71414 * v + ONE_HALF) >> SCALEBITS));
            px[3 * k + 2] = (uint8_t)clamp8(Y + ((FIX_1_40200 * v + ONE_HALF) >> SCALEBITS));
        }
    }
    uint8_t* o = out + ((size_t)y * W + x0) * 3;
    if ((W & 3) == 0) {                                                          // rows start 4-byte aligned and every quad is whole
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        const int n = min(4, W - x0) * 3;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < n) o[k] = px[k];
    }
}

}  // namespace

extern "C" int vps_jpeg_reconstruct(const int16_t* coef, const uint16_t* qt, int H, int W, int ncomp, const int32_t* samp, const int32_t* grid,
                                    uint8_t* ws, int64_t ws_bytes, uint8_t* out, void* stream) {
    if (!coef || !qt || !samp || !grid || !ws || !out || H <= 0 || W <= 0 || H > 65535 || W > 65535) return VPS_EARG(1);
    if (ncomp != 1 && ncomp != 3) return VPS_EARG(2);
    if (((uintptr_t)coef & 15) || ((uintptr_t)qt & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)out & 3)) return VPS_EARG(3);
    JpegGeom g;
    g.H = H; g.W = W; g.nc = ncomp;
    g.hs = ncomp == 1 ? 1 : samp[0]; g.vs = ncomp == 1 ? 1 : samp[1];
    if (!((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2))) return VPS_EARG(4);
    if (ncomp == 3 && (samp[2] != 1 || samp[3] != 1 || samp[4] != 1 || samp[5] != 1)) return VPS_EARG(4);
    // the block grids must be the ones the image size implies: the kernels index the planes by them
    const int mcu_rows = (H + 8 * g.vs - 1) / (8 * g.vs), mcu_cols = (W + 8 * g.hs - 1) / (8 * g.hs);
    long total = 0, off = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < ncomp;
        g.brows[c] = on ? mcu_rows * (c == 0 ? g.vs : 1) : 0;
        g.bcols[c] = on ? mcu_cols * (c == 0 ? g.hs : 1) : 0;
        if (on && (grid[2 * c] != g.brows[c] || grid[2 * c + 1] != g.bcols[c])) return VPS_EARG(5);
        g.nblk[c] = g.brows[c] * g.bcols[c];
        g.plane[c] = off;
        off += (long)g.nblk[c] * 64;
        total += g.nblk[c];
    }
    if (ws_bytes < off) return VPS_EARG(6);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(total, 32)), dim3(256), 0, (hipStream_t)stream, coef, qt, g, (int)total, ws);
    const int quads = (W + 3) / 4;
    const long items = (long)H * quads;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)ws, g, quads, items, out);
    return vps_launch_status();
}
