// Y4M video in and out (vps_amd/y4m.py): planar YCbCr frames <-> BGR on the device.
//   vps_yuv_to_bgr  planar frame as it lies in a .y4m file -> BGR uint8 [H][W][3]: chroma up-sampled at the declared siting, colour matrix
//   vps_bgr_to_yuv  BGR uint8 rows -> planar frame: colour matrix per pixel, chroma reduced by the format's filter, one launch
// All integer (include/vps_hip.h states the arithmetic; the coefficients are yuv_tables.h), so tests/y4m_restate.py is compared for
// equality. Both kernels move a byte once: HBM-bound.
// Access pattern: a lane owns 4 (decode) or 8 (encode) neighbouring pixels of a row, a wave one row segment, so the lanes of a wave
// read and write neighbouring dwords. The planes of a frame sit at any byte offset (an odd W*H puts Cb on an odd address, every row
// of an odd-width plane starts on another phase), so plane bytes come from ALIGNED dword loads of the frame - which must itself be
// 4-byte aligned - joined by a funnel shift; the last, partial word of the frame is read byte by byte, nothing beyond frame_bytes.
// The 3-byte pixels are packed in registers to three dwords per lane; a row whose first byte is not dword-aligned (W not a multiple
// of 4, or a strided source) and the last lane of a ragged row take the byte path.
#include "common.h"
#include "yuv_tables.h"

#include <utility>

namespace {

using vps_yuv::Coef;

constexpr int DEC_ROWS = 4, DEC_COLS = 256;      // decode workgroup: 4 waves, each 64 lanes x 4 pixels of one row
constexpr int ENC_ROWS = 8, ENC_COLS = 512;      // encode workgroup: 4 waves, each 64 lanes x (8 pixels x 2 rows)

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// (sum >> 16) clamped to lo..hi, computed as clamp(sum, lo << 16, (hi << 16) | 0xffff) >> 16: the same value (the shift is monotone).
// Written shift-then-clamp, the compiler packs two results with v_ashr_pk_u8_i32, and the dword it built from that came back from the
// device with a non-zero third byte where red was 0.
__device__ __forceinline__ int level(int sum, int lo, int hi) { return clamp_int(sum, lo << 16, (hi << 16) | 0xffff) >> 16; }

// aligned word `a` of the frame; a word that reaches beyond `limit` bytes is put together from the bytes that exist (zeros behind them)
__device__ __forceinline__ uint32_t word_at(const uint8_t* __restrict__ base, long a, long limit) {
    if ((a + 1) * 4 <= limit) return reinterpret_cast<const uint32_t*>(base)[a];
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k) {
        const long o = a * 4 + k;
        if (o < limit) w |= (uint32_t)base[o] << (8 * k);
    }
    return w;
}

// the four bytes at base + off (off >= 0, any phase), first byte lowest
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ base, long off, long limit) {
    const long a = off >> 2;
    const int sh = (int)(off & 3) * 8;
    const uint32_t lo = word_at(base, a, limit);
    if (sh == 0) return lo;
    const uint32_t hi = word_at(base, a + 1, limit);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// Horizontal half of the chroma up-sampling for the lane's 4 pixels x0 .. x0 + 3 (x0 a multiple of 4) from the chroma row at `row`:
// h[k] = w0 s[i0] + w1 s[i1], weights summing to 4. HM 0: the axis is not sub-sampled; 1: centre-sited (3, 1); 2: co-sited (4, 0 / 2, 2).
template <int HM>
__device__ __forceinline__ void chroma_row(const uint8_t* __restrict__ frame, long limit, long row, int x0, int CW, int (&h)[4]) {
    if (HM == 0) {
        const uint32_t w = load4(frame, row + x0, limit);
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = 4 * (int)((w >> (8 * k)) & 255);
        return;
    }
    const int j0 = x0 >> 1;                                    // samples j0 - 1 .. j0 + 2, indices clamped to the row
    uint32_t w;
    if (j0 == 0) {
        w = load4(frame, row, limit);
        w = (w << 8) | (w & 255);
    } else {
        w = load4(frame, row + j0 - 1, limit);
    }
    int s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = (int)((w >> (8 * k)) & 255);
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (j0 - 1 + k > CW - 1) s[k] = s[k - 1];                // j0 <= CW - 1 whenever x0 < W
    if (HM == 1) {
        h[0] = 3 * s[1] + s[0];
        h[1] = 3 * s[1] + s[2];
        h[2] = 3 * s[2] + s[1];
        h[3] = 3 * s[2] + s[3];
    } else {
        h[0] = 4 * s[1];
        h[1] = 2 * s[1] + 2 * s[2];
        h[2] = 4 * s[2];
        h[3] = 2 * s[2] + 2 * s[3];
    }
}

template <int HM, bool VSUB, bool MONO>
__global__ __launch_bounds__(256)
void yuv_to_bgr_kernel(const uint8_t* __restrict__ frame, long limit, int H, int W, int CW, int CH, Coef c, uint8_t* __restrict__ out) {
    const int x0 = blockIdx.x * DEC_COLS + (threadIdx.x & 63) * 4;
    const int y = blockIdx.y * DEC_ROWS + (threadIdx.x >> 6);
    if (x0 >= W || y >= H) return;
    const uint32_t yw = load4(frame, (long)y * W + x0, limit);
    int cb[4], cr[4];
    if (MONO) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cb[k] = cr[k] = 128;
    } else {
        int r0 = y, r1 = y, w0 = 4, w1 = 0;
        if (VSUB) {                                            // centre-sited rows: the nearer sample 3, the farther 1
            r0 = y >> 1;
            r1 = (y & 1) ? min(r0 + 1, CH - 1) : max(r0 - 1, 0);
            w0 = 3; w1 = 1;
        }
        const long plane = (long)CW * CH;
        const long cb0 = (long)W * H;
        int a[4], b[4];
        chroma_row<HM>(frame, limit, cb0 + (long)r0 * CW, x0, CW, a);
        chroma_row<HM>(frame, limit, cb0 + plane + (long)r0 * CW, x0, CW, b);
        if (VSUB) {                                            // wave-uniform: a wave is one row
            int a1[4], b1[4];
            chroma_row<HM>(frame, limit, cb0 + (long)r1 * CW, x0, CW, a1);
            chroma_row<HM>(frame, limit, cb0 + plane + (long)r1 * CW, x0, CW, b1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cb[k] = (w0 * a[k] + w1 * a1[k] + 8) >> 4;
                cr[k] = (w0 * b[k] + w1 * b1[k] + 8) >> 4;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cb[k] = (4 * a[k] + 8) >> 4;
                cr[k] = (4 * b[k] + 8) >> 4;
            }
        }
    }
    uint32_t px[3] = {0, 0, 0};                                 // 4 pixels x (B, G, R), first byte lowest
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = c.ky * ((int)((yw >> (8 * k)) & 255) - c.yoff) + 32768;
        const int u = cb[k] - 128, v = cr[k] - 128;
        const int bgr[3] = {level(yy + c.cb_b * u, 0, 255), level(yy + c.cb_g * u + c.cr_g * v, 0, 255), level(yy + c.cr_r * v, 0, 255)};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int i = k * 3 + ch;
            px[i >> 2] |= (uint32_t)bgr[ch] << (8 * (i & 3));
        }
    }
    uint8_t* q = out + ((long)y * W + x0) * 3;
    if (x0 + 4 <= W && ((uintptr_t)q & 3) == 0) {
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = px[0]; q4[1] = px[1]; q4[2] = px[2];
    } else {
        const int n = min(4, W - x0) * 3;
        for (int i = 0; i < n; ++i) q[i] = (uint8_t)(px[i >> 2] >> (8 * (i & 3)));
    }
}

__device__ __forceinline__ void encode_pixel(const Coef& c, int b, int g, int r, int& y, int& cb, int& cr) {
    y = level(c.y[0] * r + c.y[1] * g + c.y[2] * b + (c.yoff << 16) + 32768, c.lo, c.yhi);
    cb = level(c.cb[0] * r + c.cb[1] * g + c.cb[2] * b + (128 << 16) + 32768, c.lo, c.chi);
    cr = level(c.cr[0] * r + c.cr[1] * g + c.cr[2] * b + (128 << 16) + 32768, c.lo, c.chi);
}

// n <= 8 bytes of v[] to q: two dwords when all 8 go out and q is dword-aligned
__device__ __forceinline__ void store_row8(uint8_t* __restrict__ q, const int (&v)[8], int n) {
    if (n >= 8 && ((uintptr_t)q & 3) == 0) {
        reinterpret_cast<uint32_t*>(q)[0] = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
        reinterpret_cast<uint32_t*>(q)[1] = (uint32_t)v[4] | (uint32_t)v[5] << 8 | (uint32_t)v[6] << 16 | (uint32_t)v[7] << 24;
    } else {
        for (int k = 0; k < n && k < 8; ++k) q[k] = (uint8_t)v[k];
    }
}

__device__ __forceinline__ void store_row4(uint8_t* __restrict__ q, const int (&v)[4], int n) {
    if (n >= 4 && ((uintptr_t)q & 3) == 0) {
        reinterpret_cast<uint32_t*>(q)[0] = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
        for (int k = 0; k < n && k < 4; ++k) q[k] = (uint8_t)v[k];
    }
}

// MODE 0: 4:4:4; 1: 420jpeg (2x2 box); 2: 420mpeg2 ((1, 2, 1) on the even column x the row pair). A lane converts the 8 x 2 pixels at
// (x0, y0); its column x0 - 1, which the (1, 2, 1) filter needs, is the last column of the lane on its left and comes by a shuffle
// (the first lane of a wave converts that one pixel again), so the source is read once.
template <int MODE>
__global__ __launch_bounds__(256)
void bgr_to_yuv_kernel(const uint8_t* __restrict__ bgr, int H, int W, long stride, int CW, int CH, Coef c, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * ENC_COLS + lane * 8;
    const int y0 = blockIdx.y * ENC_ROWS + (threadIdx.x >> 6) * 2;
    const bool active = x0 < W && y0 < H;
    int Y[2][8], Cb[2][8], Cr[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) Y[r][k] = Cb[r][k] = Cr[r][k] = 0;
    if (active) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* row = bgr + (long)min(y0 + r, H - 1) * stride;      // rows and columns clamped to the image
            const uint8_t* p = row + (long)x0 * 3;
            uint32_t w[6];
            if (x0 + 8 <= W && ((uintptr_t)p & 3) == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) w[i] = 0;
#pragma unroll
                for (int i = 0; i < 24; ++i) {
                    const int x = min(x0 + i / 3, W - 1);
                    w[i >> 2] |= (uint32_t)row[(long)x * 3 + i % 3] << (8 * (i & 3));
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int v[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int i = k * 3 + ch;
                    v[ch] = (int)((w[i >> 2] >> (8 * (i & 3))) & 255);
                }
                encode_pixel(c, v[0], v[1], v[2], Y[r][k], Cb[r][k], Cr[r][k]);
            }
        }
    }
    uint32_t left = 0;                                           // (Cb, Cr) of column x0 - 1, rows 0 and 1
    if (MODE == 2) {
        const uint32_t mine = (uint32_t)Cb[0][7] | (uint32_t)Cr[0][7] << 8 | (uint32_t)Cb[1][7] << 16 | (uint32_t)Cr[1][7] << 24;
        left = __shfl_up(mine, 1, 64);                           // every lane of the wave takes part
        if (active && lane == 0) {
            left = 0;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint8_t* p = bgr + (long)min(y0 + r, H - 1) * stride + (long)max(x0 - 1, 0) * 3;
                int yy, u, v;
                encode_pixel(c, p[0], p[1], p[2], yy, u, v);
                left |= ((uint32_t)u | (uint32_t)v << 8) << (16 * r);
            }
        }
    }
    if (!active) return;
    const int n = W - x0;                                        // columns of this lane inside the image (8 or more: all)
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (y0 + r < H) store_row8(out + (long)(y0 + r) * W + x0, Y[r], n);
    uint8_t* pcb = out + (long)W * H;
    uint8_t* pcr = pcb + (long)CW * CH;
    if (MODE == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (y0 + r < H) {
                store_row8(pcb + (long)(y0 + r) * W + x0, Cb[r], n);
                store_row8(pcr + (long)(y0 + r) * W + x0, Cr[r], n);
            }
        return;
    }
    int u[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (MODE == 1) {
            u[k] = (Cb[0][2 * k] + Cb[0][2 * k + 1] + Cb[1][2 * k] + Cb[1][2 * k + 1] + 2) >> 2;
            v[k] = (Cr[0][2 * k] + Cr[0][2 * k + 1] + Cr[1][2 * k] + Cr[1][2 * k + 1] + 2) >> 2;
        } else {
            const int lu = k ? Cb[0][2 * k - 1] + Cb[1][2 * k - 1] : (int)((left & 255) + ((left >> 16) & 255));
            const int lv = k ? Cr[0][2 * k - 1] + Cr[1][2 * k - 1] : (int)(((left >> 8) & 255) + ((left >> 24) & 255));
            u[k] = (lu + 2 * (Cb[0][2 * k] + Cb[1][2 * k]) + Cb[0][2 * k + 1] + Cb[1][2 * k + 1] + 4) >> 3;
            v[k] = (lv + 2 * (Cr[0][2 * k] + Cr[1][2 * k]) + Cr[0][2 * k + 1] + Cr[1][2 * k + 1] + 4) >> 3;
        }
    }
    const int cx0 = x0 >> 1;
    const long coff = (long)(y0 >> 1) * CW + cx0;
    store_row4(pcb + coff, u, CW - cx0);
    store_row4(pcr + coff, v, CW - cx0);
}

// chroma plane size of a sampling; false for an unknown one
bool plane_size(int sampling, int H, int W, int& CH, int& CW) {
    switch (sampling) {
        case VPS_Y4M_420JPEG:
        case VPS_Y4M_420MPEG2: CW = (W + 1) / 2; CH = (H + 1) / 2; return true;
        case VPS_Y4M_422: CW = (W + 1) / 2; CH = H; return true;
        case VPS_Y4M_444: CW = W; CH = H; return true;
        case VPS_Y4M_MONO: CW = 0; CH = 0; return true;
        default: return false;
    }
}

}  // namespace

extern "C" int vps_yuv_tile(int32_t* to_bgr_rows_cols, int32_t* to_yuv_rows_cols) {
    if (to_bgr_rows_cols) { to_bgr_rows_cols[0] = DEC_ROWS; to_bgr_rows_cols[1] = DEC_COLS; }
    if (to_yuv_rows_cols) { to_yuv_rows_cols[0] = ENC_ROWS; to_yuv_rows_cols[1] = ENC_COLS; }
    return 0;
}

extern "C" int vps_yuv_to_bgr(const uint8_t* frame, int64_t frame_bytes, int H, int W, int sampling, int range, int matrix, uint8_t* out,
                              int64_t out_capacity, void* stream) {
    if (!frame || !out || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return VPS_EARG(1);
    int CH, CW;
    if (!plane_size(sampling, H, W, CH, CW)) return VPS_EARG(2);
    if ((range != VPS_YUV_LIMITED && range != VPS_YUV_FULL) || (matrix != VPS_YUV_BT601 && matrix != VPS_YUV_BT709)) return VPS_EARG(3);
    const int64_t need = (int64_t)H * W + 2 * (int64_t)CH * CW;
    if (frame_bytes < need || out_capacity < 3 * (int64_t)H * W) return VPS_EARG(4);
    if ((uintptr_t)frame & 3) return VPS_EARG(5);
    const Coef c = vps_yuv::kTable[matrix][range];
    const dim3 grid(cdiv(W, DEC_COLS), cdiv(H, DEC_ROWS)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const long limit = (long)need;
    switch (sampling) {
        case VPS_Y4M_420JPEG: hipLaunchKernelGGL((yuv_to_bgr_kernel<1, true, false>), grid, block, 0, s, frame, limit, H, W, CW, CH, c, out); break;
        case VPS_Y4M_420MPEG2: hipLaunchKernelGGL((yuv_to_bgr_kernel<2, true, false>), grid, block, 0, s, frame, limit, H, W, CW, CH, c, out); break;
        case VPS_Y4M_422: hipLaunchKernelGGL((yuv_to_bgr_kernel<2, false, false>), grid, block, 0, s, frame, limit, H, W, CW, CH, c, out); break;
        case VPS_Y4M_444: hipLaunchKernelGGL((yuv_to_bgr_kernel<0, false, false>), grid, block, 0, s, frame, limit, H, W, CW, CH, c, out); break;
        default: hipLaunchKernelGGL((yuv_to_bgr_kernel<0, false, true>), grid, block, 0, s, frame, limit, H, W, CW, CH, c, out); break;
    }
    return vps_launch_status();
}

extern "C" int vps_bgr_to_yuv(const uint8_t* bgr, int H, int W, int64_t row_stride, int rgb_order, int sampling, int range, int matrix,
                              uint8_t* out, int64_t out_capacity, void* stream) {
    if (!bgr || !out || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX) return VPS_EARG(1);
    int CH, CW;
    if ((sampling != VPS_Y4M_444 && sampling != VPS_Y4M_420JPEG && sampling != VPS_Y4M_420MPEG2) || !plane_size(sampling, H, W, CH, CW))
        return VPS_EARG(2);
    if ((range != VPS_YUV_LIMITED && range != VPS_YUV_FULL) || (matrix != VPS_YUV_BT601 && matrix != VPS_YUV_BT709)) return VPS_EARG(3);
    if (row_stride < 3 * (int64_t)W || out_capacity < (int64_t)H * W + 2 * (int64_t)CH * CW) return VPS_EARG(4);
    Coef c = vps_yuv::kTable[matrix][range];
    if (rgb_order) {                                             // the kernel reads byte 0 as B: swap the R and B columns instead
        std::swap(c.y[0], c.y[2]);
        std::swap(c.cb[0], c.cb[2]);
        std::swap(c.cr[0], c.cr[2]);
    }
    const dim3 grid(cdiv(W, ENC_COLS), cdiv(H, ENC_ROWS)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const long stride = (long)row_stride;
    switch (sampling) {
        case VPS_Y4M_444: hipLaunchKernelGGL((bgr_to_yuv_kernel<0>), grid, block, 0, s, bgr, H, W, stride, CW, CH, c, out); break;
        case VPS_Y4M_420JPEG: hipLaunchKernelGGL((bgr_to_yuv_kernel<1>), grid, block, 0, s, bgr, H, W, stride, CW, CH, c, out); break;
        default: hipLaunchKernelGGL((bgr_to_yuv_kernel<2>), grid, block, 0, s, bgr, H, W, stride, CW, CH, c, out); break;
    }
    return vps_launch_status();
}
