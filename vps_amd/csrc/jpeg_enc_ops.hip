// Device half of the JPEG output path (overlay images; the mirror image of jpeg_ops.hip):
//   vps_overlay_render    input frame (BGR) + painted panoptic map (RGB, 0 = void) -> blended RGB image with white segment borders
//   vps_jpeg_encode_coef  RGB uint8 -> quantised DCT coefficients, int16 [component][block row][block column][64] in natural order, the
//                         layout of vps_jpeg_decode_coef; the Huffman coding of them is host work (jpeg_enc_host.cpp)
// The second is the integer arithmetic of libjpeg's default compressor, restated from the published algorithms of jccolor.c (16-bit
// fixed-point RGB -> YCbCr), jcsample.c (h2v2 box filter, bias alternating 1, 2), jfdctint.c (slow-integer forward DCT: 13-bit
// constants, PASS1_BITS 2, rows first) and jcdctmgr.c (division by 8 * table entry, rounded half away from zero), including its
// edges: pixels replicated to a whole block horizontally and a whole iMCU row vertically (chroma: the last DOWN-SAMPLED row is
// repeated), and the dummy blocks that only fill the last MCU (AC zero, DC of the preceding block of the MCU). The result is
// bit-exact with it (tests/jpeg_enc_restate.py is the NumPy twin). One launch: each block converts its own pixels, so the
// source is read once for luma and once per chroma plane out of the L2; no intermediate planes, no workspace.
#include "common.h"

namespace {

constexpr int CB = 13, P1 = 2;    // CONST_BITS, PASS1_BITS
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass of jpeg_fdct_islow. FIRST: the row pass (outputs scaled up by 4); otherwise the column pass, which removes that factor
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8]) {
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int SH = FIRST ? CB - P1 : CB + P1;
    if (FIRST) {
        o[0] = (tmp10 + tmp11) * (1 << P1);
        o[4] = (tmp10 - tmp11) * (1 << P1);
    } else {
        o[0] = descale(tmp10 + tmp11, P1);
        o[4] = descale(tmp10 - tmp11, P1);
    }
    int z1 = (tmp12 + tmp13) * F_0_541196100;
    o[2] = descale(z1 + tmp13 * F_0_765366865, SH);
    o[6] = descale(z1 + tmp12 * (-F_1_847759065), SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp4 *= F_0_298631336; tmp5 *= F_2_053119869; tmp6 *= F_3_072711026; tmp7 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    o[7] = descale(tmp4 + z1 + z3, SH);
    o[5] = descale(tmp5 + z2 + z4, SH);
    o[3] = descale(tmp6 + z2 + z3, SH);
    o[1] = descale(tmp7 + z1 + z4, SH);
}

// jccolor.c: SCALEBITS 16; the chroma rows carry 128 << 16 and the rounding term ONE_HALF - 1
__device__ __forceinline__ int ycc(int c, int r, int g, int b) {
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// NPX pixels of one image row from column x0 on, columns beyond the image replicated from the last one: 3 * NPX bytes in px
template <int NPX>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ row, int x0, int W, bool aligned, uint32_t (&px)[3 * NPX / 4]) {
    if (aligned && x0 + NPX <= W) {                                              // x0 is a multiple of 8: 3 * x0 is a multiple of 4
        const uint32_t* p = reinterpret_cast<const uint32_t*>(row + (size_t)x0 * 3);
#pragma unroll
        for (int k = 0; k < 3 * NPX / 4; ++k) px[k] = p[k];
    } else {
#pragma unroll
        for (int k = 0; k < 3 * NPX / 4; ++k) px[k] = 0;
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const uint8_t* p = row + (size_t)min(x0 + k, W - 1) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) px[(3 * k + ch) >> 2] |= (uint32_t)p[ch] << (8 * ((3 * k + ch) & 3));
        }
    }
}

template <int N>
__device__ __forceinline__ int byte_of(const uint32_t (&px)[N], int i) { return (int)((px[i >> 2] >> (8 * (i & 3))) & 255); }

struct EncGeom {
    int H, W;
    int sub;                      // 1 = 4:2:0 (chroma planes halved in both directions), 0 = 4:4:4
    int brows[3], bcols[3];       // block grid per component, padded to whole MCUs
    int nblk[3];
    int wb, hb;                   // luma blocks that hold pixels: ceil(W / 8), ceil(H / 8); the rest of the grid is dummy blocks
};

// Eight lanes hold one block (a wavefront works on 8 blocks, a workgroup on 32), as in jpeg_idct_kernel. Lane j converts row j of the
// block's samples and runs the row pass on it in registers; the column pass reads COLUMN j of the results from LDS, quantises, and the
// last exchange hands lane j ROW j of the coefficients for one 16-byte store (the wave writes 1 KiB contiguous). A block is 64 words +
// 8 of padding: the column accesses of the four blocks of a 32-lane group then fall on four different 8-bank groups.
constexpr int BLK_LD = 72;

__global__ __launch_bounds__(256)
void jpeg_fdct_kernel(const uint8_t* __restrict__ rgb, long stride, bool aligned, const uint16_t* __restrict__ qt, EncGeom g, int total,
                      int16_t* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) int lds[32 * BLK_LD];
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const int blk = blockIdx.x * 32 + lb;
    const bool live = blk < total;
    int* t = lds + lb * BLK_LD;
    int c = 0;
    bool dummy = false;
    if (live) {
        int local = blk;
        if (local >= g.nblk[0]) { local -= g.nblk[0]; c = 1; }
        if (c == 1 && local >= g.nblk[1]) { local -= g.nblk[1]; c = 2; }
        int by = local / g.bcols[c], bx = local - by * g.bcols[c];
        if (c == 0) {
            // a dummy block takes the DC of the block before it in its MCU: left of it, or - in a dummy row - the right block of the row
            // above, which may be a dummy itself. It transforms that block's pixels and keeps the DC only.
            if (by >= g.hb) { dummy = true; by -= 1; bx |= 1; }
            if (bx >= g.wb) { dummy = true; bx -= 1; }
        }
        const int H = g.H, W = g.W;
        int s[8];
        if (c == 0 || !g.sub) {
            const int y = min(by * 8 + j, H - 1);
            uint32_t px[6];
            load_row<8>(rgb + (size_t)y * stride, bx * 8, W, aligned, px);
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] = ycc(c, byte_of(px, 3 * k), byte_of(px, 3 * k + 1), byte_of(px, 3 * k + 2)) - 128;
        } else {
            const int r = min(by * 8 + j, ((H + 1) >> 1) - 1);                   // beyond the last down-sampled row that row is repeated
            const int y0 = min(2 * r, H - 1), y1 = min(2 * r + 1, H - 1);
            uint32_t pa[12], pb[12];
            load_row<16>(rgb + (size_t)y0 * stride, bx * 16, W, aligned, pa);
            load_row<16>(rgb + (size_t)y1 * stride, bx * 16, W, aligned, pb);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int sum = (k & 1) ? 2 : 1;                                       // the bias alternates 1, 2 along the row
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = 3 * (2 * k + e);
                    sum += ycc(c, byte_of(pa, i), byte_of(pa, i + 1), byte_of(pa, i + 2));
                    sum += ycc(c, byte_of(pb, i), byte_of(pb, i + 1), byte_of(pb, i + 2));
                }
                s[k] = (sum >> 2) - 128;
            }
        }
        int o[8];
        fdct8<true>(s, o);
        *reinterpret_cast<int4*>(t + j * 8) = make_int4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<int4*>(t + j * 8 + 4) = make_int4(o[4], o[5], o[6], o[7]);
    }
    __syncthreads();
    if (live) {
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = t[r * 8 + j];
        fdct8<false>(in, o);
        const uint16_t* q = qt + (c ? 64 : 0) + j;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int qv = (int)q[r * 8] * 8;                                    // the transform's output is scaled up by 8
            const int v = o[r];
            int a = (v < 0 ? -v : v) + (qv >> 1);
            a = (int)((unsigned)a / (unsigned)qv);
            a = v < 0 ? -a : a;
            if (dummy && (r | j)) a = 0;
            t[r * 8 + j] = a;                                                    // its own column: no other lane touches it in this pass
        }
    }
    __syncthreads();
    if (live) {
        const int4 a = *reinterpret_cast<const int4*>(t + j * 8), b = *reinterpret_cast<const int4*>(t + j * 8 + 4);
        int4 w;
        w.x = (a.x & 0xFFFF) | (a.y << 16); w.y = (a.z & 0xFFFF) | (a.w << 16);
        w.z = (b.x & 0xFFFF) | (b.y << 16); w.w = (b.z & 0xFFFF) | (b.w << 16);
        *reinterpret_cast<int4*>(coef + (size_t)blk * 64 + j * 8) = w;
    }
}

// one thread = four horizontally adjacent pixels of a row (x0 a multiple of 4): 12 bytes of each input and of the output
__device__ __forceinline__ void load_quad(const uint8_t* __restrict__ p, int n, uint32_t (&v)[3]) {
    if (n == 4 && ((uintptr_t)p & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else {
        v[0] = v[1] = v[2] = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) v[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    }
}

__global__ __launch_bounds__(256)
void overlay_render_kernel(const uint8_t* __restrict__ frame, const uint8_t* __restrict__ colour, int H, int W, int alpha, int quads_per_row,
                           long total, uint8_t* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int y = (int)(idx / quads_per_row), x0 = (int)(idx - (long)y * quads_per_row) * 4;
    const int n = min(4, W - x0);
    const size_t off = ((size_t)y * W + x0) * 3;
    uint32_t f[3], cur[3], below[3] = {0, 0, 0};
    load_quad(frame + off, n, f);
    load_quad(colour + off, n, cur);
    const bool has_below = y + 1 < H;
    if (has_below) load_quad(colour + off + (size_t)W * 3, n, below);
    int right[3] = {0, 0, 0};                                                    // the pixel after the quad, if the row has one
    const bool has_right = x0 + 4 < W;
    if (has_right) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) right[ch] = colour[off + 12 + ch];
    }
    uint32_t o[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c0 = byte_of(cur, 3 * k), c1 = byte_of(cur, 3 * k + 1), c2 = byte_of(cur, 3 * k + 2);
        bool edge = false;
        if (k < 3) {
            if (k + 1 < n) edge = c0 != byte_of(cur, 3 * k + 3) || c1 != byte_of(cur, 3 * k + 4) || c2 != byte_of(cur, 3 * k + 5);
        } else if (has_right) {
            edge = c0 != right[0] || c1 != right[1] || c2 != right[2];
        }
        if (has_below) edge = edge || c0 != byte_of(below, 3 * k) || c1 != byte_of(below, 3 * k + 1) || c2 != byte_of(below, 3 * k + 2);
        const int fb = byte_of(f, 3 * k), fg = byte_of(f, 3 * k + 1), fr = byte_of(f, 3 * k + 2);
        int r, gg, b;
        if (edge) {
            r = gg = b = 255;
        } else if ((c0 | c1 | c2) == 0) {                                        // void: the frame shows through
            r = fr; gg = fg; b = fb;
        } else {
            r = (fr * (256 - alpha) + c0 * alpha + 128) >> 8;
            gg = (fg * (256 - alpha) + c1 * alpha + 128) >> 8;
            b = (fb * (256 - alpha) + c2 * alpha + 128) >> 8;
        }
        const int v[3] = {r, gg, b};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[(3 * k + ch) >> 2] |= (uint32_t)v[ch] << (8 * ((3 * k + ch) & 3));
    }
    uint8_t* q = out + off;
    if (n == 4 && ((uintptr_t)q & 3) == 0) {
        uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
        q4[0] = o[0]; q4[1] = o[1]; q4[2] = o[2];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) q[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

}  // namespace

extern "C" int vps_overlay_render(const uint8_t* frame_bgr, const uint8_t* colour_rgb, int H, int W, int alpha, uint8_t* out_rgb, void* stream) {
    if (!frame_bgr || !colour_rgb || !out_rgb || H <= 0 || W <= 0 || H > 65535 || W > 65535) return VPS_EARG(1);
    if (alpha < 0 || alpha > 256) return VPS_EARG(2);
    const int quads = (W + 3) / 4;
    const long items = (long)H * quads;
    hipLaunchKernelGGL(overlay_render_kernel, dim3(cdiv(items, 256)), dim3(256), 0, (hipStream_t)stream, frame_bgr, colour_rgb, H, W, alpha, quads,
                       items, out_rgb);
    return vps_launch_status();
}

extern "C" int vps_jpeg_encode_coef(const uint8_t* rgb, int H, int W, int64_t row_stride, int subsampling, const uint16_t* qt, int16_t* coef,
                                    int64_t coef_capacity, void* stream) {
    if (!rgb || !qt || !coef) return VPS_EARG(1);
    int32_t grid[6];
    int64_t need = 0;
    const int st = vps_jpeg_encode_bound(H, W, subsampling, grid, &need);       // size and mode checks live there
    if (st) return st;
    if (row_stride < (int64_t)W * 3) return VPS_EARG(3);
    if (((uintptr_t)coef & 15) || ((uintptr_t)qt & 1)) return VPS_EARG(4);
    if (coef_capacity < need) return VPS_EARG(5);
    EncGeom g;
    g.H = H; g.W = W; g.sub = subsampling == 2;
    g.wb = (W + 7) / 8; g.hb = (H + 7) / 8;
    long total = 0;
    for (int c = 0; c < 3; ++c) {
        g.brows[c] = grid[2 * c]; g.bcols[c] = grid[2 * c + 1];
        g.nblk[c] = g.brows[c] * g.bcols[c];
        total += g.nblk[c];
    }
    const bool aligned = (((uintptr_t)rgb | (uintptr_t)row_stride) & 3) == 0;
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(cdiv(total, 32)), dim3(256), 0, (hipStream_t)stream, rgb, (long)row_stride, aligned, qt, g, (int)total,
                       coef);
    return vps_launch_status();
}
