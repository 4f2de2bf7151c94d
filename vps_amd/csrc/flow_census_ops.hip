// Illumination-robust flow residual (vps_amd/flowphoto.py): the ternary census warp error of a flow between the two
// frames it was computed from - the ordering of every pixel against its 7 x 7 neighbourhood in cur, compared with the same ordering in
// prev sampled at p + flow(p) and, as the "static" twin, in prev itself. An additive brightness change cancels exactly.
//   vps_flow_census_ws_bytes  host arithmetic: three fp32 planes of the frame, each padded to a multiple of 4 pixels
//   vps_flow_census_tile      host: the rows and columns of a tile of the census launch (for tests that put edges on the seams)
//   vps_flow_census           one (cur, prev, flow) triple: every pixel is ADDED to the caller's int64 [2][13] table; optionally the mask
//                             with the flagged pixels (code 3) and the residual image are written. Nothing is zeroed, downloaded or
//                             synchronised. Two launches:
//     pass 1 (warp)    a lane owns 4 consecutive pixels (px4.h), as flow_photo_ops.hip: the warp rule (warp_rule.h) on the greys of the
//                      four corners of prev -> plane 0 (Wg, -1.0f = none); the greys of cur and prev -> planes 1, 2.
//                      Read per pixel 3 + 3 + 8 bytes and the corner bytes from the cache, written 12.
//     pass 2 (census)  a workgroup takes a tile of 32 rows x 64 columns: it stages the three planes with a halo of 3 in LDS (38 rows x 72
//                      columns x 3 planes x 4 bytes = 32 832 bytes; positions outside the image are -1.0f = none), then every lane forms
//                      the codes and counts of 2 x 4 pixels. Read per pixel 12 bytes x 38 * 72 / (32 * 64) = 16.0 and the mask byte,
//                      written 2 bytes.
// Arithmetic: greys are integers up to 255 000, exact in fp32; the sample and the code differences are fp32 operations rounded on their
// own (the file is compiled without contraction); every decision after the codes is an integer one, so the table, mask_out and residual
// equal the NumPy restatement (tests/flow_census_restate.py) bit for bit. Integer atomics only: no finishing launch, the same bytes on
// every call.
// Register blocking: the 4 pixels of a lane lie side by side in a row, so one window row of a plane is 10 values for 4 pixels, read as
// three 16-byte LDS loads (12 values) instead of 4 x 7: 63 LDS loads per plane set and lane strip where the plain form has 588.
#include "px4.h"
#include "warp_rule.h"

#pragma clang fp contract(off)

namespace {

constexpr int FC_THREADS = PX4_WG;
constexpr int FC_TR = 32, FC_TC = 64;                  // the tile of pass 2
constexpr int FC_R = 3;                                // the window is (2 FC_R + 1)^2
constexpr int FC_PAD = 4;                              // columns staged on either side: the halo of 3 and one more, so that a lane's row is 16-byte aligned
constexpr int FC_LR = FC_TR + 2 * FC_R, FC_LC = FC_TC + 2 * FC_PAD;
constexpr int FC_CELLS = 13;
constexpr float FC_NONE = -1.0f;

long fc_plane(long npix) { return (npix + 3) & ~3L; }

__device__ __forceinline__ float fc_grey(uint32_t b, uint32_t g, uint32_t r) { return (float)(299u * r + 587u * g + 114u * b); }

// the grey of pixel (iy, ix) of a [H][W][3] BGR byte map; iy and ix are inside the map
__device__ __forceinline__ float fc_corner(const uint8_t* __restrict__ prev, int W, int iy, int ix) {
    const uint8_t* a = prev + 3 * ((long)iy * W + ix);
    return fc_grey(a[0], a[1], a[2]);
}

// Pass 1. A lane owns the 4 pixels of chunk ch (linear index; a chunk may run over the end of a row).
__global__ __launch_bounds__(FC_THREADS)
void flow_census_warp_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, int H, int W, const float* __restrict__ flow, int fld,
                             int fcoff, int fmode, float* __restrict__ wg, float* __restrict__ gc, float* __restrict__ gp) {
    const long npix = (long)H * W, nchunk = (npix + PX4 - 1) / PX4;
    for (long ch = (long)blockIdx.x * FC_THREADS + threadIdx.x; ch < nchunk; ch += (long)gridDim.x * FC_THREADS) {
        const long p0 = PX4 * ch;
        const int n = (int)min((long)PX4, npix - p0);
        float u[PX4], v[PX4], ow[PX4], oc[PX4], op[PX4];
        uint32_t c4[PX4], s4[PX4];
        px4_load_flow(flow, fld, fcoff, fmode, p0, n, u, v);
        px4_load_px3(cur, 3 * npix, ch, n, c4);
        px4_load_px3(prev, 3 * npix, ch, n, s4);
        int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            ow[i] = FC_NONE;
            oc[i] = fc_grey(c4[i] & 0xffu, (c4[i] >> 8) & 0xffu, c4[i] >> 16);
            op[i] = fc_grey(s4[i] & 0xffu, (s4[i] >> 8) & 0xffu, s4[i] >> 16);
            if (i < n) {
                const float sx = warp_pos(x, u[i]), sy = warp_pos(y, v[i]);             // warp_rule.h: in view, corners, sample
                if (warp_in_view(sx, sy, W, H)) {
                    const WarpCorners k = warp_corners(sx, sy, W, H);
                    ow[i] = warp_lerp2(fc_corner(prev, W, k.y0, k.x0), fc_corner(prev, W, k.y0, k.x1), fc_corner(prev, W, k.y1, k.x0),
                                       fc_corner(prev, W, k.y1, k.x1), k.wx, k.wy);
                }
                if (++x == W) { x = 0; ++y; }
            }
        }
        if (n == PX4) {                                // p0 and the planes' stride are multiples of 4 floats, the workspace is 16-byte aligned
            *reinterpret_cast<px4_f4*>(wg + p0) = px4_f4{ow[0], ow[1], ow[2], ow[3]};
            *reinterpret_cast<px4_f4*>(gc + p0) = px4_f4{oc[0], oc[1], oc[2], oc[3]};
            *reinterpret_cast<px4_f4*>(gp + p0) = px4_f4{op[0], op[1], op[2], op[3]};
        } else {
            for (int i = 0; i < n; ++i) { wg[p0 + i] = ow[i]; gc[p0 + i] = oc[i]; gp[p0 + i] = op[i]; }
        }
    }
}

__device__ __forceinline__ int fc_code(float d, float eps, float neps) { return (int)(d > eps) - (int)(d < neps); }

// Pass 2. Workgroup = tile; lane t owns the pixels (row t / 16 + 16 h, columns 4 (t % 16) .. + 3) for h = 0, 1. The 26 counters of a
// lane stay in registers under constant indices; they are summed across the wavefront by xor shuffles, across the four wavefronts in LDS,
// and leave as one 64-bit atomic per non-zero cell. The centre itself runs through the window loop: its codes are 0 in every image, so
// it adds no difference, and it is taken out of n_w again (a scored pixel has a Wg of its own). n_s needs no loop: it is the number of
// window positions inside the image. mask_in and mask_out may be the same buffer: a lane reads its own bytes before it writes them.
__global__ __launch_bounds__(FC_THREADS)
void flow_census_kernel(const float* __restrict__ wg, const float* __restrict__ gc, const float* __restrict__ gp, int H, int W, int ntx,
                        const uint8_t* mask_in, int thr, float eps, unsigned long long* __restrict__ table, uint8_t* mask_out,
                        uint8_t* __restrict__ residual) {
    __shared__ __attribute__((aligned(16))) float tile[3][FC_LR][FC_LC];
    __shared__ uint32_t red[FC_THREADS / 64][2 * FC_CELLS];
    const int ty0 = (int)(blockIdx.x / (unsigned)ntx) * FC_TR, tx0 = (int)(blockIdx.x % (unsigned)ntx) * FC_TC;
    for (int idx = threadIdx.x; idx < FC_LR * FC_LC; idx += FC_THREADS) {
        const int r = idx / FC_LC, c = idx - r * FC_LC;
        const int gy = ty0 - FC_R + r, gx = tx0 - FC_PAD + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const long off = in ? (long)gy * W + gx : 0;
        tile[0][r][c] = in ? wg[off] : FC_NONE;
        tile[1][r][c] = in ? gc[off] : FC_NONE;
        tile[2][r][c] = in ? gp[off] : FC_NONE;
    }
    __syncthreads();
    const float neps = -eps;
    const int cg = threadIdx.x & 15;
    uint32_t cnt[2][FC_CELLS];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int k = 0; k < FC_CELLS; ++k) cnt[g][k] = 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const int ty = (threadIdx.x >> 4) + 16 * h;
        const int y = ty0 + ty, x0 = tx0 + 4 * cg;
        if (y >= H || x0 >= W) continue;
        float cw[PX4], cc[PX4], cp[PX4];
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            cw[i] = tile[0][ty + FC_R][FC_PAD + 4 * cg + i];
            cc[i] = tile[1][ty + FC_R][FC_PAD + 4 * cg + i];
            cp[i] = tile[2][ty + FC_R][FC_PAD + 4 * cg + i];
        }
        uint32_t accw[PX4] = {0, 0, 0, 0}, accs[PX4] = {0, 0, 0, 0};   // n_w + 256 d_w (the centre included in n_w), d_s
#pragma unroll 1
        for (int dy = -FC_R; dy <= FC_R; ++dy) {
            float w[12], c[12], p[12];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const px4_f4 a = *reinterpret_cast<const px4_f4*>(&tile[0][ty + FC_R + dy][4 * cg + 4 * j]);
                const px4_f4 b = *reinterpret_cast<const px4_f4*>(&tile[1][ty + FC_R + dy][4 * cg + 4 * j]);
                const px4_f4 d = *reinterpret_cast<const px4_f4*>(&tile[2][ty + FC_R + dy][4 * cg + 4 * j]);
                w[4 * j] = a.x; w[4 * j + 1] = a.y; w[4 * j + 2] = a.z; w[4 * j + 3] = a.w;
                c[4 * j] = b.x; c[4 * j + 1] = b.y; c[4 * j + 2] = b.z; c[4 * j + 3] = b.w;
                p[4 * j] = d.x; p[4 * j + 1] = d.y; p[4 * j + 2] = d.z; p[4 * j + 3] = d.w;
            }
#pragma unroll
            for (int i = 0; i < PX4; ++i) {
#pragma unroll
                for (int dx = -FC_R; dx <= FC_R; ++dx) {
                    const int k = FC_PAD + i + dx;
                    const int kc = fc_code(c[k] - cc[i], eps, neps);
                    const int kw = fc_code(w[k] - cw[i], eps, neps);
                    const int kp = fc_code(p[k] - cp[i], eps, neps);
                    accw[i] += w[k] >= 0.f ? (kc != kw ? 257u : 1u) : 0u;
                    accs[i] += (c[k] >= 0.f && kc != kp) ? 1u : 0u;
                }
            }
        }
        const int n = min(PX4, W - x0);
        const long p0 = (long)y * W + x0;
        const uint32_t M = mask_in ? px4_load_bytes_at(mask_in, p0, n) : 0u;
        const int ny = min(y + FC_R, H - 1) - max(y - FC_R, 0) + 1;
        uint32_t codes = 0, resid = 0;
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            if (i >= n) break;
            const int x = x0 + i;
            const uint32_t m = (M >> (8 * i)) & 0xffu;
            const bool in = cw[i] >= 0.f;
            const uint32_t nw = (accw[i] & 0xffu) - (in ? 1u : 0u), dw = accw[i] >> 8, ds = accs[i];
            const uint32_t ns = (uint32_t)(ny * (min(x + FC_R, W - 1) - max(x - FC_R, 0) + 1) - 1);
            const bool scored = in && nw >= 1;
            const bool flagged = scored && 100u * dw > (uint32_t)thr * nw;
            const uint32_t code = !in ? 2u : m ? m : (flagged ? 3u : 0u);
            const uint32_t res = scored ? (255u * dw + nw / 2u) / nw : 0u;
#pragma unroll
            for (int g = 0; g < 2; ++g) {              // constant indices: the table stays in registers
                const bool mine = (m != 0) == (g == 1), sc = mine && scored;
                cnt[g][0] += sc;
                cnt[g][1] += sc ? dw : 0u;   cnt[g][2] += sc ? nw : 0u;
                cnt[g][3] += sc ? ds : 0u;   cnt[g][4] += sc ? ns : 0u;
                cnt[g][5] += sc && 100u * dw > 10u * nw;   cnt[g][6] += sc && 100u * dw > 25u * nw;   cnt[g][7] += sc && 100u * dw > 50u * nw;
                cnt[g][8] += sc && dw * ns < ds * nw;      cnt[g][9] += sc && dw * ns > ds * nw;
                cnt[g][10] += mine && flagged;
                cnt[g][11] += mine && !in;
                cnt[g][12] += mine && in && nw == 0;
            }
            codes |= code << (8 * i);
            resid |= res << (8 * i);
        }
        if (mask_out) px4_store_bytes(mask_out, ((uintptr_t)(mask_out + p0) & 3) == 0, p0, n, codes);
        if (residual) px4_store_bytes(residual, ((uintptr_t)(residual + p0) & 3) == 0, p0, n, resid);
    }
    // the two rows are the table's 26 cells in order (declared flat, the kernel takes 6 more SGPRs); a cell: at most 2048 pixels x 48
    wg_counts_to_table(reinterpret_cast<const uint32_t(&)[2 * FC_CELLS]>(cnt), red, table);
}

}  // namespace

extern "C" int64_t vps_flow_census_ws_bytes(int H, int W) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    return (int64_t)(3 * fc_plane((long)H * W) * sizeof(float));
}

extern "C" int vps_flow_census_tile(int32_t* rows_cols) {
    if (!rows_cols) return VPS_EARG(1);
    rows_cols[0] = FC_TR;
    rows_cols[1] = FC_TC;
    return 0;
}

extern "C" int vps_flow_census(const uint8_t* cur_bgr, const uint8_t* prev_bgr, int H, int W, const float* flow, int flow_ld, int flow_coff,
                               const uint8_t* mask_in, int thr, float eps, int64_t* table, uint8_t* mask_out, uint8_t* residual, void* ws,
                               int64_t ws_bytes, void* stream) {
    if (!cur_bgr || !prev_bgr || !flow || !table || !ws) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    if (flow_coff < 0 || flow_ld < flow_coff + 2) return VPS_EARG(3);
    if (((uintptr_t)table & 7) || ((uintptr_t)flow & 3)) return VPS_EARG(4);
    const long npix = (long)H * W, plane = fc_plane(npix);
    if (((uintptr_t)ws & 15) || ws_bytes < (int64_t)(3 * plane * sizeof(float))) return VPS_EARG(5);
    if (thr < 0 || thr > 100) return VPS_EARG(6);
    if (!(eps >= 0.f) || !(eps <= 3.402823466e38f)) return VPS_EARG(7);             // negative, NaN or inf
    hipStream_t s = (hipStream_t)stream;
    float* wg = static_cast<float*>(ws);
    const long nchunk = (npix + PX4 - 1) / PX4, g1 = min((nchunk + FC_THREADS - 1) / FC_THREADS, 65536L);
    hipLaunchKernelGGL(flow_census_warp_kernel, dim3((unsigned)g1), dim3(FC_THREADS), 0, s, cur_bgr, prev_bgr, H, W, flow, flow_ld, flow_coff,
                       px4_flow_mode(flow, flow_ld, flow_coff), wg, wg + plane, wg + 2 * plane);
    int st = vps_launch_status();
    if (st) return st;
    const long ntx = (W + FC_TC - 1) / FC_TC, nty = (H + FC_TR - 1) / FC_TR;        // at most 2^31 / 32 tiles: a valid grid dimension
    hipLaunchKernelGGL(flow_census_kernel, dim3((unsigned)(ntx * nty)), dim3(FC_THREADS), 0, s, (const float*)wg, (const float*)(wg + plane),
                       (const float*)(wg + 2 * plane), H, W, (int)ntx, mask_in, thr, eps, reinterpret_cast<unsigned long long*>(table), mask_out,
                       residual);
    return vps_launch_status();
}
