// PNG input, device half (the host half is vps_png_inflate in png_host.cpp): the filtered scanlines as zlib
// delivers them -> BGR uint8 [H][W][3], byte for byte what vps_png_decode_bgr8 makes of the same file.
//
// The filters (PNG specification 9.2) predict a byte from the byte C to its left (a), the byte above (b) and the byte above-left (c),
// all mod 256; Average and Paeth are not associative, so no scan applies. What the format does give:
//   - a row of type None or Sub (and row 0) reads nothing above it: such rows cut the image into independent GROUPS of rows;
//   - inside a group row r may produce pixel x once row r-1 has produced it: a skewed wavefront, one lane per row.
// png_groups_kernel (one block) reads the H filter bytes and writes the group table: gend[r] = one past the last row of the group
// that starts at row r, 0 for a row that starts none. png_wave_kernel runs one workgroup per row; those of rows that start no group
// leave at once, the others work their group through in BANDS of PNG_ROWS rows. In step s lane l rebuilds chunk s - l (PNG_K pixels)
// of its row and hands it to lane l + 1 through LDS; one barrier per step, trip counts from H, W, C and the table alone. No
// workgroup waits for another. The first row of a later band finds the row above in `out` (written by the same workgroup before the
// barrier that ended the previous band). The alpha channel of an RGBA file feeds nothing that is kept and is not rebuilt.
//
// Memory: rows are 1 + W*C bytes, so no row start is aligned to anything. A lane reads its row as ALIGNED dwords around each chunk
// and shifts them by the row's own misalignment; a dword is read only if it holds at least one byte of the row. The reads of a lane run
// PNG_D steps ahead of their use (a register ring), since nothing in them depends on rebuilt data. The BGR store is fused: three dword
// stores per full chunk where the output row is 4-byte aligned, byte stores otherwise.
//
// kitti_wave_kernel (further down) is the same wavefront for the 16-bit RGB scan of a KITTI flow file, with the flow decode fused.
#include "common.h"

namespace {

constexpr int PNG_ROWS = 256;      // rows of a band = lanes of the workgroup
constexpr int PNG_K = 4;           // pixels a lane rebuilds per step
constexpr int PNG_D = 4;           // chunks a lane has in flight (even: the LDS hand-off buffer of a step is d & 1)

__global__ __launch_bounds__(256) void png_groups_kernel(const uint8_t* __restrict__ scan, int H, size_t rowb, int32_t* __restrict__ gend) {
    __shared__ int32_t first[256];
    const int t = threadIdx.x;
    const int n = (H + 255) / 256;                                   // rows per thread, contiguous
    const int r0 = t * n, r1 = min(H, r0 + n);
    int f = H;                                                        // first group start among this thread's rows
    for (int r = r1 - 1; r >= r0; --r)
        if (r == 0 || scan[(size_t)r * rowb] < 2) f = r;
    first[t] = f;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                         // first[t] = min over threads >= t
        const int v = t + off < 256 ? first[t + off] : H;
        __syncthreads();
        first[t] = min(first[t], v);
        __syncthreads();
    }
    int nxt = t + 1 < 256 ? first[t + 1] : H;                         // the next start behind this thread's rows
    for (int r = r1 - 1; r >= r0; --r) {
        const bool start = r == 0 || scan[(size_t)r * rowb] < 2;
        gend[r] = start ? nxt : 0;
        if (start) nxt = r;
    }
}

template <int C>
__global__ __launch_bounds__(PNG_ROWS) void png_wave_kernel(const uint8_t* __restrict__ scan, int H, int W, const int32_t* __restrict__ gend,
                                                            uint8_t* out) {
    constexpr int CC = C < 3 ? C : 3;              // channels rebuilt
    constexpr int NBW = PNG_K * C / 4;             // dwords of a chunk of filtered bytes
    constexpr int NW = PNG_K * CC / 4;             // dwords of a rebuilt chunk (stored order, alpha left out)
    static_assert(PNG_D % 2 == 0 && (PNG_K * C) % 4 == 0 && (PNG_K * CC) % 4 == 0, "chunk layout");
    __shared__ uint32_t hand[2][NW][PNG_ROWS];     // [step parity][dword][lane]: lane l's fresh chunk for lane l + 1 (conflict-free both ways)
    const int g0 = blockIdx.x;
    const int g1 = gend[g0];
    if (g1 == 0) return;                           // this row starts no group (the whole workgroup leaves)
    const int l = threadIdx.x;
    const size_t rowb = (size_t)W * C + 1;
    const int nchunks = (W + PNG_K - 1) / PNG_K;

    for (int y0 = g0; y0 < g1; y0 += PNG_ROWS) {
        const int nr = min(PNG_ROWS, g1 - y0);
        const bool active = l < nr;
        const int y = active ? y0 + l : y0;        // an idle lane computes addresses of a valid row and touches nothing
        const uint8_t* p = scan + (size_t)y * rowb + 1;
        const int ft = p[-1];
        const uint8_t* rend = p + (size_t)W * C;
        const unsigned sh8 = 8u * (unsigned)((uintptr_t)p & 3);
        const uint32_t* pw = (const uint32_t*)(p - ((uintptr_t)p & 3));
        uint8_t* orow = out + (size_t)y * W * 3;
        const bool oal = ((uintptr_t)orow & 3) == 0;
        const bool from_out = l == 0 && y0 > g0;   // first row of a later band: the row above is the previous band's last, in `out`
        const uint8_t* urow = orow - (size_t)W * 3;

        // filtered bytes of chunk j as NBW + 1 aligned dwords (zeros outside the row)
        auto load_raw = [&](int j, uint32_t (&w)[NBW + 1]) {
#pragma unroll
            for (int k = 0; k <= NBW; ++k) w[k] = 0;
            if (active && j >= 0 && j < nchunks) {
                const uint32_t* q = pw + (size_t)j * NBW;
#pragma unroll
                for (int k = 0; k <= NBW; ++k)
                    if ((const uint8_t*)(q + k) < rend) w[k] = q[k];
            }
        };
        // chunk j of the row above, read back from the BGR output in stored channel order
        auto load_up = [&](int j, uint32_t (&u)[NW]) {
#pragma unroll
            for (int k = 0; k < NW; ++k) u[k] = 0;
            if (from_out && j >= 0 && j < nchunks) {
#pragma unroll
                for (int px = 0; px < PNG_K; ++px) {
                    const int x = j * PNG_K + px;
                    if (x < W) {
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) {
                            const int i = px * CC + ch;
                            u[i / 4] |= (uint32_t)urow[(size_t)x * 3 + (C == 1 ? 0 : 2 - ch)] << (8 * (i % 4));
                        }
                    }
                }
            }
        };

        uint32_t ring[PNG_D][NBW + 1], upg[PNG_D][NW];
#pragma unroll
        for (int d = 0; d < PNG_D; ++d) {
            load_raw(d - l, ring[d]);
            load_up(d - l, upg[d]);
        }
        int a[CC], c[CC];                          // the pixel to the left, rebuilt, and the one above it
#pragma unroll
        for (int k = 0; k < CC; ++k) a[k] = c[k] = 0;

        const int steps = nchunks + nr - 1;
        for (int s0 = 0; s0 < steps; s0 += PNG_D) {
#pragma unroll
            for (int d = 0; d < PNG_D; ++d) {
                const int j = s0 + d - l;          // this lane's chunk in this step
                if (active && j >= 0 && j < nchunks) {
                    uint32_t v[NBW], u[NW], r[NW];
#pragma unroll
                    for (int k = 0; k < NBW; ++k) v[k] = (uint32_t)((((uint64_t)ring[d][k + 1] << 32) | ring[d][k]) >> sh8);
#pragma unroll
                    for (int k = 0; k < NW; ++k) {
                        u[k] = l > 0 ? hand[(d + 1) & 1][k][l - 1] : upg[d][k];      // lane 0 of the first band: zeros (no row above)
                        r[k] = 0;
                    }
#pragma unroll
                    for (int px = 0; px < PNG_K; ++px) {
#pragma unroll
                        for (int ch = 0; ch < CC; ++ch) {
                            const int ib = px * C + ch, iu = px * CC + ch, ic = (px - 1) * CC + ch;
                            const int x = (v[ib / 4] >> (8 * (ib % 4))) & 255;
                            const int b = (u[iu / 4] >> (8 * (iu % 4))) & 255;
                            const int cc = px == 0 ? c[ch] : (int)((u[(ic < 0 ? 0 : ic) / 4] >> (8 * ((ic < 0 ? 0 : ic) % 4))) & 255);
                            const int aa = a[ch];
                            // Paeth predictor, the decoder's form: a unless b is strictly nearer, c only if strictly nearer than both
                            const int pp = b - cc, pc0 = aa - cc;
                            const int pa = abs(pp), pb = abs(pc0), pc = abs(pp + pc0);
                            int pred = pb < pa ? b : aa;
                            pred = pc < min(pa, pb) ? cc : pred;
                            pred = ft == 3 ? (aa + b) >> 1 : pred;
                            pred = ft == 2 ? b : pred;
                            pred = ft == 1 ? aa : pred;
                            pred = ft == 0 ? 0 : pred;
                            const int val = (x + pred) & 255;
                            a[ch] = val;
                            r[iu / 4] |= (uint32_t)val << (8 * (iu % 4));
                        }
                    }
#pragma unroll
                    for (int ch = 0; ch < CC; ++ch) {
                        const int ic = (PNG_K - 1) * CC + ch;
                        c[ch] = (u[ic / 4] >> (8 * (ic % 4))) & 255;
                    }
#pragma unroll
                    for (int k = 0; k < NW; ++k) hand[d & 1][k][l] = r[k];
                    // BGR store: grey replicated, R and B swapped
                    const int x0 = j * PNG_K;
                    uint8_t* o = orow + (size_t)x0 * 3;
                    if (oal && x0 + PNG_K <= W) {
                        uint32_t ob[3] = {0, 0, 0};
#pragma unroll
                        for (int t = 0; t < 3 * PNG_K; ++t) {
                            const int i = (t / 3) * CC + (C == 1 ? 0 : 2 - t % 3);
                            ob[t / 4] |= ((r[i / 4] >> (8 * (i % 4))) & 255u) << (8 * (t % 4));
                        }
#pragma unroll
                        for (int k = 0; k < 3; ++k) ((uint32_t*)o)[k] = ob[k];
                    } else {
#pragma unroll
                        for (int px = 0; px < PNG_K; ++px)
                            if (x0 + px < W) {
#pragma unroll
                                for (int oc = 0; oc < 3; ++oc) {
                                    const int i = px * CC + (C == 1 ? 0 : 2 - oc);
                                    o[px * 3 + oc] = (uint8_t)(r[i / 4] >> (8 * (i % 4)));
                                }
                            }
                    }
                }
                load_raw(j + PNG_D, ring[d]);
                load_up(j + PNG_D, upg[d]);
                __syncthreads();                   // every lane, every step: the chunk is in LDS (and in `out`) before the next step reads it
            }
        }
    }
}

// KITTI flow files (include/vps_hip.h, vps_kitti_flow_reconstruct): the same wavefront over a 16-bit RGB scan, 6 bytes per pixel, with the
// flow decode fused behind the un-filter: a rebuilt chunk of PNG_K pixels leaves as PNG_K (u, v) pairs and PNG_K mask bytes. The decoded
// flow no longer holds the raw bytes (B is gone, R and G of an invalid pixel too), so the row above a later band cannot be read back from
// the output: the lane of a band's last row also stores its raw chunks to the band's slot of `carry`, and lane 0 of the next band reads
// them from there (same workgroup, behind the barrier that ended the band). Bands of different groups never share a slot: a band that
// is carried is full, full bands are disjoint runs of PNG_ROWS rows, so their last rows fall into different multiples of PNG_ROWS.
constexpr int KF_C = 6;                            // bytes per pixel
constexpr int KF_NW = PNG_K * KF_C / 4;            // dwords of a chunk, filtered or rebuilt

__device__ __forceinline__ uint32_t kf_byte(const uint32_t (&r)[KF_NW], int i) { return (r[i / 4] >> (8 * (i % 4))) & 255u; }

__global__ __launch_bounds__(PNG_ROWS) void kitti_wave_kernel(const uint8_t* __restrict__ scan, int H, int W, const int32_t* __restrict__ gend,
                                                              const uint8_t* __restrict__ noc, uint32_t* carry, float* __restrict__ flow,
                                                              uint8_t* __restrict__ mask) {
    static_assert(PNG_D % 2 == 0 && (PNG_K * KF_C) % 4 == 0, "chunk layout");
    __shared__ uint32_t hand[2][KF_NW][PNG_ROWS];  // [step parity][dword][lane]: lane l's fresh chunk for lane l + 1
    const int g0 = blockIdx.x;
    const int g1 = gend[g0];
    if (g1 == 0) return;                           // this row starts no group (the whole workgroup leaves)
    const int l = threadIdx.x;
    const size_t rowb = (size_t)W * KF_C + 1;
    const int nchunks = (W + PNG_K - 1) / PNG_K;
    const size_t cstride = (size_t)nchunks * KF_NW;                    // dwords of a carried row

    for (int y0 = g0; y0 < g1; y0 += PNG_ROWS) {
        const int nr = min(PNG_ROWS, g1 - y0);
        const bool active = l < nr;
        const int y = active ? y0 + l : y0;        // an idle lane computes addresses of a valid row and touches nothing
        const uint8_t* p = scan + (size_t)y * rowb + 1;
        const int ft = p[-1];
        const uint8_t* rend = p + (size_t)W * KF_C;
        const unsigned sh8 = 8u * (unsigned)((uintptr_t)p & 3);
        const uint32_t* pw = (const uint32_t*)(p - ((uintptr_t)p & 3));
        float* frow = flow + (size_t)y * W * 2;
        uint8_t* mrow = mask + (size_t)y * W;
        const uint8_t* nrow = noc ? noc + (size_t)y * W : nullptr;
        const bool fal = ((uintptr_t)frow & 15) == 0, mal = ((uintptr_t)mrow & 3) == 0, nal = ((uintptr_t)nrow & 3) == 0;
        const bool from_carry = l == 0 && y0 > g0; // first row of a later band: the row above is the previous band's last, raw, in `carry`
        const bool to_carry = active && l == PNG_ROWS - 1 && y0 + PNG_ROWS < g1;       // this lane's row is the one the next band needs
        const uint32_t* cin = carry + (size_t)((y0 > 0 ? y0 - 1 : 0) / PNG_ROWS) * cstride;
        uint32_t* cout = carry + (size_t)(y / PNG_ROWS) * cstride;

        // filtered bytes of chunk j as KF_NW + 1 aligned dwords (zeros outside the row)
        auto load_raw = [&](int j, uint32_t (&w)[KF_NW + 1]) {
#pragma unroll
            for (int k = 0; k <= KF_NW; ++k) w[k] = 0;
            if (active && j >= 0 && j < nchunks) {
                const uint32_t* q = pw + (size_t)j * KF_NW;
#pragma unroll
                for (int k = 0; k <= KF_NW; ++k)
                    if ((const uint8_t*)(q + k) < rend) w[k] = q[k];
            }
        };
        // chunk j of the row above, raw, from the carried row
        auto load_up = [&](int j, uint32_t (&u)[KF_NW]) {
#pragma unroll
            for (int k = 0; k < KF_NW; ++k) u[k] = 0;
            if (from_carry && j >= 0 && j < nchunks) {
#pragma unroll
                for (int k = 0; k < KF_NW; ++k) u[k] = cin[(size_t)j * KF_NW + k];
            }
        };
        // the PNG_K bytes of the noc file's mask for chunk j (non-zero = valid there)
        auto load_noc = [&](int j) -> uint32_t {
            uint32_t w = 0;
            if (nrow && active && j >= 0 && j < nchunks) {
                const int x0 = j * PNG_K;
                if (nal && x0 + PNG_K <= W) w = *(const uint32_t*)(nrow + x0);
                else
#pragma unroll
                    for (int px = 0; px < PNG_K; ++px)
                        if (x0 + px < W) w |= (uint32_t)nrow[x0 + px] << (8 * px);
            }
            return w;
        };

        uint32_t ring[PNG_D][KF_NW + 1], upg[PNG_D][KF_NW], nocr[PNG_D];
#pragma unroll
        for (int d = 0; d < PNG_D; ++d) {
            load_raw(d - l, ring[d]);
            load_up(d - l, upg[d]);
            nocr[d] = load_noc(d - l);
        }
        int a[KF_C], c[KF_C];                      // the pixel to the left, rebuilt, and the one above it (byte by byte)
#pragma unroll
        for (int k = 0; k < KF_C; ++k) a[k] = c[k] = 0;

        const int steps = nchunks + nr - 1;
        for (int s0 = 0; s0 < steps; s0 += PNG_D) {
#pragma unroll
            for (int d = 0; d < PNG_D; ++d) {
                const int j = s0 + d - l;          // this lane's chunk in this step
                if (active && j >= 0 && j < nchunks) {
                    uint32_t v[KF_NW], u[KF_NW], r[KF_NW];
#pragma unroll
                    for (int k = 0; k < KF_NW; ++k) {
                        v[k] = (uint32_t)((((uint64_t)ring[d][k + 1] << 32) | ring[d][k]) >> sh8);
                        u[k] = l > 0 ? hand[(d + 1) & 1][k][l - 1] : upg[d][k];      // lane 0 of the first band: zeros (no row above)
                        r[k] = 0;
                    }
#pragma unroll
                    for (int px = 0; px < PNG_K; ++px) {
#pragma unroll
                        for (int ch = 0; ch < KF_C; ++ch) {
                            const int i = px * KF_C + ch;
                            const int x = (int)kf_byte(v, i);
                            const int b = (int)kf_byte(u, i);
                            const int cc = px == 0 ? c[ch] : (int)kf_byte(u, px == 0 ? 0 : i - KF_C);
                            const int aa = a[ch];
                            // Paeth predictor, the decoder's form: a unless b is strictly nearer, c only if strictly nearer than both
                            const int pp = b - cc, pc0 = aa - cc;
                            const int pa = abs(pp), pb = abs(pc0), pc = abs(pp + pc0);
                            int pred = pb < pa ? b : aa;
                            pred = pc < min(pa, pb) ? cc : pred;
                            pred = ft == 3 ? (aa + b) >> 1 : pred;
                            pred = ft == 2 ? b : pred;
                            pred = ft == 1 ? aa : pred;
                            pred = ft == 0 ? 0 : pred;
                            const int val = (x + pred) & 255;
                            a[ch] = val;
                            r[i / 4] |= (uint32_t)val << (8 * (i % 4));
                        }
                    }
#pragma unroll
                    for (int ch = 0; ch < KF_C; ++ch) c[ch] = (int)kf_byte(u, (PNG_K - 1) * KF_C + ch);
#pragma unroll
                    for (int k = 0; k < KF_NW; ++k) hand[d & 1][k][l] = r[k];
                    if (to_carry) {
#pragma unroll
                        for (int k = 0; k < KF_NW; ++k) cout[(size_t)j * KF_NW + k] = r[k];
                    }
                    // decode: big-endian R, G, B; valid iff B > 0; u = (R - 32768) / 64, v likewise from G (exact in fp32); invalid reads (0, 0)
                    float fu[PNG_K], fv[PNG_K];
                    uint32_t mk = 0;
#pragma unroll
                    for (int px = 0; px < PNG_K; ++px) {
                        const int i = px * KF_C;
                        const int R = (int)((kf_byte(r, i) << 8) | kf_byte(r, i + 1)), G = (int)((kf_byte(r, i + 2) << 8) | kf_byte(r, i + 3));
                        const bool valid = (kf_byte(r, i + 4) | kf_byte(r, i + 5)) != 0;
                        fu[px] = valid ? (float)(R - 32768) * 0.015625f : 0.0f;
                        fv[px] = valid ? (float)(G - 32768) * 0.015625f : 0.0f;
                        const uint32_t code = !valid ? 0u : ((!nrow || ((nocr[d] >> (8 * px)) & 255u)) ? 1u : 2u);
                        mk |= code << (8 * px);
                    }
                    const int x0 = j * PNG_K;
                    if (x0 + PNG_K <= W) {
                        if (fal) {
#pragma unroll
                            for (int k = 0; k < PNG_K / 2; ++k)
                                ((float4*)(frow + (size_t)x0 * 2))[k] = make_float4(fu[2 * k], fv[2 * k], fu[2 * k + 1], fv[2 * k + 1]);
                        } else {
#pragma unroll
                            for (int px = 0; px < PNG_K; ++px) ((float2*)frow)[x0 + px] = make_float2(fu[px], fv[px]);
                        }
                        if (mal) *(uint32_t*)(mrow + x0) = mk;
                        else
#pragma unroll
                            for (int px = 0; px < PNG_K; ++px) mrow[x0 + px] = (uint8_t)(mk >> (8 * px));
                    } else {
#pragma unroll
                        for (int px = 0; px < PNG_K; ++px)
                            if (x0 + px < W) {
                                ((float2*)frow)[x0 + px] = make_float2(fu[px], fv[px]);
                                mrow[x0 + px] = (uint8_t)(mk >> (8 * px));
                            }
                    }
                }
                load_raw(j + PNG_D, ring[d]);
                load_up(j + PNG_D, upg[d]);
                nocr[d] = load_noc(j + PNG_D);
                __syncthreads();                   // every lane, every step: the chunk is in LDS (and in `carry`) before the next step reads it
            }
        }
    }
}

}  // namespace

extern "C" int vps_png_reconstruct_block_rows(void) { return PNG_ROWS; }

extern "C" int vps_png_reconstruct_ws(int H, int W, int channels, int64_t* ws_bytes) {
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || !ws_bytes) return VPS_EARG(1);
    if (channels != 1 && channels != 3 && channels != 4) return VPS_EARG(2);
    *ws_bytes = ((int64_t)H * 4 + 15) & ~(int64_t)15;                  // the group table: int32 per row
    return 0;
}

extern "C" int vps_png_reconstruct(const uint8_t* scan, int H, int W, int channels, uint8_t* out_bgr, int64_t out_capacity,
                                   void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t need = 0;
    const int st = vps_png_reconstruct_ws(H, W, channels, &need);
    if (st) return st;
    if (!scan || !out_bgr || !ws) return VPS_EARG(1);
    if (((uintptr_t)ws & 3)) return VPS_EARG(3);
    if (out_capacity < (int64_t)H * W * 3) return VPS_EARG(4);
    if (ws_bytes < need) return VPS_EARG(6);
    int32_t* gend = (int32_t*)ws;
    hipLaunchKernelGGL(png_groups_kernel, dim3(1), dim3(256), 0, stream, scan, H, (size_t)W * channels + 1, gend);
    if (channels == 1) hipLaunchKernelGGL(png_wave_kernel<1>, dim3(H), dim3(PNG_ROWS), 0, stream, scan, H, W, (const int32_t*)gend, out_bgr);
    else if (channels == 3) hipLaunchKernelGGL(png_wave_kernel<3>, dim3(H), dim3(PNG_ROWS), 0, stream, scan, H, W, (const int32_t*)gend, out_bgr);
    else hipLaunchKernelGGL(png_wave_kernel<4>, dim3(H), dim3(PNG_ROWS), 0, stream, scan, H, W, (const int32_t*)gend, out_bgr);
    return vps_launch_status();
}

// workspace of vps_kitti_flow_reconstruct: the group table, then one raw row (whole chunks) per run of PNG_ROWS rows
static inline int64_t kitti_table_bytes(int H) { return ((int64_t)H * 4 + 15) & ~(int64_t)15; }

extern "C" int vps_kitti_flow_reconstruct_ws(int H, int W, int64_t* ws_bytes) {
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535 || !ws_bytes) return VPS_EARG(1);
    const int64_t nchunks = (W + PNG_K - 1) / PNG_K, slots = (H + PNG_ROWS - 1) / PNG_ROWS;
    *ws_bytes = kitti_table_bytes(H) + slots * nchunks * KF_NW * 4;
    return 0;
}

extern "C" int vps_kitti_flow_reconstruct(const uint8_t* scan, int H, int W, const uint8_t* noc_valid, float* flow, int64_t flow_capacity,
                                          uint8_t* mask, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t need = 0;
    const int st = vps_kitti_flow_reconstruct_ws(H, W, &need);
    if (st) return st;
    if (!scan || !flow || !mask || !ws) return VPS_EARG(1);
    if (((uintptr_t)ws & 3) || ((uintptr_t)flow & 15)) return VPS_EARG(3);
    if (flow_capacity < (int64_t)H * W * 8) return VPS_EARG(4);
    if (ws_bytes < need) return VPS_EARG(6);
    int32_t* gend = (int32_t*)ws;
    uint32_t* carry = (uint32_t*)((uint8_t*)ws + kitti_table_bytes(H));
    hipLaunchKernelGGL(png_groups_kernel, dim3(1), dim3(256), 0, stream, scan, H, (size_t)W * KF_C + 1, gend);
    hipLaunchKernelGGL(kitti_wave_kernel, dim3(H), dim3(PNG_ROWS), 0, stream, scan, H, W, (const int32_t*)gend, noc_valid, carry, flow, mask);
    return vps_launch_status();
}
