// Boundary PQ / boundary VPQ on the device (vps_amd/boundary.py): the band of every segment of a panoptic map.
//   vps_boundary_band      out = the map with the INTERIOR of every segment painted 0xFFFFFF: a pixel of id s != 0 is interior when the
//                          (2d+1) x (2d+1) window centred on it lies inside the image and holds s alone; every other pixel keeps its id.
// Two separable passes, neither of which looks at a window pixel by pixel:
//   row pass     per row segment of BND_TC columns plus a halo of d: P = prefix sum of "id differs from the left neighbour"; the
//                window [x-d, x+d] is uniform when P[x+d] == P[x-d]. Writes key = id | flag << 24, one dword per pixel, to the workspace.
//   column pass  one lane per column walks BND_TR rows plus a halo of d and keeps the last row whose key differs from the row above;
//                [y-d, y+d] is interior when key[y] carries the flag and no key changed in (y-d, y+d].
// Integer work, no atomics; every output byte is a function of the input map alone, whatever the launch geometry.
#include "common.h"

namespace {

constexpr int BND_THREADS = 256;
constexpr int BND_TC = 512;                           // row pass: columns one workgroup writes
constexpr int BND_TR = 32;                            // column pass: rows one lane writes
constexpr int BND_DMAX = 255;
constexpr int BND_SPAN = BND_TC + 2 * BND_DMAX + 2;   // 1024: the longest row segment with its two halos, a multiple of BND_THREADS
constexpr int BND_PER = BND_SPAN / BND_THREADS;       // 4 span pixels per lane in the scan
constexpr int BND_BATCH = 8;                          // column pass: rows loaded before they are looked at
constexpr uint32_t BND_FILL = 0xffffffu;
static_assert(BND_SPAN % BND_THREADS == 0 && BND_TC + 2 * BND_DMAX <= BND_SPAN, "span");

// One workgroup: row y, columns [x0, x0 + BND_TC). The span [lo, hi) = the columns with a halo of d, cut to the image.
__global__ __launch_bounds__(BND_THREADS)
void boundary_row_kernel(const uint8_t* __restrict__ pan, int H, int W, int d, int ntx, uint32_t* __restrict__ keys) {
    __shared__ uint32_t raw[(3 * BND_SPAN + 3) / 4 + 1];      // the span's bytes, from the aligned address in front of its first one
    __shared__ uint32_t ids[BND_SPAN];
    __shared__ uint16_t pre[BND_SPAN];                        // inclusive prefix sum of the changes (at most BND_SPAN - 1)
    __shared__ uint32_t wave_sum[BND_THREADS / 64];
    const int t = threadIdx.x;
    const long y = blockIdx.x / ntx;
    const int x0 = (int)(blockIdx.x % ntx) * BND_TC, x1 = min(x0 + BND_TC, W);
    const int lo = max(x0 - d, 0), hi = min(x1 + d, W), n = hi - lo;
    const long total = 3L * H * W, b0 = 3 * (y * W + lo);
    const int a = (int)((uintptr_t)(pan + b0) & 3);           // the dwords are aligned in memory, not in the map
    const int nd = (a + 3 * n + 3) >> 2;
    for (int k = t; k < nd; k += BND_THREADS) {
        const long off = b0 - a + 4L * k;
        uint32_t w = 0;
        if (off >= 0 && off + 4 <= total) {
            w = *reinterpret_cast<const uint32_t*>(pan + off);
        } else {                                              // a dword that reaches in front of the map or past its end
            for (int j = 0; j < 4; ++j)
                if (off + j >= 0 && off + j < total) w |= (uint32_t)pan[off + j] << (8 * j);
        }
        raw[k] = w;
    }
    __syncthreads();
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(raw) + a;
    for (int i = t; i < BND_SPAN; i += BND_THREADS)
        ids[i] = i < n ? (uint32_t)rb[3 * i] | ((uint32_t)rb[3 * i + 1] << 8) | ((uint32_t)rb[3 * i + 2] << 16) : 0u;
    __syncthreads();
    // lane t scans span pixels 4t .. 4t+3; a change at i means ids[i] != ids[i-1]; the span's first pixel counts as no change
    uint32_t loc[BND_PER], run = 0;
    uint32_t prev = t > 0 ? ids[BND_PER * t - 1] : ids[0];
#pragma unroll
    for (int j = 0; j < BND_PER; ++j) {
        const uint32_t v = ids[BND_PER * t + j];
        run += v != prev;
        loc[j] = run;
        prev = v;
    }
    uint32_t inc = run;                                       // inclusive scan of the lanes' totals over the wavefront
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    uint32_t base = inc - run;
    for (int w = 0; w < wv; ++w) base += wave_sum[w];
#pragma unroll
    for (int j = 0; j < BND_PER; ++j) pre[BND_PER * t + j] = (uint16_t)(base + loc[j]);
    __syncthreads();
    uint32_t* krow = keys + y * W;
    for (int x = x0 + t; x < x1; x += BND_THREADS) {
        const uint32_t s = ids[x - lo];
        bool flag = false;
        if (s != 0 && x - d >= 0 && x + d < W) flag = pre[x + d - lo] == pre[x - d - lo];
        krow[x] = s | ((uint32_t)flag << 24);
    }
}

// One workgroup: 256 columns, rows [y0, y0 + BND_TR). A lane owns one column and walks rows r = max(y0 - d, 0) .. y0 + BND_TR - 1 + d.
// last = the latest row whose key differs from the row above it; the first row walked, row 0 and every row below the image count as
// such. Row y = r - d is decided when row r has been seen: interior when its key carries the flag, y - d >= 0 and last <= y - d.
__global__ __launch_bounds__(BND_THREADS)
void boundary_col_kernel(const uint32_t* __restrict__ keys, int H, int W, int d, int nbx, uint8_t* __restrict__ out) {
    const int x = (int)(blockIdx.x % nbx) * BND_THREADS + threadIdx.x;
    const int y0 = (int)(blockIdx.x / nbx) * BND_TR, y1 = min(y0 + BND_TR, H);
    if (x >= W) return;
    const int rend = y1 - 1 + d;
    uint32_t prev = 0xffffffffu;                              // no key looks like this
    int last = 0;
    for (int r0 = max(y0 - d, 0); r0 <= rend; r0 += BND_BATCH) {
        uint32_t k[BND_BATCH], ky[BND_BATCH];
#pragma unroll
        for (int j = 0; j < BND_BATCH; ++j) {
            const int r = r0 + j, y = r - d;
            k[j] = r < H && r <= rend ? keys[(long)r * W + x] : 0xffffffffu;
            ky[j] = y >= y0 && r <= rend ? keys[(long)y * W + x] : 0u;
        }
#pragma unroll
        for (int j = 0; j < BND_BATCH; ++j) {
            const int r = r0 + j, y = r - d;
            if (r > rend) break;
            if (k[j] != prev || r >= H) last = r;
            prev = k[j];
            if (y >= y0) {
                const bool interior = (ky[j] >> 24) && y - d >= 0 && last <= y - d;
                const uint32_t v = interior ? BND_FILL : (ky[j] & 0xffffffu);
                uint8_t* o = out + 3 * ((long)y * W + x);
                o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
            }
        }
    }
}

int boundary_args(int H, int W, int d) {
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);
    if (d < 1 || d > BND_DMAX) return VPS_EARG(3);
    return 0;
}

}  // namespace

extern "C" int vps_boundary_band_ws(int H, int W, int d, int64_t* ws_bytes) {
    if (!ws_bytes) return VPS_EARG(1);
    *ws_bytes = 0;
    if (int e = boundary_args(H, W, d)) return e;
    *ws_bytes = 4 * (int64_t)H * W;                           // one key per pixel
    return 0;
}

extern "C" int vps_boundary_band(const uint8_t* pan_rgb, int H, int W, int d, uint8_t* out_rgb, void* ws, int64_t ws_bytes, void* stream) {
    if (!pan_rgb || !out_rgb || !ws) return VPS_EARG(1);
    if (int e = boundary_args(H, W, d)) return e;
    if (ws_bytes < 4 * (int64_t)H * W || ((uintptr_t)ws & 3)) return VPS_EARG(4);
    const int ntx = cdiv(W, BND_TC), nbx = cdiv(W, BND_THREADS), nby = cdiv(H, BND_TR);
    if ((long)ntx * H >= (1L << 31) || (long)nbx * nby >= (1L << 31)) return VPS_EARG(2);   // cannot happen below 2^31 pixels
    hipStream_t s = (hipStream_t)stream;
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws);
    hipLaunchKernelGGL(boundary_row_kernel, dim3((unsigned)((long)ntx * H)), dim3(BND_THREADS), 0, s, pan_rgb, H, W, d, ntx, keys);
    hipLaunchKernelGGL(boundary_col_kernel, dim3((unsigned)((long)nbx * nby)), dim3(BND_THREADS), 0, s, (const uint32_t*)keys, H, W, d, nbx, out_rgb);
    return vps_launch_status();
}

extern "C" int vps_boundary_tile(int32_t* rows_cols) {
    if (!rows_cols) return VPS_EARG(1);
    rows_cols[0] = BND_TR;
    rows_cols[1] = BND_TC;
    return 0;
}
