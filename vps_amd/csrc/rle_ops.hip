// Track tubes, device half (vps_amd/tubes.py): the run list of a panoptic map in the order COCO's run-length encoding reads it.
//   vps_rle_runs   uint8 [H][W][3] map -> (run_start, run_key): a run starts at position q = x * H + y (column-major) when q = 0 or
//                  key(q) != key(q - 1), key = ch0 * 256 + ch[id_channel]. A run that leaves column x at its bottom and goes on at
//                  the top of column x + 1 is ONE run. csrc/rle_host.cpp turns the list into COCO strings on the host.
// The start flag of pixel (y, x) needs the pixel above it, (H-1, x-1) for y = 0: the map is read row-major - a lane per column,
// adjacent lanes adjacent pixels - although the list is column-major. A cell is one column of a band of BAND rows. Three launches:
//   sweep 1  a thread per cell counts the starts of its cell                      -> cell[x][band]
//   scan     one block turns the counts into exclusive offsets in (column, band) order, which is ascending q, and leaves the total
//   sweep 2  the same walk; the thread writes its starts from its cell's offset on, in ascending q, below `cap` only
// Each sweep reads channel 0 and the id channel of every pixel once (and the row above each band once more). No atomics: the place
// of every run follows from the scan alone, so the list is the same on every call.
#include "common.h"

namespace {

constexpr int BAND = 32;                       // rows of a cell: 1024 x 2048 gives 32 bands x 16 column blocks = 512 blocks
constexpr int COLS = 128;                      // columns of a block, a thread each
constexpr int CHUNK = 8;                       // rows a thread loads before it looks at them
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_PER = 16;                   // cells per thread and step of the scan, four 16-byte loads

__device__ __forceinline__ uint32_t key_at(const uint8_t* __restrict__ pan, size_t pix, int idc) {
    const uint8_t* p = pan + pix * 3;
    return ((uint32_t)p[0] << 8) | p[idc];
}

static inline long pad_cells(long ncells) { return (ncells + SCAN_PER - 1) / SCAN_PER * SCAN_PER; }

template <bool WRITE>
__global__ __launch_bounds__(COLS)
void rle_sweep_kernel(const uint8_t* __restrict__ pan, int H, int W, int idc, int nbands, int col_blocks, int32_t* __restrict__ cell,
                      uint32_t* __restrict__ run_start, uint16_t* __restrict__ run_key, int cap) {
    const int band = blockIdx.x / col_blocks;
    const int x = (blockIdx.x - band * col_blocks) * COLS + threadIdx.x;
    if (x >= W) return;
    const int y0 = band * BAND, y1 = min(y0 + BAND, H);
    uint32_t prev = 0xFFFFFFFFu;                                         // no key: q = 0 starts a run
    if (y0 > 0) prev = key_at(pan, (size_t)(y0 - 1) * W + x, idc);
    else if (x > 0) prev = key_at(pan, (size_t)(H - 1) * W + (x - 1), idc);
    const size_t c = (size_t)x * nbands + band;
    int n = WRITE ? cell[c] : 0;
    for (int yb = y0; yb < y1; yb += CHUNK) {
        uint32_t k[CHUNK];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) k[j] = key_at(pan, (size_t)min(yb + j, y1 - 1) * W + x, idc);   // all loads before the first store
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            if (yb + j < y1 && k[j] != prev) {
                if (WRITE && n < cap) {
                    run_start[n] = (uint32_t)((size_t)x * H + (yb + j));
                    run_key[n] = (uint16_t)k[j];
                }
                ++n;
            }
            prev = k[j];
        }
    }
    if (!WRITE) cell[c] = n;
}

// exclusive scan of cell[0 .. ncells) in place; cell is padded to a multiple of SCAN_PER ints, so the 16-byte accesses stay inside it
__global__ __launch_bounds__(SCAN_THREADS)
void rle_scan_kernel(int32_t* __restrict__ cell, long ncells, int32_t* __restrict__ nruns) {
    __shared__ int32_t wave_sum[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t carry = 0;                                                   // the same value in every thread
    for (long base = 0; base < ncells; base += (long)SCAN_THREADS * SCAN_PER) {
        const long i0 = base + (long)threadIdx.x * SCAN_PER;
        int32_t v[SCAN_PER];
        int32_t t = 0;
        if (i0 < ncells) {
#pragma unroll
            for (int j = 0; j < SCAN_PER; j += 4) {
                const int4 q = *reinterpret_cast<const int4*>(cell + i0 + j);
                v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
            }
#pragma unroll
            for (int j = 0; j < SCAN_PER; ++j) {
                if (i0 + j >= ncells) v[j] = 0;                          // the padding holds anything
                t += v[j];
            }
        }
        int32_t inc = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t u = __shfl_up(inc, d, 64);
            if (lane >= d) inc += u;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            const int32_t s = wave_sum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i0 < ncells) {
            int32_t ex = carry + before + inc - t;
#pragma unroll
            for (int j = 0; j < SCAN_PER; j += 4) {
                int4 q;
                q.x = ex; ex += v[j];
                q.y = ex; ex += v[j + 1];
                q.z = ex; ex += v[j + 2];
                q.w = ex; ex += v[j + 3];
                *reinterpret_cast<int4*>(cell + i0 + j) = q;
            }
        }
        carry += total;
        __syncthreads();                                                 // wave_sum is written again in the next step
    }
    if (threadIdx.x == 0) nruns[0] = carry;
}

}  // namespace

extern "C" int vps_rle_band_rows(void) { return BAND; }

extern "C" int64_t vps_rle_runs_ws(int H, int W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    return (int64_t)pad_cells((long)W * cdiv(H, BAND)) * (int64_t)sizeof(int32_t);
}

extern "C" int vps_rle_runs(const uint8_t* pan_2ch, int H, int W, int id_channel, uint32_t* run_start, uint16_t* run_key, int cap,
                            int32_t* nruns, void* ws, size_t ws_bytes, void* stream) {
    if (!pan_2ch) return VPS_EARG(1);
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return VPS_EARG(2);
    if (id_channel != 1 && id_channel != 2) return VPS_EARG(4);
    if (!run_start || ((uintptr_t)run_start & 3)) return VPS_EARG(5);
    if (!run_key || ((uintptr_t)run_key & 1)) return VPS_EARG(6);
    if (cap < 0) return VPS_EARG(7);
    if (!nruns || ((uintptr_t)nruns & 3)) return VPS_EARG(8);
    if (!ws || ((uintptr_t)ws & 15) || (int64_t)ws_bytes < vps_rle_runs_ws(H, W)) return VPS_EARG(9);
    const int nbands = cdiv(H, BAND), col_blocks = cdiv(W, COLS);
    const long ncells = (long)W * nbands;
    const long nblocks = (long)nbands * col_blocks;                      // < 2^31 / 32 + a few
    int32_t* cell = static_cast<int32_t*>(ws);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rle_sweep_kernel<false>, dim3((unsigned)nblocks), dim3(COLS), 0, s, pan_2ch, H, W, id_channel, nbands, col_blocks, cell,
                       run_start, run_key, cap);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, cell, ncells, nruns);
    hipLaunchKernelGGL(rle_sweep_kernel<true>, dim3((unsigned)nblocks), dim3(COLS), 0, s, pan_2ch, H, W, id_channel, nbands, col_blocks, cell,
                       run_start, run_key, cap);
    return vps_launch_status();
}
