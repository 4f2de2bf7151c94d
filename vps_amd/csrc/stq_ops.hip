// STQ video evaluation on the device (vps_amd/stq.py): the counting pass of Segmentation and Tracking Quality.
//   vps_stq_accumulate     one frame's (gt segment, predicted segment) pixel pairs ADDED to the video's four int64 tables: the class
//                          confusion matrix, the size of every gt track and predicted track, and their intersections. The tables stay
//                          on the device for the whole video; nothing is zeroed, downloaded or synchronised here.
// Integer work: the result does not depend on the order of the adds, so two runs give identical tables.
#include "common.h"

namespace {

constexpr int STQ_THREADS = 256;
constexpr int STQ_PIX = 4;                            // pixels per lane and step: 12 bytes = 3 dwords of each map
constexpr int STQ_LDS_CELLS = 12288;                  // 48 KiB of uint32 cells per workgroup: 3 workgroups in the 160 KiB of a CU
constexpr long STQ_MAX_CELLS = 1L << 26;              // all four tables together: 512 MiB of int64

struct StqTables { unsigned long long *conf, *gt_size, *pred_size, *inter; };

__device__ __forceinline__ int stq_id_index(const uint32_t* __restrict__ ids, int n, uint32_t v) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {                                // sorted, unique
        const int mid = (lo + hi) >> 1;
        const uint32_t m = ids[mid];
        if (m == v) return mid;
        if (m < v) lo = mid + 1; else hi = mid - 1;
    }
    return n;                                         // not listed
}

// The ids of pixels 4 * ch .. 4 * ch + n - 1 of a [npix][3] byte map whose base need not be dword-aligned. The 12 bytes sit in 3 aligned
// dwords (4 when the base is off a dword boundary); they are loaded as dwords and shifted into place. A chunk whose dwords would reach
// in front of the base or past byte 3 * npix (the first one of an unaligned map, the last one or two of any map) is read byte by byte.
__device__ __forceinline__ void stq_load_ids(const uint8_t* __restrict__ p, long nbytes, long ch, int n, uint32_t (&id)[STQ_PIX]) {
    const unsigned o = (unsigned)((uintptr_t)p & 3);
    const long b0 = 12 * ch;                          // first byte of the chunk's dwords, counted from the aligned address p - o
    if (b0 >= (long)o && b0 + (o ? 16 : 12) <= (long)o + nbytes) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p - o) + 3 * ch;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = o ? w[3] : 0u;
        const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, o), d1 = __builtin_amdgcn_alignbyte(w2, w1, o),
                       d2 = __builtin_amdgcn_alignbyte(w3, w2, o);
        id[0] = d0 & 0xffffffu;
        id[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
        id[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
        id[3] = d2 >> 8;
    } else {
#pragma unroll
        for (int i = 0; i < STQ_PIX; ++i) {
            id[i] = 0;
            if (i < n) {
                const uint8_t* a = p + b0 + 3 * i;
                id[i] = a[0] | (a[1] << 8) | (a[2] << 16);
            }
        }
    }
}

// the cells one (G, P) pair adds to; -1 = none
struct StqCells { int conf, gt, pred, inter; };

template <bool LDS>
__device__ __forceinline__ void stq_add(const StqCells& c, uint32_t n, uint32_t* tab, int o_gt, int o_pred, int o_inter, const StqTables& t) {
    if (LDS) {
        if (c.conf >= 0) atomicAdd(&tab[c.conf], n);
        if (c.gt >= 0) atomicAdd(&tab[o_gt + c.gt], n);
        if (c.pred >= 0) atomicAdd(&tab[o_pred + c.pred], n);
        if (c.inter >= 0) atomicAdd(&tab[o_inter + c.inter], n);
    } else {
        if (c.conf >= 0) atomicAdd(&t.conf[c.conf], (unsigned long long)n);
        if (c.gt >= 0) atomicAdd(&t.gt_size[c.gt], (unsigned long long)n);
        if (c.pred >= 0) atomicAdd(&t.pred_size[c.pred], (unsigned long long)n);
        if (c.inter >= 0) atomicAdd(&t.inter[c.inter], (unsigned long long)n);
    }
}

// Masks are contiguous: each lane folds the equal neighbouring (G, P) pairs of its 4 pixels in registers and resolves a pair to its
// cells once per run; the run a lane ends with is compared across the wavefront, and where every lane holds the same pair (the inside
// of a region) the lengths are summed by shuffles and one lane adds them. LDS = true: the adds go to the workgroup's own uint32 image
// of the four tables (conf | gt_size | pred_size | inter) and the workgroup adds its non-zero cells to the caller's int64 tables once.
// LDS = false (tables larger than STQ_LDS_CELLS): every add is a 64-bit global atomic. No workgroup reads what another one writes.
template <bool LDS>
__global__ __launch_bounds__(STQ_THREADS)
void stq_accumulate_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred, long npix, const uint32_t* __restrict__ gt_ids,
                           const uint8_t* __restrict__ gt_info, int ngt, const uint32_t* __restrict__ pred_ids,
                           const uint8_t* __restrict__ pred_info, int npred, int C, StqTables t) {
    extern __shared__ uint32_t stq_tab[];
    const int o_gt = C * (C + 1), o_pred = o_gt + ngt, o_inter = o_pred + npred + 1, cells = o_inter + ngt * npred;
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += STQ_THREADS) stq_tab[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long nbytes = 3 * npix, nchunk = (npix + STQ_PIX - 1) / STQ_PIX;
    for (long ch0 = (long)blockIdx.x * STQ_THREADS; ch0 < nchunk; ch0 += (long)gridDim.x * STQ_THREADS) {     // uniform per workgroup
        const long ch = ch0 + threadIdx.x;
        uint32_t run_g = 0xffffffffu, run_p = 0xffffffffu, run_len = 0;       // ids are below 2^24
        StqCells cell = {-1, -1, -1, -1};
        if (ch < nchunk) {
            const int n = (int)min((long)STQ_PIX, npix - STQ_PIX * ch);
            uint32_t G[STQ_PIX], P[STQ_PIX];
            stq_load_ids(gt, nbytes, ch, n, G);
            stq_load_ids(pred, nbytes, ch, n, P);
#pragma unroll
            for (int i = 0; i < STQ_PIX; ++i) {
                if (i >= n) break;
                if (G[i] != run_g || P[i] != run_p) {
                    if (run_len) stq_add<LDS>(cell, run_len, stq_tab, o_gt, o_pred, o_inter, t);
                    run_g = G[i]; run_p = P[i]; run_len = 0;
                    // ---- the definition's per-pixel rules, once per run
                    int gi = -1, cg = C; bool gthing = false, crowd = false;
                    if (run_g) {
                        gi = stq_id_index(gt_ids, ngt, run_g);
                        if (gi < ngt) {
                            const int info = gt_info[gi];
                            if ((info & 63) < C) { cg = info & 63; gthing = info & 64; crowd = gthing && (info & 128); }
                        }
                    }
                    int pi = -1, cp = C; bool pthing = false, unlisted = false;
                    if (run_p) {
                        pi = stq_id_index(pred_ids, npred, run_p);
                        if (pi < npred) {
                            const int info = pred_info[pi];
                            if ((info & 63) < C) { cp = info & 63; pthing = info & 64; }
                        } else {
                            unlisted = true;
                        }
                    }
                    const bool gt_track = gthing && !crowd, pred_track = pthing && !crowd;
                    cell.conf = cg != C ? cg * (C + 1) + cp : -1;
                    cell.gt = gt_track ? gi : -1;
                    cell.pred = unlisted ? npred : (pred_track ? pi : -1);
                    cell.inter = gt_track && pred_track ? gi * npred + pi : -1;
                }
                ++run_len;
            }
        }
        // the run each lane is left with: one add per wavefront where all of them are the same pair
        const bool has = run_len > 0;
        const unsigned long long act = __ballot(has);
        if (act) {
            const int src = __ffsll((long long)act) - 1;
            const uint32_t fg = __shfl(run_g, src, 64), fp = __shfl(run_p, src, 64);
            if (__ballot(has && (run_g != fg || run_p != fp)) == 0) {
                uint32_t sum = has ? run_len : 0;
                for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
                if (lane == src) stq_add<LDS>(cell, sum, stq_tab, o_gt, o_pred, o_inter, t);
            } else if (has) {
                stq_add<LDS>(cell, run_len, stq_tab, o_gt, o_pred, o_inter, t);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += STQ_THREADS) {
            const uint32_t v = stq_tab[i];
            if (!v) continue;
            unsigned long long* dst = i < o_gt ? t.conf + i : i < o_pred ? t.gt_size + (i - o_gt) : i < o_inter ? t.pred_size + (i - o_pred)
                                                                                                          : t.inter + (i - o_inter);
            atomicAdd(dst, (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" int vps_stq_accumulate(const uint8_t* gt_rgb, const uint8_t* pred_rgb, int64_t npix, const uint32_t* gt_ids, const uint8_t* gt_info,
                                  int ngt, const uint32_t* pred_ids, const uint8_t* pred_info, int npred, int num_classes, int64_t* conf,
                                  int64_t* gt_size, int64_t* pred_size, int64_t* inter, void* stream) {
    if (!gt_rgb || !pred_rgb || !conf || !pred_size) return VPS_EARG(1);
    if (npix <= 0 || npix > 0x7fffffffL) return VPS_EARG(2);                   // a workgroup's uint32 cells cannot wrap
    if (num_classes < 1 || num_classes > 63) return VPS_EARG(3);
    if (ngt < 0 || npred < 0) return VPS_EARG(4);
    if ((ngt > 0 && (!gt_ids || !gt_info || !gt_size)) || (npred > 0 && (!pred_ids || !pred_info)) || (ngt > 0 && npred > 0 && !inter))
        return VPS_EARG(1);
    const long cells = (long)num_classes * (num_classes + 1) + ngt + npred + 1 + (long)ngt * npred;
    if (cells > STQ_MAX_CELLS) return VPS_EARG(5);
    if (((uintptr_t)conf | (uintptr_t)gt_size | (uintptr_t)pred_size | (uintptr_t)inter) & 7) return VPS_EARG(6);
    StqTables t = {reinterpret_cast<unsigned long long*>(conf), reinterpret_cast<unsigned long long*>(gt_size),
                   reinterpret_cast<unsigned long long*>(pred_size), reinterpret_cast<unsigned long long*>(inter)};
    const long nchunk = (npix + STQ_PIX - 1) / STQ_PIX;
    long g = nchunk / (STQ_THREADS * 4); if (g > 512) g = 512; if (g < 1) g = 1;          // >= 4 chunks per lane, <= 2 workgroups per CU
    hipStream_t s = (hipStream_t)stream;
    if (cells <= STQ_LDS_CELLS)                                                             // the path depends on the table sizes alone
        hipLaunchKernelGGL(stq_accumulate_kernel<true>, dim3((unsigned)g), dim3(STQ_THREADS), sizeof(uint32_t) * cells, s, gt_rgb, pred_rgb,
                           (long)npix, gt_ids, gt_info, ngt, pred_ids, pred_info, npred, num_classes, t);
    else
        hipLaunchKernelGGL(stq_accumulate_kernel<false>, dim3((unsigned)g), dim3(STQ_THREADS), 0, s, gt_rgb, pred_rgb, (long)npix, gt_ids,
                           gt_info, ngt, pred_ids, pred_info, npred, num_classes, t);
    return vps_launch_status();
}

// the largest number of table cells (conf + gt_size + pred_size + inter) that takes the workgroup-private path
extern "C" int vps_stq_lds_cells(void) { return STQ_LDS_CELLS; }
