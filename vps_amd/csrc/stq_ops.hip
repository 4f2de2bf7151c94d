// STQ video evaluation on the device (vps_amd/stq.py): the counting pass of Segmentation and Tracking Quality.
//   vps_stq_accumulate     one frame's (gt segment, predicted segment) pixel pairs ADDED to the video's four int64 tables: the class
//                          confusion matrix, the size of every gt track and predicted track, and their intersections. The tables stay
//                          on the device for the whole video; nothing is zeroed, downloaded or synchronised here.
// Integer work: the result does not depend on the order of the adds, so two runs give identical tables.
#include "px4.h"

namespace {

constexpr int STQ_THREADS = 256;
constexpr int STQ_LDS_CELLS = 12288;                  // 48 KiB of uint32 cells per workgroup: 3 workgroups in the 160 KiB of a CU
constexpr long STQ_MAX_CELLS = 1L << 26;              // all four tables together: 512 MiB of int64

struct StqTables { unsigned long long *conf, *gt_size, *pred_size, *inter; };

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
    const long nbytes = 3 * npix, nchunk = (npix + PX4 - 1) / PX4;
    for (long ch0 = (long)blockIdx.x * STQ_THREADS; ch0 < nchunk; ch0 += (long)gridDim.x * STQ_THREADS) {     // uniform per workgroup
        const long ch = ch0 + threadIdx.x;
        uint32_t run_g = 0xffffffffu, run_p = 0xffffffffu, run_len = 0;       // ids are below 2^24
        StqCells cell = {-1, -1, -1, -1};
        if (ch < nchunk) {
            const int n = (int)min((long)PX4, npix - PX4 * ch);
            uint32_t G[PX4], P[PX4];
            px4_load_px3(gt, nbytes, ch, n, G);
            px4_load_px3(pred, nbytes, ch, n, P);
#pragma unroll
            for (int i = 0; i < PX4; ++i) {
                if (i >= n) break;
                if (G[i] != run_g || P[i] != run_p) {
                    if (run_len) stq_add<LDS>(cell, run_len, stq_tab, o_gt, o_pred, o_inter, t);
                    run_g = G[i]; run_p = P[i]; run_len = 0;
                    // ---- the definition's per-pixel rules, once per run
                    int gi = -1, cg = C; bool gthing = false, crowd = false;
                    if (run_g) {
                        gi = px4_sorted_index(gt_ids, ngt, run_g);
                        if (gi < ngt) {
                            const int info = gt_info[gi];
                            if ((info & 63) < C) { cg = info & 63; gthing = info & 64; crowd = gthing && (info & 128); }
                        }
                    }
                    int pi = -1, cp = C; bool pthing = false, unlisted = false;
                    if (run_p) {
                        pi = px4_sorted_index(pred_ids, npred, run_p);
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
        int src;
        uint32_t sum;
        if (wave_same_run(has, run_g | (uint64_t)run_p << 32, run_len, src, sum)) {
            if (lane == src) stq_add<LDS>(cell, sum, stq_tab, o_gt, o_pred, o_inter, t);
        } else if (has) {
            stq_add<LDS>(cell, run_len, stq_tab, o_gt, o_pred, o_inter, t);
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
    const long nchunk = (npix + PX4 - 1) / PX4;
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
