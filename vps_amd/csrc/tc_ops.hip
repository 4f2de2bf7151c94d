// Temporal consistency without ground truth (vps_amd/tc.py): the counting pass of the flow-warped map agreement.
//   vps_tc_accumulate      one (prev, cur, flow) pair: prev is read at p + flow(p) for every pixel p of cur and the (warped, cur) pixel
//                          pairs are ADDED to the caller's int64 tables - the class confusion matrix, the sizes of the listed tracks in
//                          both maps and their agreement, the in-view / outside counts. Optionally one byte per pixel says how the
//                          pixel disagrees. The tables stay on the device; nothing is zeroed, downloaded or synchronised here.
//   vps_tc_accumulate_masked   the same with a byte mask (vps_flow_occlusion's): an in-view pixel whose mask byte is not 0 is counted in
//                          one extra cell and in nothing else
// Where a pixel lands and whether that is in view: warp_rule.h (warp_nearest), the one implementation.
// Integer adds only: the result does not depend on their order, so two runs (and the two table paths) give identical tables.
#include "px4.h"
#include "warp_rule.h"
#include <string.h>

namespace {

constexpr int TC_THREADS = 256;

struct TcClasses { uint32_t w[64]; };                 // seg_class[256], handed over in the kernel arguments
struct TcTables { unsigned long long *conf, *prev_size, *cur_size, *same, *misc, *masked; };   // masked: the MASKED instances only

// the cells one run of in-view (warped, cur) pairs adds to; -1 = none
struct TcCells { int conf, prev, cur, same; };

template <bool LDS>
__device__ __forceinline__ void tc_add(const TcCells& c, uint32_t n, uint32_t* tab, int o_prev, int o_cur, int o_same, const TcTables& t) {
    if (LDS) {
        atomicAdd(&tab[c.conf], n);
        if (c.prev >= 0) atomicAdd(&tab[o_prev + c.prev], n);
        if (c.cur >= 0) atomicAdd(&tab[o_cur + c.cur], n);
        if (c.same >= 0) atomicAdd(&tab[o_same + c.same], n);
    } else {
        atomicAdd(&t.conf[c.conf], (unsigned long long)n);
        if (c.prev >= 0) atomicAdd(&t.prev_size[c.prev], (unsigned long long)n);
        if (c.cur >= 0) atomicAdd(&t.cur_size[c.cur], (unsigned long long)n);
        if (c.same >= 0) atomicAdd(&t.same[c.same], (unsigned long long)n);
    }
}

// A lane owns 4 consecutive pixels of cur (linear index, a chunk may run over the end of a row): cur as aligned dwords, the flow as two
// 16-byte loads (fmode 2: dense [h,w,2], 16-byte aligned), one 8-byte load per pixel (fmode 1) or two 4-byte ones (fmode 0), the two
// bytes of prev that the pair needs from wherever the flow points. Equal neighbouring (warped, cur, in view) states are folded in
// registers and resolved to their cells once per run (two table lookups, up to two binary searches); the run a lane ends with is
// compared across the wavefront and, where every lane holds the same one, summed by shuffles and added by one lane. The in-view /
// outside counts stay in registers until the end. LDS = true: the adds go to the workgroup's own uint32 image (conf | prev_size |
// cur_size | same | misc) and leave as one 64-bit atomic per non-zero cell; LDS = false: 64-bit global atomics per run. No workgroup
// reads what another one writes.
// MASKED: `mask` holds one byte per pixel of cur. An in-view pixel whose byte is not 0 is counted in t.masked (the cell behind misc in
// the LDS image) and in nothing else, its code is 4; the masked flag is part of a run's state, so such a pixel ends the run in front of
// it and joins none. A pixel that is not in view counts as outside whatever its byte says. MASKED = false is the kernel as it was.
template <bool LDS, bool MASKED>
__global__ __launch_bounds__(TC_THREADS)
void tc_accumulate_kernel(const uint8_t* __restrict__ prev, const uint8_t* __restrict__ cur, int H, int W, const float* __restrict__ flow, int ld,
                          int coff, int fmode, int idch, TcClasses sc, int C, const uint16_t* __restrict__ keys, int nkeys, TcTables t,
                          uint8_t* __restrict__ flick, const uint8_t* __restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tc_lds[];
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(tc_lds);             // 256 bytes in front of the tables
    uint32_t* tab = tc_lds + 64;
    const int C1 = C + 1, o_prev = C1 * C1, o_cur = o_prev + nkeys, o_same = o_cur + nkeys, o_misc = o_same + nkeys, cells = o_misc + (MASKED ? 3 : 2);
    if (threadIdx.x < 64) tc_lds[threadIdx.x] = sc.w[threadIdx.x];
    if (LDS)
        for (int i = threadIdx.x; i < cells; i += TC_THREADS) tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long npix = (long)H * W, nbytes = 3 * npix, nchunk = (npix + PX4 - 1) / PX4;
    const int sh = 8 * idch;
    const bool flick4 = flick && ((uintptr_t)flick & 3) == 0;
    uint32_t n_in = 0, n_out = 0, n_msk = 0;
    for (long ch0 = (long)blockIdx.x * TC_THREADS; ch0 < nchunk; ch0 += (long)gridDim.x * TC_THREADS) {       // uniform per workgroup
        const long ch = ch0 + threadIdx.x;
        uint32_t run_st = 0, run_len = 0, code = 0;
        bool run_in = false, run_msk = false;
        TcCells cell = {-1, -1, -1, -1};
        if (ch < nchunk) {
            const long p0 = PX4 * ch;
            const int n = (int)min((long)PX4, npix - p0);
            uint32_t A[PX4];
            px4_load_px3(cur, nbytes, ch, n, A);
            float u[PX4], v[PX4];
            px4_load_flow(flow, ld, coff, fmode, p0, n, u, v);
            const uint32_t M = MASKED ? px4_load_bytes(mask, npix, p0, n) : 0;      // the chunk's mask bytes
            int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
            uint32_t codes = 0;
#pragma unroll
            for (int i = 0; i < PX4; ++i) {
                if (i >= n) break;
                // ---- the definition's warp (warp_rule.h): fp32, one add each, compared as floats before any conversion
                int ix, iy;
                bool in = warp_nearest(warp_pos(x, u[i]), warp_pos(y, v[i]), W, H, ix, iy);
                const bool msk = MASKED && in && ((M >> (8 * i)) & 0xffu) != 0;
                if (msk) in = false;                  // from here on: in = in view and counted
                uint32_t st = 0;
                if (in) {
                    const uint8_t* b = prev + 3 * ((long)iy * W + ix);
                    st = (((A[i] & 0xffu) << 8) | ((A[i] >> sh) & 0xffu)) | ((uint32_t)b[0] << 24) | ((uint32_t)b[idch] << 16);
                    ++n_in;
                } else if (msk) {
                    ++n_msk;
                } else {
                    ++n_out;
                }
                if (!run_len || in != run_in || st != run_st || (MASKED && msk != run_msk)) {
                    if (run_len && run_in) tc_add<LDS>(cell, run_len, tab, o_prev, o_cur, o_same, t);
                    run_in = in; run_st = st; run_len = 0;
                    if (MASKED) run_msk = msk;
                    code = msk ? 4 : 3;
                    if (in) {                         // ---- the definition's per-pixel rules, once per run
                        const uint32_t ak = st & 0xffffu, bk = st >> 16;
                        int ca = cls[ak >> 8], cb = cls[bk >> 8];
                        if (ca > C) ca = C;
                        if (cb > C) cb = C;
                        const int ka = px4_sorted_index(keys, nkeys, ak), kb = ak == bk ? ka : px4_sorted_index(keys, nkeys, bk);
                        cell.conf = cb * C1 + ca;
                        cell.cur = ka < nkeys ? ka : -1;
                        cell.prev = kb < nkeys ? kb : -1;
                        cell.same = ka < nkeys && ka == kb ? ka : -1;
                        code = ca != cb ? 1 : (ka < nkeys && kb < nkeys && ka != kb ? 2 : 0);
                    }
                }
                ++run_len;
                codes |= code << (8 * i);
                if (++x == W) { x = 0; ++y; }
            }
            if (flick) px4_store_bytes(flick, flick4, p0, n, codes);
        }
        // the in-view run each lane is left with: one add per wavefront where all of them are the same
        const bool has = run_len > 0;
        int src;
        uint32_t sum;
        if (wave_same_run(has, run_st | (uint64_t)run_in << 32 | (uint64_t)run_msk << 33, run_len, src, sum)) {
            if (lane == src && run_in) tc_add<LDS>(cell, sum, tab, o_prev, o_cur, o_same, t);
        } else if (has && run_in) {
            tc_add<LDS>(cell, run_len, tab, o_prev, o_cur, o_same, t);
        }
    }
    n_in = wave_sum(n_in);
    n_out = wave_sum(n_out);
    if (MASKED) n_msk = wave_sum(n_msk);
    if (lane == 0) {
        if (LDS) {
            if (n_in) atomicAdd(&tab[o_misc], n_in);
            if (n_out) atomicAdd(&tab[o_misc + 1], n_out);
            if (MASKED && n_msk) atomicAdd(&tab[o_misc + 2], n_msk);
        } else {
            if (n_in) atomicAdd(&t.misc[0], (unsigned long long)n_in);
            if (n_out) atomicAdd(&t.misc[1], (unsigned long long)n_out);
            if (MASKED && n_msk) atomicAdd(&t.masked[0], (unsigned long long)n_msk);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += TC_THREADS) {
            const uint32_t val = tab[i];
            if (!val) continue;
            unsigned long long* dst = i < o_prev ? t.conf + i : i < o_cur ? t.prev_size + (i - o_prev) : i < o_same ? t.cur_size + (i - o_cur)
                                    : i < o_misc ? t.same + (i - o_same) : i < o_misc + 2 ? t.misc + (i - o_misc) : t.masked;
            atomicAdd(dst, (unsigned long long)val);
        }
    }
}

}  // namespace

// the checks and the launch of both entry points; mask == NULL: the unmasked instances
static int tc_launch(const uint8_t* prev, const uint8_t* cur, int H, int W, const float* flow, int flow_ld, int flow_coff, int id_channel,
                     const uint8_t* seg_class, int num_classes, const uint16_t* keys, int nkeys, int64_t* conf, int64_t* prev_size, int64_t* cur_size,
                     int64_t* same, int64_t* misc, uint8_t* flicker, const uint8_t* mask, int64_t* masked, void* stream) {
    if (!prev || !cur || !flow || !seg_class || !conf || !misc) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);       // a workgroup's uint32 cells cannot wrap
    if (num_classes < 1 || num_classes > 63) return VPS_EARG(3);
    if (nkeys < 0 || nkeys > 65536) return VPS_EARG(4);
    if (id_channel != 1 && id_channel != 2) return VPS_EARG(5);
    if (nkeys > 0 && (!keys || !prev_size || !cur_size || !same)) return VPS_EARG(1);
    if (((uintptr_t)conf | (uintptr_t)prev_size | (uintptr_t)cur_size | (uintptr_t)same | (uintptr_t)misc | (uintptr_t)masked) & 7) return VPS_EARG(6);
    if (flow_coff < 0 || flow_ld < flow_coff + 2) return VPS_EARG(7);
    TcTables t = {reinterpret_cast<unsigned long long*>(conf), reinterpret_cast<unsigned long long*>(prev_size),
                  reinterpret_cast<unsigned long long*>(cur_size), reinterpret_cast<unsigned long long*>(same),
                  reinterpret_cast<unsigned long long*>(misc), reinterpret_cast<unsigned long long*>(masked)};
    TcClasses sc;
    memcpy(sc.w, seg_class, 256);                                                // the caller's table may go once the call returns
    const int fmode = px4_flow_mode(flow, flow_ld, flow_coff);
    const long cells = (long)(num_classes + 1) * (num_classes + 1) + 3L * nkeys + (mask ? 3 : 2);
    const long nchunk = ((long)H * W + PX4 - 1) / PX4;
    long g = nchunk / (TC_THREADS * 4); if (g > 512) g = 512; if (g < 1) g = 1;            // >= 4 chunks per lane, <= 2 workgroups per CU
    hipStream_t s = (hipStream_t)stream;
    const bool lds = cells <= vps_stq_lds_cells();                                          // the path depends on the table sizes alone
    const size_t shm = 256 + (lds ? sizeof(uint32_t) * cells : 0);
    auto kernel = mask ? (lds ? tc_accumulate_kernel<true, true> : tc_accumulate_kernel<false, true>)
                       : (lds ? tc_accumulate_kernel<true, false> : tc_accumulate_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)g), dim3(TC_THREADS), shm, s, prev, cur, H, W, flow, flow_ld, flow_coff, fmode, id_channel, sc, num_classes,
                       keys, nkeys, t, flicker, mask);
    return vps_launch_status();
}

extern "C" int vps_tc_accumulate(const uint8_t* prev, const uint8_t* cur, int H, int W, const float* flow, int flow_ld, int flow_coff, int id_channel,
                                 const uint8_t* seg_class, int num_classes, const uint16_t* keys, int nkeys, int64_t* conf, int64_t* prev_size,
                                 int64_t* cur_size, int64_t* same, int64_t* misc, uint8_t* flicker, void* stream) {
    return tc_launch(prev, cur, H, W, flow, flow_ld, flow_coff, id_channel, seg_class, num_classes, keys, nkeys, conf, prev_size, cur_size, same, misc,
                     flicker, nullptr, nullptr, stream);
}

extern "C" int vps_tc_accumulate_masked(const uint8_t* prev, const uint8_t* cur, int H, int W, const float* flow, int flow_ld, int flow_coff,
                                        int id_channel, const uint8_t* seg_class, int num_classes, const uint16_t* keys, int nkeys, int64_t* conf,
                                        int64_t* prev_size, int64_t* cur_size, int64_t* same, int64_t* misc, uint8_t* flicker, const uint8_t* mask,
                                        int64_t* masked, void* stream) {
    if (!mask || !masked) return VPS_EARG(1);
    return tc_launch(prev, cur, H, W, flow, flow_ld, flow_coff, id_channel, seg_class, num_classes, keys, nkeys, conf, prev_size, cur_size, same, misc,
                     flicker, mask, masked, stream);
}
