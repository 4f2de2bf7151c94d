// Image-level evaluation on the device: the per-image passes behind tools/test_eval_ipq.py.
//   vps_sseg_confusion     Cityscapes.evaluate_ssegs (tools/dataset/cityscapes.py:120-135) + get_confusion_matrix
//                          (base_dataset.py:449-467) for one image: NEAREST resample by index tables, drop label 255, count
//                          idx = gt * class_num + pred for idx < class_num^2 into a caller-owned int64 matrix
//   vps_segment_stats_ch   vps_segment_stats with the id taken from a chosen channel: (0, 1) is the key of
//   vps_segment_paint_ch   _converter_2ch_single_core (base_dataset.py:288-335), 1000 * pan_seg + pan_ins
// Integer work, bit-exact against the reference functions (tests/test_ipq_gpu.py, goldens from the real functions).
#include "px4.h"

namespace {

constexpr int CONF_MAX_CLASSES = 32;                  // class_num^2 <= 1024 bins per wavefront
constexpr int CONF_BINS = CONF_MAX_CLASSES * CONF_MAX_CLASSES;
constexpr int CONF_WAVES = 4;
constexpr int CONF_RUN = 16;                          // consecutive label pixels per lane: one 16-byte load

// Semantic maps are large uniform regions: an atomic per pixel would serialise on one address. Each lane takes 16 consecutive pixels
// of one label row and folds equal neighbouring (gt, pred) pairs in registers; a run that ends inside the chunk goes to the
// wavefront's own LDS histogram, the run the chunk ends with is first compared across the wavefront: where every lane holds the same
// pair (the inside of a region) the lengths are summed by shuffles and one lane adds them. The workgroup adds its non-zero bins to
// the caller's int64 matrix once. Index tables are clamped to the prediction: no read outside it whatever they hold.
__global__ __launch_bounds__(64 * CONF_WAVES)
void sseg_confusion_kernel(const uint8_t* __restrict__ gt, int Hg, int Wg, const uint8_t* __restrict__ pred, int Hp, int Wp,
                           const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab, int C,
                           unsigned long long* __restrict__ counts) {
    __shared__ int32_t hist[CONF_WAVES][CONF_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bins = C * C;
    for (int i = threadIdx.x; i < CONF_WAVES * CONF_BINS; i += blockDim.x) (&hist[0][0])[i] = 0;
    __syncthreads();
    int32_t* h = hist[wave];
    const int cpr = (Wg + CONF_RUN - 1) / CONF_RUN;   // chunks per label row
    const long nchunk = (long)Hg * cpr;
    for (long ch0 = (long)blockIdx.x * blockDim.x; ch0 < nchunk; ch0 += (long)gridDim.x * blockDim.x) {   // uniform per workgroup
        const long ch = ch0 + threadIdx.x;
        int run_key = -1, run_len = 0;
        if (ch < nchunk) {
            const int y = (int)(ch / cpr), x0 = (int)(ch - (long)y * cpr) * CONF_RUN;
            const int n = min(CONF_RUN, Wg - x0);
            const uint8_t* g = gt + (size_t)y * Wg + x0;
            const int ys = ytab ? min(max(ytab[y], 0), Hp - 1) : y;
            const uint8_t* prow = pred + (size_t)ys * Wp;
            alignas(16) uint8_t gv[CONF_RUN], pv[CONF_RUN];
            if (n == CONF_RUN && !((uintptr_t)g & 15)) {
                *reinterpret_cast<uint4*>(gv) = *reinterpret_cast<const uint4*>(g);
            } else {
                for (int i = 0; i < n; ++i) gv[i] = g[i];
            }
            if (!xtab) {                              // equal sizes: the prediction is read like the label
                const uint8_t* p = prow + x0;
                if (n == CONF_RUN && !((uintptr_t)p & 15)) {
                    *reinterpret_cast<uint4*>(pv) = *reinterpret_cast<const uint4*>(p);
                } else {
                    for (int i = 0; i < n; ++i) pv[i] = p[i];
                }
            } else {
                for (int i = 0; i < n; ++i) pv[i] = prow[min(max(xtab[x0 + i], 0), Wp - 1)];
            }
            for (int i = 0; i < n; ++i) {
                const int idx = gv[i] * C + pv[i];
                const int key = (gv[i] != 255 && idx < bins) ? idx : -1;      // label 255 and cells past the matrix are dropped
                if (key != run_key) {
                    if (run_len && run_key >= 0) atomicAdd(&h[run_key], run_len);
                    run_key = key; run_len = 0;
                }
                ++run_len;
            }
            if (run_key < 0) run_len = 0;
        }
        // the run each lane is left with: one add per wavefront where all of them are the same pair
        const bool has = run_len > 0;
        int src;
        uint32_t sum;
        if (wave_same_run(has, (uint32_t)run_key, run_len, src, sum)) {
            if (lane == src) atomicAdd(&h[run_key], (int)sum);
        } else if (has) {
            atomicAdd(&h[run_key], run_len);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x) {
        long v = 0;
#pragma unroll
        for (int w = 0; w < CONF_WAVES; ++w) v += hist[w][i];
        if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256)
void segment_stats_ch_init_kernel(int32_t* __restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;     // 65536 entries
    stats[5 * i] = 0; stats[5 * i + 1] = 0x7fffffff; stats[5 * i + 2] = 0x7fffffff; stats[5 * i + 3] = -1; stats[5 * i + 4] = -1;
}

// one thread per 8-pixel run of a row, as segment_stats_kernel (post_ops.hip); the id byte is channel `idc`
__global__ __launch_bounds__(256)
void segment_stats_ch_kernel(const uint8_t* __restrict__ pan2, int H, int W, int idc, int32_t* __restrict__ stats) {
    const int runs_per_row = (W + 7) >> 3;
    const long total = (long)H * runs_per_row;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int y = (int)(idx / runs_per_row), x0 = (int)(idx % runs_per_row) * 8;
        const int n = min(8, W - x0);
        const uint8_t* p = pan2 + ((size_t)y * W + x0) * 3;
        int key = -1, cnt = 0, xs = 0;
        for (int i = 0; i <= n; ++i) {
            const int k = i < n ? (p[3 * i] << 8 | p[3 * i + idc]) : -2;
            if (k != key) {
                if (cnt) {
                    int32_t* s = stats + 5 * key;
                    atomicAdd(&s[0], cnt); atomicMin(&s[1], xs); atomicMin(&s[2], y); atomicMax(&s[3], x0 + i - 1); atomicMax(&s[4], y);
                }
                key = k; cnt = 0; xs = x0 + i;
            }
            ++cnt;
        }
    }
}

__global__ __launch_bounds__(256)
void segment_paint_ch_kernel(const uint8_t* __restrict__ pan2, long npix, int idc, const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const int key = pan2[3 * p] << 8 | pan2[3 * p + idc];
        const uint8_t* c = lut + 3 * key;
        out[3 * p] = c[0]; out[3 * p + 1] = c[1]; out[3 * p + 2] = c[2];
    }
}

}  // namespace

extern "C" int vps_sseg_confusion(const uint8_t* gt, int Hg, int Wg, const uint8_t* pred, int Hp, int Wp, const int32_t* ytab,
                                  const int32_t* xtab, int class_num, int64_t* counts, void* stream) {
    if (class_num < 1 || class_num > CONF_MAX_CLASSES) return VPS_EARG(1);
    if (!gt || !pred || !counts || Hg <= 0 || Wg <= 0 || Hp <= 0 || Wp <= 0) return VPS_EARG(2);
    if ((!ytab || !xtab) && (ytab || xtab || Hg != Hp || Wg != Wp)) return VPS_EARG(3);     // no tables: equal sizes only
    if (((uintptr_t)counts & 7) || (long)Hg * Wg >= (1L << 31)) return VPS_EARG(4);    // per-wavefront bins are int32
    const long nchunk = (long)Hg * ((Wg + CONF_RUN - 1) / CONF_RUN);
    long g = nchunk / (64 * CONF_WAVES * 4); if (g > 512) g = 512; if (g < 1) g = 1;        // >= 4 chunks per lane, <= 2 workgroups per CU
    hipLaunchKernelGGL(sseg_confusion_kernel, dim3((unsigned)g), dim3(64 * CONF_WAVES), 0, (hipStream_t)stream, gt, Hg, Wg, pred, Hp, Wp,
                       ytab, xtab, class_num, reinterpret_cast<unsigned long long*>(counts));
    return vps_launch_status();
}

extern "C" int vps_segment_stats_ch(const uint8_t* pan_2ch, int H, int W, int id_channel, int32_t* stats, void* stream) {
    if (!pan_2ch || !stats || H <= 0 || W <= 0) return VPS_EARG(1);
    if (id_channel != 1 && id_channel != 2) return VPS_EARG(2);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(segment_stats_ch_init_kernel, dim3(256), dim3(256), 0, s, stats);
    hipLaunchKernelGGL(segment_stats_ch_kernel, dim3(stream_grid((long)H * ((W + 7) >> 3), 256)), dim3(256), 0, s, pan_2ch, H, W, id_channel,
                       stats);
    return vps_launch_status();
}

extern "C" int vps_segment_paint_ch(const uint8_t* pan_2ch, int64_t npix, int id_channel, const uint8_t* lut, uint8_t* out, void* stream) {
    if (!pan_2ch || !lut || !out || npix <= 0) return VPS_EARG(1);
    if (id_channel != 1 && id_channel != 2) return VPS_EARG(2);
    hipLaunchKernelGGL(segment_paint_ch_kernel, dim3(stream_grid((long)npix, 256)), dim3(256), 0, (hipStream_t)stream, pan_2ch, (long)npix,
                       id_channel, lut, out);
    return vps_launch_status();
}
