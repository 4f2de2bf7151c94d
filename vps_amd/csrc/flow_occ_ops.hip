// Occlusion-aware temporal consistency (vps_amd/tc.py): the forward-backward flow check.
//   vps_flow_occlusion   fwd (on the grid of cur, pointing into prev) and back (on the grid of prev, pointing into cur) -> one byte per
//                        pixel of cur (0 visible, 1 occluded, 2 not in view) and / or three int64 counts the call ADDS to. A pixel is
//                        visible where fwd(p) and back(p + fwd(p)) cancel: |fwd + back|^2 <= alpha (|fwd|^2 + |back|^2) + beta.
// Arithmetic: fp32, the operations of the definition (vps_amd/tc.py, include/vps_hip.h) in its order, every one rounded on its own - the
// whole file is compiled without contraction, so that the mask equals the NumPy float32 restatement (tests/flow_occ_restate.py) on every
// pixel: d2 <= thr sits on the boundary for whole-pixel shifts against a zero flow, where a fused multiply-add decides differently.
// No index is formed from a float before the in-view test has passed, and every address of `back` is clamped to the map: NaN, inf and
// 1e30 flows read nothing outside it.
#include "px4.h"

#pragma clang fp contract(off)

namespace {

constexpr int OCC_THREADS = 256;

__device__ __forceinline__ float2 occ_load2(const float* __restrict__ f, bool pair) {
    if (pair) return *reinterpret_cast<const float2*>(f);
    return make_float2(f[0], f[1]);
}

// A lane owns 4 consecutive pixels of cur (linear index, a chunk may run over the end of a row): fwd as two 16-byte loads (fmode 2: dense
// [h,w,2], 16-byte aligned), one 8-byte load per pixel (fmode 1) or two 4-byte ones (fmode 0); the four corners of back as 8-byte loads
// (bpair) or two 4-byte ones each; the four codes leave as one dword where occ is dword-aligned. The three counts stay in registers,
// are summed across the wavefront by shuffles and across the workgroup in LDS, and leave as one 64-bit atomic per non-zero cell and
// workgroup.
__global__ __launch_bounds__(OCC_THREADS)
void flow_occlusion_kernel(const float* __restrict__ fwd, int fld, int fcoff, int fmode, const float* __restrict__ back, int bld, int bcoff,
                           int bpair, int H, int W, float alpha, float beta, uint8_t* __restrict__ occ, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t red[OCC_THREADS / 64][3];
    const long npix = (long)H * W, nchunk = (npix + PX4 - 1) / PX4;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const bool occ4 = occ && ((uintptr_t)occ & 3) == 0;
    uint32_t cnt[3] = {0, 0, 0};
    for (long ch = (long)blockIdx.x * OCC_THREADS + threadIdx.x; ch < nchunk; ch += (long)gridDim.x * OCC_THREADS) {
        const long p0 = PX4 * ch;
        const int n = (int)min((long)PX4, npix - p0);
        float u[PX4], v[PX4];
        px4_load_flow(fwd, fld, fcoff, fmode, p0, n, u, v);
        int y = (int)(p0 / W), x = (int)(p0 - (long)y * W);
        uint32_t codes = 0;
#pragma unroll
        for (int i = 0; i < PX4; ++i) {
            if (i >= n) break;
            // ---- the definition, in its order
            const float sx = (float)x + u[i], sy = (float)y + v[i];
            const float qx = floorf(sx + 0.5f), qy = floorf(sy + 0.5f);
            const bool in = qx >= 0.f && qx <= xmax && qy >= 0.f && qy <= ymax;    // as floats: NaN, +-inf, 1e30 fall out here
            uint32_t code = 2;
            if (in) {
                const float x0 = floorf(sx), y0 = floorf(sy);                      // -1 .. W-1 resp. -1 .. H-1 once in view
                const float wx = sx - x0, wy = sy - y0;
                const float x1 = x0 + 1.f, y1 = y0 + 1.f;
                const int ix0 = min(max((int)x0, 0), W - 1), ix1 = min(max((int)x1, 0), W - 1);
                const int iy0 = min(max((int)y0, 0), H - 1), iy1 = min(max((int)y1, 0), H - 1);
                const float* r0 = back + (long)iy0 * W * bld + bcoff;
                const float* r1 = back + (long)iy1 * W * bld + bcoff;
                const float2 b00 = occ_load2(r0 + (long)ix0 * bld, bpair), b01 = occ_load2(r0 + (long)ix1 * bld, bpair);
                const float2 b10 = occ_load2(r1 + (long)ix0 * bld, bpair), b11 = occ_load2(r1 + (long)ix1 * bld, bpair);
                const float top_u = b00.x + wx * (b01.x - b00.x), bot_u = b10.x + wx * (b11.x - b10.x), bt_u = top_u + wy * (bot_u - top_u);
                const float top_v = b00.y + wx * (b01.y - b00.y), bot_v = b10.y + wx * (b11.y - b10.y), bt_v = top_v + wy * (bot_v - top_v);
                const float dx = u[i] + bt_u, dy = v[i] + bt_v;
                const float d2 = dx * dx + dy * dy;
                const float m = (u[i] * u[i] + v[i] * v[i]) + (bt_u * bt_u + bt_v * bt_v);
                const float thr = alpha * m + beta;
                code = d2 <= thr ? 0 : 1;                                          // a NaN anywhere: occluded
            }
            cnt[0] += code == 0; cnt[1] += code == 1; cnt[2] += code == 2;         // (no dynamic index: the counts stay in registers)
            codes |= code << (8 * i);
            if (++x == W) { x = 0; ++y; }
        }
        if (occ) px4_store_bytes(occ, occ4, p0, n, codes);
    }
    if (!counts) return;                                                           // uniform: a kernel argument
#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k] = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0;
        for (int w = 0; w < OCC_THREADS / 64; ++w) s += red[w][threadIdx.x];
        if (s) atomicAdd(&counts[threadIdx.x], (unsigned long long)s);
    }
}

}  // namespace

extern "C" int vps_flow_occlusion(const float* fwd, int fwd_ld, int fwd_coff, const float* back, int back_ld, int back_coff, int H, int W, float alpha,
                                  float beta, uint8_t* occ, int64_t* counts, void* stream) {
    if (!fwd || !back || (!occ && !counts)) return VPS_EARG(1);
    if (H < 1 || W < 1 || (long)H * W >= (1L << 31)) return VPS_EARG(2);           // a lane's uint32 counts cannot wrap
    if (fwd_coff < 0 || fwd_ld < fwd_coff + 2 || back_coff < 0 || back_ld < back_coff + 2) return VPS_EARG(3);
    if ((uintptr_t)counts & 7) return VPS_EARG(4);
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return VPS_EARG(5);                      // negative or NaN
    const int fmode = px4_flow_mode(fwd, fwd_ld, fwd_coff), bpair = px4_flow_mode(back, back_ld, back_coff) >= 1;
    const long nchunk = ((long)H * W + PX4 - 1) / PX4;
    long g = (nchunk + OCC_THREADS - 1) / OCC_THREADS; if (g > 2048) g = 2048;      // <= 8 workgroups per CU, then grid-stride
    hipLaunchKernelGGL(flow_occlusion_kernel, dim3((unsigned)g), dim3(OCC_THREADS), 0, (hipStream_t)stream, fwd, fwd_ld, fwd_coff, fmode, back, back_ld,
                       back_coff, bpair, H, W, alpha, beta, occ, reinterpret_cast<unsigned long long*>(counts));
    return vps_launch_status();
}
