// Occlusion-aware temporal consistency (vps_amd/tc.py): the forward-backward flow check.
//   vps_flow_occlusion   fwd (on the grid of cur, pointing into prev) and back (on the grid of prev, pointing into cur) -> one byte per
//                        pixel of cur (0 visible, 1 occluded, 2 not in view) and / or three int64 counts the call ADDS to. A pixel is
//                        visible where fwd(p) and back(p + fwd(p)) cancel: |fwd + back|^2 <= alpha (|fwd|^2 + |back|^2) + beta.
// Arithmetic: fp32, the operations of the definition (vps_amd/tc.py, include/vps_hip.h) in its order, every one rounded on its own - the
// whole file is compiled without contraction, so that the mask equals the NumPy float32 restatement (tests/flow_occ_restate.py) on every
// pixel: d2 <= thr sits on the boundary for whole-pixel shifts against a zero flow, where a fused multiply-add decides differently.
// The in-view test, the corners and the sample are warp_rule.h, the one implementation: NaN, inf and 1e30 flows read nothing outside `back`.
#include "px4.h"
#include "warp_rule.h"

#pragma clang fp contract(off)

namespace {

constexpr int OCC_THREADS = PX4_WG;

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
            // ---- the definition, in its order (warp_rule.h: in view, corners, sample)
            const float sx = warp_pos(x, u[i]), sy = warp_pos(y, v[i]);
            uint32_t code = 2;
            if (warp_in_view(sx, sy, W, H)) {
                const WarpCorners c = warp_corners(sx, sy, W, H);
                const float* r0 = back + (long)c.y0 * W * bld + bcoff;
                const float* r1 = back + (long)c.y1 * W * bld + bcoff;
                const float2 b00 = occ_load2(r0 + (long)c.x0 * bld, bpair), b01 = occ_load2(r0 + (long)c.x1 * bld, bpair);
                const float2 b10 = occ_load2(r1 + (long)c.x0 * bld, bpair), b11 = occ_load2(r1 + (long)c.x1 * bld, bpair);
                const float bt_u = warp_lerp2(b00.x, b01.x, b10.x, b11.x, c.wx, c.wy);
                const float bt_v = warp_lerp2(b00.y, b01.y, b10.y, b11.y, c.wx, c.wy);
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
    wg_counts_to_table(cnt, red, counts);
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
