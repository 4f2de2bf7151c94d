// The kernel choice of vps_conv2d: see conv_plan.h. Host-only; order of precedence
//   small -> thin -> 256-column deformable -> n16 family -> h8s2 -> h8p / h8 -> 4-wave halo -> pw -> q -> f32 / bf16p.
// A new family gets an id in conv_plan.h, its conditions at its place in vpsi_conv_plan, a launcher in its own .hip file, a case
// in the switch of vps_conv2d and rows in tests/conv_plan_cases.json.
#include "conv_plan.h"
#include <stdint.h>

namespace {

constexpr int BM = 128, BK = 32;   // rows and k-steps of the block tiles (conv_common.h)

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline size_t in_bytes(const vps_conv_desc& d) { return (size_t)d.N * d.H * d.W * d.in_ld * sizeof(float); }
inline size_t out_bytes(const vps_conv_desc& d) { return (size_t)d.N * d.Ho * d.Wo * d.out_ld * sizeof(float); }
inline bool two_plane(int prec) { return prec == VPS_PREC_F16X3 || prec == VPS_PREC_BF16X3 || prec == VPS_PREC_BF16; }

// layers with fewer than this many 32-channel chunks stay on the 4-wave halo kernel (two blocks per CU: one block's store drain
// overlaps the other's k loop; the 8-wave kernel holds a CU alone and its short-K tiles are mostly drain)
// round 5, measured: `64->128 3x3 @512x1024` 0.303 -> 0.264 ms on the 4-wave kernel, layers with >= 4 chunks unchanged -> 3
constexpr int H8_MIN_CHUNKS = 3;
// layers with fewer than this many rounds of resident blocks stay on the uniform-lead kernel (persistence pays from the second tile
// of a block on)
constexpr int PW_MIN_ROUNDS = 2;

conv_plan fail(conv_plan p, int n) { p.kernel = CONV_K_NONE; p.err = VPS_EARG(n); return p; }

// narrow outputs (cout <= 4) in exact fp32 on the vector ALU: conv_small.hip
conv_plan plan_small(const vps_conv_desc& d, conv_plan p) {
    p.block = 256;
    p.G = 1; p.logG = 0;
    while (p.G < 64 && p.G < (d.cin_pad >> 2)) { p.G <<= 1; ++p.logG; }
    const size_t wbytes = (size_t)(d.cout <= 2 ? 2 : 4) * d.kpad * sizeof(float);
    if (d.KH == 3 && d.KW == 3 && d.stride == 1 && d.nclass == 1 && d.pad_y[0] == 1 && d.pad_x[0] == 1 && d.Ho == d.H && d.Wo == d.W &&
        wbytes <= 150 * 1024 && (d.cout <= 2 || d.cout_pad >= 4) && in_bytes(d) < 0xFFFFFFF0ull &&
        (long)d.N * d.H * d.W < 0x7fffffffL) {               // 32-bit run index
        const int run = d.cout <= 2 ? 4 : 2;
        p.runs_per_row = (d.W + run - 1) / run;
        const long total_runs = (long)d.N * d.H * p.runs_per_row;
        const int ppw = 64 >> p.logG;
        long blocks = (total_runs + 4 * ppw - 1) / (4 * ppw);
        if (blocks > 768) blocks = 768;               // 3 blocks of 4 waves per CU (152 VGPRs: all 18 loads of a run in flight): one resident round, the weights are staged once per block
        p.kernel = CONV_K_SMALL3X3V; p.total_runs = (int)total_runs; p.grid = (unsigned)blocks; p.smem = wbytes;
        return p;
    }
    const long total = (long)d.nclass * p.M;
    // eight loads per lane in flight, weights in LDS: conv_small_batched_kernel (the one-load-per-step kernel keeps the layers with
    // fewer than eight loads per pixel - the 2 -> 2 up-flow layers measured 31 us there against 36 us here)
    const size_t wb = (size_t)d.nclass * (d.cout <= 2 ? 2 : 4) * d.kpad * sizeof(float);
    if ((d.cin_pad >> 2) * d.KH * d.KW >= 8 && wb <= 48 * 1024 && (d.cout <= 2 || d.cout_pad >= 4) && in_bytes(d) < 0xFFFFFFF0ull) {
        const int c4n = d.cin_pad >> 2, ntap = d.KH * d.KW;
        p.G = 1; p.logG = 0;
        while (p.G < 64 && p.G * 8 < c4n * ntap && p.G < c4n) { p.G <<= 1; ++p.logG; }
        p.nslot = (c4n + p.G - 1) >> p.logG;
        const int ppw = 64 >> p.logG;
        const long waves = (total + ppw - 1) / ppw;
        long blocks = (waves + 3) / 4; if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;   // 8 blocks per CU: one resident round
        p.kernel = CONV_K_SMALL_BATCHED; p.grid = (unsigned)blocks; p.smem = wb;
        return p;
    }
    const long waves = (total + (64 >> p.logG) - 1) / (64 >> p.logG);
    long blocks = (waves + 3) / 4; if (blocks > 8192) blocks = 8192; if (blocks < 1) blocks = 1;
    p.kernel = CONV_K_SMALL; p.grid = (unsigned)blocks;
    return p;
}

// thin-input layers at full resolution (3 / 6 / 11 / 12 -> 64 channels) with their own weight packing: conv_thin.hip
bool plan_thin(const vps_conv_desc& d, const conv_limits& lim, const conv_switches& sw, conv_plan& p) {
    if (!sw.thin || !d.w_thin || d.prec != VPS_PREC_F16X3 || d.offset || d.res || d.nclass != 1 || d.ksplit != 1 || d.korder != 0) return false;
    if (d.KH != d.KW || d.cout_pad != 64 || d.tile_n != 64 || (d.cout & 3) || ((uintptr_t)d.w_thin & 15)) return false;
    if (d.pad_y[0] != d.KH / 2 || d.pad_x[0] != d.KH / 2 || d.pad_y[1] != d.KH / 2 || d.pad_x[1] != d.KH / 2) return false;
    // the input is addressed through a 32-bit buffer resource: a narrow window inside a buffer of >= 4 GiB would wrap (loads beyond the
    // truncated size return zeros, silently) -> the pipelined kernel takes such a launch
    if (in_bytes(d) >= 0xFFFFFFF0ull) return false;
    // float4 buffer stores: 16-byte aligned channel windows of an output below 4 GiB
    if (((d.out_ld | d.out_coff) & 3) || ((uintptr_t)d.out & 15) || out_bytes(d) >= 0xFFFFFFF0ull) return false;
    int i = 0;
    while (i < 4 && !(d.KH == conv_thin_shapes[i].ks && d.stride == conv_thin_shapes[i].s && d.cin_pad == conv_thin_shapes[i].c4)) ++i;
    if (i == 4) return false;
    const int ph = conv_thin_shapes[i].ph;
    const int tiles_x = (d.Qw + 31) / 32, tiles_y = (d.Qh + ph - 1) / ph;
    const long ntiles = (long)d.N * tiles_x * tiles_y;
    if (ntiles < 512 || ntiles > 0x7fffffffL) return false;      // small maps: the pipelined kernels (split-K, fewer idle lanes)
    const int resident = (lim.thin_per_cu[i] > 0 ? lim.thin_per_cu[i] : 1) * (lim.cus > 0 ? lim.cus : 256);   // blocks the chip holds at once
    // whole rounds: every block walks the same number of tiles (+-1)
    const long rounds = (ntiles + resident - 1) / resident;
    p.kernel = CONV_K_THIN; p.thin = i; p.tiles_n = tiles_x; p.tiles_m = tiles_y; p.ntiles = (int)ntiles;
    p.grid = (unsigned)((ntiles + rounds - 1) / rounds); p.block = 256;
    return true;
}

// 1x1 layers with at least two rounds of resident blocks: the persistent pointwise kernel (conv_pw.hip)
bool plan_pw(const vps_conv_desc& d, const conv_limits& lim, const conv_switches& sw, conv_plan& p) {
    if (!sw.pw || d.prec != VPS_PREC_F16X3 || d.offset || d.KH != 1 || d.KW != 1 || d.nclass != 1 || d.ksplit != 1 || d.gn_stats) return false;
    if (d.pad_y[0] || d.pad_x[0] || (d.cin_pad & 31) || d.kpad != d.cin_pad || (d.tile_n != 128 && d.tile_n != 64)) return false;
    const int nk = d.kpad / BK;
    if (nk < 2 || (nk & 1)) return false;
    if (d.Ho != d.Qh || d.Wo != d.Qw || (d.stride == 1 && (d.H != d.Qh || d.W != d.Qw))) return false;
    // float4 buffer stores / residual loads: 16-byte aligned channel windows of tensors below 4 GiB
    if (((d.cout | d.out_ld | d.out_coff) & 3) || ((uintptr_t)d.out & 15) || out_bytes(d) >= 0xFFFFFE00ull) return false;
    if (d.res && (((d.res_ld | d.res_coff) & 3) || ((uintptr_t)d.res & 15) || d.res_shift < 0 || d.res_shift > 4 ||
                  (size_t)d.N * (d.Ho >> d.res_shift) * (d.Wo >> d.res_shift) * d.res_ld * sizeof(float) >= 0xFFFFFE00ull)) return false;
    if (in_bytes(d) >= 0xFFFFFE00ull) return false;
    const int per_cu = lim.pw_per_cu[d.tile_n == 128 ? 1 : 0];
    const int resident = (per_cu > 0 ? per_cu : 1) * (lim.cus > 0 ? lim.cus : 256);
    const long total = (long)p.tiles_m * p.tiles_n;
    const int unit = 8 * p.tiles_n;                            // a grid is whole groups of (8 XCDs x the column tiles)
    if (resident < unit || total < (long)PW_MIN_ROUNDS * resident) return false;
    // whole rounds: every block walks the same number of tiles
    const long rounds = (total + resident - 1) / resident;
    long grid = (total + rounds - 1) / rounds;
    grid = (grid + unit - 1) / unit * unit;
    if (grid > resident) grid = resident / unit * unit;
    const int mper = (int)(grid / unit);
    p.kernel = CONV_K_PW; p.grid = (unsigned)grid; p.nk = nk; p.nit = (p.tiles_m + mper * 8 - 1) / (mper * 8);
    return true;
}

}  // namespace

const conv_thin_shape conv_thin_shapes[4] = {{8, 3, 1, 8}, {12, 3, 1, 8}, {4, 7, 2, 8}, {12, 7, 2, 4}};

const char* vpsi_conv_kernel_name(int kernel) {
    static const char* const names[] = {"none", "small3x3v", "small_batched", "small", "thin", "dcn256", "n16t", "n32", "n16",
                                        "h8s2", "h8p", "h8", "halo", "pw", "q", "f32", "bf16p"};
    return kernel >= 0 && kernel <= CONV_K_BF16P ? names[kernel] : "?";
}

int vpsi_conv_check(const vps_conv_desc& d) {
    if (!d.in || !d.out) return VPS_EARG(2);
    if (d.prec < VPS_PREC_F32 || d.prec > VPS_PREC_F16X3) return VPS_EARG(12);
    if (d.prec == VPS_PREC_F32 ? !d.w : !d.w_split) return VPS_EARG(13);
    if ((d.in_ld & 3) || (d.in_coff & 3) || (d.cin_pad & 3) || d.cin_pad <= 0) return VPS_EARG(3);
    if ((d.kpad % BK) || d.kpad < d.KH * d.KW * d.cin_pad || (d.korder != 0 && d.korder != 1)) return VPS_EARG(4);
    if (d.korder == 1 && d.kpad != d.KH * d.KW * ((d.cin_pad + BK - 1) / BK) * BK) return VPS_EARG(14);
    if (d.tile_n != 32 && d.tile_n != 64 && d.tile_n != 128 && !(d.tile_n == 256 && d.offset && d.prec == VPS_PREC_F16X3 && d.korder == 1)) return VPS_EARG(5);
    if (d.cout_pad % d.tile_n || d.cout > d.cout_pad || d.cout <= 0) return VPS_EARG(6);
    if (d.nclass != d.os_y * d.os_x || d.nclass < 1 || d.os_y > 2 || d.os_x > 2) return VPS_EARG(7);
    if (d.ksplit < 1 || (d.ksplit > 1 && !d.ws)) return VPS_EARG(8);
    if (d.offset && (d.nclass != 1 || d.off_ld < 2 * d.KH * d.KW || d.KH * d.KW > 9 || d.H > 65535 || d.W > 65535)) return VPS_EARG(9);
    // deformable layers of the split-operand modes: chunk-major k order only (every layer of the path; the tap-major two-barrier kernel of
    // rounds 1-2 is gone) - a tap-major deformable layer runs in VPS_PREC_F32 (vps_amd/nhwc.py packs it that way)
    if (d.offset && d.prec != VPS_PREC_F32 && d.korder != 1) return VPS_EARG(17);
    if (((uintptr_t)d.in & 15) || ((uintptr_t)d.w & 15) || ((uintptr_t)d.w_split & 15)) return VPS_EARG(10);
    // the split-operand kernels address the input and the weights through 32-bit buffer offsets
    if (d.prec != VPS_PREC_F32 && in_bytes(d) >= 0xFFFFFFF0ull) return VPS_EARG(16);
    // GroupNorm sums in the epilogue: the deformable kernel of the split-operand modes only, unsplit, float4 stores, groups of 4 | 8 | 16 ...
    // One image: the slot has no image dimension, and GroupNorm normalises per image
    if (d.gn_stats && (!d.offset || d.N != 1 ||d.prec == VPS_PREC_F32 || d.ksplit != 1 || d.gn_rep < 1 || (d.gn_rep & (d.gn_rep - 1)) || (d.gn_cpg != 4 && (d.gn_cpg < 8 || (d.gn_cpg & 7))) || d.cout % d.gn_cpg ||
                       ((d.cout | d.out_ld | d.out_coff) & 3) || ((uintptr_t)d.out & 15) || d.res || ((uintptr_t)d.gn_stats & 7)))
        return VPS_EARG(15);
    const long Ml = (long)d.N * d.Qh * d.Qw;
    if (Ml <= 0 || Ml > 0x7fffffffL) return VPS_EARG(11);
    return 0;
}

conv_plan vpsi_conv_plan(const vps_conv_desc& d, const conv_limits& lim, const conv_switches& sw) {
    conv_plan p = {};
    const int M = p.M = (int)((long)d.N * d.Qh * d.Qw);
    if (d.cout <= 4 && d.prec == VPS_PREC_F32 && !d.offset && d.ksplit == 1 && d.tile_n == 32) return plan_small(d, p);
    if (plan_thin(d, lim, sw, p)) return p;

    // every other kernel: 128-row (or patch) tiles x tile_n columns, 256 threads unless the family says otherwise
    const int BN = d.tile_n;
    const int tiles_m = p.tiles_m = cdiv(M, BM);
    const int tiles_n = p.tiles_n = d.cout_pad / BN;
    const int ksteps = d.kpad / BK;
    p.block = 256;
    p.needs_reduce = d.ksplit > 1 && !d.tile_counter;
    if (BN == 256) {
        // deformable layers with >= 256 output channels (round 5): ONE block computes all 256 columns of its 128 pixels - the bilinear
        // loader (4 corner loads + 16 multiply-adds + the fp16 split per staged float4: 8.3 VALU per MFMA with 128 columns) runs once
        // instead of twice. 2 x 2 waves of 64 x 128, accumulators in AGPRs, one block per CU.
        p.per_split = cdiv(ksteps, d.ksplit);
        if (cdiv(ksteps, p.per_split) != d.ksplit) return fail(p, 20);
        p.kernel = CONV_K_DCN256; p.grid = (unsigned)((long)tiles_m * tiles_n * d.ksplit); p.reduce_v4 = true;
        return p;
    }
    // split-K: `ksplit` ranges of ceil(steps / ksplit) k-steps, the last one shorter when the division leaves a rest (every kernel clamps
    // its range). Chunk-major layers (k = (32-channel chunk, tap)) are split over WHOLE chunks when ceil-division of the chunk count
    // reproduces ksplit - the halo-staged kernels need that, and since round 6 the ranges may be uneven: FlowNet's 1026- / 770- / 386-
    // channel decoder layers have 33 / 25 / 13 chunks, no even split exists, and unsplit they filled half of the chip.
    const int ntap = d.KH * d.KW;
    const int nch = d.korder == 1 ? ksteps / ntap : 0;
    const bool chunk_split = d.ksplit > 1 && d.korder == 1 && nch > 0 && cdiv(nch, cdiv(nch, d.ksplit)) == d.ksplit;
    const int per_split = p.per_split = chunk_split ? cdiv(nch, d.ksplit) * ntap : cdiv(ksteps, d.ksplit);
    p.chunks_per_split = per_split / ntap;
    if (cdiv(ksteps, per_split) != d.ksplit) return fail(p, 20);  // caller must pick ksplit | ceil-consistent
    const long nblk = (long)tiles_m * tiles_n * d.nclass * d.ksplit;
    if (nblk <= 0 || nblk > 0x7fffffffL) return fail(p, 21);
    p.reduce_v4 = !((d.cout | d.cout_pad | d.out_ld | d.out_coff) & 3) && !((uintptr_t)d.out & 15) &&
                  (!d.res || (!((d.res_ld | d.res_coff) & 3) && !((uintptr_t)d.res & 15)));
    // stride-1 3x3 / 2x2-class layers on whole 8x16 output patches: halo-staged kernel
    // (patches may overhang the right / bottom edge; used when that wastes less than a third of the computed rows)
    const long tiles2d = (long)d.N * ((d.Qh + 7) / 8) * ((d.Qw + 15) / 16);
    // split-K there is over whole 32-channel chunks: the k-steps of a split must be a whole number of chunks
    const bool halo = d.prec != VPS_PREC_F32 && !d.offset && d.stride == 1 && d.korder == 1 && d.KH == d.KW && (d.KH == 3 || d.KH == 2) &&
                      tiles2d * 128 * 2 <= (long)M * 3 && (d.ksplit == 1 || chunk_split);
    // 8-wave variant (256-row tiles, weights through LDS): 128-column layers in the modes whose two activation planes leave room
    // for the weight buffers, when the 8 x 32 patches waste little and there are enough tiles to give every CU one
    const long tiles2d8 = (long)d.N * ((d.Qh + 7) / 8) * ((d.Qw + 31) / 32);
    const bool h8 = halo && BN == 128 && two_plane(d.prec) && tiles2d8 * 256 * 2 <= (long)M * 3 &&
                    tiles2d8 * tiles_n * d.nclass * d.ksplit >= 256 && ksteps / ntap >= H8_MIN_CHUNKS;
    // stride-2 3x3 / 5x5 layers on the phase-split 8-wave halo kernel (VPS_S2_HALO=0 in the environment switches it off: A/B runs)
    const bool h8s2 = sw.s2_halo && (BN == 128 || BN == 64) && two_plane(d.prec) && !d.offset &&
                      d.stride == 2 && d.nclass == 1 && d.korder == 1 && d.KH == d.KW && (d.KH == 3 || d.KH == 5) &&
                      d.pad_y[0] == d.KH / 2 && d.pad_x[0] == d.KW / 2 && tiles2d8 * 256 * 2 <= (long)M * 3 &&
                      tiles2d8 * tiles_n * d.ksplit >= 256 && (d.ksplit == 1 || chunk_split);
    // 5..32 output channels, stride-1 3x3 / 2x2-class layers with enough 8 x 32 patches: the 16x16x32 kernels
    // (VPS_N32=0: layers with 17 .. 32 output channels stay on the 32-column halo kernel; the two-column-block instance is round 6's)
    const bool n16 = BN == 32 && d.prec == VPS_PREC_F16X3 && halo && d.cout > 4 && d.cout <= (sw.n32 ? 32 : 16) && d.cout_pad == 32 && d.ksplit == 1 &&
                     !d.gn_stats && tiles2d8 * 256 * 2 <= (long)M * 3 && tiles2d8 * d.nclass >= 256;
    if (n16) {
        // VPS_N16T=0 switches the class-fused instance for transposed layers off
        const bool fused = sw.n16t && d.KH == 2 && d.KW == 2 && d.nclass == 4 && d.os_y == 2 && d.os_x == 2 &&
                           d.pad_y[0] >= 0 && d.pad_y[0] <= 1 && d.pad_y[1] >= 0 && d.pad_y[1] <= 1 &&
                           d.pad_x[0] >= 0 && d.pad_x[0] <= 1 && d.pad_x[1] >= 0 && d.pad_x[1] <= 1;
        p.tiles_m = (int)tiles2d8; p.block = 512;
        if (fused && d.cout <= 16) { p.kernel = CONV_K_N16T; p.grid = (unsigned)tiles2d8; }
        else { p.kernel = d.cout > 16 ? CONV_K_N32 : CONV_K_N16; p.grid = (unsigned)(tiles2d8 * d.nclass); }   // 17 .. 32 channels: two column blocks per wave
    } else if (h8s2) {
        p.kernel = CONV_K_H8S2; p.tiles_m = (int)tiles2d8; p.block = 512; p.grid = (unsigned)(tiles2d8 * tiles_n * d.ksplit);
    } else if (h8) {
        // f16x3 3x3: the pipelined instance (conv_h8p.hip, round 6; its 2x2 instance - three chunks of 4 taps unrolled - spills:
        // conv_mfma_h8_kernel keeps those layers)
        p.kernel = sw.h8p && d.prec == VPS_PREC_F16X3 && d.KH == 3 ? CONV_K_H8P : CONV_K_H8;
        p.tiles_m = (int)tiles2d8; p.block = 512; p.grid = (unsigned)(tiles2d8 * tiles_n * d.nclass * d.ksplit);
    } else if (halo) {
        const long nblk2 = tiles2d * tiles_n * d.nclass * d.ksplit;
        if (nblk2 > 0x7fffffffL) return fail(p, 21);
        p.kernel = CONV_K_HALO; p.tiles_m = (int)tiles2d; p.grid = (unsigned)nblk2;
    } else {
        p.grid = (unsigned)nblk;
        const bool tapmajor = d.korder == 0 && ntap > 1;      // small channel counts; a 1x1 layer is the one-tap case of the chunk-major order
        // uniform-lead kernel (conv_q.hip: both operands two k-steps ahead, weights through LDS): every non-deformable layer of the
        // modes with two activation planes on 64- / 128-column tiles. Chunk-major layers only: the tap-major thin first layers measured
        // 12 .. 23 % slower here than on the pipelined kernel - 3 .. 7 k-steps per tile, the longer prologue is not paid back
        const bool q_ok = BN >= 64 && !tapmajor;
        if (q_ok && plan_pw(d, lim, sw, p)) return p;
        if (q_ok && !d.offset && two_plane(d.prec)) p.kernel = CONV_K_Q;
        // deformable layers run the pipelined kernel too (chunk-major k order: vpsi_conv_check)
        else p.kernel = d.prec == VPS_PREC_F32 ? CONV_K_F32 : CONV_K_BF16P;
    }
    return p;
}
