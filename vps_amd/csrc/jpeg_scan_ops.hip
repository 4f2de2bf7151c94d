// Entropy coding of the JPEG output path on the DEVICE (opt-in: `entropy='device'`): quantised coefficients in the layout of
// vps_jpeg_decode_coef -> the entropy-coded segment vps_jpeg_write (jpeg_enc_host.cpp) puts between the SOS header and EOI, byte for
// byte: interleaved MCU order, DC prediction per component, zigzag, ZRL / EOB, one's-complement value bits, the Annex K tables
// (jpeg_tables.h, shared with the host coder), a zero stuffed after every 0xFF, the last byte padded with ones.
// Encoding is parallel: a block's bits depend on its 64 coefficients and one neighbour's DC, its position is a prefix sum, and the
// stuffing is a second one. Five launches on the caller's stream, no sync, no allocation, no memset:
//   1 size    one wavefront per block, 64 blocks of the scan order per workgroup: lane k holds zigzag coefficient k, a 64-bit ballot of
//             the non-zero lanes gives every lane its zero run, and the lane builds its own code (<= 3 ZRL + symbol + value bits, + EOB
//             on the last non-zero lane: <= 63 bits). -> bits per block, bits per workgroup, "a coefficient is out of range"
//   2 offsets one workgroup scans the workgroup sums (768 of them at 1024x2048) and clears the words two workgroups will share
//   3 pack    the same code as 1, now with its position: a wave scan places each lane's code, LDS atomics assemble the workgroup's bits
//             as big-endian words (stream bit 32 w + i = bit 31 - i of word w). Words that lie wholly inside the workgroup's range are
//             stored, the first and last one are OR-ed into the words launch 2 cleared: order-independent, so every call gives the same bytes
//   4 count   0xFF bytes per 4 KiB chunk of the unstuffed stream
//   5 stuff   a chunk's output position = its start + the 0xFF bytes before it; the chunk is laid out with the zeros in LDS and copied
//             to `out` byte-coalesced, every store checked against the capacity; the last chunk writes result = {true size, status}
// Bit offsets are 32-bit: vps_jpeg_scan_bound (and with it the launcher) refuses a size whose worst case does not fit them.
#include "common.h"
#include "jpeg_tables.h"

namespace {

using namespace vps_jpeg;

constexpr int SCAN_THREADS = 256, SCAN_WAVES = SCAN_THREADS / 64;
constexpr int BPW = 16;                                   // blocks per wavefront
constexpr int BPG = BPW * SCAN_WAVES;                     // blocks per workgroup, consecutive in scan order
constexpr int WIN_WORDS = (31 + BPG * (int)kBlockBitsMax + 7 + 31) / 32 + 1;      // a workgroup's bits from a word boundary on, + the pad
constexpr int CHUNK = 4096;                               // bytes of the unstuffed stream per workgroup of launches 4 and 5: 16 per thread
constexpr int OFFS_THREADS = 1024;
constexpr uint32_t BAD = 0x80000000u;                     // flag in a workgroup's bit count: a coefficient no baseline code exists for

// code << 8 | length per symbol: AC [luma, chroma][256], DC [luma, chroma][16]; then the zigzag order. One copy per workgroup in LDS
struct DevHuff {
    uint32_t ac[2][256];
    uint32_t dc[2][16];
    uint32_t zig[64];
};

constexpr void fill(uint32_t* t, const uint8_t* bits, const uint8_t* vals) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) t[vals[k]] = (code << 8) | (uint32_t)l;
        code <<= 1;
    }
}

constexpr DevHuff make_tables() {
    DevHuff h = {};
    fill(h.ac[0], kAcLumaBits, kAcLumaVals);
    fill(h.ac[1], kAcChromaBits, kAcChromaVals);
    fill(h.dc[0], kDcLumaBits, kDcVals);
    fill(h.dc[1], kDcChromaBits, kDcVals);
    for (int k = 0; k < 64; ++k) h.zig[k] = kZigzag[k];
    return h;
}

__device__ const DevHuff kHuff = make_tables();
constexpr int HUFF_WORDS = sizeof(DevHuff) / 4;

struct ScanGeom {
    int sub;                      // 1 = 4:2:0: an MCU is four luma blocks and one of each chroma plane; 0 = 4:4:4: one of each
    int bpm;                      // blocks per MCU: 6 or 3
    int mcu_cols;
    int bcols[3];
    int plane[3];                 // first block of each component in the coefficient array
    int nblk;
};

// the block of the coefficient array that stands at place s of the scan, and its component
__device__ __forceinline__ int block_at(const ScanGeom& g, int s, int& c) {
    const int mcu = s / g.bpm, j = s - mcu * g.bpm;
    const int my = mcu / g.mcu_cols, mx = mcu - my * g.mcu_cols;
    int v = 0, u = 0, f = 1;
    if (g.sub) {
        if (j < 4) { c = 0; v = j >> 1; u = j & 1; f = 2; }
        else c = j - 3;
    } else {
        c = j;
    }
    return g.plane[c] + (my * f + v) * g.bcols[c] + mx * f + u;
}

// the place in the scan of the block whose DC predicts block s: the one before it of the same component; < 0 = none (predictor 0)
__device__ __forceinline__ int pred_of(const ScanGeom& g, int s) {
    if (!g.sub) return s - 3;
    const int j = s % 6;
    if (j == 0) return s - 3;                             // the fourth luma block of the MCU before
    if (j < 4) return s - 1;
    return s - 6;
}

__device__ __forceinline__ void append(uint64_t& v, int& len, uint32_t bits, int n) {
    v = (v << n) | bits;
    len += n;
}

// This lane's share of block s: `v` holds `len` bits (0 = nothing), the first one highest. Lane 0 codes the DC difference (and EOB
// for a block without AC), lane k >= 1 a non-zero coefficient k of the zigzag order with the run in front of it (the last of them
// EOB too, unless it is coefficient 63). bad: a category vps_jpeg_write refuses; such a lane sends nothing.
__device__ __forceinline__ void lane_code(const int16_t* __restrict__ coef, const ScanGeom& g, int s, int lane, const uint32_t* __restrict__ huff,
                                          uint64_t& v, int& len, bool& bad) {
    int c;
    const int16_t* blk = coef + (size_t)block_at(g, s, c) * 64;
    const int t = c ? 1 : 0;
    const uint32_t* ac = huff + 256 * t;
    const uint32_t* dc = huff + 512 + 16 * t;
    int a = blk[huff[544 + lane]];
    if (lane == 0) {
        const int ps = pred_of(g, s);
        if (ps >= 0) {
            int pc;
            a -= coef[(size_t)block_at(g, ps, pc) * 64];
        }
    }
    const uint64_t acm = __ballot(a != 0) & ~1ull;        // the non-zero AC coefficients
    v = 0; len = 0; bad = false;
    if (lane != 0 && a == 0) return;
    const int mag = a < 0 ? -a : a;
    const uint32_t vbits = (uint32_t)(a < 0 ? a - 1 : a); // a negative value is sent as its one's complement
    int cat = mag ? 32 - __clz(mag) : 0;
    bool eob;
    if (lane == 0) {
        if (cat > 11) { bad = true; return; }
        const uint32_t e = dc[cat];
        append(v, len, e >> 8, (int)(e & 255));
        eob = acm == 0;
    } else {
        if (cat > 10) { bad = true; return; }
        const uint64_t below = acm & ((1ull << lane) - 1);
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const int run = lane - prev - 1;
        const uint32_t zrl = ac[0xF0];
        for (int r = run >> 4; r > 0; --r) append(v, len, zrl >> 8, (int)(zrl & 255));
        const uint32_t e = ac[((run & 15) << 4) | cat];
        append(v, len, e >> 8, (int)(e & 255));
        eob = lane != 63 && (acm >> lane) == 1;           // nothing non-zero above this lane
    }
    if (cat) append(v, len, vbits & ((1u << cat) - 1), cat);
    if (eob) append(v, len, ac[0] >> 8, (int)(ac[0] & 255));
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ void load_tables(uint32_t* huff) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&kHuff);
    for (int i = threadIdx.x; i < HUFF_WORDS; i += SCAN_THREADS) huff[i] = src[i];
}

// launch 1
__global__ __launch_bounds__(SCAN_THREADS)
void jpeg_scan_size_kernel(const int16_t* __restrict__ coef, ScanGeom g, uint32_t* __restrict__ nbits, uint32_t* __restrict__ partial) {
    __shared__ uint32_t huff[HUFF_WORDS];
    __shared__ uint32_t wsum[SCAN_WAVES];
    load_tables(huff);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s0 = blockIdx.x * BPG + wave * BPW;
    uint32_t sum = 0;
    for (int i = 0; i < BPW && s0 + i < g.nblk; ++i) {    // the bound is the same for the whole wave
        uint64_t v; int len; bool bad;
        lane_code(coef, g, s0 + i, lane, huff, v, len, bad);
        const uint32_t tot = __shfl(wave_incl_scan((uint32_t)len, lane), 63);
        if (__any(bad)) sum |= BAD;
        if (lane == 0) nbits[s0 + i] = tot;
        sum += tot;
    }
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0, flag = 0;
        for (int w = 0; w < SCAN_WAVES; ++w) { t += wsum[w] & ~BAD; flag |= wsum[w] & BAD; }
        partial[blockIdx.x] = t | flag;
    }
}

// launch 2: base[k] = bits in front of workgroup k, base[ngrp] = all of them; hdr = {bits, bad}; the words the workgroups share are
// cleared. A bad coefficient ends the call here: result = {0, 2}
__global__ __launch_bounds__(OFFS_THREADS)
void jpeg_scan_offsets_kernel(const uint32_t* __restrict__ partial, int ngrp, uint32_t* __restrict__ base, uint32_t* __restrict__ hdr,
                              uint32_t* __restrict__ bitsw, int64_t* __restrict__ result) {
    constexpr int NW = OFFS_THREADS / 64;
    __shared__ uint32_t wl[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0, flag = 0;
    for (int c = 0; c < ngrp; c += OFFS_THREADS) {
        const int k = c + tid;
        const uint32_t p = k < ngrp ? partial[k] : 0u;
        const uint32_t n = p & ~BAD;
        const uint32_t incl = wave_incl_scan(n, lane);
        __syncthreads();                                  // the previous round's reads of wl are done
        if (lane == 63) wl[wave] = incl;
        flag |= p & BAD;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < NW; ++w) {
            if (w < wave) before += wl[w];
            total += wl[w];
        }
        if (k < ngrp) {
            const uint32_t b = carry + before + incl - n;
            base[k] = b;
            bitsw[b >> 5] = 0;
        }
        carry += total;
    }
    const int bad = __syncthreads_or(flag != 0);
    if (tid == 0) {
        base[ngrp] = carry;
        bitsw[carry >> 5] = 0;
        hdr[0] = carry;
        hdr[1] = bad ? 1u : 0u;
        if (bad) { result[0] = 0; result[1] = 2; }
    }
}

// launch 3
__global__ __launch_bounds__(SCAN_THREADS)
void jpeg_scan_pack_kernel(const int16_t* __restrict__ coef, ScanGeom g, const uint32_t* __restrict__ nbits, const uint32_t* __restrict__ base,
                           const uint32_t* __restrict__ hdr, uint32_t* __restrict__ bitsw) {
    __shared__ uint32_t huff[HUFF_WORDS];
    __shared__ uint32_t blkoff[BPG];
    __shared__ uint32_t win[WIN_WORDS];
    if (hdr[1]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b0 = base[blockIdx.x], b1 = base[blockIdx.x + 1];
    const uint32_t pos0 = b0 & 31, end = pos0 + (b1 - b0);                       // the workgroup's bits, counted from its first word
    const uint32_t npad = blockIdx.x == gridDim.x - 1 ? (0u - b1) & 7u : 0u;     // the last byte of the stream is padded with ones
    const int nwords = (int)((end + npad + 31) >> 5);                            // <= WIN_WORDS: a block has at most kBlockBitsMax bits
    for (int w = tid; w < nwords; w += SCAN_THREADS) win[w] = 0;
    load_tables(huff);
    if (wave == 0) {
        const int s = blockIdx.x * BPG + lane;
        const uint32_t n = s < g.nblk ? nbits[s] : 0u;
        blkoff[lane] = pos0 + wave_incl_scan(n, lane) - n;
    }
    __syncthreads();
    if (tid == 0 && npad) atomicOr(&win[end >> 5], ((1u << npad) - 1u) << (32 - (end & 31) - npad));   // within one byte, so one word
    const int s0 = blockIdx.x * BPG + wave * BPW;
    for (int i = 0; i < BPW && s0 + i < g.nblk; ++i) {
        uint64_t v; int len; bool bad;
        lane_code(coef, g, s0 + i, lane, huff, v, len, bad);
        const uint32_t p = blkoff[wave * BPW + i] + wave_incl_scan((uint32_t)len, lane) - (uint32_t)len;
        if (len) {                                        // p + len <= end: the sizes are those of launch 1
            const uint64_t hi = v << (64 - len);
            const uint32_t w = p >> 5, q = p & 31;
            const uint32_t x0 = (uint32_t)((hi >> q) >> 32), x1 = (uint32_t)(hi >> q), x2 = (uint32_t)(hi << (32 - q));
            if (x0) atomicOr(&win[w], x0);
            if (x1) atomicOr(&win[w + 1], x1);            // a non-zero word holds bits of the code, so it lies inside the window
            if (x2) atomicOr(&win[w + 2], x2);
        }
    }
    __syncthreads();
    uint32_t* dst = bitsw + (b0 >> 5);
    for (int w = tid; w < nwords; w += SCAN_THREADS) {
        const uint32_t x = win[w];
        const bool owned = (uint32_t)w * 32 >= pos0 && (uint32_t)(w + 1) * 32 <= end;
        if (owned) dst[w] = x;
        else if (x) atomicOr(&dst[w], x);                 // the word of base[k] or of base[k + 1]: cleared by launch 2
    }
}

// 16 bytes of the unstuffed stream per thread: byte i of the stream is bits 31 - 8 (i & 3) .. of word i / 4
__device__ __forceinline__ int chunk_bytes(const uint32_t* __restrict__ bitsw, uint32_t chunk, uint32_t nbytes, int tid, uint8_t (&b)[16], int& ff) {
    const uint4 q = reinterpret_cast<const uint4*>(bitsw)[(size_t)chunk * (CHUNK / 16) + tid];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    const uint32_t i0 = chunk * CHUNK + tid * 16;
    const int n = i0 >= nbytes ? 0 : (int)min(16u, nbytes - i0);                 // words beyond the stream's end hold anything
    ff = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        b[k] = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
        if (k < n && b[k] == 0xFF) ++ff;
    }
    return n;
}

// sum over the workgroup; every thread gets it. red: SCAN_WAVES words
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < SCAN_WAVES; ++w) t += red[w];
    return t;
}

// launch 4
__global__ __launch_bounds__(SCAN_THREADS)
void jpeg_scan_count_kernel(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bitsw, uint32_t* __restrict__ ffcount) {
    __shared__ uint32_t red[SCAN_WAVES];
    if (hdr[1]) return;
    const uint32_t nbytes = (hdr[0] + 7) >> 3;
    if ((uint64_t)blockIdx.x * CHUNK >= nbytes) return;
    uint8_t b[16]; int ff;
    chunk_bytes(bitsw, blockIdx.x, nbytes, threadIdx.x, b, ff);
    const uint32_t t = block_sum((uint32_t)ff, red);
    if (threadIdx.x == 0) ffcount[blockIdx.x] = t;
}

// launch 5
__global__ __launch_bounds__(SCAN_THREADS)
void jpeg_scan_stuff_kernel(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ bitsw, const uint32_t* __restrict__ ffcount,
                            uint8_t* __restrict__ out, int64_t capacity, int64_t* __restrict__ result) {
    __shared__ uint32_t red[SCAN_WAVES];
    __shared__ uint32_t wtot[SCAN_WAVES];
    __shared__ uint8_t lay[2 * CHUNK];
    if (hdr[1]) return;
    const uint32_t nbytes = (hdr[0] + 7) >> 3;
    if ((uint64_t)blockIdx.x * CHUNK >= nbytes) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t mine = 0;
    for (uint32_t k = tid; k < blockIdx.x; k += SCAN_THREADS) mine += ffcount[k];
    const uint32_t before = block_sum(mine, red);         // 0xFF bytes in the chunks in front of this one
    uint8_t b[16]; int ff;
    const int n = chunk_bytes(bitsw, blockIdx.x, nbytes, tid, b, ff);
    const uint32_t incl = wave_incl_scan((uint32_t)ff, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t lead = 0, here = 0;
    for (int w = 0; w < SCAN_WAVES; ++w) {
        if (w < wave) lead += wtot[w];
        here += wtot[w];
    }
    uint32_t p = tid * 16 + lead + incl - (uint32_t)ff;   // < 2 * CHUNK: at most one zero per byte
    for (int k = 0; k < n; ++k) {
        lay[p++] = b[k];
        if (b[k] == 0xFF) lay[p++] = 0;
    }
    __syncthreads();
    const uint32_t len = min((uint32_t)CHUNK, nbytes - blockIdx.x * CHUNK) + here;
    const int64_t at = (int64_t)blockIdx.x * CHUNK + before;
    for (uint32_t j = tid; j < len; j += SCAN_THREADS)
        if (at + j < capacity) out[at + j] = lay[j];
    if (tid == 0 && blockIdx.x == (nbytes - 1) / CHUNK) {
        result[0] = at + len;
        result[1] = at + len > capacity ? 1 : 0;
    }
}

struct ScanWs {
    uint32_t *hdr, *nbits, *partial, *base, *ffcount, *bitsw;
    int ngrp, nchunk;
    int64_t bytes;
};

inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }

ScanWs scan_layout(uint8_t* ws, int64_t nblk) {
    ScanWs w;
    w.ngrp = (int)((nblk + BPG - 1) / BPG);
    w.nchunk = (int)((nblk * (kBlockBytesMax / 2) + CHUNK - 1) / CHUNK + 1);     // the unstuffed worst case + the word of the last offset
    int64_t at = 0;
    auto take = [&](int64_t n) { uint8_t* p = ws ? ws + at : nullptr; at += up16(n); return reinterpret_cast<uint32_t*>(p); };
    w.hdr = take(16);
    w.nbits = take(nblk * 4);
    w.partial = take((int64_t)w.ngrp * 4);
    w.base = take((int64_t)(w.ngrp + 1) * 4);
    w.ffcount = take((int64_t)w.nchunk * 4);
    w.bitsw = take((int64_t)w.nchunk * CHUNK);
    w.bytes = at;
    return w;
}

}  // namespace

extern "C" int vps_jpeg_scan_bound(int H, int W, int subsampling, int64_t* ws_bytes, int64_t* scan_bytes) {
    int32_t grid[6];
    int64_t file = 0;
    int st = vps_jpeg_encode_bound(H, W, subsampling, grid, nullptr);            // size and mode checks live there
    if (st) return st;
    st = vps_jpeg_write_bound(H, W, subsampling, &file);
    if (st) return st;
    int64_t nblk = 0;
    for (int c = 0; c < 3; ++c) nblk += (int64_t)grid[2 * c] * grid[2 * c + 1];
    // 32-bit bit offsets: the worst case of the unstuffed stream, in whole bytes per block, has to fit them
    if (nblk * (kBlockBytesMax / 2) * 8 + 8 > 0xFFFFFFFFll) return VPS_EARG(7);
    if (ws_bytes) *ws_bytes = scan_layout(nullptr, nblk).bytes;
    if (scan_bytes) *scan_bytes = file - kHeaderBytes - kTrailerBytes;           // vps_jpeg_write_bound's own arithmetic
    return 0;
}

extern "C" int vps_jpeg_encode_scan(const int16_t* coef, int H, int W, int subsampling, uint8_t* out, int64_t capacity, int64_t* result,
                                    void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int64_t need = 0;
    const int st = vps_jpeg_scan_bound(H, W, subsampling, &need, nullptr);
    if (st) return st;
    if (!coef || (!out && capacity > 0) || !result || !ws || capacity < 0) return VPS_EARG(3);      // capacity 0 only asks for the size
    if (((uintptr_t)coef & 1) || ((uintptr_t)ws & 15) || ((uintptr_t)result & 7)) return VPS_EARG(4);
    if (ws_bytes < need) return VPS_EARG(5);
    int32_t grid[6];
    vps_jpeg_encode_bound(H, W, subsampling, grid, nullptr);
    ScanGeom g;
    g.sub = subsampling == 2;
    g.bpm = g.sub ? 6 : 3;
    g.mcu_cols = grid[3];
    g.nblk = 0;
    for (int c = 0; c < 3; ++c) {
        g.bcols[c] = grid[2 * c + 1];
        g.plane[c] = g.nblk;
        g.nblk += grid[2 * c] * grid[2 * c + 1];
    }
    const ScanWs w = scan_layout(static_cast<uint8_t*>(ws), g.nblk);
    hipLaunchKernelGGL(jpeg_scan_size_kernel, dim3(w.ngrp), dim3(SCAN_THREADS), 0, stream, coef, g, w.nbits, w.partial);
    hipLaunchKernelGGL(jpeg_scan_offsets_kernel, dim3(1), dim3(OFFS_THREADS), 0, stream, (const uint32_t*)w.partial, w.ngrp, w.base, w.hdr, w.bitsw,
                       result);
    hipLaunchKernelGGL(jpeg_scan_pack_kernel, dim3(w.ngrp), dim3(SCAN_THREADS), 0, stream, coef, g, (const uint32_t*)w.nbits,
                       (const uint32_t*)w.base, (const uint32_t*)w.hdr, w.bitsw);
    hipLaunchKernelGGL(jpeg_scan_count_kernel, dim3(w.nchunk), dim3(SCAN_THREADS), 0, stream, (const uint32_t*)w.hdr, (const uint32_t*)w.bitsw,
                       w.ffcount);
    hipLaunchKernelGGL(jpeg_scan_stuff_kernel, dim3(w.nchunk), dim3(SCAN_THREADS), 0, stream, (const uint32_t*)w.hdr, (const uint32_t*)w.bitsw,
                       (const uint32_t*)w.ffcount, out, capacity, result);
    return vps_launch_status();
}
