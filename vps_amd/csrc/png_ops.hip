// Device PNG encoder for the output side of the clip pipeline: a uint8 [H][W][C] label map (C = 1 or 3) ->
// one zlib stream that any inflate reads, without a match search. The stream format is fixed (include/vps_hip.h, vps_png_deflate) so
// that tests/png_restate.py can produce the same bytes on the CPU:
//   kernel 1  png_filter_kernel   per row, libpng's minimum-sum-of-absolute-residuals choice among None / Sub / Up -> one byte per row
//   kernel 2  png_encode_kernel   per SEG bytes of the filtered stream S (never stored): residuals on the fly -> runs of equal bytes ->
//                                 literals and distance-1 matches in the fixed Huffman code -> the segment's worst-case slot in the
//                                 workspace, with its byte length and its Adler-32 sums
//   kernel 3  png_scan_kernel     exclusive scan of the segment lengths, Adler-32 of S from the per-segment sums, header, trailer, size
//   kernel 4  png_gather_kernel   segments -> the contiguous stream
// A label map after Sub / Up is nearly all zeros, so almost every token is a 13-bit match of 258 bytes: the output is 1/46 .. 1/72 of
// the image and the kernels are bound by reading the image twice.
#include "common.h"

namespace {

constexpr int PNG_SEG = 8192;                                   // bytes of S per independently encoded segment (power of two, 4 .. 32 KiB)
constexpr int PNG_THREADS = 256;
constexpr int PNG_CHUNK = PNG_SEG / PNG_THREADS;                // consecutive positions of a segment one thread owns
static_assert(PNG_CHUNK == 32, "one 32-bit run-start mask per thread");
constexpr int PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_SEG_MAX = (9 * PNG_SEG + 7) / 8 + 7;          // worst-case bytes of an encoded segment
constexpr int PNG_SLOT = (PNG_SEG_MAX + 4 + 15) / 16 * 16;      // its slot in the workspace (+ 4: the gather reads whole words)
constexpr int PNG_OUT_WORDS = PNG_SLOT / 4;
constexpr uint32_t ADLER_MOD = 65521;
constexpr int SCAN_THREADS = 256;                              // segments per step of the scan: a full-size map (766) takes three

struct PngSegInfo {
    uint32_t nbytes;              // encoded bytes of the segment
    uint32_t s1, s2;              // sum of its bytes, sum of (n - i) * byte[i]; both mod 65521
    uint32_t n;                   // bytes of S it covers
};

struct PngWs {
    uint8_t* ftype;               // [H] filter type per row
    PngSegInfo* info;             // [nseg]
    int64_t* offset;              // [nseg] exclusive scan of nbytes
    int32_t* ok;                  // [1] 1 = the stream fits the output
    uint8_t* slots;               // [nseg][PNG_SLOT]
    int64_t bytes;
};

static inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

static PngWs png_layout(uint8_t* base, int H, int64_t nseg) {
    PngWs w;
    int64_t off = 0;
    w.ftype = base + off; off += align16(H);
    w.info = reinterpret_cast<PngSegInfo*>(base + off); off += align16(nseg * (int64_t)sizeof(PngSegInfo));
    w.offset = reinterpret_cast<int64_t*>(base + off); off += align16(nseg * 8);
    w.ok = reinterpret_cast<int32_t*>(base + off); off += 16;
    w.slots = base + off; off += nseg * PNG_SLOT;
    w.bytes = off;
    return w;
}

__device__ __forceinline__ uint32_t abs_i8(uint32_t v) { v &= 255u; return v < 128u ? v : 256u - v; }

// ---------------------------------------------------------------------------------------------------------------------------------
// kernel 1: one block per row. A thread takes four bytes per step; with 4-byte aligned rows it reads them (and the row above) as one
// word and takes the bytes to the left from the previous word.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS)
void png_filter_kernel(const uint8_t* __restrict__ img, int rowbytes, int C, int64_t stride, int aligned, uint8_t* __restrict__ ftype) {
    __shared__ uint32_t red[3][PNG_WAVES];
    const int y = blockIdx.x;
    const uint8_t* row = img + (int64_t)y * stride;
    const uint8_t* up = y > 0 ? row - stride : nullptr;
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (int x0 = threadIdx.x * 4; x0 < rowbytes; x0 += PNG_THREADS * 4) {
        uint32_t cur, above = 0, left;
        if (aligned && x0 + 4 <= rowbytes) {
            cur = *reinterpret_cast<const uint32_t*>(row + x0);
            if (up) above = *reinterpret_cast<const uint32_t*>(up + x0);
            const uint32_t before = x0 ? *reinterpret_cast<const uint32_t*>(row + x0 - 4) : 0u;
            if (C <= 4) {
                left = (uint32_t)(((((uint64_t)cur) << 32) | before) >> (8 * (4 - C)));
            } else {                                             // C in 5 .. 8 (16-bit RGB: 6): the bytes to the left lie in the two words before
                const uint32_t before2 = x0 >= 8 ? *reinterpret_cast<const uint32_t*>(row + x0 - 8) : 0u;
                left = (uint32_t)(((((uint64_t)before) << 32) | before2) >> (8 * (8 - C)));
            }
        } else {
            cur = 0; left = 0;
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (x >= rowbytes) break;
                cur |= (uint32_t)row[x] << (8 * k);
                if (up) above |= (uint32_t)up[x] << (8 * k);
                if (x >= C) left |= (uint32_t)row[x - C] << (8 * k);
            }
        }
        const int nb = min(4, rowbytes - x0);
        for (int k = 0; k < 4; ++k) {
            if (k >= nb) break;
            const uint32_t r = cur >> (8 * k), l = left >> (8 * k), a = above >> (8 * k);
            s0 += abs_i8(r); s1 += abs_i8(r - l); s2 += abs_i8(r - a);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_down(s0, d); s1 += __shfl_down(s1, d); s2 += __shfl_down(s2, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; red[2][wave] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t0 = 0, t1 = 0, t2 = 0;
        for (int w = 0; w < PNG_WAVES; ++w) { t0 += red[0][w]; t1 += red[1][w]; t2 += red[2][w]; }
        int best = 0;
        uint32_t bs = t0;
        if (t1 < bs) { best = 1; bs = t1; }
        if (t2 < bs) best = 2;                                   // a tie keeps the lower type number
        ftype[y] = (uint8_t)best;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kernel 2
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lit_bits(uint32_t v) { return v < 144u ? 8 : 9; }

// length 3 .. 257 -> (Huffman code bit-reversed | extra bits, total bits without the distance code)
__device__ __forceinline__ void len_code(int L, uint32_t& val, int& nbits) {
    const int l = L - 3;
    int e = 0, sym = 257 + l;
    if (l >= 8) {
        e = 29 - __clz(l);
        sym = 261 + 4 * e + ((l >> e) & 3);
    }
    const int hb = sym < 280 ? 7 : 8;
    const uint32_t code = sym < 280 ? (uint32_t)(sym - 256) : (uint32_t)(0xC0 + sym - 280);
    val = (__brev(code) >> (32 - hb)) | ((uint32_t)(l & ((1 << e) - 1)) << hb);
    nbits = hb + e;
}

__device__ __forceinline__ int run_bits(uint32_t v, int R) {
    const int lb = lit_bits(v);
    const int r = R - 1, nfull = r / 258, rem = r - nfull * 258;
    int bits = lb + 13 * nfull;
    if (rem >= 3) {
        uint32_t val; int nb;
        len_code(rem, val, nb);
        bits += nb + 5;
    } else {
        bits += rem * lb;
    }
    return bits;
}

// a thread's tokens are contiguous in the bit stream: whole words are OR-ed into the zeroed LDS image (the first and last word of a
// thread's range are shared with its neighbours)
struct BitWriter {
    uint32_t* out;
    uint64_t acc;
    int nacc, word;
    __device__ __forceinline__ void put(uint32_t v, int n) {           // n <= 18
        acc |= (uint64_t)v << nacc;
        nacc += n;
        if (nacc >= 32) {
            atomicOr(&out[word++], (uint32_t)acc);
            acc >>= 32; nacc -= 32;
        }
    }
    __device__ __forceinline__ void flush() { if (nacc > 0 && (uint32_t)acc) atomicOr(&out[word], (uint32_t)acc); }
};

__device__ __forceinline__ void put_literal(BitWriter& bw, uint32_t v) {
    if (v < 144u) bw.put(__brev(0x30u + v) >> 24, 8);
    else bw.put(__brev(0x190u + v - 144u) >> 23, 9);
}

__device__ __forceinline__ void emit_run(BitWriter& bw, uint32_t v, int R) {
    put_literal(bw, v);
    const int r = R - 1, nfull = r / 258, rem = r - nfull * 258;
    for (int k = 0; k < nfull; ++k) bw.put(0xA3u, 13);                 // symbol 285 (0xC5, 8 bits, reversed) + distance code 0
    if (rem >= 3) {
        uint32_t val; int nb;
        len_code(rem, val, nb);
        bw.put(val, nb + 5);
    } else {
        for (int k = 0; k < rem; ++k) put_literal(bw, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the dynamic-Huffman instance of kernel 2 (vps_png_deflate_h, huffman = 1; the format is in include/vps_hip.h). Same tokens; the
// workgroup then builds the segment's own code in LDS and writes an RFC 1951 dynamic block where that is shorter:
//   histogram   286 literal/length counts (end-of-block 1) by LDS atomics, from the same walk over the run starts as pass A
//   lengths     package-merge, limit 15 (pm_lengths below; limit 7 for the 19 code-length symbols through the same routine). Leaves =
//               the symbols with a count, ascending by (count, symbol). List 1 = the leaves; list j = the leaves merged by weight with
//               the packages of list j-1 (item 2k + item 2k+1, an odd last item dropped), a LEAF IN FRONT OF A PACKAGE OF EQUAL WEIGHT,
//               cut to its first 2n-2 items. Top list: take k = 2n-2 items; a of them are leaves -> the a first leaves gain one bit,
//               the list below gives 2 (k - a) items. Only "is item p of list j a leaf" is kept (one bit each), so the walk down
//               is one masked popcount per level. Package-merge is optimal under the limit, so where the Huffman tree fits the cost is
//               the Huffman cost. One symbol with a count gets length 1 (cannot happen here: a literal and end-of-block are always there)
//   codes       canonical (RFC 1951 3.2.2), kept bit-reversed with the length in bits 16..
//   header      by wave 0, five entries of the HLIT + 2 code lengths per lane: runs of equal lengths -> 16 / 17 / 18 by the greedy rule
//               of cl_run, counted, coded with the limit-7 code, HCLEN trimmed in the RFC's order
//   choice      dynamic only if the fixed block has >= PNG_DYN_MIN_FIXED bits and the dynamic one is strictly shorter; else pass B is
//               the fixed instance's, bit for bit
// LDS beside res32 / outw / msk and the wave sums (18.1 KiB): PngDyn, 10.6 KiB -> 28.7 KiB per workgroup.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int PNG_NSYM = 286;
constexpr int PNG_NSYM_PAD = 288;
constexpr int PNG_PM_ITEMS = 2 * PNG_NSYM - 2;                  // longest list of the package-merge
constexpr int PNG_PM_WORDS = (PNG_PM_ITEMS + 31) / 32;
constexpr uint32_t PNG_DYN_MIN_FIXED = 512;                     // bits of the fixed block below which a segment stays fixed
__device__ const uint8_t PNG_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngDyn {
    uint32_t hist[PNG_NSYM_PAD];              // literal/length counts
    uint32_t leaf[PNG_NSYM_PAD];              // weights of the leaves in order
    uint32_t rank[PNG_NSYM_PAD];              // place of a symbol among the leaves
    uint32_t list[2][PNG_PM_ITEMS + 2];       // weights of list j-1 and list j
    uint32_t lmask[15][PNG_PM_WORDS];         // bit p of level j: item p of list j is a leaf
    uint32_t nleaf_taken[16];                 // a of each level
    uint32_t code[PNG_NSYM_PAD];              // reversed code | length << 16
    uint32_t clfreq[20], clcode[20];
    uint8_t len[PNG_NSYM_PAD];
    uint8_t cllen[20];
    uint32_t wsum_d[PNG_WAVES];
    uint32_t hdr_bits;
};

// freq[nsym] -> len[nsym], every length <= limit (nsym <= 286 <= 2^limit). Every thread of the workgroup calls it.
__device__ void pm_lengths(const uint32_t* freq, int nsym, int limit, uint8_t* len, PngDyn& d) {
    const int tid = threadIdx.x, lane = tid & 63;
    // order of the leaves: key = count << 9 | symbol
    const int sa = tid, sb = tid + PNG_THREADS;
    const uint32_t ca = sa < nsym ? freq[sa] : 0u, cb = sb < nsym ? freq[sb] : 0u;
    const uint32_t ka = (ca << 9) | (uint32_t)sa, kb = (cb << 9) | (uint32_t)sb;
    int n = 0, ra = 0, rb = 0;
    for (int s = 0; s < nsym; ++s) {
        const uint32_t c = freq[s];
        const uint32_t k = c ? ((c << 9) | (uint32_t)s) : 0xFFFFFFFFu;
        n += c != 0u; ra += k < ka; rb += k < kb;
    }
    if (ca) { d.rank[sa] = (uint32_t)ra; d.leaf[ra] = ca; }
    if (cb) { d.rank[sb] = (uint32_t)rb; d.leaf[rb] = cb; }
    for (int i = tid; i < 15 * PNG_PM_WORDS; i += PNG_THREADS) (&d.lmask[0][0])[i] = 0u;
    __syncthreads();
    if (n < 2) {
        if (sa < nsym) len[sa] = ca ? 1 : 0;
        if (sb < nsym) len[sb] = cb ? 1 : 0;
        __syncthreads();
        return;
    }
    const int cut = 2 * n - 2;
    int mprev = 0;
    for (int j = 0; j < limit; ++j) {
        const uint32_t* prev = d.list[(j + 1) & 1];
        uint32_t* cur = d.list[j & 1];
        const int np = mprev >> 1;
        for (int i = tid; i < n + np; i += PNG_THREADS) {
            uint32_t w;
            int pos;
            if (i < n) {                                          // leaf i: in front of it, the packages lighter than it
                w = d.leaf[i];
                int lo = 0, hi = np;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (prev[2 * mid] + prev[2 * mid + 1] < w) lo = mid + 1; else hi = mid;
                }
                pos = i + lo;
                if (pos < cut) atomicOr(&d.lmask[j][pos >> 5], 1u << (pos & 31));
            } else {                                              // package k: in front of it, the leaves not heavier than it
                const int k = i - n;
                w = prev[2 * k] + prev[2 * k + 1];
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (d.leaf[mid] <= w) lo = mid + 1; else hi = mid;
                }
                pos = k + lo;
            }
            if (pos < cut) cur[pos] = w;
        }
        mprev = min(n + np, cut);
        __syncthreads();
    }
    if (tid < 64) {                                               // the walk down, by wave 0
        int k = cut;
        for (int j = limit - 1; j >= 0; --j) {
            uint32_t c = 0;
            if (lane < PNG_PM_WORDS) {
                const int lo = 32 * lane;
                const uint32_t keep = k >= lo + 32 ? 0xFFFFFFFFu : (k > lo ? (1u << (k - lo)) - 1u : 0u);
                c = (uint32_t)__popc(d.lmask[j][lane] & keep);
            }
            for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
            if (lane == 0) d.nleaf_taken[j] = c;
            k = 2 * (k - (int)c);
        }
    }
    __syncthreads();
    int la = 0, lb = 0;
    for (int j = 0; j < limit; ++j) {
        const uint32_t a = d.nleaf_taken[j];
        la += a > (uint32_t)ra; lb += a > (uint32_t)rb;
    }
    if (sa < nsym) len[sa] = (uint8_t)(ca ? la : 0);
    if (sb < nsym) len[sb] = (uint8_t)(cb ? lb : 0);
    __syncthreads();
}

// canonical codes of len[nsym]: code = (sum over shorter symbols of 2^(own length - theirs)) + (symbols of the own length before it)
__device__ void canonical_codes(const uint8_t* len, int nsym, uint32_t* code) {
    for (int s = threadIdx.x; s < nsym; s += PNG_THREADS) {
        const int l = len[s];
        uint32_t c = 0;
        if (l) {
            for (int t = 0; t < nsym; ++t) {
                const int lt = len[t];
                if (lt && lt < l) c += 1u << (l - lt);
                else if (lt == l && t < s) ++c;
            }
            c = (__brev(c) >> (32 - l)) | ((uint32_t)l << 16);
        }
        code[s] = c;
    }
    __syncthreads();
}

// length 3 .. 258 -> its symbol and the number of extra bits (RFC 1951 3.2.5)
__device__ __forceinline__ int len_symbol(int L, int& e) {
    const int l = L - 3;
    e = 0;
    if (L == 258) return 285;
    if (l < 8) return 257 + l;
    e = 29 - __clz(l);
    return 261 + 4 * e + ((l >> e) & 3);
}

// the code-length tokens of one run of R equal lengths v: f(symbol, extra value, extra bits)
template <class F>
__device__ __forceinline__ void cl_run(int v, int R, F&& f) {
    if (v == 0) {
        while (R >= 11) { const int c = min(R, 138); f(18, c - 11, 7); R -= c; }
        if (R >= 3) { f(17, R - 3, 3); R = 0; }
        for (; R > 0; --R) f(0, 0, 0);
    } else {
        f(v, 0, 0); --R;
        while (R >= 3) { const int c = min(R, 6); f(16, c - 3, 2); R -= c; }
        for (; R > 0; --R) f(v, 0, 0);
    }
}

// a lane's runs of the code-length sequence (entry i < hlit: len[i]; the two behind: 1, the distance code)
template <class F>
__device__ __forceinline__ void cl_walk(const uint8_t* len, int hlit, int lane, uint32_t m5, int nxt5, F&& f) {
    for (uint32_t mm = m5; mm;) {
        const int p = 5 * lane + __ffs((int)mm) - 1;
        mm &= mm - 1;
        const int q = mm ? 5 * lane + __ffs((int)mm) - 1 : nxt5;
        cl_run(p < hlit ? (int)len[p] : 1, q - p, f);
    }
}

__device__ __forceinline__ int dyn_run_bits(const uint32_t* code, uint32_t v, int R) {
    const int lb = (int)(code[v] >> 16);
    const int r = R - 1, nfull = r / 258, rem = r - nfull * 258;
    int bits = lb + nfull * ((int)(code[285] >> 16) + 1);
    if (rem >= 3) {
        int e;
        const int sym = len_symbol(rem, e);
        bits += (int)(code[sym] >> 16) + e + 1;
    } else {
        bits += rem * lb;
    }
    return bits;
}

// a match is up to 15 + 5 + 1 bits: the code in one put, the extra bits and the distance code (one 0 bit) in a second
__device__ __forceinline__ void dyn_emit_run(BitWriter& bw, const uint32_t* code, uint32_t v, int R) {
    const uint32_t cv = code[v];
    bw.put(cv & 0xFFFFu, (int)(cv >> 16));
    const int r = R - 1, nfull = r / 258, rem = r - nfull * 258;
    const uint32_t c285 = code[285];
    for (int k = 0; k < nfull; ++k) bw.put(c285 & 0xFFFFu, (int)(c285 >> 16) + 1);
    if (rem >= 3) {
        int e;
        const uint32_t c = code[len_symbol(rem, e)];
        bw.put(c & 0xFFFFu, (int)(c >> 16));
        bw.put((uint32_t)((rem - 3) & ((1 << e) - 1)), e + 1);
    } else {
        for (int k = 0; k < rem; ++k) bw.put(cv & 0xFFFFu, (int)(cv >> 16));
    }
}

template <bool DYN>
__global__ __launch_bounds__(PNG_THREADS)
void png_encode_kernel(const uint8_t* __restrict__ img, int H, int rowlen, int C, int64_t stride, int64_t N,
                       const uint8_t* __restrict__ ftype, PngSegInfo* __restrict__ info, uint8_t* __restrict__ slots) {
    __shared__ __attribute__((aligned(16))) uint32_t res32[PNG_SEG / 4];     // the segment's bytes of S
    __shared__ __attribute__((aligned(16))) uint32_t outw[PNG_OUT_WORDS];    // its encoded image
    __shared__ uint32_t msk[PNG_THREADS];                                    // run starts, bit j of word t = position 32 t + j
    __shared__ unsigned long long nzmask[PNG_WAVES];                         // which words of a wave hold a run start
    __shared__ uint32_t wsum[PNG_WAVES];
    __shared__ unsigned long long asum[2][PNG_WAVES];
    __shared__ __attribute__((aligned(16))) uint32_t dyn_words[DYN ? (sizeof(PngDyn) + 3) / 4 : 1];
    PngDyn& dy = *reinterpret_cast<PngDyn*>(dyn_words);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * PNG_SEG;
    const int n = (int)min((int64_t)PNG_SEG, N - base);
    const int64_t row0 = base / rowlen;
    const uint32_t col0 = (uint32_t)(base - row0 * rowlen);

    for (int w = tid; w < PNG_OUT_WORDS; w += PNG_THREADS) outw[w] = 0;
    if constexpr (DYN) {
        for (int i = tid; i < PNG_NSYM_PAD; i += PNG_THREADS) dy.hist[i] = i == 256 ? 1u : 0u;
        if (tid < 20) dy.clfreq[tid] = 0u;
    }
    // stage 1: filter on the fly; four consecutive bytes of S per thread and step
    for (int w = tid; w < PNG_SEG / 4; w += PNG_THREADS) {
        const int i0 = 4 * w;
        uint32_t word = 0;
        if (i0 < n) {
            const uint32_t q = (col0 + (uint32_t)i0) / (uint32_t)rowlen;
            int64_t row = row0 + q;
            int col = (int)(col0 + (uint32_t)i0 - q * (uint32_t)rowlen);
            int f = ftype[row];
            const uint8_t* p = img + row * stride;
            for (int k = 0; k < 4; ++k) {
                if (i0 + k >= n) break;
                uint32_t b;
                if (col == 0) {
                    b = (uint32_t)f;
                } else {
                    const int x = col - 1;
                    b = p[x];
                    if (f == 1) { if (x >= C) b -= p[x - C]; }
                    else if (f == 2) { if (row > 0) b -= p[x - stride]; }
                }
                word |= (b & 255u) << (8 * k);
                if (++col == rowlen) {
                    col = 0; ++row;
                    if (row < H) { f = ftype[row]; p = img + row * stride; }
                }
            }
        }
        res32[w] = word;
    }
    __syncthreads();

    // stage 2: run starts and Adler sums of the thread's 32 positions
    const uint8_t* res8 = reinterpret_cast<const uint8_t*>(res32);
    const int p0 = tid * PNG_CHUNK;
    uint32_t m = 0, a1 = 0, a2 = 0;
    {
        uint32_t prev = tid ? res8[p0 - 1] : 0u;
#pragma unroll
        for (int w = 0; w < PNG_CHUNK / 4; ++w) {
            const uint32_t cur = res32[tid * (PNG_CHUNK / 4) + w];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t b = (cur >> (8 * k)) & 255u;
                const int j = 4 * w + k;
                m |= (uint32_t)(b != prev) << j;
                a1 += b; a2 += (uint32_t)(PNG_CHUNK - j) * b;
                prev = b;
            }
        }
    }
    const int cnt = max(0, min(PNG_CHUNK, n - p0));
    m &= cnt == PNG_CHUNK ? 0xFFFFFFFFu : ((1u << cnt) - 1u);
    if (tid == 0) m |= 1u;                                                   // n >= 1: a segment opens with a literal
    msk[tid] = m;
    const unsigned long long nz = __ballot(m != 0);
    if (lane == 0) nzmask[wave] = nz;
    // bytes past n are zero, so the sums need no mask; weight of position i is (n - i)
    long long s1 = a1, s2 = (long long)(n - p0 - PNG_CHUNK) * (long long)a1 + (long long)a2;
    for (int d = 32; d >= 1; d >>= 1) { s1 += __shfl_down(s1, d); s2 += __shfl_down(s2, d); }
    if (lane == 0) { asum[0][wave] = (unsigned long long)s1; asum[1][wave] = (unsigned long long)s2; }
    __syncthreads();

    // first run start after this thread's word (or n)
    int nxt = n;
    {
        const unsigned long long later = lane == 63 ? 0ull : (nzmask[wave] >> (lane + 1)) << (lane + 1);
        int word = -1;
        if (later) word = wave * 64 + __ffsll((long long)later) - 1;
        else
            for (int w = wave + 1; w < PNG_WAVES; ++w)
                if (nzmask[w]) { word = w * 64 + __ffsll((long long)nzmask[w]) - 1; break; }
        if (word >= 0) nxt = word * PNG_CHUNK + __ffs((int)msk[word]) - 1;
    }
    // pass A: bits of the thread's runs
    uint32_t bits = 0;
    for (uint32_t mm = m; mm;) {
        const int p = __ffs((int)mm) - 1;
        mm &= mm - 1;
        const int q = mm ? p0 + __ffs((int)mm) - 1 : nxt;
        bits += (uint32_t)run_bits(res8[p0 + p], q - (p0 + p));
    }
    uint32_t incl = bits;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tok_bits = 0;
    for (int w = 0; w < PNG_WAVES; ++w) {
        if (w < wave) before += wsum[w];
        tok_bits += wsum[w];
    }
    bool use_dyn = false;
    uint32_t dyn_total = 0;
    if constexpr (DYN) {
        if (3u + tok_bits + 7u >= PNG_DYN_MIN_FIXED) {                         // the same for the whole workgroup
            // histogram: the walk of pass A
            for (uint32_t mm = m; mm;) {
                const int p = __ffs((int)mm) - 1;
                mm &= mm - 1;
                const int q = mm ? p0 + __ffs((int)mm) - 1 : nxt;
                const uint32_t v = res8[p0 + p];
                const int r = q - (p0 + p) - 1, nfull = r / 258, rem = r - nfull * 258;
                atomicAdd(&dy.hist[v], 1u + (rem < 3 ? (uint32_t)rem : 0u));
                if (nfull) atomicAdd(&dy.hist[285], (uint32_t)nfull);
                if (rem >= 3) { int e; atomicAdd(&dy.hist[len_symbol(rem, e)], 1u); }
            }
            __syncthreads();
            pm_lengths(dy.hist, PNG_NSYM, 15, dy.len, dy);
            canonical_codes(dy.len, PNG_NSYM, dy.code);
            // header, first half (wave 0): HLIT, the lane's run starts among its five entries, the counts of the code-length symbols
            int hlit = 257, nxt5 = 0;
            uint32_t m5 = 0;
            if (wave == 0) {
                const unsigned long long used = __ballot(lane < 29 && dy.len[257 + lane] != 0);
                if (used) hlit = 257 + 64 - __clzll((long long)used);
                const int T = hlit + 2;
                for (int k = 0; k < 5; ++k) {
                    const int i = 5 * lane + k;
                    if (i >= T) break;
                    const int cur = i < hlit ? (int)dy.len[i] : 1;
                    const int prv = i == 0 ? -1 : (i - 1 < hlit ? (int)dy.len[i - 1] : 1);
                    m5 |= (uint32_t)(cur != prv) << k;
                }
                const unsigned long long nz5 = __ballot(m5 != 0);
                const unsigned long long later = lane == 63 ? 0ull : (nz5 >> (lane + 1)) << (lane + 1);
                const int src = later ? __ffsll((long long)later) - 1 : lane;
                const uint32_t ms = __shfl(m5, src);
                nxt5 = later ? 5 * src + __ffs((int)ms) - 1 : T;
                cl_walk(dy.len, hlit, lane, m5, nxt5, [&](int sym, int, int) { atomicAdd(&dy.clfreq[sym], 1u); });
            }
            __syncthreads();
            pm_lengths(dy.clfreq, 19, 7, dy.cllen, dy);
            canonical_codes(dy.cllen, 19, dy.clcode);
            // header, second half: HCLEN, the bits of each lane's code-length tokens and where they start
            int hclen = 4;
            uint32_t hoff = 0;
            if (wave == 0) {
                const unsigned long long usedcl = __ballot(lane < 19 && dy.cllen[PNG_CL_ORDER[lane < 19 ? lane : 0]] != 0);
                hclen = usedcl ? max(4, 64 - __clzll((long long)usedcl)) : 4;
                uint32_t hb = 0;
                cl_walk(dy.len, hlit, lane, m5, nxt5, [&](int sym, int, int eb) { hb += (dy.clcode[sym] >> 16) + (uint32_t)eb; });
                uint32_t hincl = hb;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(hincl, d);
                    if (lane >= d) hincl += o;
                }
                hoff = 17u + 3u * (uint32_t)hclen + hincl - hb;
                if (lane == 63) dy.hdr_bits = 17u + 3u * (uint32_t)hclen + hincl;
            }
            // pass A again with the segment's own code
            uint32_t bits_d = 0;
            for (uint32_t mm = m; mm;) {
                const int p = __ffs((int)mm) - 1;
                mm &= mm - 1;
                const int q = mm ? p0 + __ffs((int)mm) - 1 : nxt;
                bits_d += (uint32_t)dyn_run_bits(dy.code, res8[p0 + p], q - (p0 + p));
            }
            uint32_t incl_d = bits_d;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl_d, d);
                if (lane >= d) incl_d += o;
            }
            if (lane == 63) dy.wsum_d[wave] = incl_d;
            __syncthreads();
            uint32_t before_d = 0, tok_d = 0;
            for (int w = 0; w < PNG_WAVES; ++w) {
                if (w < wave) before_d += dy.wsum_d[w];
                tok_d += dy.wsum_d[w];
            }
            const uint32_t hdr_bits = dy.hdr_bits;
            dyn_total = hdr_bits + tok_d + (dy.code[256] >> 16);
            use_dyn = dyn_total < 3u + tok_bits + 7u;
            if (use_dyn) {
                // pass B with the segment's own code; the header's bits come first and are wave 0's
                if (wave == 0) {
                    BitWriter hw{outw, 0ull, (int)(hoff & 31u), (int)(hoff >> 5)};
                    if (lane == 0) {
                        hw = BitWriter{outw, 0ull, 0, 0};
                        // BFINAL 0, BTYPE 10, HLIT - 257, HDIST - 1 = 1, HCLEN - 4
                        hw.put(4u | ((uint32_t)(hlit - 257) << 3) | (1u << 8), 13);
                        hw.put((uint32_t)(hclen - 4), 4);
                        for (int i = 0; i < hclen; ++i) hw.put(dy.cllen[PNG_CL_ORDER[i]], 3);
                    }
                    cl_walk(dy.len, hlit, lane, m5, nxt5, [&](int sym, int ev, int eb) {
                        const uint32_t c = dy.clcode[sym];
                        hw.put((c & 0xFFFFu) | ((uint32_t)ev << (c >> 16)), (int)(c >> 16) + eb);
                    });
                    hw.flush();
                }
                const uint32_t off = hdr_bits + before_d + incl_d - bits_d;
                BitWriter bw{outw, 0ull, (int)(off & 31u), (int)(off >> 5)};
                for (uint32_t mm = m; mm;) {
                    const int p = __ffs((int)mm) - 1;
                    mm &= mm - 1;
                    const int q = mm ? p0 + __ffs((int)mm) - 1 : nxt;
                    dyn_emit_run(bw, dy.code, res8[p0 + p], q - (p0 + p));
                }
                if (tid == PNG_THREADS - 1) { const uint32_t c = dy.code[256]; bw.put(c & 0xFFFFu, (int)(c >> 16)); }   // end of block
                bw.flush();
            }
        }
    }
    // pass B: the same walk, emitting. 3 header bits (BFINAL 0, BTYPE 01) come first
    if (!use_dyn) {
        const uint32_t off = 3u + before + incl - bits;
        BitWriter bw{outw, 0ull, (int)(off & 31u), (int)(off >> 5)};
        for (uint32_t mm = m; mm;) {
            const int p = __ffs((int)mm) - 1;
            mm &= mm - 1;
            const int q = mm ? p0 + __ffs((int)mm) - 1 : nxt;
            emit_run(bw, res8[p0 + p], q - (p0 + p));
        }
        bw.flush();
    }
    // end of block (7 zero bits), empty stored block: 3 zero bits, zero bits to the byte boundary, 00 00 FF FF
    const uint32_t total_bits = (use_dyn ? dyn_total : 3u + tok_bits + 7u) + 3u;
    const uint32_t nbytes = min((total_bits + 7u) / 8u + 4u, (uint32_t)PNG_SEG_MAX);           // (the bound holds by construction)
    if (tid == 0) {
        if (!use_dyn) atomicOr(&outw[0], 2u);
        for (uint32_t b = nbytes - 2; b < nbytes; ++b) atomicOr(&outw[b >> 2], 0xFFu << (8 * (b & 3u)));
        unsigned long long t1 = 0, t2 = 0;
        for (int w = 0; w < PNG_WAVES; ++w) { t1 += asum[0][w]; t2 += asum[1][w]; }
        PngSegInfo si;
        si.nbytes = nbytes; si.s1 = (uint32_t)(t1 % ADLER_MOD); si.s2 = (uint32_t)(t2 % ADLER_MOD); si.n = (uint32_t)n;
        info[blockIdx.x] = si;
    }
    __syncthreads();
    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + (int64_t)blockIdx.x * PNG_SLOT);
    const int nwords = (int)((nbytes + 3u) / 4u);
    for (int w = tid; w < nwords; w += PNG_THREADS) slot[w] = outw[w];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kernel 3: one block walks the segments SCAN_THREADS at a time with a carry. Adler-32 of S: with A_k = 1 + sum of the s1 before segment k,
// A = A_nseg and B = sum over k of (n_k * A_k + s2_k), all mod 65521.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(SCAN_THREADS)
void png_scan_kernel(const PngSegInfo* __restrict__ info, int64_t nseg, int64_t* __restrict__ offset, int32_t* __restrict__ ok,
                     uint8_t* __restrict__ out, int64_t capacity, int64_t* __restrict__ out_nbytes) {
    constexpr int NW = SCAN_THREADS / 64;
    __shared__ unsigned long long wl[NW], wa[NW], wb[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry_len = 0, carry_a = 1, sum_b = 0;             // carry_a < 65521 between chunks
    for (int64_t c = 0; c < nseg; c += SCAN_THREADS) {
        const int64_t k = c + tid;
        PngSegInfo si = {0u, 0u, 0u, 0u};
        if (k < nseg) si = info[k];
        const unsigned long long il = wave_incl_scan(si.nbytes, lane), ia = wave_incl_scan(si.s1, lane);
        __syncthreads();                                                    // the previous chunk's reads of wl / wa / wb are done
        if (lane == 63) { wl[wave] = il; wa[wave] = ia; }
        __syncthreads();
        unsigned long long bl = 0, ba = 0, tl = 0, ta = 0;
        for (int w = 0; w < NW; ++w) {
            if (w < wave) { bl += wl[w]; ba += wa[w]; }
            tl += wl[w]; ta += wa[w];
        }
        const unsigned long long a_k = (carry_a + ba + ia - si.s1) % ADLER_MOD;
        unsigned long long term = ((unsigned long long)si.n * a_k + si.s2) % ADLER_MOD;
        if (k < nseg) offset[k] = (int64_t)(carry_len + bl + il - si.nbytes);
        for (int d = 32; d >= 1; d >>= 1) term += __shfl_down(term, d);
        if (lane == 0) wb[wave] = term;
        __syncthreads();
        for (int w = 0; w < NW; ++w) sum_b += wb[w];
        sum_b %= ADLER_MOD;
        carry_len += tl;
        carry_a = (carry_a + ta) % ADLER_MOD;
    }
    if (tid == 0) {
        const int64_t total = 2 + (int64_t)carry_len + 6;
        if (total > capacity) {
            *ok = 0;
            *out_nbytes = -1;
        } else {
            *ok = 1;
            *out_nbytes = total;
            out[0] = 0x78; out[1] = 0x01;
            uint8_t* t = out + 2 + carry_len;
            t[0] = 0x03; t[1] = 0x00;                                       // empty final block in the fixed code
            t[2] = (uint8_t)(sum_b >> 8); t[3] = (uint8_t)sum_b; t[4] = (uint8_t)(carry_a >> 8); t[5] = (uint8_t)carry_a;
        }
    }
}

// kernel 4: one block per segment; the destination is aligned byte-wise, then written in words put together from two source words
__global__ __launch_bounds__(PNG_THREADS)
void png_gather_kernel(const PngSegInfo* __restrict__ info, const int64_t* __restrict__ offset, const int32_t* __restrict__ ok,
                       const uint8_t* __restrict__ slots, uint8_t* __restrict__ out) {
    if (*ok == 0) return;
    const int tid = threadIdx.x;
    const int len = (int)info[blockIdx.x].nbytes;
    const uint8_t* src = slots + (int64_t)blockIdx.x * PNG_SLOT;
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);
    uint8_t* dst = out + 2 + offset[blockIdx.x];
    const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    const int nw = (len - head) / 4;
    if (tid < head) dst[tid] = src[tid];
    uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + head);
    const int sh = 8 * head;
    for (int j = tid; j < nw; j += PNG_THREADS) {
        const uint32_t w0 = src32[j];
        dst32[j] = sh ? (w0 >> sh) | (src32[j + 1] << (32 - sh)) : w0;
    }
    const int tail = head + 4 * nw + tid;
    if (tail < len) dst[tail] = src[tail];
}

static int png_geometry(int H, int W, int channels, int64_t& rowlen, int64_t& N, int64_t& nseg) {
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535) return VPS_EARG(1);
    if (channels != 1 && channels != 3) return VPS_EARG(2);
    rowlen = 1 + (int64_t)W * channels;
    N = (int64_t)H * rowlen;
    nseg = (N + PNG_SEG - 1) / PNG_SEG;
    return 0;
}

// the same for a row given in bytes and a pixel of bpp bytes (1 grey, 3 RGB, 6 RGB with 16-bit samples): Sub reaches back bpp bytes
static int png_geometry_bpp(int H, int64_t rowbytes, int bpp, int64_t& rowlen, int64_t& N, int64_t& nseg) {
    if (bpp != 1 && bpp != 3 && bpp != 6) return VPS_EARG(2);
    if (H <= 0 || H > 65535 || rowbytes <= 0 || rowbytes > (int64_t)65535 * bpp || rowbytes % bpp != 0) return VPS_EARG(1);
    rowlen = 1 + rowbytes;
    N = (int64_t)H * rowlen;
    nseg = (N + PNG_SEG - 1) / PNG_SEG;
    return 0;
}

static int png_bound(int H, int64_t N, int64_t nseg, int64_t* out_capacity, int64_t* ws_bytes) {
    if (!out_capacity || !ws_bytes) return VPS_EARG(3);
    const int64_t last = N - (nseg - 1) * PNG_SEG;
    *out_capacity = 2 + (nseg - 1) * (int64_t)PNG_SEG_MAX + ((9 * last + 7) / 8 + 7) + 6;
    *ws_bytes = png_layout(nullptr, H, nseg).bytes;
    return 0;
}

static int png_deflate_launch(const uint8_t* img, int H, int bpp, int64_t rowlen, int64_t N, int64_t nseg, int64_t row_stride, uint8_t* out,
                              int64_t out_capacity, int64_t* out_nbytes, void* ws, int64_t ws_bytes, int huffman, hipStream_t stream);

}  // namespace

extern "C" int vps_png_encode_bound(int H, int W, int channels, int64_t* out_capacity, int64_t* ws_bytes) {
    int64_t rowlen, N, nseg;
    const int rc = png_geometry(H, W, channels, rowlen, N, nseg);
    if (rc) return rc;
    return png_bound(H, N, nseg, out_capacity, ws_bytes);
}

extern "C" int vps_png_encode_bound_bpp(int H, int64_t rowbytes, int bpp, int64_t* out_capacity, int64_t* ws_bytes) {
    int64_t rowlen, N, nseg;
    const int rc = png_geometry_bpp(H, rowbytes, bpp, rowlen, N, nseg);
    if (rc) return rc;
    return png_bound(H, N, nseg, out_capacity, ws_bytes);
}

extern "C" int vps_png_deflate(const uint8_t* img, int H, int W, int channels, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                               int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream_) {
    int64_t rowlen, N, nseg;
    const int rc = png_geometry(H, W, channels, rowlen, N, nseg);
    if (rc) return rc;
    return png_deflate_launch(img, H, channels, rowlen, N, nseg, row_stride, out, out_capacity, out_nbytes, ws, ws_bytes, 0, (hipStream_t)stream_);
}

extern "C" int vps_png_deflate_h(const uint8_t* img, int H, int W, int channels, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                                 int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream_, int huffman) {
    if (huffman != 0 && huffman != 1) return VPS_EARG(7);
    int64_t rowlen, N, nseg;
    const int rc = png_geometry(H, W, channels, rowlen, N, nseg);
    if (rc) return rc;
    return png_deflate_launch(img, H, channels, rowlen, N, nseg, row_stride, out, out_capacity, out_nbytes, ws, ws_bytes, huffman,
                              (hipStream_t)stream_);
}

extern "C" int vps_png_deflate_bpp(const uint8_t* img, int H, int64_t rowbytes, int bpp, int64_t row_stride, uint8_t* out, int64_t out_capacity,
                                   int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream_) {
    int64_t rowlen, N, nseg;
    const int rc = png_geometry_bpp(H, rowbytes, bpp, rowlen, N, nseg);
    if (rc) return rc;
    return png_deflate_launch(img, H, bpp, rowlen, N, nseg, row_stride, out, out_capacity, out_nbytes, ws, ws_bytes, 0, (hipStream_t)stream_);
}

extern "C" int vps_png_deflate_bpp_h(const uint8_t* img, int H, int64_t rowbytes, int bpp, int64_t row_stride, uint8_t* out,
                                     int64_t out_capacity, int64_t* out_nbytes, void* ws, int64_t ws_bytes, void* stream_, int huffman) {
    if (huffman != 0 && huffman != 1) return VPS_EARG(7);
    int64_t rowlen, N, nseg;
    const int rc = png_geometry_bpp(H, rowbytes, bpp, rowlen, N, nseg);
    if (rc) return rc;
    return png_deflate_launch(img, H, bpp, rowlen, N, nseg, row_stride, out, out_capacity, out_nbytes, ws, ws_bytes, huffman,
                              (hipStream_t)stream_);
}

namespace {

static int png_deflate_launch(const uint8_t* img, int H, int channels, int64_t rowlen, int64_t N, int64_t nseg, int64_t row_stride, uint8_t* out,
                              int64_t out_capacity, int64_t* out_nbytes, void* ws, int64_t ws_bytes, int huffman, hipStream_t stream) {
    if (!img || !out || !out_nbytes || !ws) return VPS_EARG(3);
    if (row_stride < rowlen - 1 || out_capacity < 0) return VPS_EARG(4);
    if (((uintptr_t)ws & 15) || ((uintptr_t)out_nbytes & 7)) return VPS_EARG(5);
    const PngWs w = png_layout(static_cast<uint8_t*>(ws), H, nseg);
    if (ws_bytes < w.bytes) return VPS_EARG(6);
    const int rowbytes = (int)(rowlen - 1);
    const int aligned = (((uintptr_t)img & 3) == 0 && (row_stride & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(png_filter_kernel, dim3(H), dim3(PNG_THREADS), 0, stream, img, rowbytes, channels, row_stride, aligned, w.ftype);
    if (huffman)
        hipLaunchKernelGGL(png_encode_kernel<true>, dim3((unsigned)nseg), dim3(PNG_THREADS), 0, stream, img, H, (int)rowlen, channels,
                           row_stride, N, (const uint8_t*)w.ftype, w.info, w.slots);
    else
        hipLaunchKernelGGL(png_encode_kernel<false>, dim3((unsigned)nseg), dim3(PNG_THREADS), 0, stream, img, H, (int)rowlen, channels,
                           row_stride, N, (const uint8_t*)w.ftype, w.info, w.slots);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, (const PngSegInfo*)w.info, nseg, w.offset, w.ok, out,
                       out_capacity, out_nbytes);
    hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)nseg), dim3(PNG_THREADS), 0, stream, (const PngSegInfo*)w.info,
                       (const int64_t*)w.offset, (const int32_t*)w.ok, (const uint8_t*)w.slots, out);
    return vps_launch_status();
}

}  // namespace
