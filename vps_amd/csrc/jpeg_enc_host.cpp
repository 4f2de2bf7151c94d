// Host half of the JPEG output path (overlay images): the mirror image of jpeg_host.cpp. The device (jpeg_enc_ops.hip) delivers the
// quantised coefficients of a frame in the layout vps_jpeg_decode_coef defines; this file turns them into a baseline JFIF file:
// SOI, APP0, two DQT, SOF0, the four Annex K Huffman tables, SOS, one interleaved scan, EOI - the segments and the bit stream
// libjpeg's default compressor writes for the same tables and coefficients (DC prediction per component, zero runs with ZRL / EOB,
// 0xFF stuffing, the last byte padded with ones). Also here: the quality rule that scales the Annex K quantisation tables
// (vps_jpeg_quant_tables) and the host arithmetic of the sizes (vps_jpeg_encode_bound, vps_jpeg_write_bound).
// Plain C++, no allocation, no global state written after load: any number of threads may write different files at once, and
// called through the C-ABI nothing here holds the interpreter lock. Written from the format's published description (ITU-T T.81,
// JFIF 1.02) and libjpeg's documented quality scaling. Out of scope: restart intervals, optimised tables, progressive, grey.
#include <stdint.h>
#include <string.h>
#include "../../include/vps_hip.h"

#define VPS_EARG(x) (-1000 - (x))

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.1: the example quantisation tables (natural order)
const uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                            69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37, 56,  68,  109, 103, 77, 24, 35, 55,  64,
                            81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 Annex K.3: the typical Huffman tables (codes per length 1..16, then the symbols in code order)
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct EncHuff {                  // encoding form of a table: code and length per symbol (length 0 = the symbol has no code)
    uint16_t code[256];
    uint8_t len[256];
};

void build(const uint8_t* bits, const uint8_t* vals, EncHuff& t) {
    memset(&t, 0, sizeof(t));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            t.code[vals[k]] = (uint16_t)code;
            t.len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

// header bytes: SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 2 x 33 + 2 x 183, SOS 14
constexpr int64_t kHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14;
// a block's worst case: an 11-bit DC category (9-bit code + 11 bits) and 63 coefficients of category 10 (16-bit code + 10 bits) =
// 1658 bits; every byte may be 0xFF and take a stuffed zero
constexpr int64_t kBlockBytesMax = 2 * 208;

struct Geom {
    int hs, vs;                   // luma sampling factors (chroma is 1x1)
    int mcu_rows, mcu_cols;
    int brows[3], bcols[3];
    int64_t nblk;
};

int geometry(int H, int W, int subsampling, Geom& g) {
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535) return VPS_EARG(1);
    if (subsampling == 0) g.hs = g.vs = 1;
    else if (subsampling == 2) g.hs = g.vs = 2;
    else return VPS_EARG(2);
    g.mcu_rows = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.mcu_cols = (W + 8 * g.hs - 1) / (8 * g.hs);
    g.nblk = 0;
    for (int c = 0; c < 3; ++c) {
        g.brows[c] = g.mcu_rows * (c == 0 ? g.vs : 1);
        g.bcols[c] = g.mcu_cols * (c == 0 ? g.hs : 1);
        g.nblk += (int64_t)g.brows[c] * g.bcols[c];
    }
    return 0;
}

struct Out {
    uint8_t* p;
    uint8_t* end;
    uint64_t acc;                 // pending bits, right-aligned
    int cnt;                      // how many (< 8 between calls of put)
    bool full;

    inline void byte(uint32_t b) {
        if (p < end) *p++ = (uint8_t)b;
        else full = true;
    }
    inline void put(uint32_t v, int n) {                                         // n <= 27 bits, the value's high bits first
        acc = (acc << n) | (v & ((1u << n) - 1));
        cnt += n;
        while (cnt >= 8) {
            const uint32_t b = (uint32_t)(acc >> (cnt - 8)) & 255;
            byte(b);
            if (b == 0xFF) byte(0);
            cnt -= 8;
        }
    }
    inline void be16(uint32_t v) { byte(v >> 8); byte(v & 255); }
    inline void bytes(const uint8_t* s, int n) { for (int i = 0; i < n; ++i) byte(s[i]); }
};

inline int category(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

void dht(Out& o, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
    o.be16(0xFFC4); o.be16(2 + 1 + 16 + nvals);
    o.byte(tc_th);
    o.bytes(bits, 16);
    o.bytes(vals, nvals);
}

}  // namespace

extern "C" int vps_jpeg_quant_tables(int quality, uint16_t* qt) {
    if (!qt) return VPS_EARG(1);
    if (quality < 1 || quality > 100) return VPS_EARG(2);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t) {
        const uint8_t* base = t ? kChromaQ : kLumaQ;
        for (int k = 0; k < 64; ++k) {
            long v = ((long)base[k] * scale + 50) / 100;
            qt[64 * t + k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));        // 255: baseline (8-bit) tables forced
        }
    }
    return 0;
}

extern "C" int vps_jpeg_encode_bound(int H, int W, int subsampling, int32_t* grid, int64_t* coef_bytes) {
    Geom g;
    const int st = geometry(H, W, subsampling, g);
    if (st) return st;
    for (int c = 0; c < 3; ++c)
        if (grid) { grid[2 * c] = g.brows[c]; grid[2 * c + 1] = g.bcols[c]; }
    if (coef_bytes) *coef_bytes = g.nblk * 128;
    return 0;
}

extern "C" int vps_jpeg_write_bound(int H, int W, int subsampling, int64_t* capacity) {
    Geom g;
    const int st = geometry(H, W, subsampling, g);
    if (st) return st;
    if (!capacity) return VPS_EARG(3);
    *capacity = kHeaderBytes + g.nblk * kBlockBytesMax + 2 /* the padded last byte, stuffed */ + 2 /* EOI */;
    return 0;
}

extern "C" int vps_jpeg_write(const int16_t* coef, int H, int W, int subsampling, const uint16_t* qt, uint8_t* out, int64_t capacity,
                              int64_t* nbytes) {
    Geom g;
    const int st = geometry(H, W, subsampling, g);
    if (st) return st;
    if (!coef || !qt || !out || !nbytes || capacity < 0) return VPS_EARG(3);
    for (int k = 0; k < 128; ++k)
        if (qt[k] < 1 || qt[k] > 255) return VPS_EARG(4);
    *nbytes = 0;
    Out o;
    o.p = out; o.end = out + capacity; o.acc = 0; o.cnt = 0; o.full = false;
    o.be16(0xFFD8);
    static const uint8_t app0[16] = {0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};   // JFIF 1.01, aspect ratio 1:1, no thumbnail
    o.be16(0xFFE0); o.bytes(app0, 16);
    for (int t = 0; t < 2; ++t) {
        o.be16(0xFFDB); o.be16(67); o.byte(t);
        for (int k = 0; k < 64; ++k) o.byte(qt[64 * t + kZigzag[k]]);
    }
    o.be16(0xFFC0); o.be16(17); o.byte(8); o.be16(H); o.be16(W); o.byte(3);
    o.byte(1); o.byte((g.hs << 4) | g.vs); o.byte(0);
    o.byte(2); o.byte(0x11); o.byte(1);
    o.byte(3); o.byte(0x11); o.byte(1);
    dht(o, 0x00, kDcLumaBits, kDcVals, 12);
    dht(o, 0x10, kAcLumaBits, kAcLumaVals, 162);
    dht(o, 0x01, kDcChromaBits, kDcVals, 12);
    dht(o, 0x11, kAcChromaBits, kAcChromaVals, 162);
    static const uint8_t sos[12] = {0x00, 0x0C, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    o.be16(0xFFDA); o.bytes(sos, 12);
    if (o.full) return VPS_EARG(5);

    EncHuff dc[2], ac[2];
    build(kDcLumaBits, kDcVals, dc[0]);
    build(kDcChromaBits, kDcVals, dc[1]);
    build(kAcLumaBits, kAcLumaVals, ac[0]);
    build(kAcChromaBits, kAcChromaVals, ac[1]);
    const int16_t* plane[3];
    {
        const int16_t* q = coef;
        for (int c = 0; c < 3; ++c) { plane[c] = q; q += (int64_t)g.brows[c] * g.bcols[c] * 64; }
    }
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < g.mcu_rows; ++my) {
        for (int mx = 0; mx < g.mcu_cols; ++mx) {
            for (int c = 0; c < 3; ++c) {
                const int hs = c == 0 ? g.hs : 1, vs = c == 0 ? g.vs : 1;
                const EncHuff& tdc = dc[c ? 1 : 0];
                const EncHuff& tac = ac[c ? 1 : 0];
                for (int v = 0; v < vs; ++v) {
                    for (int u = 0; u < hs; ++u) {
                        const int16_t* blk = plane[c] + (((int64_t)(my * vs + v)) * g.bcols[c] + (mx * hs + u)) * 64;
                        int d = (int)blk[0] - pred[c];
                        pred[c] = blk[0];
                        int bits = d;
                        if (d < 0) { d = -d; --bits; }                           // a negative value is sent as its one's complement
                        int s = category(d);
                        if (s > 11) return VPS_EARG(6);
                        o.put(tdc.code[s], tdc.len[s]);
                        if (s) o.put((uint32_t)bits, s);
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            int a = blk[kZigzag[k]];
                            if (a == 0) { ++run; continue; }
                            while (run > 15) { o.put(tac.code[0xF0], tac.len[0xF0]); run -= 16; }   // ZRL
                            bits = a;
                            if (a < 0) { a = -a; --bits; }
                            s = category(a);
                            if (s > 10) return VPS_EARG(6);                      // not a coefficient of an 8-bit baseline image
                            const int sym = (run << 4) | s;
                            o.put(((uint32_t)tac.code[sym] << s) | ((uint32_t)bits & ((1u << s) - 1)), tac.len[sym] + s);
                            run = 0;
                        }
                        if (run) o.put(tac.code[0x00], tac.len[0x00]);           // EOB
                    }
                }
            }
            if (o.full) return VPS_EARG(5);
        }
    }
    if (o.cnt) o.put(0x7F, 8 - o.cnt);                                           // the last byte is padded with ones
    o.be16(0xFFD9);
    if (o.full) return VPS_EARG(5);
    *nbytes = o.p - out;
    return 0;
}
