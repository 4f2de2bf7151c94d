// Host half of the JPEG output path (overlay images): the mirror image of jpeg_host.cpp. The device (jpeg_enc_ops.hip) delivers the
// quantised coefficients of a frame in the layout vps_jpeg_decode_coef defines; this file turns them into a baseline JFIF file:
// SOI, APP0, two DQT, SOF0, the four Annex K Huffman tables, SOS, one interleaved scan, EOI - the segments and the bit stream
// libjpeg's default compressor writes for the same tables and coefficients (DC prediction per component, zero runs with ZRL / EOB,
// 0xFF stuffing, the last byte padded with ones). Also here: the quality rule that scales the Annex K quantisation tables
// (vps_jpeg_quant_tables) and the host arithmetic of the sizes (vps_jpeg_encode_bound, vps_jpeg_write_bound).
// vps_jpeg_wrap writes the same header and EOI round a scan that was coded elsewhere: on the device, by jpeg_scan_ops.hip.
// Plain C++, no allocation, no global state written after load: any number of threads may write different files at once, and
// called through the C-ABI nothing here holds the interpreter lock. Written from the format's published description (ITU-T T.81,
// JFIF 1.02) and libjpeg's documented quality scaling. Out of scope: restart intervals, optimised tables, progressive, grey.
#include <stdint.h>
#include <string.h>
#include "../../include/vps_hip.h"
#include "jpeg_tables.h"

#define VPS_EARG(x) (-1000 - (x))

namespace {

using namespace vps_jpeg;          // zigzag, Annex K.3 Huffman tables, kHeaderBytes, kBlockBytesMax: shared with jpeg_scan_ops.hip

// T.81 Annex K.1: the example quantisation tables (natural order)
const uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                            69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37, 56,  68,  109, 103, 77, 24, 35, 55,  64,
                            81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

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

// SOI ... SOS: the kHeaderBytes in front of the entropy-coded segment
void header(Out& o, const Geom& g, int H, int W, const uint16_t* qt) {
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
    *capacity = kHeaderBytes + g.nblk * kBlockBytesMax + kScanTailBytes /* the padded last byte, stuffed */ + kTrailerBytes /* EOI */;
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
    header(o, g, H, W, qt);
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

extern "C" int vps_jpeg_wrap(const uint8_t* scan, int64_t scan_bytes, int H, int W, int subsampling, const uint16_t* qt, uint8_t* out,
                             int64_t capacity, int64_t* nbytes) {
    Geom g;
    const int st = geometry(H, W, subsampling, g);
    if (st) return st;
    if (!scan || !qt || !out || !nbytes || capacity < 0 || scan_bytes < 0) return VPS_EARG(3);
    for (int k = 0; k < 128; ++k)
        if (qt[k] < 1 || qt[k] > 255) return VPS_EARG(4);
    *nbytes = 0;
    if (scan_bytes > g.nblk * kBlockBytesMax + kScanTailBytes) return VPS_EARG(6);   // no scan of this geometry is that long
    if (capacity < kHeaderBytes + scan_bytes + kTrailerBytes) return VPS_EARG(5);
    Out o;
    o.p = out; o.end = out + capacity; o.acc = 0; o.cnt = 0; o.full = false;
    header(o, g, H, W, qt);
    memcpy(o.p, scan, (size_t)scan_bytes);
    o.p += scan_bytes;
    o.be16(0xFFD9);
    if (o.full) return VPS_EARG(5);
    *nbytes = o.p - out;
    return 0;
}
