// Host half of the JPEG input path (the VIPER frames are .jpg files). A baseline JPEG decodes in two parts: the
// Huffman bit stream, which is serial and stays on the host, and dequantisation + 8x8 inverse DCT + chroma upsampling + colour
// conversion, which is per-block / per-pixel integer arithmetic and runs on the device (jpeg_ops.hip). This file is the first
// part: a marker parser (vps_jpeg_info) and an entropy decoder (vps_jpeg_decode_coef) that writes the quantised coefficients
// straight into the caller's staging buffer. Called through the C-ABI both run without the interpreter lock, like png_host.cpp.
// Scope: 8-bit Huffman-coded sequential files (SOF0 / SOF1) with one interleaved scan, 1 or 3 (YCbCr) components, 4:4:4 / 4:2:2
// (h2v1) / 4:2:0 (h2v2); everything else returns VPS_EARG and the caller uses its general decoder. Written from the format's
// published description (ITU-T T.81); no allocation, no global state.
#include <stdint.h>
#include <string.h>
#include "../../include/vps_hip.h"

#define VPS_EARG(x) (-1000 - (x))

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

struct RawHuff {                  // a DHT table as the file states it
    uint8_t bits[17];             // codes of length 1..16
    uint8_t vals[256];
    bool present;
};

struct Header {
    int H, W, nc;
    int hs[3], vs[3], tq[3], td[3], ta[3], id[3];
    int mcu_rows, mcu_cols;
    int brows[3], bcols[3];       // block grid of a component, padded to whole MCUs
    uint16_t qt[4][64];           // natural (row-major) order
    bool have_qt[4];
    RawHuff dc[4], ac[4];
    int restart;                  // MCUs per restart interval, 0 = none
    int64_t scan;                 // offset of the first entropy-coded byte
    int64_t coef_bytes;
};

// EXIF orientation (tag 0x0112 of IFD0) of an APP1 payload that starts with "Exif\0\0"; 1 when the tag is absent
int exif_orientation(const uint8_t* p, int64_t n) {
    if (n < 14) return 1;
    const uint8_t* t = p + 6;
    const int64_t tn = n - 6;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
    auto r16 = [&](int64_t o) -> uint32_t { return le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1]); };
    auto r32 = [&](int64_t o) -> uint32_t { return le ? (r16(o) | (r16(o + 2) << 16)) : ((r16(o) << 16) | r16(o + 2)); };
    if (r16(2) != 42) return 1;
    const int64_t ifd = r32(4);
    if (ifd + 2 > tn) return 1;
    const int cnt = (int)r16(ifd);
    for (int i = 0; i < cnt; ++i) {
        const int64_t e = ifd + 2 + 12 * (int64_t)i;
        if (e + 12 > tn) break;
        if (r16(e) == 0x0112) return (int)r16(e + 8);
    }
    return 1;
}

// markers up to and including SOS; 0 or the argument error that names what this path does not take
int parse(const uint8_t* f, int64_t n, Header& h) {
    memset(&h, 0, sizeof(h));
    if (!f || n < 4 || f[0] != 0xFF || f[1] != 0xD8) return VPS_EARG(1);
    int64_t pos = 2;
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    for (;;) {
        if (pos + 2 > n || f[pos] != 0xFF) return VPS_EARG(2);                 // truncated / not at a marker
        while (pos < n && f[pos] == 0xFF) ++pos;                                 // fill bytes
        if (pos >= n) return VPS_EARG(2);
        const int m = f[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                     // stand-alone markers
        if (m == 0xD9 || m == 0xD8 || m == 0x00) return VPS_EARG(2);            // EOI before a scan / stray data
        if (pos + 2 > n) return VPS_EARG(2);
        const int64_t L = be16(f + pos);
        if (L < 2 || pos + L > n) return VPS_EARG(2);
        const uint8_t* s = f + pos + 2;
        const int64_t sn = L - 2;
        if (m == 0xC0 || m == 0xC1) {                                            // baseline / extended sequential, Huffman
            if (sof || sn < 6) return VPS_EARG(2);
            if (s[0] != 8) return VPS_EARG(3);                                   // 12-bit samples
            h.H = (int)be16(s + 1); h.W = (int)be16(s + 3); h.nc = s[5];
            if (h.H == 0 || h.W == 0) return VPS_EARG(3);                        // height by DNL marker
            if (h.nc != 1 && h.nc != 3) return VPS_EARG(4);                      // CMYK / YCCK / two components
            if (sn < 6 + 3 * h.nc) return VPS_EARG(2);
            for (int c = 0; c < h.nc; ++c) {
                h.id[c] = s[6 + 3 * c];
                h.hs[c] = s[7 + 3 * c] >> 4; h.vs[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
                if (h.tq[c] > 3 || h.hs[c] < 1 || h.vs[c] < 1) return VPS_EARG(2);
            }
            sof = true;
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4) {                      // progressive, lossless, differential, arithmetic (DAC too)
            return VPS_EARG(3);
        } else if (m == 0xC4) {                                                  // DHT: any number of tables, later ones replace earlier ones
            int64_t o = 0;
            while (o < sn) {
                if (o + 17 > sn) return VPS_EARG(2);
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return VPS_EARG(2);
                RawHuff& t = tc ? h.ac[th] : h.dc[th];
                int total = 0;
                t.bits[0] = 0;
                for (int i = 1; i <= 16; ++i) { t.bits[i] = s[o + i]; total += s[o + i]; }
                if (total > 256 || o + 17 + total > sn) return VPS_EARG(2);
                memcpy(t.vals, s + o + 17, total);
                t.present = true;
                o += 17 + total;
            }
        } else if (m == 0xDB) {                                                  // DQT
            int64_t o = 0;
            while (o < sn) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > sn) return VPS_EARG(2);
                for (int k = 0; k < 64; ++k)
                    h.qt[tq][kZigzag[k]] = pq ? (uint16_t)be16(s + o + 1 + 2 * k) : s[o + 1 + k];
                h.have_qt[tq] = true;
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {                                                  // DRI
            if (sn < 2) return VPS_EARG(2);
            h.restart = (int)be16(s);
        } else if (m == 0xE0) {
            if (sn >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xE1) {
            if (sn >= 6 && memcmp(s, "Exif\0\0", 6) == 0 && exif_orientation(s, sn) != 1) return VPS_EARG(6);   // cv2.imread rotates, PIL does not
        } else if (m == 0xEE) {
            if (sn >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {                                                  // SOS
            if (!sof || sn < 1) return VPS_EARG(2);
            const int ns = s[0];
            if (ns != h.nc) return VPS_EARG(5);                                  // one scan per component: not taken
            if (sn < 1 + 2 * ns + 3) return VPS_EARG(2);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.id[c]) return VPS_EARG(5);
                h.td[c] = s[2 + 2 * c] >> 4; h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3 || !h.dc[h.td[c]].present || !h.ac[h.ta[c]].present || !h.have_qt[h.tq[c]]) return VPS_EARG(2);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return VPS_EARG(3);
            h.scan = pos + L;
            break;
        }
        pos += L;
    }
    // colour space: three components are YCbCr unless an Adobe segment says otherwise or, without JFIF / Adobe, the ids spell RGB
    if (h.nc == 3) {
        if (adobe && adobe_transform != 1) return VPS_EARG(4);
        if (!adobe && !jfif && h.id[0] == 'R' && h.id[1] == 'G' && h.id[2] == 'B') return VPS_EARG(4);
        const bool chroma11 = h.hs[1] == 1 && h.vs[1] == 1 && h.hs[2] == 1 && h.vs[2] == 1;
        const bool luma_ok = (h.hs[0] == 1 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 1) || (h.hs[0] == 2 && h.vs[0] == 2);
        if (!chroma11 || !luma_ok) return VPS_EARG(5);
    } else {
        h.hs[0] = h.vs[0] = 1;                                                   // a single component is never interleaved: its MCU is one block
    }
    const int mw = 8 * h.hs[0], mh = 8 * h.vs[0];
    h.mcu_cols = (h.W + mw - 1) / mw;
    h.mcu_rows = (h.H + mh - 1) / mh;
    h.coef_bytes = 0;
    for (int c = 0; c < h.nc; ++c) {
        h.brows[c] = h.mcu_rows * h.vs[c];
        h.bcols[c] = h.mcu_cols * h.hs[c];
        h.coef_bytes += (int64_t)h.brows[c] * h.bcols[c] * 128;
    }
    return 0;
}

// the entropy-coded segment must end in an EOI marker (RSTn and stuffed 0xFF00 pass): a file cut short mid-scan is refused
bool scan_reaches_eoi(const uint8_t* f, int64_t n, int64_t pos) {
    while (pos < n) {
        const uint8_t* q = (const uint8_t*)memchr(f + pos, 0xFF, (size_t)(n - pos));
        if (!q) return false;
        pos = (q - f) + 1;
        while (pos < n && f[pos] == 0xFF) ++pos;
        if (pos >= n) return false;
        const int m = f[pos++];
        if (m == 0xD9) return true;
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) continue;
        return false;                                                            // any other marker inside the scan: a second scan, DNL, damage
    }
    return false;
}

struct Huff {                     // decoding form of a table: 9-bit lookup + the standard's maxcode / valptr walk for longer codes
    uint16_t fast[512];           // (length << 8) | symbol, 0 = longer than 9 bits
    int32_t maxcode[18];
    int32_t valoff[17];
    const uint8_t* vals;
};

bool build(const RawHuff& r, Huff& t) {
    memset(t.fast, 0, sizeof(t.fast));
    t.vals = r.vals;
    int32_t code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.valoff[len] = k - code;
        for (int i = 0; i < r.bits[len]; ++i, ++k, ++code) {
            if (len <= 9) {
                const int lo = code << (9 - len), cnt = 1 << (9 - len);
                if (lo + cnt > 512) return false;
                for (int j = 0; j < cnt; ++j) t.fast[lo + j] = (uint16_t)((len << 8) | r.vals[k]);
            }
        }
        if (code > (1 << len)) return false;                                     // more codes than the length admits
        t.maxcode[len] = r.bits[len] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
    return true;
}

struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;                 // next bit = bit 63
    int cnt;                      // valid bits in buf
    int fake;                     // zero bits appended at a marker / the end of the data (the LAST `fake` bits of buf)

    inline void refill() {
        if (cnt <= 32 && end - p >= 4) {
            uint32_t v;
            memcpy(&v, p, 4);
            if (!((~v - 0x01010101u) & v & 0x80808080u)) {                       // no 0xFF among the four bytes (zero-byte test on ~v)
                buf |= (uint64_t)__builtin_bswap32(v) << (32 - cnt);
                cnt += 32;
                p += 4;
                return;
            }
        }
        while (cnt <= 56) {
            uint32_t b = 0;
            if (p < end && *p != 0xFF) {
                b = *p++;
            } else if (p + 1 < end && p[1] == 0x00) {                            // stuffed 0xFF
                b = 0xFF;
                p += 2;
            } else {                                                             // a marker (or the end): the decoder sees zeros from here
                fake += 8;
            }
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    inline void drop(int nb) { buf <<= nb; cnt -= nb; }
    inline bool overran() const { return fake > cnt; }
};

inline int decode_sym(Bits& b, const Huff& t) {
    const uint32_t e = t.fast[b.buf >> 55];
    if (e) {
        b.drop((int)(e >> 8));
        return (int)(e & 255);
    }
    int len = 10;
    int32_t code = (int32_t)(b.buf >> 54);
    while (code > t.maxcode[len]) {
        ++len;
        code = (int32_t)(b.buf >> (64 - len));
    }
    if (len > 16) return -1;
    b.drop(len);
    return t.vals[(code + t.valoff[len]) & 255];
}

inline int receive_extend(Bits& b, int s) {
    const int v = (int)(b.buf >> (64 - s));
    b.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

extern "C" int vps_jpeg_info(const uint8_t* file, int64_t nbytes, int32_t* H, int32_t* W, int32_t* ncomp, int32_t* samp, int32_t* grid,
                             uint16_t* qt, int64_t* coef_bytes) {
    Header h;
    const int st = parse(file, nbytes, h);
    if (st) return st;
    if (!scan_reaches_eoi(file, nbytes, h.scan)) return VPS_EARG(7);
    if (H) *H = h.H;
    if (W) *W = h.W;
    if (ncomp) *ncomp = h.nc;
    for (int c = 0; c < 3; ++c) {
        const int k = c < h.nc ? c : 0;                                          // a grey file repeats its one component
        if (samp) { samp[2 * c] = h.hs[k]; samp[2 * c + 1] = h.vs[k]; }
        if (grid) { grid[2 * c] = h.brows[k]; grid[2 * c + 1] = h.bcols[k]; }
        if (qt) memcpy(qt + 64 * c, h.qt[h.tq[k]], 128);
    }
    if (coef_bytes) *coef_bytes = h.coef_bytes;
    return 0;
}

extern "C" int vps_jpeg_decode_coef(const uint8_t* file, int64_t nbytes, int16_t* coef, int64_t capacity) {
    Header h;
    const int st = parse(file, nbytes, h);
    if (st) return st;
    if (!coef || capacity < h.coef_bytes) return VPS_EARG(8);
    Huff dc[3], ac[3];
    for (int c = 0; c < h.nc; ++c)
        if (!build(h.dc[h.td[c]], dc[c]) || !build(h.ac[h.ta[c]], ac[c])) return VPS_EARG(9);
    int16_t* plane[3];
    {
        int16_t* q = coef;
        for (int c = 0; c < h.nc; ++c) { plane[c] = q; q += (int64_t)h.brows[c] * h.bcols[c] * 64; }
    }
    Bits b;
    b.p = file + h.scan; b.end = file + nbytes; b.buf = 0; b.cnt = 0; b.fake = 0;
    int pred[3] = {0, 0, 0};
    int to_restart = h.restart, next_rst = 0;
    for (int my = 0; my < h.mcu_rows; ++my) {
        for (int mx = 0; mx < h.mcu_cols; ++mx) {
            if (h.restart && to_restart == 0) {
                // the interval's last byte is padded with 1-bits; then fill bytes and RSTn. Anything else is damage.
                if (b.overran() || b.cnt - b.fake >= 8) return VPS_EARG(10);
                const uint8_t* p = b.p;
                if (p >= b.end || *p != 0xFF) return VPS_EARG(10);
                while (p < b.end && *p == 0xFF) ++p;
                if (p >= b.end || *p != 0xD0 + next_rst) return VPS_EARG(10);
                b.p = p + 1; b.buf = 0; b.cnt = 0; b.fake = 0;
                next_rst = (next_rst + 1) & 7;
                to_restart = h.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < h.nc; ++c) {
                const Huff& tdc = dc[c];
                const Huff& tac = ac[c];
                for (int v = 0; v < h.vs[c]; ++v) {
                    for (int u = 0; u < h.hs[c]; ++u) {
                        int16_t* blk = plane[c] + (((int64_t)(my * h.vs[c] + v)) * h.bcols[c] + (mx * h.hs[c] + u)) * 64;
                        memset(blk, 0, 128);
                        if (b.cnt < 32) b.refill();
                        int s = decode_sym(b, tdc);
                        if (s < 0 || s > 15) return VPS_EARG(10);
                        if (s) pred[c] += receive_extend(b, s);
                        blk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            if (b.cnt < 32) b.refill();
                            const int rs = decode_sym(b, tac);
                            if (rs < 0) return VPS_EARG(10);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;                              // EOB
                                k += 16;                                         // ZRL
                                continue;
                            }
                            k += r;
                            if (k > 63) return VPS_EARG(10);
                            blk[kZigzag[k]] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                    }
                }
            }
            if (b.overran()) return VPS_EARG(10);                                // the decoder ran into a marker or off the end of the file
            if (h.restart) --to_restart;
        }
    }
    return 0;
}
