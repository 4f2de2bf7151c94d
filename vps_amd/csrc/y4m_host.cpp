// YUV4MPEG2 (.y4m) container: the two header lines, parsed from untrusted bytes, and the stream header written back (vps_amd/y4m.py).
// Host-only, no allocation, no exceptions, no read past the length given; the frames themselves are raw planes that go to the device
// as they lie in the file (csrc/yuv_ops.hip). include/vps_hip.h has the grammar and the refusal codes.
#include <stdint.h>
#include <string.h>

#include "../../include/vps_hip.h"

#define VPS_EARG(x) (-1000 - (x))

namespace {

constexpr int HEADER_MAX = 256;
constexpr int FRAME_MAX = 80;
const char MAGIC[] = "YUV4MPEG2 ";
constexpr int MAGIC_LEN = 10;

// decimal number in [p, e), optional leading '-': false when empty or not a number; a value beyond 10^18 is reported as 10^18
bool number(const uint8_t* p, const uint8_t* e, int64_t* v) {
    bool neg = false;
    if (p < e && *p == '-') { neg = true; ++p; }
    if (p >= e) return false;
    constexpr int64_t BIG = 1000000000000000000LL;
    int64_t a = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        a = a >= BIG / 10 ? BIG : a * 10 + (*p - '0');
    }
    *v = neg ? -a : a;
    return true;
}

// "num:den", both non-negative and within int32
bool ratio(const uint8_t* p, const uint8_t* e, int32_t* num, int32_t* den) {
    const uint8_t* c = p;
    while (c < e && *c != ':') ++c;
    int64_t a, b;
    if (c >= e || !number(p, c, &a) || !number(c + 1, e, &b)) return false;
    if (a < 0 || b < 0 || a > INT32_MAX || b > INT32_MAX) return false;
    *num = (int32_t)a;
    *den = (int32_t)b;
    return true;
}

bool is(const uint8_t* p, const uint8_t* e, const char* s) {
    const size_t n = strlen(s);
    return (size_t)(e - p) == n && memcmp(p, s, n) == 0;
}

bool ends_with(const uint8_t* p, const uint8_t* e, const char* s) {
    const size_t n = strlen(s);
    return (size_t)(e - p) >= n && memcmp(e - n, s, n) == 0;
}

int colourspace(const uint8_t* p, const uint8_t* e, int32_t* sampling) {
    if (is(p, e, "420jpeg") || is(p, e, "420")) { *sampling = VPS_Y4M_420JPEG; return 0; }
    if (is(p, e, "420mpeg2")) { *sampling = VPS_Y4M_420MPEG2; return 0; }
    if (is(p, e, "422")) { *sampling = VPS_Y4M_422; return 0; }
    if (is(p, e, "444")) { *sampling = VPS_Y4M_444; return 0; }
    if (is(p, e, "mono")) { *sampling = VPS_Y4M_MONO; return 0; }
    if (is(p, e, "420paldv")) return VPS_EARG(9);
    if (is(p, e, "444alpha")) return VPS_EARG(11);
    static const char* const deep[] = {"p9", "p10", "p12", "p14", "p16", "mono9", "mono10", "mono12", "mono14", "mono16"};
    for (const char* d : deep)
        if (ends_with(p, e, d)) return VPS_EARG(10);
    return VPS_EARG(12);
}

void plane_sizes(vps_y4m_desc* d) {
    const int32_t hw = (d->W + 1) / 2, hh = (d->H + 1) / 2;
    switch (d->sampling) {
        case VPS_Y4M_420JPEG:
        case VPS_Y4M_420MPEG2: d->CW = hw; d->CH = hh; break;
        case VPS_Y4M_422: d->CW = hw; d->CH = d->H; break;
        case VPS_Y4M_444: d->CW = d->W; d->CH = d->H; break;
        default: d->CW = 0; d->CH = 0; break;
    }
    d->frame_bytes = (int64_t)d->W * d->H + 2 * (int64_t)d->CW * d->CH;
}

// length of the line that starts at buf, newline included; 0 when there is none within min(n, cap) bytes
int line_length(const uint8_t* buf, int64_t n, int cap) {
    const int lim = (int)(n < cap ? n : cap);
    for (int i = 0; i < lim; ++i)
        if (buf[i] == '\n') return i + 1;
    return 0;
}

int put(uint8_t* out, int cap, int pos, const char* s) {
    for (; *s; ++s, ++pos)
        if (pos < cap) out[pos] = (uint8_t)*s;
    return pos;
}

int put_number(uint8_t* out, int cap, int pos, int32_t v) {
    char tmp[12];
    int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) {
        if (pos < cap) out[pos] = (uint8_t)tmp[k - 1];
        --k; ++pos;
    }
    return pos;
}

}  // namespace

extern "C" int vps_y4m_info(const uint8_t* buf, int64_t nbytes, vps_y4m_desc* info) {
    if (!buf || !info || nbytes < 0) return VPS_EARG(1);
    const int have = (int)(nbytes < MAGIC_LEN ? nbytes : MAGIC_LEN);
    if (memcmp(buf, MAGIC, have) != 0) return VPS_EARG(2);
    if (have < MAGIC_LEN) return VPS_EARG(3);
    const int len = line_length(buf, nbytes, HEADER_MAX);
    if (!len) return VPS_EARG(3);
    vps_y4m_desc d;
    memset(&d, 0, sizeof(d));
    d.sampling = VPS_Y4M_420JPEG;
    d.range = VPS_YUV_LIMITED;
    d.header_bytes = len;
    bool have_w = false, have_h = false;
    const uint8_t* p = buf + MAGIC_LEN;
    const uint8_t* end = buf + len - 1;                       // the newline
    while (p < end) {
        if (*p == ' ') { ++p; continue; }
        const uint8_t* e = p;
        while (e < end && *e != ' ') ++e;
        const uint8_t tag = *p;
        const uint8_t* v = p + 1;
        if (tag == 'W' || tag == 'H') {
            int64_t a;
            if (!number(v, e, &a)) return VPS_EARG(4);
            if (a <= 0) return VPS_EARG(6);
            if (a > INT32_MAX) return VPS_EARG(7);
            if (tag == 'W') { d.W = (int32_t)a; have_w = true; } else { d.H = (int32_t)a; have_h = true; }
        } else if (tag == 'F') {
            if (!ratio(v, e, &d.fps_num, &d.fps_den)) return VPS_EARG(4);
        } else if (tag == 'A') {
            if (!ratio(v, e, &d.aspect_num, &d.aspect_den)) return VPS_EARG(4);
        } else if (tag == 'I') {
            if (is(v, e, "p")) d.interlace = 1;
            else if (is(v, e, "?")) d.interlace = 0;
            else if (is(v, e, "t") || is(v, e, "b") || is(v, e, "m")) return VPS_EARG(8);
            else return VPS_EARG(14);
        } else if (tag == 'C') {
            const int st = colourspace(v, e, &d.sampling);
            if (st) return st;
        } else if (tag == 'X') {
            const char key[] = "COLORRANGE=";
            const size_t kl = sizeof(key) - 1;
            if ((size_t)(e - v) >= kl && memcmp(v, key, kl) == 0) {
                if (is(v + kl, e, "FULL")) d.range = VPS_YUV_FULL;
                else if (is(v + kl, e, "LIMITED")) d.range = VPS_YUV_LIMITED;
                else return VPS_EARG(13);
            }
        }                                                     // any other tag: ignored
        p = e;
    }
    if (!have_w || !have_h) return VPS_EARG(5);
    if ((int64_t)d.W * d.H > INT32_MAX) return VPS_EARG(7);
    plane_sizes(&d);
    *info = d;
    return 0;
}

extern "C" int vps_y4m_frame_header(const uint8_t* buf, int64_t nbytes, int32_t* len) {
    if (!buf || !len || nbytes < 0) return VPS_EARG(1);
    const int have = (int)(nbytes < 5 ? nbytes : 5);
    if (memcmp(buf, "FRAME", have) != 0) return VPS_EARG(20);
    if (have < 5 || nbytes < 6) return VPS_EARG(21);
    if (buf[5] != '\n' && buf[5] != ' ') return VPS_EARG(20);
    const int n = line_length(buf, nbytes, FRAME_MAX);
    if (!n) return VPS_EARG(21);
    *len = n;
    return 0;
}

extern "C" int vps_y4m_write_header(const vps_y4m_desc* info, uint8_t* out, int64_t capacity, int32_t* len) {
    if (!info || !out || !len || capacity < 0) return VPS_EARG(1);
    const vps_y4m_desc& d = *info;
    if (d.W <= 0 || d.H <= 0 || (int64_t)d.W * d.H > INT32_MAX || d.sampling < VPS_Y4M_420JPEG || d.sampling > VPS_Y4M_MONO ||
        (d.range != VPS_YUV_LIMITED && d.range != VPS_YUV_FULL) || d.fps_num < 0 || d.fps_den < 0 || d.aspect_num < 0 ||
        d.aspect_den < 0 || (d.interlace != 0 && d.interlace != 1))
        return VPS_EARG(30);
    static const char* const names[] = {"420jpeg", "420mpeg2", "422", "444", "mono"};
    uint8_t line[HEADER_MAX];
    int pos = put(line, HEADER_MAX, 0, "YUV4MPEG2 W");
    pos = put_number(line, HEADER_MAX, pos, d.W);
    pos = put(line, HEADER_MAX, pos, " H");
    pos = put_number(line, HEADER_MAX, pos, d.H);
    if (d.fps_num || d.fps_den) {
        pos = put(line, HEADER_MAX, pos, " F");
        pos = put_number(line, HEADER_MAX, pos, d.fps_num);
        pos = put(line, HEADER_MAX, pos, ":");
        pos = put_number(line, HEADER_MAX, pos, d.fps_den);
    }
    if (d.interlace) pos = put(line, HEADER_MAX, pos, " Ip");
    pos = put(line, HEADER_MAX, pos, " A");
    pos = put_number(line, HEADER_MAX, pos, d.aspect_num);
    pos = put(line, HEADER_MAX, pos, ":");
    pos = put_number(line, HEADER_MAX, pos, d.aspect_den);
    pos = put(line, HEADER_MAX, pos, " C");
    pos = put(line, HEADER_MAX, pos, names[d.sampling]);
    pos = put(line, HEADER_MAX, pos, d.range == VPS_YUV_FULL ? " XCOLORRANGE=FULL\n" : " XCOLORRANGE=LIMITED\n");
    if (pos > HEADER_MAX) return VPS_EARG(30);                // cannot happen with int32 fields (at most 109 bytes)
    if (pos > capacity) return VPS_EARG(31);
    memcpy(out, line, pos);
    *len = pos;
    return 0;
}
