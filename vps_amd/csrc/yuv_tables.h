// The one table of colour coefficients the two kernels of yuv_ops.hip share (as jpeg_tables.h is shared): YCbCr <-> RGB for
// (matrix, range), integers with 16 fractional bits, round(65536 * c), c derived here from the matrix's (Kr, Kb) and the range's
// scales at compile time. A kernel gets its row by value; tests/y4m_restate.py derives the same integers on its own in float64.
//   decode:  R = ky (Y - yoff) + cr_r (Cr - 128)                        G = ky (Y - yoff) + cb_g (Cb - 128) + cr_g (Cr - 128)
//            B = ky (Y - yoff) + cb_b (Cb - 128)
//   encode:  Y = yoff + y . (R, G, B)     Cb = 128 + cb . (R, G, B)     Cr = 128 + cr . (R, G, B)
// every result (sum + 32768) >> 16 with the integer offsets inside the sum, then clamped (decode 0..255; encode lo..yhi / lo..chi).
#pragma once
#include <stdint.h>

namespace vps_yuv {

struct Coef {
    int32_t yoff;                            // 16 limited, 0 full
    int32_t ky, cr_r, cb_g, cr_g, cb_b;      // decode
    int32_t y[3], cb[3], cr[3];              // encode, each in R, G, B order
    int32_t lo, yhi, chi;                    // encode clamps: 16, 235, 240 limited; 0, 255, 255 full
};

constexpr int32_t q16(double c) {            // round(65536 c), halves away from zero (no coefficient sits on one)
    return c >= 0 ? (int32_t)(c * 65536.0 + 0.5) : -(int32_t)(-c * 65536.0 + 0.5);
}

constexpr Coef make(double kr, double kb, bool full) {
    const double kg = 1.0 - kr - kb;
    const double ys = full ? 1.0 : 219.0 / 255.0;      // luma levels per unit of R'G'B' / 255
    const double cs = full ? 1.0 : 224.0 / 255.0;      // chroma levels
    return Coef{full ? 0 : 16,
                q16(1.0 / ys), q16(2.0 * (1.0 - kr) / cs), q16(-2.0 * kb * (1.0 - kb) / kg / cs), q16(-2.0 * kr * (1.0 - kr) / kg / cs),
                q16(2.0 * (1.0 - kb) / cs),
                {q16(kr * ys), q16(kg * ys), q16(kb * ys)},
                {q16(-kr / (2.0 * (1.0 - kb)) * cs), q16(-kg / (2.0 * (1.0 - kb)) * cs), q16(0.5 * cs)},
                {q16(0.5 * cs), q16(-kg / (2.0 * (1.0 - kr)) * cs), q16(-kb / (2.0 * (1.0 - kr)) * cs)},
                full ? 0 : 16, full ? 255 : 235, full ? 255 : 240};
}

// [matrix: VPS_YUV_BT601, VPS_YUV_BT709][range: VPS_YUV_LIMITED, VPS_YUV_FULL]
constexpr Coef kTable[2][2] = {{make(0.299, 0.114, false), make(0.299, 0.114, true)},
                               {make(0.2126, 0.0722, false), make(0.2126, 0.0722, true)}};

}  // namespace vps_yuv
