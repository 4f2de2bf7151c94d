// "prev at p + flow(p)": the ONE implementation of the warp rule that include/vps_hip.h defines (tc_ops.hip, flow_occ_ops.hip,
// flow_photo_ops.hip, pass 1 of flow_census_ops.hip). What is read at the corners stays with the caller. fp32, every operation rounded
// on its own: a function that multiplies and adds switches contraction off in its own body, whatever the including file does. A float
// becomes an int only behind an in-view test that compared it AS A FLOAT, so NaN, +-inf and 1e30 never reach a conversion. No HIP
// builtins: tests/test_warp_rule_host.py runs the header as plain C++ under the host sanitizers against NumPy.
#pragma once
#include <math.h>
#include <stdint.h>
#ifdef __HIPCC__
#define WARP_FN __device__ __forceinline__
#else
#define WARP_FN static inline
#endif

WARP_FN float warp_pos(int x, float u) { return (float)x + u; }

WARP_FN bool warp_in_floats(float sx, float sy, int W, int H, float& qx, float& qy) {
    qx = floorf(sx + 0.5f); qy = floorf(sy + 0.5f);
    return qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1);
}

// for the callers that go on to warp_corners, which clamps every index after its conversion: no guard beyond the float comparison
WARP_FN bool warp_in_view(float sx, float sy, int W, int H) {
    float qx, qy;
    return warp_in_floats(sx, sy, W, H, qx, qy);
}

// nearest pixel, (int)qx unclamped: (float)(W - 1) is W itself for some W above 2^24 (the first is 16777220), so the float comparison
// lets qx == W through and the integer comparison keeps such a pixel off the map
WARP_FN bool warp_nearest(float sx, float sy, int W, int H, int& ix, int& iy) {
    float qx, qy;
    ix = iy = 0;
    if (!warp_in_floats(sx, sy, W, H, qx, qy)) return false;
    ix = (int)qx; iy = (int)qy;
    return ix < W && iy < H;
}

struct WarpCorners { int x0, x1, y0, y1; float wx, wy; };

WARP_FN int warp_clamp(float f, int n) {
    const int i = (int)f, lo = i > 0 ? i : 0;
    return lo < n - 1 ? lo : n - 1;
}

// of an IN-VIEW position; a clamped corner keeps its weight
WARP_FN WarpCorners warp_corners(float sx, float sy, int W, int H) {
#pragma clang fp contract(off)
    const float x0 = floorf(sx), y0 = floorf(sy);
    return {warp_clamp(x0, W), warp_clamp(x0 + 1.f, W), warp_clamp(y0, H), warp_clamp(y0 + 1.f, H), sx - x0, sy - y0};
}

// b00 (y0, x0), b01 (y0, x1), b10 (y1, x0), b11 (y1, x1): top, bot, then s
WARP_FN float warp_lerp2(float b00, float b01, float b10, float b11, float wx, float wy) {
#pragma clang fp contract(off)
    const float top = b00 + wx * (b01 - b00), bot = b10 + wx * (b11 - b10);
    return top + wy * (bot - top);
}
