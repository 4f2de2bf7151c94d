"""The warp rule of vps_amd/csrc/warp_rule.h off the device: the header is plain C++, so it is compiled here with a small driver (no GPU,
no HIP) under the address, undefined-behaviour and float-cast-overflow sanitizers and run as a child process; nothing is preloaded. The
driver walks positions at and one ulp around every edge of the in-view interval, and the special values, for small maps and for maps
wider than 2^24, and prints what the header answers. Here that is compared with the rule as the docstrings of vps_amd/tc.py and
vps_amd/flowphoto.py state it, evaluated in NumPy float32, and every index handed out with "in view" must lie on the map. A float that
is converted to an int before the in-view test has passed ends the driver (NaN, inf, 1e30 are in the grid). Built twice: with g++, and
with clang told to fuse multiply-adds, where only the pragma in the header's functions keeps the sample unfused."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vps_amd', 'csrc')
WIDTHS = (1, 2, 5, 64, 16777217, 16777220)               # 16777220: the first W whose float(W - 1) is W itself
F = np.float32

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "warp_rule.h"

static float from_bits(const char* s) { const uint32_t b = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// argv: "grid" W, then lines "x u(bits)" on stdin -> in, x0, x1, wx(bits), nearest, ix per line (the same position on both axes, H = W)
//       "lerp", then lines of six floats as bits -> s(bits)
int main(int argc, char** argv) {
    char a[6][32];
    if (argc == 3 && !strcmp(argv[1], "grid")) {
        const int W = atoi(argv[2]);
        while (scanf("%31s %31s", a[0], a[1]) == 2) {
            const int x = atoi(a[0]);
            const float u = from_bits(a[1]), sx = warp_pos(x, u);
            const bool in = warp_in_view(sx, sx, W, W);
            int ix, iy;
            const bool near = warp_nearest(sx, sx, W, W, ix, iy);
            WarpCorners c = {0, 0, 0, 0, 0.f, 0.f};
            if (in) c = warp_corners(sx, sx, W, W);        // only behind the test, as the kernels call it
            if (c.x0 != c.y0 || c.x1 != c.y1 || bits(c.wx) != bits(c.wy) || ix != iy) return 2;
            printf("%d %d %d %08x %d %d\n", (int)in, c.x0, c.x1, bits(c.wx), (int)near, ix);
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "lerp")) {
        while (scanf("%31s %31s %31s %31s %31s %31s", a[0], a[1], a[2], a[3], a[4], a[5]) == 6)
            printf("%08x\n", bits(warp_lerp2(from_bits(a[0]), from_bits(a[1]), from_bits(a[2]), from_bits(a[3]), from_bits(a[4]), from_bits(a[5]))));
        return 0;
    }
    return 1;
}
'''


def _bits(f):
    return '%08x' % struct.unpack('<I', struct.pack('<f', float(f)))[0]


def _clang():
    c = shutil.which('clang++') or os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin', 'clang++')
    return c if os.path.exists(c) else None


# g++ ignores the header's `#pragma clang fp contract(off)` and has no FMA target here: that build pins the ORDER of the operations only.
# The clang build fuses wherever a pragma does not forbid it (-ffp-contract=fast-honor-pragmas, the HIP compiler's default, and -mfma):
# there the pragma inside warp_lerp2 is what keeps the result unfused, and deleting it fails the lerp2 test.
@pytest.fixture(scope='module', params=['g++', 'clang++ fused'])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp('warp_rule')
    src, exe = d / 'warp_driver.cpp', d / 'warp_driver'
    src.write_text(DRIVER)
    san = ['-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fsanitize=float-cast-overflow', '-fno-sanitize-recover=all',
           '-I', CSRC, str(src), '-o', str(exe)]
    if request.param == 'g++':
        cmd = ['g++', '-Wno-unknown-pragmas', '-ffp-contract=off'] + san
        if subprocess.run(cmd + ['-static-libasan', '-static-libubsan'], capture_output=True).returncode != 0:  # as tests/test_px4_host.py
            subprocess.check_call(cmd)
    else:
        if _clang() is None or ' fma ' not in open('/proc/cpuinfo').read():
            pytest.skip('needs clang++ and a CPU with FMA')
        subprocess.check_call([_clang(), '-ffp-contract=fast-honor-pragmas', '-mfma', '-static-libsan'] + san)

    def run(args, lines):
        r = subprocess.run([str(exe)] + args, input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])       # the sanitizers are silent
        out = r.stdout.split('\n')[:-1]
        assert len(out) == len(lines)
        return out
    return run


def _grid(W):
    """(x, u) whose float32 sum is each wanted position: the edges of the in-view interval and of the map with one ulp either side,
    reached from x = 0, from the last column and from the middle, and the special values"""
    edges = [-0.5, 0.0, float(W - 1), float(W) - 0.5]
    want = []
    for e in edges:
        e = F(e)
        want += [np.nextafter(e, F(-np.inf)), e, np.nextafter(e, F(np.inf))]
    want += [F(0.25), F(0.5), F(W - 1) - F(0.75)]
    pts = []
    for x in sorted({0, W - 1, W // 2}):
        for s in want:
            pts.append((x, F(s) - F(x)))                 # float32: the driver's sum need not be s exactly, the restatement repeats it
    for x in (0, W - 1):
        pts += [(x, F(v)) for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 2147483648.0, -2147483904.0, 4294967296.0)]
    return pts


def _restate(W, x, u):
    """the rule as the module docstrings state it, float32 NumPy -> in, x0, x1, wx, nearest, ix"""
    with np.errstate(invalid='ignore', over='ignore'):
        sx = F(x) + F(u)
        q = np.floor(sx + F(0.5))
        inview = bool(q >= F(0) and q <= F(W - 1))       # compared as floats
        if not inview:
            return False, 0, 0, F(0), False, 0
        x0 = np.floor(sx)
        wx = sx - x0
        x1 = x0 + F(1)
        ix0, ix1 = min(max(int(x0), 0), W - 1), min(max(int(x1), 0), W - 1)
        ix = int(q)
        near = ix < W
        return True, ix0, ix1, F(wx), near, ix


@pytest.mark.parametrize('W', WIDTHS)
def test_in_view_corners_and_nearest_equal_the_float32_restatement_and_stay_on_the_map(driver, W):
    pts = _grid(W)
    out = driver(['grid', str(W)], ['%d %s' % (x, _bits(u)) for x, u in pts])
    seen_in = seen_out = 0
    for (x, u), line in zip(pts, out):
        got_in, x0, x1, wx, near, ix = line.split()
        got = (got_in == '1', int(x0), int(x1), wx, near == '1', int(ix))
        ref = _restate(W, x, u)
        assert got == ref[:3] + (_bits(ref[3]),) + ref[4:], (W, x, float(u), got, ref)
        if got[0]:
            seen_in += 1
            assert 0 <= got[1] <= W - 1 and 0 <= got[2] <= W - 1, (W, x, float(u), got)
        else:
            seen_out += 1
        if got[4]:
            assert got[0] and 0 <= got[5] <= W - 1, (W, x, float(u), got)
    assert seen_in >= 6 and seen_out >= 12
    if W == 16777220:                                    # the guard of the nearest variant has a case: in view as floats, yet off the map
        assert any(line.split()[0] == '1' and line.split()[4] == '0' for line in out)


def _fused(b00, b01, b10, b11, wx, wy):
    """what a fused multiply-add in each of the three steps gives: the product unrounded (float64 holds a float32 product exactly)"""
    def fma(a, w, d):
        return F(np.float64(a) + np.float64(w) * np.float64(d))
    top, bot = fma(b00, wx, F(b01 - b00)), fma(b10, wx, F(b11 - b10))
    return fma(top, wy, F(bot - top))


def _unfused(b00, b01, b10, b11, wx, wy):
    top = F(b00 + F(wx * F(b01 - b00)))
    bot = F(b10 + F(wx * F(b11 - b10)))
    return F(top + F(wy * F(bot - top)))


def test_lerp2_rounds_every_operation_on_its_own(driver):
    # e = 2^-23. top = 1 + 3e, bot = 2 + 4e (a float32: the spacing at 2 is 2e), so bot - top = 1 + e exactly, and wy = 1 + e: the product
    # 1 + 2e + e^2 rounds to 1 + 2e, and top + that is 2 + 5e: exactly between the neighbours 2 + 4e and 2 + 6e, which goes to the even
    # one, 2 + 4e. Fused, the e^2 is still there and tips it to 2 + 6e. The same boundary in top and bot (wx), and with the corners scaled.
    e = F(2.0 ** -23)
    w = F(1) + e
    cases = []
    for k in (F(1), F(4), F(0.5), F(256)):
        top, bot = k * (F(1) + F(3) * e), k * (F(2) + F(4) * e)
        cases.append((top, top, bot, bot, F(0), w))                           # the boundary in the last step
        cases.append((top, bot, top, bot, w, F(0)))                           # ... in top and bot
    cases.append((F(1) + F(3) * e, F(2) + F(4) * e, F(1) + F(3) * e, F(2) + F(4) * e, w, F(0.5)))
    for c in cases:
        assert _bits(_fused(*c)) != _bits(_unfused(*c)), c                      # the cases tell the two apart
    out = driver(['lerp'], [' '.join(_bits(v) for v in c) for c in cases])
    for c, got in zip(cases, out):
        assert got == _bits(_unfused(*c)), (c, got, _bits(_unfused(*c)), _bits(_fused(*c)))
