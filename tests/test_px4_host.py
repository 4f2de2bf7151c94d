"""The loads, stores and the search of vps_amd/csrc/px4.h off the device: Part A of the header is plain C++, so it is compiled here with
a small driver (no GPU, no HIP) under the address and undefined-behaviour sanitizers and run as a child process. Every map ends at the
last byte of a heap block of exactly its size and every wide load is checked for its alignment, so a chunk that reads past the end
of a map, or loads a dword, a pair or a quad off its boundary, ends the driver with an error. (A read of the 1-3 bytes in FRONT of an
unaligned base stays inside the block and is not seen here: the condition of the fast paths is the one the kernels had.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vps_amd', 'csrc')

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "px4.h"

static long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { printf("line %d: %s (o %d npix %ld)\n", __LINE__, #c, o, npix); return 1; } } while (0)

// a block of exactly `front + bytes` bytes (malloc: 16-byte aligned), the payload behind `front` bytes of 0xEE
struct Block {
    uint8_t* raw; uint8_t* p;
    Block(size_t front, size_t bytes) : raw((uint8_t*)malloc(front + bytes)), p(raw + front) { memset(raw, 0xEE, front + bytes); }
    ~Block() { free(raw); }
};
static uint32_t rnd() { static uint32_t s = 12345; s = s * 1664525u + 1013904223u; return s >> 8; }

static int sweep(int o, long npix) {
    const long nchunk = (npix + PX4 - 1) / PX4;
    // ---- [npix][3] and [npix] byte maps at byte offset o
    Block m3(o, 3 * npix), m1(o, npix);
    for (long i = 0; i < 3 * npix; ++i) m3.p[i] = (uint8_t)rnd();
    for (long i = 0; i < npix; ++i) m1.p[i] = (uint8_t)rnd();
    for (long ch = 0; ch < nchunk; ++ch) {
        const long p0 = PX4 * ch;
        const int n = (int)(npix - p0 < PX4 ? npix - p0 : PX4);
        uint32_t px[PX4];
        px4_load_px3(m3.p, 3 * npix, ch, n, px);
        const uint32_t b = px4_load_bytes(m1.p, npix, p0, n);
        for (int i = 0; i < PX4; ++i) {
            const uint8_t* a = m3.p + 3 * (p0 + i);
            CHECK(px[i] == (i < n ? (uint32_t)(a[0] | a[1] << 8 | a[2] << 16) : 0u));
            CHECK(((b >> (8 * i)) & 0xffu) == (i < n ? m1.p[p0 + i] : 0u));
        }
    }
    // ---- the stores, into blocks of exactly the map's size: bytes when dst4 is false, dwords where the caller may say true
    for (int dst4 = 0; dst4 <= (o == 0); ++dst4) {
        Block d1(o, npix), d3(o, 3 * npix);
        for (long ch = 0; ch < nchunk; ++ch) {
            const long p0 = PX4 * ch;
            const int n = (int)(npix - p0 < PX4 ? npix - p0 : PX4);
            uint32_t px[PX4];
            px4_load_px3(m3.p, 3 * npix, ch, n, px);
            px4_store_px3(d3.p, dst4 != 0, p0, n, px);
            px4_store_bytes(d1.p, dst4 != 0, p0, n, px4_load_bytes(m1.p, npix, p0, n));
        }
        CHECK(memcmp(d1.p, m1.p, npix) == 0 && memcmp(d3.p, m3.p, 3 * npix) == 0);
        for (int i = 0; i < o; ++i) CHECK(d1.raw[i] == 0xEE && d3.raw[i] == 0xEE);
    }
    // ---- flows of ld floats per pixel, the base o floats behind a 16-byte boundary, the block ending with the last pixel's pair
    const int lays[5][2] = {{2, 0}, {4, 0}, {4, 2}, {3, 0}, {3, 1}};
    bool seen[3] = {false, false, false};
    for (const auto& lay : lays) {
        const int ld = lay[0], coff = lay[1];
        const long nfl = (npix - 1) * ld + coff + 2;
        Block fb(4 * o, 4 * nfl);
        float* f = reinterpret_cast<float*>(fb.p);
        for (long i = 0; i < nfl; ++i) f[i] = (float)(int)(rnd() & 0xffff) - 32768.f;
        const int mode = px4_flow_mode(f, ld, coff);
        CHECK(mode == (ld == 3 ? 0 : ld == 4 ? (o & 1 ? 0 : 1) : o == 0 ? 2 : o == 2 ? 1 : 0));
        for (int fmode = 0; fmode <= mode; ++fmode) {                 // a lower mode is always allowed
            seen[fmode] = true;
            for (long ch = 0; ch < nchunk; ++ch) {
                const long p0 = PX4 * ch;
                const int n = (int)(npix - p0 < PX4 ? npix - p0 : PX4);
                float u[PX4], v[PX4];
                px4_load_flow(f, ld, coff, fmode, p0, n, u, v);
                for (int i = 0; i < PX4; ++i) {
                    CHECK(u[i] == (i < n ? f[(p0 + i) * ld + coff] : 0.f));
                    CHECK(v[i] == (i < n ? f[(p0 + i) * ld + coff + 1] : 0.f));
                }
            }
        }
    }
    CHECK(seen[0] && seen[1] == (o % 2 == 0) && seen[2] == (o == 0));
    return 0;
}

template <class K>
static int search() {
    const int o = 0; const long npix = 0;
    const uint32_t top = sizeof(K) == 2 ? 0xffffu : 0xffffffu;
    for (int n : {0, 1, 2, 7}) {
        std::vector<K> keys(n);                                       // exact size: a probe of keys[n] is an error
        for (int i = 0; i < n; ++i) keys[i] = (K)(i == n - 1 ? top : 3 * i + (n > 2));     // with and without key 0, the largest value
        for (int i = 0; i < n; ++i) CHECK(px4_sorted_index(keys.data(), n, keys[i]) == i);
        for (uint32_t v : {0u, 1u, 2u, 5u, 17u, top - 1, top}) {
            bool listed = false;
            for (int i = 0; i < n; ++i) listed = listed || keys[i] == v;
            if (!listed) CHECK(px4_sorted_index(keys.data(), n, v) == n);
        }
    }
    return 0;
}

static int modes() {
    const int o = 0; const long npix = 0;
    Block b(0, 64);
    const float* f = reinterpret_cast<const float*>(b.p);
    CHECK(px4_flow_mode(f, 2, 0) == 2 && px4_flow_mode(f + 4, 2, 0) == 2);      // dense, 16-byte aligned
    CHECK(px4_flow_mode(f + 2, 2, 0) == 1 && px4_flow_mode(f + 1, 2, 0) == 0 && px4_flow_mode(f + 3, 2, 0) == 0);
    CHECK(px4_flow_mode(f, 4, 0) == 1 && px4_flow_mode(f, 4, 2) == 1 && px4_flow_mode(f, 4, 1) == 0);     // a view of a wider map
    CHECK(px4_flow_mode(f + 1, 4, 1) == 1 && px4_flow_mode(f + 1, 4, 0) == 0);                             // base + coff decides
    CHECK(px4_flow_mode(f, 3, 0) == 0 && px4_flow_mode(f, 3, 1) == 0 && px4_flow_mode(f, 5, 2) == 0);     // odd ld: every other pair is off
    CHECK(px4_flow_mode(f, 6, 0) == 1 && px4_flow_mode(f, 6, 4) == 1);
    return 0;
}

int main() {
    for (int o = 0; o < 4; ++o)
        for (long npix = 1; npix <= 13; ++npix)
            if (sweep(o, npix)) return 1;
    if (search<uint16_t>() || search<uint32_t>() || modes()) return 1;
    printf("ok %ld\n", checks);
    return 0;
}
'''


def test_px4_loads_stores_and_search_under_the_host_sanitizers(tmp_path):
    src = tmp_path / 'px4_driver.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'px4_driver'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC, str(src),
           '-o', str(exe)]
    # the runtimes linked statically where the compiler has them (as tests/test_rle.py: the program then does not care what else the loader
    # brings along), dynamically otherwise
    if subprocess.run(cmd + ['-static-libasan', '-static-libubsan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    word, n = run.stdout.split()
    assert word == 'ok' and int(n) > 5000
