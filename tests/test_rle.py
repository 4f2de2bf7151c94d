"""CPU: the host half of the track tubes (`vps_rle_strings`, csrc/rle_host.cpp; `rle_decode` and `TubeCollector.add_runs` of
vps_amd/tubes.py) against the NumPy restatement of the COCO mask API (tests/rle_restate.py). Every comparison is exact equality.
The device half, `vps_rle_runs`, is compared with `runs_of` in tests/test_rle_gpu.py."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rle_restate as R
from vps_amd import hip, tubes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (7, 1), (5, 7), (37, 129)]


def label_map(H, W, nkeys, seed):
    """blocky random labels: runs of every length, several keys per column, runs that go on in the next column"""
    rng = np.random.default_rng(seed)
    keys = rng.choice(65536, size=nkeys, replace=False)
    small = rng.integers(0, nkeys, size=((H + 2) // 3, (W + 3) // 4))
    m = keys[small].repeat(3, 0).repeat(4, 1)[:H, :W].copy()
    noise = rng.random((H, W)) < 0.1
    m[noise] = keys[rng.integers(0, nkeys, size=int(noise.sum()))]
    return m


def test_restatement_gives_the_known_answers():
    for counts, s in R.KNOWN:
        assert R.rle_to_string(counts) == s, counts
        assert R.rle_from_string(s) == counts, s
    m = np.zeros((2, 2), np.uint8)
    assert R.rle_encode(m) == [4] and R.encode(m)['counts'] == '4'
    m[:] = 1
    assert R.rle_encode(m) == [0, 4] and R.encode(m)['counts'] == '04'
    m = np.array([[0, 1], [1, 0], [1, 1]], np.uint8)                 # Fortran order: 0 1 1 | 1 0 1
    assert R.rle_encode(m) == [1, 3, 1, 1] and R.to_bbox([1, 3, 1, 1], 3, 2) == [0, 0, 2, 3]
    assert np.array_equal(R.rle_decode([1, 3, 1, 1], 3, 2), m)


def test_restatement_equals_pycocotools_where_it_is_installed():
    cm = pytest.importorskip('pycocotools.mask')
    for (H, W) in SIZES:
        m = label_map(H, W, 5, H * 1000 + W)
        for k in np.unique(m):
            mask = np.asfortranarray((m == k).astype(np.uint8))
            enc = cm.encode(mask)
            assert enc['counts'].decode('ascii') == R.encode(mask)['counts'] and list(enc['size']) == [H, W]
            assert np.array_equal(cm.decode(enc), mask)
            assert [int(v) for v in cm.toBbox(enc)] == R.to_bbox(R.rle_encode(mask), H, W)


def test_known_answers_through_the_library():
    # counts [c0, c1, ...] as a run list: key 1 on the one-runs, key 0 on the zero-runs
    for counts, s in R.KNOWN:
        flat = np.repeat(np.arange(len(counts)) & 1, counts)
        start, key = R.runs_of(flat.reshape(-1, 1))
        assert tubes.rle_strings(start, key, flat.size, [1]) == [s.encode('ascii')], counts


@pytest.mark.parametrize('H,W', SIZES)
def test_strings_equal_the_restatement(H, W):
    for nkeys, seed in ((1, 1), (3, 2), (40, 3)):
        m = label_map(H, W, nkeys, seed + 10 * H + W)
        start, key = R.runs_of(m)
        present = np.unique(m)
        absent = next(k for k in range(65536) if k not in set(present.tolist()))
        for wanted in (present, present[:1], present[-1:], present[::2], np.sort(np.append(present, absent)), np.array([absent]), np.array([], np.int64)):
            got = tubes.rle_strings(start, key, H * W, wanted)
            want = [R.encode(m == k)['counts'].encode('ascii') for k in wanted]
            assert got == want, (H, W, nkeys, wanted.tolist())
        assert tubes.rle_strings(start, key, H * W, [absent]) == [R.rle_to_string([H * W]).encode('ascii')]


@pytest.mark.parametrize('H,W', SIZES)
def test_decode_inverts_encode(H, W):
    m = label_map(H, W, 4, H + 100 * W)
    start, key = R.runs_of(m)
    keys = np.unique(m)
    for k, s in zip(keys, tubes.rle_strings(start, key, H * W, keys)):
        for counts in (s, s.decode('ascii')):
            got = tubes.rle_decode({'size': [H, W], 'counts': counts})
            assert got.dtype == np.uint8 and got.shape == (H, W) and np.array_equal(got, m == k)
        assert tubes.rle_counts({'counts': s}) == R.rle_encode(m == k) == R.rle_from_string(s)
    with pytest.raises(ValueError):
        tubes.rle_decode({'size': [H + 1, W], 'counts': tubes.rle_strings(start, key, H * W, keys[:1])[0]})


def _call(start, key, npix, keys, cap, guard=64):
    """vps_rle_strings on a buffer with `guard` canary bytes behind its capacity -> (status, buffer, offset, length)"""
    host = hip.load_host()
    start, key, keys = np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(key, np.uint16), np.ascontiguousarray(keys, np.uint16)
    out = np.full(cap + guard, 0xA5, np.uint8)
    off, ln, scr = np.full(keys.size, -7, np.int64), np.full(keys.size, -7, np.int64), np.zeros(4 * keys.size, np.int64)
    st = host.vps_rle_strings(start.ctypes.data, key.ctypes.data, start.size, npix, keys.ctypes.data, keys.size, out.ctypes.data, cap,
                              off.ctypes.data, ln.ctypes.data, scr.ctypes.data)
    return st, out, off, ln


def test_a_capacity_one_byte_short_is_refused_and_nothing_is_stored():
    H, W = 37, 129
    m = label_map(H, W, 6, 77)
    start, key = R.runs_of(m)
    keys = np.unique(m)
    want = [R.encode(m == k)['counts'].encode('ascii') for k in keys]
    need = sum(len(s) for s in want)
    assert need <= hip.load_host().vps_rle_strings_bound(start.size, keys.size)
    st, out, off, ln = _call(start, key, H * W, keys, need)           # exactly enough, far below the bound
    assert st == 0 and out[:need].tobytes() == b''.join(want) and (out[need:] == 0xA5).all()
    assert ln.tolist() == [len(s) for s in want] and off.tolist() == np.cumsum([0] + [len(s) for s in want[:-1]]).tolist()
    for cap in (need - 1, need // 2, 1, 0):
        st, out, off, ln = _call(start, key, H * W, keys, cap)
        assert st <= -1000, cap
        assert (out == 0xA5).all(), cap                               # the canary and the buffer itself: nothing was stored
        assert ln.tolist() == [len(s) for s in want]                  # the defined partial state: what it would have taken


def test_bad_arguments_are_refused():
    start, key = R.runs_of(label_map(5, 7, 3, 1))
    keys = np.unique(key)
    ok = _call(start, key, 35, keys, 4096)
    assert ok[0] == 0
    assert _call(start, key, 35, keys[::-1], 4096)[0] <= -1000 or keys.size < 2          # unsorted keys
    assert _call(start, key, 34, keys, 4096)[0] <= -1000 or start[-1] < 34               # a start at or behind npix
    assert _call(start[1:], key[1:], 35, keys, 4096)[0] <= -1000                         # does not start at 0
    assert _call(start[::-1], key, 35, keys, 4096)[0] <= -1000                           # not ascending
    assert _call(start, np.zeros_like(key), 35, keys, 4096)[0] <= -1000 or start.size < 2   # neighbours with one key
    assert _call(start, key, 0, keys, 4096)[0] <= -1000 and _call(start, key, 1 << 31, keys, 4096)[0] <= -1000
    host = hip.load_host()
    assert host.vps_rle_strings(None, None, 1, 35, None, 0, None, 0, None, None, None) <= -1000
    assert host.vps_rle_strings_bound(10, 3) >= 7 * 23 and host.vps_rle_strings_bound(-1, 3) == 0


def test_runs_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    P = ctypes.c_void_p(256)                                          # never dereferenced: every call below is refused before a launch
    assert lib.vps_rle_runs(None, 4, 4, 2, P, P, 4, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 2, None, P, 4, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 2, P, None, 4, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 2, P, P, 4, None, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 2, P, P, 4, P, None, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 0, P, P, 4, P, P, 4096, None) <= -1000 and lib.vps_rle_runs(P, 4, 4, 3, P, P, 4, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 4, 4, 2, P, P, -1, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 1 << 16, 1 << 15, 2, P, P, 4, P, P, 1 << 40, None) <= -1000     # H * W = 2^31
    assert lib.vps_rle_runs(P, 0, 4, 2, P, P, 4, P, P, 4096, None) <= -1000
    assert lib.vps_rle_runs(P, 64, 64, 2, P, P, 4, P, P, lib.vps_rle_runs_ws(64, 64) - 1, None) <= -1000   # a short workspace
    assert lib.vps_rle_runs_ws(1 << 16, 1 << 15) == 0 and lib.vps_rle_runs_ws(1024, 2048) == 2048 * 32 * 4
    assert lib.vps_rle_band_rows() == tubes.BAND_ROWS


def _stats_of(m):
    """what vps_segment_stats gives for a key map: (keys, rows of count, xmin, ymin, xmax, ymax)"""
    keys = np.unique(m)
    rows = []
    for k in keys:
        ys, xs = np.nonzero(m == k)
        rows.append([ys.size, xs.min(), ys.min(), xs.max(), ys.max()])
    return keys.astype(np.int64), np.asarray(rows, np.int64)


@pytest.mark.parametrize('workers', [0, 2])
def test_tube_collector_json_on_host_made_runs(tmp_path, workers):
    H, W = 12, 20
    frames = []
    for f in range(3):
        m = np.full((H, W), 3 * 256 + 0, np.int64)                    # stuff class 3, id 0
        m[:2, :3] = 255 * 256 + 255                                   # void
        m[2:6, 1 + f:5 + f] = 12 * 256 + 1                            # a thing that moves
        if f != 1:
            m[7:, 15:] = 13 * 256 + 2                                 # a thing that is absent in frame 1
        if f == 2:
            m[8:, 0:2] = 12 * 256 + 7                                 # a thing that appears late
        frames.append(m)
    col = tubes.TubeCollector(things_only=True, workers=workers)
    both = tubes.TubeCollector(things_only=False)
    for vid in (5, 9):
        for f, m in enumerate(frames if vid == 5 else frames[:1]):
            start, key = R.runs_of(m)
            for c in (col, both):
                c.add_runs(vid, 'v%d_f%d.png' % (vid, f), H, W, start, key, _stats_of(m))
    res = col.write(str(tmp_path / 'out' / 'tubes.json'))
    col.close()
    assert json.load(open(tmp_path / 'out' / 'tubes.json')) == res
    assert [v['video_id'] for v in res['videos']] == [5, 9]
    v = res['videos'][0]
    assert v['file_names'] == ['v5_f0.png', 'v5_f1.png', 'v5_f2.png'] and (v['height'], v['width']) == (H, W)
    assert [t['track_id'] for t in v['tracks']] == [12001, 12007, 13002] and [t['category_id'] for t in v['tracks']] == [12, 12, 13]
    for t in v['tracks']:
        k = t['category_id'] * 256 + t['track_id'] % 1000
        for f, (seg, box, area) in enumerate(zip(t['segmentations'], t['bboxes'], t['areas'])):
            mask = frames[f] == k
            if not mask.any():
                assert seg is None and box is None and area is None
                continue
            assert isinstance(seg['counts'], str) and seg == R.encode(mask)
            assert area == int(mask.sum()) and box == R.to_bbox(R.rle_encode(mask), H, W)
            assert np.array_equal(tubes.rle_decode(seg), mask)
    assert [s is None for s in v['tracks'][1]['segmentations']] == [True, True, False]
    assert [s is None for s in v['tracks'][2]['segmentations']] == [False, True, False]
    assert [len(t['segmentations']) for t in res['videos'][1]['tracks']] == [1, 1]
    # stuff as well: class 3 joins, the void class never does
    assert [t['track_id'] for t in both.result()['videos'][0]['tracks']] == [3000, 12001, 12007, 13002]
    # things by class: a stuff segment that carries its class as id (a unified video map) is no track
    by_class = tubes.TubeCollector(things_only=True, id_last_stuff=10)
    m = frames[0].copy()
    m[m == 3 * 256] = 3 * 256 + 3
    by_class.add_runs(0, 'a', H, W, *R.runs_of(m), _stats_of(m))
    assert [t['track_id'] for t in by_class.result()['videos'][0]['tracks']] == [12001, 13002]


SAN_MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vps_hip.h"

// generated label sequences -> run lists -> vps_rle_strings into exactly sized heap buffers (so that any byte too many is a report),
// decoded again and compared with the sequence; then the same call one byte short
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int decode_ok(const char* p, int64_t len, const std::vector<uint16_t>& lab, uint16_t key) {
    std::vector<int64_t> cnt;
    int64_t i = 0;
    while (i < len) {
        int64_t x = 0; int k = 0; bool more = true;
        while (more) {
            if (i >= len) return 0;
            int c = p[i++] - 48;
            x |= (int64_t)(c & 0x1f) << (5 * k);
            more = c & 0x20;
            ++k;
            if (!more && (c & 0x10)) x |= -((int64_t)1 << (5 * k));
        }
        if (cnt.size() > 2) x += cnt[cnt.size() - 2];
        cnt.push_back(x);
    }
    size_t q = 0;
    for (size_t j = 0; j < cnt.size(); ++j)
        for (int64_t r = 0; r < cnt[j]; ++r, ++q)
            if (q >= lab.size() || (lab[q] == key) != (bool)(j & 1)) return 0;
    return q == lab.size();
}

int main() {
    uint32_t seed = 12345;
    int cases = 0;
    for (int t = 0; t < 60; ++t) {
        const int npix = 1 + rnd(seed) % (t < 10 ? 8 : 3000), nlab = 1 + rnd(seed) % 6, stick = 1 + rnd(seed) % 40;
        std::vector<uint16_t> lab(npix);
        uint16_t cur = 0;
        for (int q = 0; q < npix; ++q) {
            if (q == 0 || rnd(seed) % stick == 0) cur = (uint16_t)(1000 * (rnd(seed) % nlab) + 7);
            lab[q] = cur;
        }
        std::vector<uint32_t> start; std::vector<uint16_t> key;
        for (int q = 0; q < npix; ++q)
            if (q == 0 || lab[q] != lab[q - 1]) { start.push_back(q); key.push_back(lab[q]); }
        std::vector<uint16_t> keys;
        for (int l = 0; l < nlab; ++l) keys.push_back((uint16_t)(1000 * l + 7));
        keys.push_back(65000);                                                   // absent
        const int nk = (int)keys.size(), nr = (int)start.size();
        std::vector<int64_t> off(nk), len(nk), scr(4 * nk);
        // measure with capacity 0 (refused unless nothing is needed), then call with exactly what it takes
        char* none = (char*)malloc(1);
        int st = vps_rle_strings(start.data(), key.data(), nr, npix, keys.data(), nk, none, 0, off.data(), len.data(), scr.data());
        free(none);
        int64_t need = 0;
        for (int s = 0; s < nk; ++s) need += len[s];
        if (st > -1000 || need <= 0 || need > vps_rle_strings_bound(nr, nk)) { printf("FAIL measure %d %d\n", t, st); return 1; }
        char* out = (char*)malloc(need);
        st = vps_rle_strings(start.data(), key.data(), nr, npix, keys.data(), nk, out, need, off.data(), len.data(), scr.data());
        if (st != 0) { printf("FAIL exact %d %d\n", t, st); return 1; }
        for (int s = 0; s < nk; ++s)
            if (!decode_ok(out + off[s], len[s], lab, keys[s])) { printf("FAIL decode %d key %d\n", t, s); return 1; }
        free(out);
        char* shortbuf = (char*)malloc(need - 1 > 0 ? need - 1 : 1);
        st = vps_rle_strings(start.data(), key.data(), nr, npix, keys.data(), nk, shortbuf, need - 1, off.data(), len.data(), scr.data());
        free(shortbuf);
        if (st > -1000) { printf("FAIL short %d %d\n", t, st); return 1; }
        ++cases;
    }
    printf("OK %d\n", cases);
    return 0;
}
'''


def test_host_coder_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, no Python) built with rle_host.cpp under -fsanitize=address,undefined:
    generated run lists into exactly sized heap buffers, the short-capacity call included"""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    base = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g', '-O1', '-std=c++17']
    # the runtimes linked statically where the compiler has them (the program then does not care what else the loader brings along)
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libsan'], []):
        flags = base + extra
        if subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode == 0 and \
                subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip('the compiler has no sanitizer runtime')
    src = tmp_path / 'rle_san.cpp'
    src.write_text(SAN_MAIN)
    exe = tmp_path / 'rle_san'
    subprocess.check_call([cxx] + flags + ['-I', os.path.join(ROOT, 'include'), str(src), os.path.join(ROOT, 'vps_amd', 'csrc', 'rle_host.cpp'), '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'OK 60', (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
