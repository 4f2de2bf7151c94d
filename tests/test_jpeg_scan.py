"""CPU: the host side of the device entropy coder - `vps_jpeg_wrap` (csrc/jpeg_enc_host.cpp), `vps_jpeg_scan_bound` (host arithmetic in
csrc/jpeg_scan_ops.hip) - and the crafted coefficient arrays of tests/jpeg_scan_cases.py: what their reference scans contain is
asserted here, on the bytes `vps_jpeg_write` writes, so that the GPU tests (tests/test_jpeg_scan_gpu.py) are known to meet those
cases. Every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import jpeg_enc_restate as E
import jpeg_scan_cases as C
from vps_amd import hip

SUBS = [2, 0]


@pytest.mark.parametrize('sub', SUBS)
def test_wrap_around_the_scan_of_a_written_file_reproduces_the_file(sub):
    host = hip.load_host()
    for name, img in E.images():
        H, W = img.shape[:2]
        for q in (1, 90, 100):
            st, qt = E.quant_tables(host, q)
            st, ref = E.write_file(host, E.restate(img, qt, sub), H, W, sub, qt)
            assert st == 0, (name, q)
            sos = E.scan_of(ref)
            assert len(ref) - len(sos) + 14 == C.HEADER_BYTES                    # scan_of starts at the SOS marker: 14 bytes of header
            scan = sos[14:-2]
            st, ours = C.wrap(host, scan, H, W, sub, qt, len(ref))
            assert st == 0 and ours == ref, (name, q, st)
            st, ours = C.wrap(host, scan, H, W, sub, qt, len(ref) + 1000)
            assert st == 0 and ours == ref, (name, q, st)


def test_wrap_refuses_a_short_capacity_and_bad_arguments():
    host = hip.load_host()
    img = E.smooth_noise(24, 40, 3)
    st, qt = E.quant_tables(host, 90)
    st, ref = E.write_file(host, E.restate(img, qt, 2), 24, 40, 2, qt)
    scan = ref[C.HEADER_BYTES:-2]
    for cap in (len(ref) - 1, len(ref) - 2, C.HEADER_BYTES + 1, C.HEADER_BYTES, 100, 0):       # wrap checks the bytes behind the capacity
        st, part = C.wrap(host, scan, 24, 40, 2, qt, cap)
        assert st <= -1000 and part == b'', cap
    st, empty = C.wrap(host, b'', 24, 40, 2, qt, 1000)                                          # the scan is copied, not parsed
    assert st == 0 and empty == ref[:C.HEADER_BYTES] + b'\xff\xd9'
    assert C.wrap(host, scan, 24, 40, 1, qt, 1 << 16)[0] <= -1000                               # 4:2:2 is not written
    assert C.wrap(host, scan, 0, 40, 2, qt, 1 << 16)[0] <= -1000
    assert C.wrap(host, scan, 24, 40, 2, np.zeros((2, 64), np.uint16), 1 << 16)[0] <= -1000     # no table entry is 0
    n = ctypes.c_int64(0)
    assert host.vps_jpeg_wrap(None, 0, 24, 40, 2, None, None, 0, ctypes.byref(n)) <= -1000
    # longer than any scan of an 8x8 image (3 blocks): refused whatever the capacity
    assert C.wrap(host, bytes(3 * 416 + 3), 8, 8, 0, qt, 1 << 16)[0] <= -1000
    assert C.wrap(host, bytes(3 * 416 + 2), 8, 8, 0, qt, 1 << 16)[0] == 0


def test_scan_bound_agrees_with_the_write_and_encode_bounds():
    host = hip.load_host()
    for sub in SUBS:
        for H, W in E.SIZES + [(1, 1), (1024, 2048), (65535, 1), (1, 65535)]:
            st, wsb, cap = C.scan_bound(host, H, W, sub)
            assert st == 0, (H, W, sub)
            file_cap, coef_bytes = ctypes.c_int64(0), ctypes.c_int64(0)
            assert host.vps_jpeg_write_bound(H, W, sub, ctypes.byref(file_cap)) == 0
            assert host.vps_jpeg_encode_bound(H, W, sub, None, ctypes.byref(coef_bytes)) == 0
            nblk = coef_bytes.value // 128
            assert cap == file_cap.value - C.HEADER_BYTES - 2 == nblk * 416 + 2
            # the workspace holds at least a 32-bit size per block and the unstuffed worst case (208 bytes per block)
            assert wsb >= nblk * (4 + 208) and wsb % 16 == 0
    assert C.scan_bound(host, 24, 40, 1)[0] <= -1000 and C.scan_bound(host, 0, 40, 2)[0] <= -1000
    assert host.vps_jpeg_scan_bound(24, 40, 2, None, None) == 0                  # either output may be NULL


def test_scan_bound_refuses_sizes_whose_worst_case_does_not_fit_32_bit_offsets():
    """bit offsets on the device are 32-bit: 208 bytes * 8 bits per block + one byte must stay below 2^32"""
    host = hip.load_host()
    limit = ((1 << 32) - 1 - 8) // (208 * 8)                                     # blocks
    for sub, per_mcu, px in ((0, 3, 8), (2, 6, 16)):
        mcus = limit // per_mcu
        cols = 2048
        rows = mcus // cols                                                      # rows * cols MCUs fit, one more row of MCUs may not
        assert C.scan_bound(host, rows * px, cols * px, sub)[0] == 0
        over = (limit // per_mcu + cols) // cols + 1
        assert over * cols * per_mcu > limit
        assert C.scan_bound(host, over * px, cols * px, sub)[0] <= -1000
        n = ctypes.c_int64(0)
        assert host.vps_jpeg_write_bound(over * px, cols * px, sub, ctypes.byref(n)) == 0      # the host coder has no such limit
    assert C.scan_bound(host, 65535, 65535, 0)[0] <= -1000


@pytest.mark.parametrize('sub', SUBS)
def test_the_crafted_cases_contain_what_the_gpu_tests_rely_on(sub):
    host = hip.load_host()
    H, W = C.SIZE[sub]
    assert E.grid_of(H, W, sub)[1] == (3, 5)                                     # 3 x 5 MCUs
    st, some = E.write_file(host, np.zeros(len(C.scan_order(H, W, sub)) * 64, np.int16), H, W, sub, np.ones((2, 64), np.uint16))
    tables = C.tables_of(some)
    chunk = C.stuff_chunk()
    seen = dict(runs=set(), dc=set(), ac=set(), no_eob=0, zero_blocks=0)
    ffff = last_ff_aligned = last_ff_padded = aligned = unaligned = boundaries = 0
    for name, coef in C.cases(sub):
        st, ref = C.reference_scan(host, coef, H, W, sub)
        assert st == 0, name
        r = C.restate_scan(tables, coef, H, W, sub)
        assert r['stuffed'] == ref, name                                         # the counting restatement is the host coder
        for k in ('runs', 'dc', 'ac'):
            seen[k] |= r[k]
        seen['no_eob'] += r['no_eob']
        seen['zero_blocks'] += r['zero_blocks']
        ffff += b'\xff\x00\xff\x00' in ref
        aligned += r['bits'] % 8 == 0
        unaligned += r['bits'] % 8 != 0
        last_ff_aligned += r['bits'] % 8 == 0 and r['raw'][-1] == 0xFF
        last_ff_padded += r['bits'] % 8 != 0 and r['raw'][-1] == 0xFF and ref[-2:] == b'\xff\x00'
        raw = np.frombuffer(r['raw'], np.uint8)
        if name == 'all_1023':
            assert len(raw) > 2 * chunk
            for b in range(chunk, len(raw), chunk):                              # a stuffed byte within 4 bytes either side of every boundary
                assert (raw[b - 4:b] == 0xFF).any() and (raw[b:b + 4] == 0xFF).any(), (name, b)
                boundaries += 1
    assert boundaries >= 2
    assert set(C.RUNS) <= seen['runs'] and 0 in seen['runs']
    assert {2047, -2047, 1, -1, 0} <= seen['dc'] and {1023, -1023, 1, -1} <= seen['ac']
    assert seen['no_eob'] > 0 and seen['zero_blocks'] > 0
    assert ffff and aligned and unaligned and last_ff_aligned and last_ff_padded
