"""Crafted coefficient arrays for the device entropy coder (`vps_jpeg_encode_scan`: csrc/jpeg_scan_ops.hip), built on the CPU, and the
tools to say what a reference scan contains. The reference is always `vps_jpeg_write` (pinned to libjpeg-turbo in
tests/test_jpeg_enc.py); `restate_scan` is a bit-level restatement in Python that reads its Huffman tables from the DHT segments of a
file `vps_jpeg_write` wrote - it exists to COUNT (bits, runs, categories), and tests/test_jpeg_scan.py pins it to the host coder byte
for byte. Grids: 3 x 5 MCUs in both samplings (48x80 at 4:2:0, 24x40 at 4:4:4), so DC prediction crosses MCUs and MCU rows."""
import ctypes
import os
import re

import numpy as np

import jpeg_enc_restate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14
SIZE = {2: (48, 80), 0: (24, 40)}
RUNS = (15, 16, 31, 32, 47, 48, 62)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def stuff_chunk():
    """bytes of the unstuffed stream per workgroup of the device's stuffing pass: the constant of the source"""
    src = open(os.path.join(ROOT, 'vps_amd', 'csrc', 'jpeg_scan_ops.hip')).read()
    return int(re.search(r'constexpr int CHUNK = (\d+);', src).group(1))


def scan_order(H, W, sub):
    """[(component, index of the block in the coefficient array)] in the order of the interleaved scan"""
    grid = E.grid_of(H, W, sub)
    base = np.cumsum([0] + [r * c for r, c in grid])
    f = 2 if sub == 2 else 1
    out = []
    for my in range(grid[1][0]):
        for mx in range(grid[1][1]):
            for c in range(3):
                k = f if c == 0 else 1
                for v in range(k):
                    for u in range(k):
                        out.append((c, int(base[c]) + (my * k + v) * grid[c][1] + mx * k + u))
    return out


def scan_bound(host, H, W, sub):
    wsb, cap = ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = host.vps_jpeg_scan_bound(H, W, sub, ctypes.byref(wsb), ctypes.byref(cap))
    return st, wsb.value, cap.value


def wrap(host, scan, H, W, sub, qt, capacity):
    """vps_jpeg_wrap -> (status, bytes); the bytes behind the capacity must stay as they are"""
    buf = np.frombuffer(bytes(scan) + b'\0', dtype=np.uint8)                     # one more byte: an empty scan still has an address
    qt = np.ascontiguousarray(qt, dtype=np.uint16)
    out = np.full(capacity + 64, 0xA5, dtype=np.uint8)
    n = ctypes.c_int64(-1)
    st = host.vps_jpeg_wrap(buf.ctypes.data_as(ctypes.c_void_p), len(scan), H, W, sub, qt.ctypes.data_as(ctypes.c_void_p),
                            out.ctypes.data_as(ctypes.c_void_p), capacity, ctypes.byref(n))
    assert (out[capacity:] == 0xA5).all(), 'vps_jpeg_wrap stored beyond its capacity'
    return st, out[:max(n.value, 0)].tobytes()


def reference_scan(host, coef, H, W, sub):
    """the entropy-coded segment of the file vps_jpeg_write writes: (status, bytes between the SOS header and EOI)"""
    st, data = E.write_file(host, coef, H, W, sub, np.ones((2, 64), np.uint16))
    return st, data[HEADER_BYTES:-2]


def tables_of(data):
    """{(class, id): {symbol: (code, length)}} from the DHT segments of a file"""
    out, pos = {}, 2
    while data[pos + 1] != 0xDA:
        n = (data[pos + 2] << 8) | data[pos + 3]
        if data[pos + 1] == 0xC4:
            tc_th, bits, vals = data[pos + 4], data[pos + 5:pos + 21], data[pos + 21:pos + 2 + n]
            t, code, k = {}, 0, 0
            for length in range(1, 17):
                for _ in range(bits[length - 1]):
                    t[vals[k]] = (code, length)
                    code, k = code + 1, k + 1
                code <<= 1
            out[(tc_th >> 4, tc_th & 15)] = t
        pos += 2 + n
    return out


def restate_scan(tables, coef, H, W, sub):
    """-> dict(bits, unstuffed bytes (padded with ones), stuffed bytes, runs = zero runs that were coded, dc = DC differences, ac = AC
    values, no_eob = blocks whose coefficient 63 is non-zero, zero_blocks)"""
    acc, nbits = 0, 0
    runs, dcs, acs, no_eob, zero_blocks = set(), set(), set(), 0, 0
    pred = [0, 0, 0]

    def put(v, n):
        nonlocal acc, nbits
        acc = (acc << n) | (v & ((1 << n) - 1))
        nbits += n
    for c, b in scan_order(H, W, sub):
        blk = coef[b * 64:(b + 1) * 64].astype(np.int64)[ZIGZAG]
        dc, ac = tables[(0, min(c, 1))], tables[(1, min(c, 1))]
        d = int(blk[0]) - pred[c]
        pred[c] = int(blk[0])
        dcs.add(d)
        s = abs(d).bit_length()
        put(*dc[s])
        put(d if d >= 0 else d - 1, s)
        run = 0
        zero_blocks += not blk.any()
        for k in range(1, 64):
            a = int(blk[k])
            if a == 0:
                run += 1
                continue
            runs.add(run)
            acs.add(a)
            while run > 15:
                put(*ac[0xF0])
                run -= 16
            s = abs(a).bit_length()
            put(*ac[(run << 4) | s])
            put(a if a >= 0 else a - 1, s)
            run = 0
        if run:
            put(*ac[0])
        else:
            no_eob += 1
    pad = -nbits % 8
    raw = ((acc << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, 'big')
    return dict(bits=nbits, raw=raw, stuffed=raw.replace(b'\xff', b'\xff\x00'), runs=runs, dc=dcs, ac=acs, no_eob=no_eob, zero_blocks=zero_blocks)


def _empty(sub):
    H, W = SIZE[sub]
    return np.zeros(sum(r * c for r, c in E.grid_of(H, W, sub)) * 64, np.int16), H, W


def _set(coef, b, k, v):
    coef[b * 64 + ZIGZAG[k]] = v


def cases(sub):
    """[(name, int16 coefficients)] on the 3 x 5 MCU grid of `sub`"""
    out = []
    zero, H, W = _empty(sub)
    order = scan_order(H, W, sub)
    out.append(('zero', zero))                                                   # 4:2:0: 15 x 32 bits, a whole number of bytes; 4:4:4: 210 bits
    # one non-zero coefficient behind a run of exactly r zeros, +-1 and +-1023, then sometimes a second one; DC differences +-1 / +-2047
    c1 = zero.copy()
    for i, (c, b) in enumerate(order):
        r = RUNS[i % len(RUNS)]
        _set(c1, b, r + 1, (1, -1, 1023, -1023)[(i // len(RUNS)) % 4])
        if i % 3 == 0 and r + 1 < 63:
            _set(c1, b, 63, -1 if i % 2 else 1)                                  # coefficient 63: no EOB
        c1[b * 64] = (0, 1, 0, -1, 1023, -1024)[i % 6] if i % 5 else 0
    out.append(('runs', c1))
    # DC alternating between the ends of its range per component: differences of +-2047; no AC
    c2 = zero.copy()
    seen = [0, 0, 0]
    for c, b in order:
        c2[b * 64] = 1023 if seen[c] % 2 == 0 else -1024
        seen[c] += 1
    out.append(('dc_extremes', c2))
    # every AC coefficient 1023: a 16-bit code that starts with nine ones behind ten value bits of ones - runs of 19 ones every 26 bits,
    # so 0xFF bytes everywhere (also next to every chunk boundary of the stuffing pass), FF FF among them
    c3 = np.full_like(zero, 1023)
    for i, (c, b) in enumerate(order):
        c3[b * 64] = (i * 37) % 512 - 256
    out.append(('all_1023', c3))
    rng = np.random.RandomState(11 + sub)
    c4 = rng.randint(-1023, 1024, zero.size).astype(np.int16)
    c4[::64] = rng.randint(-1024, 1024, zero.size // 64)                         # any two DCs differ by at most 2047
    out.append(('dense_random', c4))
    c5 = np.where(rng.rand(zero.size) < 0.12, rng.randint(-40, 41, zero.size), 0).astype(np.int16)
    c5[::64] = rng.randint(-300, 300, zero.size // 64)
    out.append(('sparse_random', c5))
    # the stream ends in ten ones (coefficient 63 of the last block = 1023): whatever the alignment, the last byte is 0xFF. The
    # magnitude of one earlier coefficient moves the end of the stream bit by bit
    for cat in range(1, 9):
        c6 = zero.copy()
        _set(c6, order[-1][1], 63, 1023)
        _set(c6, order[0][1], 1, (1 << cat) - 1)
        out.append(('ends_in_ones_%d' % cat, c6))
    return out
