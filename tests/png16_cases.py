"""16-bit RGB PNG files (colour type 2, bit depth 16: 6 bytes per pixel, samples big-endian) written with a CHOSEN filter type per scanline,
and read back byte by byte, in NumPy / stdlib only: with tests/kitti_flow_restate.py the whole reference of the KITTI flow tests
(tests/test_png16_host.py, tests/test_kitti_flow_gpu.py, tests/test_kitti_flow_tools.py). Nothing here shares code with vps_amd or with
tests/png_filter_cases.py. An image is its RAW rows: uint8 [H, 6 W], the bytes of a row in file order.

    filtered(raw, types)            the filtered scanlines, H rows of 1 + 6 W bytes (PNG specification 9.2, the byte to the left = 6 back)
    unfilter(scan, H, W)            the reverse, one byte at a time in plain Python integers
    container(...), encode(...)     the file round a zlib stream; chunks(file) takes it apart again and checks every CRC
    device_filter_rows(raw, bpp)    the filter rule of vps_png_deflate_bpp as include/vps_hip.h states it: None / Sub / Up by the smallest
                                    sum of |int8(residual)|, a tie to the lower number
"""
import struct
import zlib

import numpy as np

SIG = b'\x89PNG\r\n\x1a\n'
BPP = 6
# every ordered pair of adjacent filter types: an Euler circuit of the complete directed graph on 0..4 with loops (25 edges, 26 rows)
ALL_PAIRS = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 2, 4, 1, 3, 0, 3, 1, 4, 2, 0, 4, 3, 2, 1, 0]
assert {(a, b) for a, b in zip(ALL_PAIRS, ALL_PAIRS[1:])} == {(a, b) for a in range(5) for b in range(5)}


def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filtered(raw, types, bpp=BPP):
    """raw uint8 [H, rowbytes] + one filter type per row -> the filtered scanlines as bytes (an encoder predicts from ORIGINAL bytes)"""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2 and raw.shape[1] % bpp == 0
    H, n = raw.shape
    rows = raw.astype(np.int64)
    out = np.empty((H, 1 + n), dtype=np.uint8)
    zero = np.zeros(n, np.int64)
    for y in range(H):
        ft = int(types[y])
        cur, up = rows[y], rows[y - 1] if y else zero
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        if ft == 4:
            p = a + up - c
            pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        else:
            pred = (zero, a, up, (a + up) >> 1)[ft]
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def unfilter(scan, H, W, bpp=BPP):
    """filtered scanlines (bytes or uint8 array, H rows of 1 + bpp W) -> raw uint8 [H, bpp W], byte by byte"""
    n = bpp * W
    s = bytes(scan)
    assert len(s) == H * (1 + n)
    out = [[0] * n for _ in range(H)]
    for y in range(H):
        ft = s[y * (1 + n)]
        assert ft <= 4
        line, cur = s[y * (1 + n) + 1:(y + 1) * (1 + n)], out[y]
        up = out[y - 1] if y else [0] * n
        for i in range(n):
            a = cur[i - bpp] if i >= bpp else 0
            b = up[i]
            c = up[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[ft]
            cur[i] = (line[i] + pred) & 255
    return np.array(out, dtype=np.uint8).reshape(H, n)


def container(H, W, stream, idat_parts=3, depth=16, ctype=2, interlace=0):
    """IHDR + the zlib stream cut into `idat_parts` IDAT chunks + IEND"""
    n = max(-(-len(stream) // idat_parts), 1)
    parts = [stream[i:i + n] for i in range(0, len(stream), n)] or [b'']
    ihdr = struct.pack('>IIBBBBB', W, H, depth, ctype, 0, 0, interlace)
    return SIG + chunk(b'IHDR', ihdr) + b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b'')


def encode(raw, types, idat_parts=3, level=6):
    """raw uint8 [H, 6 W] -> (file bytes, filtered scanlines)"""
    raw = np.asarray(raw)
    H, W = raw.shape[0], raw.shape[1] // BPP
    scan = filtered(raw, types)
    return container(H, W, zlib.compress(scan, level), idat_parts), scan


def chunks(data):
    """-> [(tag, payload, offset of the chunk's end)]; raises on a wrong CRC or a chunk that leaves the file"""
    assert data[:8] == SIG
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        payload = data[pos + 8:pos + 8 + n]
        assert len(payload) == n and pos + 12 + n <= len(data), 'chunk %r leaves the file' % tag
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + payload) & 0xFFFFFFFF, 'CRC of %r' % tag
        pos += 12 + n
        out.append((tag, payload, pos))
    return out


def idat_of(data):
    return b''.join(p for t, p, _ in chunks(data) if t == b'IDAT')


def ihdr_of(data):
    """-> (W, H, depth, colour type, compression, filter method, interlace)"""
    tag, payload, _ = chunks(data)[0]
    assert tag == b'IHDR' and len(payload) == 13
    return struct.unpack('>IIBBBBB', payload)


def read_raw(data):
    """a 16-bit RGB file -> raw uint8 [H, 6 W]"""
    W, H, depth, ctype, comp, fm, interlace = ihdr_of(data)
    assert (depth, ctype, comp, fm, interlace) == (16, 2, 0, 0, 0)
    return unfilter(zlib.decompress(idat_of(data)), H, W)


def rgb16(raw):
    """raw uint8 [H, 6 W] -> uint16 [H, W, 3] (R, G, B): high byte first"""
    raw = np.asarray(raw, dtype=np.uint8)
    H, W = raw.shape[0], raw.shape[1] // BPP
    b = raw.reshape(H, W, 3, 2).astype(np.uint16)
    return b[..., 0] * np.uint16(256) + b[..., 1]


def raw_of(rgb):
    """uint16 [H, W, 3] -> raw uint8 [H, 6 W]"""
    rgb = np.asarray(rgb, dtype=np.uint16)
    H, W = rgb.shape[:2]
    return np.stack([(rgb >> 8).astype(np.uint8), (rgb & 255).astype(np.uint8)], axis=-1).reshape(H, W * BPP)


def noise(H, W, seed, values=None):
    """raw rows of noise; `values`: the byte values to draw from ({0, 1, 255}: the ties of the Paeth predictor)"""
    rg = np.random.default_rng(seed)
    if values is None:
        return rg.integers(0, 256, (H, W * BPP), dtype=np.uint8)
    return np.asarray(values, dtype=np.uint8)[rg.integers(0, len(values), (H, W * BPP))]


def types_all_pairs(H, start=0):
    n = len(ALL_PAIRS) - 1
    return [ALL_PAIRS[(start + y) % n] for y in range(H)]


def device_filter_rows(raw, bpp=BPP):
    """-> (S uint8 [H * (1 + rowbytes)], filter type per row) by the rule of vps_png_deflate_bpp"""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2
    H, n = raw.shape
    v = raw.astype(np.int32)
    left = np.zeros_like(v); left[:, bpp:] = v[:, :-bpp]
    up = np.zeros_like(v); up[1:] = v[:-1]
    cands = [v & 255, (v - left) & 255, (v - up) & 255]
    scores = np.stack([np.where(c < 128, c, 256 - c).sum(axis=1) for c in cands], axis=1)
    ftype = np.argmin(scores, axis=1)                                     # the first minimum: the lower type number
    S = np.empty((H, 1 + n), np.uint8)
    S[:, 0] = ftype
    S[:, 1:] = np.stack(cands, axis=0)[ftype, np.arange(H)]
    return S.reshape(-1), ftype.astype(np.uint8)
