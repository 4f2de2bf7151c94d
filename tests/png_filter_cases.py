"""PNG files written with a CHOSEN filter type per scanline (PNG specification 9.2: 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth), for the
tests of `vps_png_inflate` (tests/test_png_inflate.py) and `vps_png_reconstruct` (tests/test_png_reconstruct_gpu.py). An encoder
predicts from ORIGINAL pixels, so every row is plain array arithmetic here; the decoder's dependent chains are what the tests check."""
import struct
import zlib

import numpy as np

SIG = b'\x89PNG\r\n\x1a\n'
CTYPE = {1: 0, 3: 2, 4: 6}

# every ordered pair of adjacent filter types: an Euler circuit of the complete directed graph on 0..4 with loops (25 edges, 26 rows)
ALL_PAIRS = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 0, 2, 4, 1, 3, 0, 3, 1, 4, 2, 0, 4, 3, 2, 1, 0]
assert {(a, b) for a, b in zip(ALL_PAIRS, ALL_PAIRS[1:])} == {(a, b) for a in range(5) for b in range(5)}


def chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def filtered(img, types):
    """uint8 [H,W] or [H,W,C] + one filter type per row -> the filtered scanlines, H rows of 1 + W*C bytes (what zlib has to deliver)"""
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(H, W * C).astype(np.int64)
    raw = np.empty((H, 1 + W * C), dtype=np.uint8)
    zero = np.zeros(W * C, np.int64)
    for y in range(H):
        ft = int(types[y])
        cur, up = rows[y], rows[y - 1] if y else zero
        a = np.concatenate([np.zeros(C, np.int64), cur[:-C]])
        c = np.concatenate([np.zeros(C, np.int64), up[:-C]])
        if ft == 4:
            p = a + up - c
            pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        else:
            pred = (zero, a, up, (a + up) >> 1)[ft]
        raw[y, 0] = ft
        raw[y, 1:] = (cur - pred) & 255
    return raw.tobytes()


def container(H, W, C, stream, idat_parts=3, depth=8, ctype=None, interlace=0):
    """IHDR + the zlib stream cut into `idat_parts` IDAT chunks + IEND"""
    n = max(len(stream) // idat_parts, 1)
    parts = [stream[i:i + n] for i in range(0, len(stream), n)] or [b'']
    ihdr = struct.pack('>IIBBBBB', W, H, depth, CTYPE[C] if ctype is None else ctype, 0, 0, interlace)
    return SIG + chunk(b'IHDR', ihdr) + b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b'')


def encode(img, types, idat_parts=3, level=6):
    """-> (file bytes, filtered scanlines)"""
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else img.shape[2]
    raw = filtered(img, types)
    return container(H, W, C, zlib.compress(raw, level), idat_parts), raw


def bgr(img):
    """what cv2.imread(IMREAD_COLOR) makes of the stored array: grey replicated, alpha dropped, R and B swapped"""
    if img.ndim == 2:
        return np.ascontiguousarray(np.repeat(img[:, :, None], 3, 2))
    return np.ascontiguousarray(img[:, :, [2, 1, 0]])


def noise(H, W, C, seed, high=256):
    rg = np.random.default_rng(seed)
    return rg.integers(0, high, (H, W, C) if C > 1 else (H, W), dtype=np.uint8)


def types_all_pairs(H):
    """H filter types, cycling through ALL_PAIRS (26 rows cover all 25 ordered pairs; the cycle closes 0 -> 0)"""
    return [ALL_PAIRS[y % (len(ALL_PAIRS) - 1)] for y in range(H)]
