"""NumPy / Python restatement of the device PNG encoder (`vps_amd/csrc/png_ops.hip`, format in include/vps_hip.h at vps_png_deflate):
uint8 [H][W][C] (C = 1 or 3) -> the bytes of the PNG file. It is the CPU twin the device stage does not have: the GPU tests ask for
the same bytes, the CPU tests check that PIL, the library's own PNG decoder and zlib read them back. Written from RFC 1951 (the code
tables below are section 3.2.5 / 3.2.6 typed out, not computed), RFC 1950 (Adler-32) and the PNG specification (filters 0-2, chunks)."""
import struct
import zlib

import numpy as np

SEG = 8192                                   # bytes of the filtered stream per independently coded segment

# RFC 1951 3.2.5: length codes 257..285 = (extra bits, first length)
_LEN_TABLE = [(0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10), (1, 11), (1, 13), (1, 15), (1, 17), (2, 19), (2, 23),
              (2, 27), (2, 31), (3, 35), (3, 43), (3, 51), (3, 59), (4, 67), (4, 83), (4, 99), (4, 115), (5, 131), (5, 163), (5, 195),
              (5, 227), (0, 258)]


def _rev(code, n):
    return int(format(code, '0%db' % n)[::-1], 2)


def _fixed_code(sym):
    """RFC 1951 3.2.6: (code, bits) of a literal/length symbol in the fixed Huffman code"""
    if sym <= 143:
        return 0b00110000 + sym, 8
    if sym <= 255:
        return 0b110010000 + (sym - 144), 9
    if sym <= 279:
        return sym - 256, 7
    return 0b11000000 + (sym - 280), 8


def _tables():
    lit_val, lit_n = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for v in range(256):
        c, n = _fixed_code(v)
        lit_val[v], lit_n[v] = _rev(c, n), n              # Huffman codes enter the LSB-first bit stream most-significant bit first
    len_val, len_n = np.zeros(259, np.int64), np.zeros(259, np.int64)
    for L in range(3, 259):
        k = max(i for i, (_, first) in enumerate(_LEN_TABLE) if first <= L)
        eb, first = _LEN_TABLE[k]
        c, n = _fixed_code(257 + k)
        # code, then the extra bits LSB first, then the 5-bit distance code 0 (distance 1, no extra bits)
        len_val[L], len_n[L] = _rev(c, n) | ((L - first) << n), n + eb + 5
    return lit_val, lit_n, len_val, len_n


LIT_VAL, LIT_N, LEN_VAL, LEN_N = _tables()


def filter_rows(img):
    """-> (S as a uint8 array of H * (1 + W*C), filter type per row). Candidates None 0 / Sub 1 / Up 2, smallest sum of |int8(residual)|,
    a tie to the lower type number."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (1, 3)
    H, W, C = img.shape
    raw = img.reshape(H, W * C).astype(np.int32)
    left = np.zeros_like(raw); left[:, C:] = raw[:, :-C]
    up = np.zeros_like(raw); up[1:] = raw[:-1]
    cands = [(raw & 255), ((raw - left) & 255), ((raw - up) & 255)]
    scores = np.stack([np.where(c < 128, c, 256 - c).sum(axis=1) for c in cands], axis=1)        # [H][3]
    ftype = np.argmin(scores, axis=1)                                                             # first minimum = lower type number
    S = np.empty((H, 1 + W * C), np.uint8)
    S[:, 0] = ftype
    allc = np.stack(cands, axis=0)
    S[:, 1:] = allc[ftype, np.arange(H)]
    return S.reshape(-1), ftype.astype(np.uint8)


def segment_tokens(seg):
    """tokens of one segment as arrays (value, bits): maximal runs of equal bytes; first byte literal, then matches of 258 at distance 1
    while >= 258 remain, then one match of the rest if >= 3, else that many literals"""
    seg = np.asarray(seg, np.uint8)
    n = len(seg)
    starts = np.flatnonzero(np.concatenate(([True], seg[1:] != seg[:-1])))
    R = np.diff(np.concatenate((starts, [n])))
    v = seg[starts].astype(np.int64)
    nfull, rem = (R - 1) // 258, (R - 1) % 258
    ntok = 1 + nfull + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(len(starts)), ntok)
    j = np.arange(ntok.sum()) - np.repeat(np.cumsum(ntok) - ntok, ntok)             # index of the token inside its run
    rv, rfull, rrem = v[run], nfull[run], rem[run]
    is_full = (j >= 1) & (j <= rfull)
    is_rest = (j > rfull) & (rrem >= 3)
    val = np.where(is_full, LEN_VAL[258], np.where(is_rest, LEN_VAL[np.maximum(rrem, 3)], LIT_VAL[rv]))
    nb = np.where(is_full, LEN_N[258], np.where(is_rest, LEN_N[np.maximum(rrem, 3)], LIT_N[rv]))
    return val, nb


def segment_token_bits(seg):
    return int(segment_tokens(seg)[1].sum())


def encode_segment(seg):
    """fixed-Huffman block (BFINAL 0, BTYPE 01), tokens, end of block, then an empty stored block: ends on a byte boundary"""
    val, nb = segment_tokens(seg)
    val = np.concatenate(([0b010], val, [0], [0]))                                  # header; EOB = 7 zero bits; stored header 000
    nb = np.concatenate(([3], nb, [7], [3]))
    start = np.cumsum(nb) - nb
    total = int(nb.sum())
    within = np.arange(total) - np.repeat(start, nb)
    bits = ((np.repeat(val, nb) >> within) & 1).astype(np.uint8)
    body = np.packbits(bits, bitorder='little').tobytes()                           # zero bits up to the byte boundary
    out = body + b'\x00\x00\xff\xff'
    assert len(out) <= (9 * len(seg) + 7) // 8 + 7
    return out


def deflate_stream(S):
    S = np.asarray(S, np.uint8)
    parts = [b'\x78\x01']
    for o in range(0, len(S), SEG):
        parts.append(encode_segment(S[o:o + SEG]))
    parts.append(b'\x03\x00')                                                       # empty final fixed block
    parts.append(struct.pack('>I', zlib.adler32(S.tobytes()) & 0xFFFFFFFF))
    return b''.join(parts)


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def container(stream, H, W, channels):
    ihdr = struct.pack('>IIBBBBB', W, H, 8, {1: 0, 3: 2}[channels], 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', bytes(stream)) + _chunk(b'IEND', b'')


def png_stream(img):
    return deflate_stream(filter_rows(img)[0])


def png_file(img):
    img = np.asarray(img)
    H, W = img.shape[:2]
    return container(png_stream(img), H, W, 1 if img.ndim == 2 else img.shape[2])


def idat_of(file_bytes):
    """the concatenated IDAT payload of a PNG file"""
    pos, out = 8, b''
    while pos < len(file_bytes):
        n, tag = struct.unpack('>I4s', file_bytes[pos:pos + 8])
        if tag == b'IDAT':
            out += file_bytes[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out
