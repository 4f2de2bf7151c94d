"""NumPy / Python restatement of the device PNG encoder's dynamic-Huffman stream (`vps_png_deflate_h` with huffman = 1; the format is
the "dynamic" paragraph of include/vps_hip.h at vps_png_deflate_h). Written from RFC 1951 (3.2.2 canonical codes, 3.2.5 symbols,
3.2.7 block header) and that header text, not from the kernel: the GPU tests ask the device for the same bytes, the CPU tests check
that zlib, PIL and the library's own decoder read them. Filters, segments, tokens, framing and the fixed block come from
png_restate.py unchanged."""
import struct
import zlib

import numpy as np

import png_restate as R

SEG = R.SEG
MIN_FIXED_BITS = 512                         # a segment whose fixed block (header, tokens, end-of-block) is shorter stays fixed
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]                # RFC 1951 3.2.7


def _len_tables():
    sym, eb, ex = np.zeros(259, np.int64), np.zeros(259, np.int64), np.zeros(259, np.int64)
    for L in range(3, 259):
        k = max(i for i, (_, first) in enumerate(R._LEN_TABLE) if first <= L)
        sym[L], eb[L], ex[L] = 257 + k, R._LEN_TABLE[k][0], L - R._LEN_TABLE[k][1]
    return sym, eb, ex


LEN_SYM, LEN_EB, LEN_EX = _len_tables()


def segment_symbols(seg):
    """the tokens of png_restate.segment_tokens as (symbol, extra value, extra bits, is a match) arrays"""
    seg = np.asarray(seg, np.uint8)
    n = len(seg)
    starts = np.flatnonzero(np.concatenate(([True], seg[1:] != seg[:-1])))
    Rn = np.diff(np.concatenate((starts, [n])))
    v = seg[starts].astype(np.int64)
    nfull, rem = (Rn - 1) // 258, (Rn - 1) % 258
    ntok = 1 + nfull + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(len(starts)), ntok)
    j = np.arange(ntok.sum()) - np.repeat(np.cumsum(ntok) - ntok, ntok)
    rv, rfull, rrem = v[run], nfull[run], np.maximum(rem[run], 3)
    is_full = (j >= 1) & (j <= rfull)
    is_rest = (j > rfull) & (rem[run] >= 3)
    sym = np.where(is_full, 285, np.where(is_rest, LEN_SYM[rrem], rv))
    ex = np.where(is_rest, LEN_EX[rrem], 0)
    eb = np.where(is_rest, LEN_EB[rrem], 0)
    return sym, ex, eb, is_full | is_rest


def limited_lengths(freq, limit):
    """Code lengths <= limit by package-merge, as the header states it. Symbols with a count are the leaves, in ascending order of
    (count, symbol). List 1 is the leaves. List j is the leaves merged by weight with the packages of list j-1 (item 2k + item 2k+1, the
    odd last item dropped), a leaf in front of a package of equal weight, cut to its first 2n-2 items. From the top list take k = 2n-2
    items; if a of them are leaves, the a first leaves gain one bit and the list below gives 2 (k - a) items. One symbol: length 1."""
    used = [s for s, c in enumerate(freq) if c]
    n = len(used)
    lens = [0] * len(freq)
    if n == 1:
        lens[used[0]] = 1
    if n < 2:
        return lens
    leaves = sorted(used, key=lambda s: (freq[s], s))
    w = [int(freq[s]) for s in leaves]
    lists, prev = [], []
    for _ in range(limit):
        pk = [prev[2 * k][0] + prev[2 * k + 1][0] for k in range(len(prev) // 2)]
        merged, a, b = [], 0, 0
        while a < n or b < len(pk):
            if b >= len(pk) or (a < n and w[a] <= pk[b]):
                merged.append((w[a], True)); a += 1
            else:
                merged.append((pk[b], False)); b += 1
        prev = merged[:2 * n - 2]
        lists.append(prev)
    k = 2 * n - 2
    for lst in reversed(lists):
        assert k <= len(lst)
        a = sum(1 for _, leaf in lst[:k] if leaf)
        for r in range(a):
            lens[leaves[r]] += 1
        k = 2 * (k - a)
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2"""
    maxl = max(lens) if len(lens) else 0
    bl = [0] * (maxl + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = nxt[l]; nxt[l] += 1
    return out


def code_length_tokens(seq):
    """the greedy rule of the header over the HLIT + HDIST lengths as one sequence: per maximal run of equal lengths. A run of R zeros:
    18 with min(R, 138) while R >= 11, then 17 if R >= 3, else R times 0. A run of R lengths v: v once, then 16 with min(R, 6) while the
    rest R >= 3, then the rest as v. -> [(symbol, extra value, extra bits)]"""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        v, r = seq[i], j - i
        if v == 0:
            while r >= 11:
                c = min(r, 138); out.append((18, c - 11, 7)); r -= c
            if r >= 3:
                out.append((17, r - 3, 3)); r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0)); r -= 1
            while r >= 3:
                c = min(r, 6); out.append((16, c - 3, 2)); r -= c
            out += [(v, 0, 0)] * r
        i = j
    return out


def dynamic_block(seg):
    """-> dict: the (value, bits) arrays of the dynamic block of one segment up to and including end-of-block, and what the tests look at"""
    sym, ex, eb, is_match = segment_symbols(seg)
    freq = np.bincount(sym, minlength=286)
    freq[256] = 1
    lens = limited_lengths(freq.tolist(), 15)
    codes = canonical_codes(lens)
    hlit = max(257, max(s for s in range(286) if lens[s]) + 1)
    seq = lens[:hlit] + [1, 1]                                   # the distance code: symbols 0 and 1, one bit each
    cltok = code_length_tokens(seq)
    clfreq = [0] * 19
    for s, _, _ in cltok:
        clfreq[s] += 1
    cllens = limited_lengths(clfreq, 7)
    clcodes = canonical_codes(cllens)
    hclen = max(4, max(i for i in range(19) if cllens[CL_ORDER[i]]) + 1)
    val, nb = [0b100, hlit - 257, 2 - 1, hclen - 4], [3, 5, 5, 4]     # BFINAL 0, BTYPE 10 (its low bit first)
    for i in range(hclen):
        val.append(cllens[CL_ORDER[i]]); nb.append(3)
    for s, e, b in cltok:
        val.append(R._rev(clcodes[s], cllens[s]) | (e << cllens[s])); nb.append(cllens[s] + b)
    header_bits = sum(nb)
    lens_a = np.array(lens, np.int64)
    rev_a = np.array([R._rev(c, l) if l else 0 for c, l in zip(codes, lens)], np.int64)
    # a match: length code, extra bits LSB first, the one-bit distance code 0
    tval = rev_a[sym] | (ex << lens_a[sym])
    tnb = lens_a[sym] + eb + is_match
    token_bits = int(tnb.sum())
    val = np.concatenate((np.array(val, np.int64), tval, [rev_a[256]]))
    nb = np.concatenate((np.array(nb, np.int64), tnb, [lens_a[256]]))
    return dict(val=val, nb=nb, lens=lens, cllens=cllens, hlit=hlit, hclen=hclen, header_bits=header_bits, token_bits=token_bits,
                freq=freq, clfreq=clfreq, total_bits=int(nb.sum()))


def fixed_total_bits(seg):
    return 3 + R.segment_token_bits(seg) + 7


def _pack(val, nb):
    start = np.cumsum(nb) - nb
    within = np.arange(int(nb.sum())) - np.repeat(start, nb)
    bits = ((np.repeat(val, nb) >> within) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder='little').tobytes()


def segment_is_dynamic(seg):
    f = fixed_total_bits(seg)
    return f >= MIN_FIXED_BITS and dynamic_block(seg)['total_bits'] < f


def encode_segment(seg):
    """the dynamic block if the fixed block has at least MIN_FIXED_BITS bits and the dynamic block is strictly shorter in bits, else
    png_restate's fixed block; either way followed by the empty stored block"""
    if not segment_is_dynamic(seg):
        return R.encode_segment(seg)
    d = dynamic_block(seg)
    out = _pack(np.concatenate((d['val'], [0])), np.concatenate((d['nb'], [3]))) + b'\x00\x00\xff\xff'
    assert len(out) <= (9 * len(seg) + 7) // 8 + 7
    return out


def deflate_stream(S):
    S = np.asarray(S, np.uint8)
    parts = [b'\x78\x01']
    for o in range(0, len(S), SEG):
        parts.append(encode_segment(S[o:o + SEG]))
    parts.append(b'\x03\x00')
    parts.append(struct.pack('>I', zlib.adler32(S.tobytes()) & 0xFFFFFFFF))
    return b''.join(parts)


def png_stream(img):
    return deflate_stream(R.filter_rows(img)[0])


def png_file(img):
    img = np.asarray(img)
    H, W = img.shape[:2]
    return R.container(png_stream(img), H, W, 1 if img.ndim == 2 else img.shape[2])


def zrle(S, level=6):
    """the size reference: zlib restricted to literals and distance-1 runs"""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(bytes(S)) + c.flush()
