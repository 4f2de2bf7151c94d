"""CPU: the dynamic-Huffman stream of the device PNG encoder (`vps_png_deflate_h`, huffman = 1; format in include/vps_hip.h), checked on
its NumPy restatement tests/png_dyn_restate.py for every case of tests/png_dyn_cases.py: zlib, PIL and the library's own decoder read
it; a header parser written here checks the block header and both codes; the token bits are the Huffman cost; the stream is never
longer than the fixed one; two blocks derived by hand are known answers; the size stays inside a derived cap over zlib's Z_RLE."""
import ctypes
import heapq
import io
import os
import sys
import zlib

import numpy as np
import pytest

import png_dyn_cases as C
import png_dyn_restate as D
import png_restate as R
from vps_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(C.cases())
DENSE = ['n8191', 'n8192', 'n8193', 'three_and_tail', 'random', 'seam_runs', 'fibonacci', 'fibonacci_forced', 'cl_limit', 'rgb', 'grey', 'all_symbols']
SEG = R.SEG


def _segments(S):
    return [S[o:o + SEG] for o in range(0, len(S), SEG)]


def _huffman(freq, deep=False):
    """(cost in bits, depth) of a Huffman tree over the nonzero counts; of equal weights the shallower subtree is merged first, so the
    depth is the least any Huffman tree of these counts has (deep: the deeper first)"""
    h = [(int(c), 0) for c in freq if c]
    if deep:
        h = [(c, -d) for c, d in h]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a[0] + b[0]
        heapq.heappush(h, (a[0] + b[0], min(a[1], b[1]) - 1 if deep else max(a[1], b[1]) + 1))
    return cost, abs(h[0][1])


class _Bits:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder='little')
        self.pos = 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= int(self.bits[self.pos + k]) << k
        self.pos += n
        return v

    def symbol(self, table):
        code, n = 0, 0
        while True:
            code = (code << 1) | int(self.bits[self.pos]); self.pos += 1; n += 1
            if (code, n) in table:
                return table[(code, n)]
            assert n <= 15


def _table(lens):
    return {(c, l): s for s, (c, l) in enumerate(zip(D.canonical_codes(lens), lens)) if l}


def parse_dynamic_header(block):
    """RFC 1951 3.2.7, written out: -> (hlit, hdist, hclen, code-length code lengths [19], literal/length lengths, distance lengths,
    bit position of the first token)"""
    b = _Bits(block)
    assert b.take(1) == 0 and b.take(2) == 2
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[D.CL_ORDER[i]] = b.take(3)
    table, lens = _table(cl), []
    while len(lens) < hlit + hdist:
        s = b.symbol(table)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.take(2))
        elif s == 17:
            lens += [0] * (3 + b.take(3))
        else:
            lens += [0] * (11 + b.take(7))
    assert len(lens) == hlit + hdist
    return hlit, hdist, hclen, cl, lens[:hlit], lens[hlit:], b.pos


def _kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


@pytest.mark.parametrize('name', NAMES)
def test_restated_stream_reads_back_and_its_headers_are_right(name):
    from PIL import Image
    img = C.cases()[name]
    data = C.restated(name)
    S = R.filter_rows(img)[0]
    stream = R.idat_of(data)
    assert zlib.decompress(stream) == S.tobytes()
    with Image.open(io.BytesIO(data)) as im:
        assert np.array_equal(np.asarray(im), img)
    H, W = img.shape[:2]
    host = hip.load_host()
    buf = np.frombuffer(data, np.uint8)
    out = np.empty((H, W, 3), np.uint8)
    assert host.vps_png_decode_bgr8(buf.ctypes.data, len(data), out.ctypes.data, out.size) == 0
    assert np.array_equal(out, np.repeat(img[:, :, None], 3, 2) if img.ndim == 2 else img[:, :, ::-1])
    fixed = R.png_stream(img)
    assert len(stream) <= len(fixed)
    if name in DENSE:
        assert len(stream) < len(fixed)
    pos = 2
    for seg in _segments(S):
        block = D.encode_segment(seg)
        assert stream[pos:pos + len(block)] == block and len(block) <= len(R.encode_segment(seg)) <= (9 * len(seg) + 7) // 8 + 7
        pos += len(block)
        if not D.segment_is_dynamic(seg):
            assert block == R.encode_segment(seg)
            continue
        hlit, hdist, hclen, cl, lens, dl, first = parse_dynamic_header(block)
        d = D.dynamic_block(seg)
        assert hdist == 2 and dl == [1, 1]
        assert hlit == max(257, max(s for s in range(286) if d['freq'][s]) + 1) and lens == d['lens'][:hlit]
        assert 4 <= hclen <= 19 and (hclen == 4 or cl[D.CL_ORDER[hclen - 1]] != 0) and not any(cl[s] for s in D.CL_ORDER[hclen:])
        assert max(lens) <= 15 and max(cl) <= 7 and _kraft(lens) == 1.0 and _kraft(cl) == 1.0
        assert all((l > 0) == (d['freq'][s] > 0) for s, l in enumerate(lens))
        assert first == d['header_bits']
        cost, depth = _huffman(d['freq'])
        mine = sum(int(c) * l for c, l in zip(d['freq'], lens))
        assert mine == cost if depth <= 15 else (mine > cost and max(lens) == 15)
        cost, depth = _huffman(d['clfreq'])
        mine = sum(c * l for c, l in zip(d['clfreq'], cl))
        assert mine == cost if depth <= 7 else (mine > cost and max(cl) == 7)
    assert pos + 6 == len(stream)


def test_the_case_list_is_the_one_the_format_needs():
    c = C.cases()
    assert [len(R.filter_rows(c[k])[0]) for k in ('n2', 'n8191', 'n8192', 'n8193', 'three_and_tail')] == [2, 8191, 8192, 8193, 3 * SEG + 37]
    d = D.dynamic_block(R.filter_rows(c['all_symbols'])[0])
    assert all(d['freq'][:256]) and all(d['freq'][257:286]) and d['hlit'] == 286 and D.segment_is_dynamic(R.filter_rows(c['all_symbols'])[0])
    fib = C.last_segment(c['fibonacci'])
    d = D.dynamic_block(fib)
    assert sorted(int(x) for x in d['freq'] if x) == sorted(C.FIB + [1]) and len(fib) == 4180
    # three ones: ties. A Huffman build that merges the deeper subtree first is 17 deep, one that merges the shallower first 9: the tree
    # "fits", and the limited lengths must cost what it costs
    assert _huffman(d['freq'], deep=True)[1] == 17 and _huffman(d['freq'])[1] <= 15 and max(d['lens']) <= 15
    assert sum(int(c) * l for c, l in zip(d['freq'], d['lens'])) == _huffman(d['freq'])[0]
    d = D.dynamic_block(C.last_segment(c['fibonacci_forced']))
    assert sorted(int(x) for x in d['freq'] if x) == [1] + C.FIB_FORCED and _huffman(d['freq'])[1] == 17 and max(d['lens']) == 15
    d = D.dynamic_block(C.last_segment(c['cl_limit']))
    assert _huffman(d['clfreq'])[1] == 8 and max(d['cllens']) == 7
    # runs of 1 + 258 k + j bytes, and one across the seam
    S = R.filter_rows(c['seam_runs'])[0]
    starts = np.flatnonzero(np.concatenate(([True], S[1:] != S[:-1])))
    runs = set(np.diff(np.concatenate((starts, [len(S)]))).tolist())
    assert {258 * k + j + 1 for k in (1, 2) for j in range(4)} <= runs and S[SEG - 1] == S[SEG] == 9
    # the choice rule on its edge
    diff = {k: D.dynamic_block(C.last_segment(c[k]))['total_bits'] - D.fixed_total_bits(C.last_segment(c[k])) for k in C.EDGE}
    assert diff == {'edge_win_1': -1, 'edge_equal': 0, 'edge_lose_1': 1}
    assert all(D.fixed_total_bits(C.last_segment(c[k])) >= D.MIN_FIXED_BITS for k in C.EDGE)
    assert [D.segment_is_dynamic(C.last_segment(c[k])) for k in ('edge_win_1', 'edge_equal', 'edge_lose_1')] == [True, False, False]


def test_one_byte_and_the_all_zero_map_stay_fixed():
    for S in (np.array([3], np.uint8), np.array([3, 3], np.uint8), np.zeros(SEG, np.uint8), np.zeros(100, np.uint8)):
        assert D.deflate_stream(S) == R.deflate_stream(S) and zlib.decompress(D.deflate_stream(S)) == S.tobytes()
    assert D.fixed_total_bits(np.zeros(SEG, np.uint8)) == 439 < D.MIN_FIXED_BITS
    img = C.cases()['zeros']
    assert C.restated('zeros') == R.png_file(img)
    S = R.filter_rows(img)[0]
    assert not S.any() and all(D.encode_segment(s) == R.encode_segment(s) for s in _segments(S))


def _pack(fields):
    """fields: a Huffman code as a string of bits, first bit first; anything else as (value, bits), low bit first"""
    bits = []
    for f in fields:
        if isinstance(f, str):
            bits += [int(ch) for ch in f]
        else:
            bits += [(f[0] >> k) & 1 for k in range(f[1])]
    return np.packbits(np.array(bits, np.uint8), bitorder='little').tobytes()


def test_two_blocks_derived_by_hand():
    # 600 bytes of value 5. Tokens: literal 5, then 599 = 258 + 258 + 83: two matches of 258 (symbol 285), one of 83 (symbol 278 = 83..98,
    # 4 extra bits, value 0). Counts: 5, 256, 278 once, 285 twice -> leaves (1,5) (1,256) (1,278) (2,285), n = 4, lists cut to 6 items.
    # List 1 = 1 1 1 2. Every list above = 1L 1L 1L 2L + two packages. Top: 6 items, 4 leaves -> all +1, k = 4; next: 4 items, 4 leaves ->
    # all +1, k = 0. Every length is 2; canonical codes in symbol order: 5 = 00, 256 = 01, 278 = 10, 285 = 11.
    # Length sequence (HLIT 286, + distance 1 1): 0 x5, 2, 0 x250, 2, 0 x21, 2, 0 x6, 2, 1, 1 ->
    # 17(5) 2 18(138) 18(112) 2 18(21) 2 17(6) 2 1 1. Counts: 1 x2, 2 x4, 17 x2, 18 x3 -> again four leaves, all lengths 2:
    # 1 = 00, 2 = 01, 17 = 10, 18 = 11. The last nonzero in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 is symbol 1, place 18.
    five = _pack([(0, 1), (2, 2), (286 - 257, 5), (2 - 1, 5), (18 - 4, 4)]
                 + [(n, 3) for n in (0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2)]
                 + ['10', (5 - 3, 3), '01', '11', (138 - 11, 7), '11', (112 - 11, 7), '01', '11', (21 - 11, 7), '01', '10', (6 - 3, 3), '01', '00', '00']
                 + ['00', '11', (0, 1), '11', (0, 1), '10', (0, 4), (0, 1), '01']
                 + [(0, 3)]) + b'\x00\x00\xff\xff'
    seg = np.full(600, 5, np.uint8)
    d = D.dynamic_block(seg)
    assert five.hex() == 'ecc1210100000080a0e4ffcbaeb0096c01010000ffff'
    assert D._pack(np.concatenate((d['val'], [0])), np.concatenate((d['nb'], [3]))) + b'\x00\x00\xff\xff' == five
    assert zlib.decompress(b'\x78\x01' + five + b'\x03\x00' + zlib.adler32(seg.tobytes()).to_bytes(4, 'big')) == seg.tobytes()
    assert d['total_bits'] == 137 and D.fixed_total_bits(seg) == 60 and D.encode_segment(seg) == R.encode_segment(seg)   # and it stays fixed
    # 300 zeros, 300 ones. Tokens: literal 0, 299 = 258 + 41: symbol 285, symbol 273 (35..42, 3 extra bits, value 6); the same behind
    # literal 1. Leaves (1,0) (1,1) (1,256) (2,273) (2,285), n = 5, cut 8. List 1 = 1 1 1 2 2; list 2 = 1L 1L 1L 2L 2L 2P 3P; every list
    # above = 1L 1L 1L 2L 2L 2P 3P 4P. Top: 8 items, 5 leaves, k = 6; next: 6 items, 5 leaves, k = 2; next: 2 items, 2 leaves, k = 0:
    # symbols 0 and 1 get 3 bits, the others 2. Codes: 256 = 00, 273 = 01, 285 = 10, 0 = 110, 1 = 111.
    # Sequence: 3 3, 0 x254, 2, 0 x16, 2, 0 x11, 2, 1 1 -> 3 3 18(138) 18(116) 2 18(16) 2 18(11) 2 1 1. Counts 1 x2, 2 x3, 3 x2, 18 x4:
    # all lengths 2: 1 = 00, 2 = 01, 3 = 10, 18 = 11.
    two = _pack([(0, 1), (2, 2), (29, 5), (1, 5), (14, 4)]
                + [(n, 3) for n in (0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2, 0, 2)]
                + ['10', '10', '11', (127, 7), '11', (116 - 11, 7), '01', '11', (5, 7), '01', '11', (0, 7), '01', '00', '00']
                + ['110', '10', (0, 1), '01', (6, 3), (0, 1), '111', '10', (0, 1), '01', (6, 3), (0, 1), '00']
                + [(0, 3)]) + b'\x00\x00\xff\xff'
    seg = np.repeat(np.array([0, 1], np.uint8), 300)
    d = D.dynamic_block(seg)
    assert two.hex() == 'ecc1010100000082a0fa7fda0b0e1016edd1000000ffff'
    assert D._pack(np.concatenate((d['val'], [0])), np.concatenate((d['nb'], [3]))) + b'\x00\x00\xff\xff' == two
    assert zlib.decompress(b'\x78\x01' + two + b'\x03\x00' + zlib.adler32(seg.tobytes()).to_bytes(4, 'big')) == seg.tobytes()


def test_limited_lengths_are_optimal_under_the_limit():
    """against a brute-force reference on small alphabets: the cheapest Kraft-feasible multiset of lengths <= L, by dynamic programming"""
    rg = np.random.default_rng(4)
    for trial in range(60):
        n, L = int(rg.integers(2, 9)), int(rg.integers(3, 5))
        freq = sorted((rg.integers(1, 40, n) ** int(rg.integers(1, 4))).tolist())
        lens = D.limited_lengths(freq, L)
        assert max(lens) <= L and _kraft(lens) <= 1.0
        # the heaviest symbols get the shortest codes: choose the lengths non-increasing in weight, Kraft sum in units of 2^-L
        best = {0: 0}
        for w in sorted(freq, reverse=True):
            nxt = {}
            for used, cost in best.items():
                for l in range(1, L + 1):
                    u = used + (1 << (L - l))
                    if u <= 1 << L and (u not in nxt or nxt[u] > cost + w * l):
                        nxt[u] = cost + w * l
            best = nxt
        assert sum(f * l for f, l in zip(freq, lens)) == min(best.values()), (freq, L, lens)


def test_size_on_the_kitti_field_stays_inside_the_derived_cap_over_z_rle():
    """the synthetic field of tools/bench_kitti_flow.py at 375 x 1242, all pixels valid, 6 bytes per pixel. Cap: Z_RLE + nseg * 274 (the
    worst dynamic header 261 bytes + 5 of the stored block + 8 for a run cut at a seam)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bench_kitti_flow as B
    H, W = 375, 1242
    flow, _ = B.synth_flow(H, W, 0)
    S = B.np_filter(B.np_encode(flow, np.ones((H, W), bool)), 'nsu')[0].reshape(-1)
    nseg = -(-len(S) // SEG)
    dyn, fixed, rle, z6 = len(D.deflate_stream(S)), len(R.deflate_stream(S)), len(D.zrle(S.tobytes())), len(zlib.compress(S.tobytes(), 6))
    print('375x1242 flow: raw %d, fixed %d, dynamic %d, Z_RLE %d, zlib-6 %d; dynamic / Z_RLE %.4f, / zlib-6 %.4f, / fixed %.4f'
          % (len(S), fixed, dyn, rle, z6, dyn / rle, dyn / z6, dyn / fixed))
    assert dyn <= rle + nseg * 274
    assert dyn < fixed
