"""The cases of the dynamic-Huffman PNG stream (tests/test_png_dyn.py on the CPU, tests/test_png_dyn_gpu.py on the device). A case is an
image; most are one grey row whose filtered stream S is a chosen byte string D behind the filter byte (`row_image`), so that a segment's
content is what the case is about. Segments are 8192 bytes of S; a case is a few segments at most."""
import functools

import numpy as np

import png_dyn_restate as D
import png_restate as R

SEG = R.SEG


def row_image(d):
    """a [1][len(d)] grey image whose filtered stream is the filter byte + d: the row is d itself where the filter rule picks None, else
    its running sum where the rule then picks Sub"""
    d = np.asarray(d, np.uint8)
    for img in (d[None, :], np.cumsum(d, dtype=np.uint64).astype(np.uint8)[None, :]):
        S, _ = R.filter_rows(img)
        if np.array_equal(S[1:], d):
            return np.ascontiguousarray(img)
    raise AssertionError('neither None nor Sub reproduces the bytes')


def peaked(n, seed, sigma=3.0):
    """the byte statistics of a filtered smooth field: small residuals around 0 / 255"""
    rg = np.random.default_rng(seed)
    return (np.rint(rg.standard_normal(n) * sigma).astype(np.int64) & 255).astype(np.uint8)


def no_two_equal(counts):
    """bytes with value i counts[i] times, no two neighbours equal (the largest count is at most half): values by falling count into the
    even places, then the odd ones"""
    order = np.argsort(-np.asarray(counts), kind='stable')
    vals = np.concatenate([np.full(counts[i], i, np.uint8) for i in order])
    out = np.empty(len(vals), np.uint8)
    half = (len(vals) + 1) // 2
    out[0::2], out[1::2] = vals[:half], vals[half:]
    assert (out[1:] != out[:-1]).all()
    return out


FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]        # sum 4180
# With end-of-block (count 1) FIB has three ones, and the ties let a Huffman tree be 9 deep as well as 17. FIB_FORCED + end-of-block is
# 1, 1, 2, 3, .., 2584 exactly: every subtree is lighter than the next leaf, every Huffman tree is 17 deep, the limit of 15 binds.
FIB_FORCED = FIB[1:] + [2584]                                                       # sum 6763


def all_symbols():
    """every byte value once, a run for the first length of each of the 29 length symbols (a literal + one match), and peaked bytes
    that make the segment's own code the shorter one: all 286 symbols are in the header"""
    parts = [peaked(5000, 12), np.arange(256, dtype=np.uint8)]
    for k, (_, first) in enumerate(R._LEN_TABLE):
        parts.append(np.full(first + 1, 17 + (k & 1), np.uint8))
    return np.concatenate(parts)


def seam_runs():
    """a run across the first seam, then runs whose matches cover 258 k + {0, 1, 2, 3} bytes, k = 1, 2, between noise"""
    parts = [peaked(8000, 21), np.full(500, 9, np.uint8)]
    for k in (1, 2):
        for j in range(4):
            parts += [peaked(11, 30 + 4 * k + j) | 1, np.full(258 * k + j + 1, 2 * j, np.uint8)]
    parts.append(peaked(300, 22))
    return np.concatenate(parts)


def cl_limit():
    """a segment whose 19 code-length counts give a Huffman tree 8 deep (found by search, checked in the CPU test)"""
    rg = np.random.default_rng(197)
    nsym = int(rg.integers(20, 200)); p = rg.random(nsym) ** rg.uniform(1, 8); p /= p.sum()
    n = int(rg.integers(600, 8192))
    return rg.choice(rg.permutation(256)[:nsym], size=n, p=p).astype(np.uint8)


def edge_segment(seed):
    """short near-uniform segments on the edge of the choice rule (found by search): dynamic minus fixed bits = -1 (10174), 0 (10676),
    +1 (10114)"""
    rg = np.random.default_rng(seed)
    n = int(rg.integers(70, 400)); k = int(rg.integers(30, 144))
    return rg.integers(0, k, n).astype(np.uint8)


EDGE = {'edge_win_1': 10174, 'edge_equal': 10676, 'edge_lose_1': 10114}


def behind_filler(seg):
    """the bytes of a case whose LAST segment is seg: 8191 filler bytes + the filter byte fill the first one"""
    return np.concatenate((peaked(SEG - 1, 5), seg))


def smooth_flow(H, W, seed=3):
    """a smooth flow plus noise, fp32 [H][W][2], for the 16-bit KITTI coding (6 bytes per pixel)"""
    rg = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u = 12.0 * np.sin(x / 17.0) + 0.05 * y + rg.standard_normal((H, W)) * 0.02
    v = 7.0 * np.cos(y / 9.0) - 0.03 * x + rg.standard_normal((H, W)) * 0.02
    return np.stack([u, v], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    rg = np.random.default_rng(11)
    c = {}
    c['n2'] = row_image([7])
    for n in (8191, 8192, 8193):
        c['n%d' % n] = row_image(peaked(n - 1, n))
    c['three_and_tail'] = row_image(peaked(3 * SEG + 37 - 1, 40))
    c['zeros'] = np.zeros((40, 700), np.uint8)
    two = np.zeros((64, 300), np.uint8); two[20:50, 100:260] = 200
    c['two_value'] = two
    c['random'] = rg.integers(0, 256, (20, 1000), dtype=np.uint8)         # whatever the filters make of it
    c['all_symbols'] = row_image(all_symbols())
    c['seam_runs'] = row_image(seam_runs())
    c['fibonacci'] = row_image(behind_filler(no_two_equal(FIB)))
    c['fibonacci_forced'] = row_image(behind_filler(no_two_equal(FIB_FORCED)))
    c['cl_limit'] = row_image(behind_filler(cl_limit()))
    for name, seed in EDGE.items():
        c[name] = row_image(behind_filler(edge_segment(seed)))
    lab = np.zeros((33, 251, 3), np.uint8)
    lab[5:20, 30:200] = (3, 120, 7); lab[15:30, 100:240] = (250, 1, 99)
    lab[::2, ::3, 1] += (peaked(17 * 84, 8, 9.0).reshape(17, 84))
    c['rgb'] = lab
    c['grey'] = np.ascontiguousarray((lab[:, :, 0] + peaked(33 * 251, 9, 2.0).reshape(33, 251)))
    return c


def last_segment(img):
    S = R.filter_rows(img)[0]
    return S[(len(S) - 1) // SEG * SEG:]


@functools.lru_cache(maxsize=None)
def restated(name):
    """the dynamic file of a case, computed once"""
    return D.png_file(cases()[name])
