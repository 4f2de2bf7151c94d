"""NumPy restatement of the published COCO mask API (cocoapi, common/maskApi.c: rleEncode, rleToString, rleFrString, rleDecode,
rleToBbox), plus `runs_of`, the run list `vps_rle_runs` has to produce. Everything reads a mask in Fortran (column-major) order.

Not pinned to the library: pycocotools was not installed where this was written, so the restatement rests on the published
algorithm and on the known answers in KNOWN, which follow from it by hand (tests/test_rle.py compares with pycocotools wherever it
can be imported). One of them settles a point the prose descriptions of the format get wrong: `[1, 2, 3, 1]` is "123O", so the
difference to the count two places before starts at index 3 (`if (i > 2)` in rleToString), not at the third count."""
import numpy as np

# counts -> string
KNOWN = [([4], '4'), ([0, 4], '04'), ([15], '?'), ([16], '`0'), ([1, 2, 3, 1], '123O')]


def rle_encode(mask):
    """rleEncode: counts of a binary [H, W] mask: alternating zero- and one-runs in Fortran order, the first a zero-run"""
    flat = np.asarray(mask).astype(bool).ravel(order='F')
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate(([0], change, [flat.size]))
    counts = np.diff(edges).tolist()
    if flat[0]:
        counts = [0] + counts
    return counts


def rle_to_string(counts):
    """rleToString"""
    out = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5                                              # Python's >> of a negative int is arithmetic, as C's on a long
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out).decode('ascii')


def rle_from_string(s):
    """rleFrString"""
    if isinstance(s, bytes):
        s = s.decode('ascii')
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(counts, H, W):
    """rleDecode: uint8 [H, W]"""
    vals = np.arange(len(counts)) & 1
    flat = np.repeat(vals.astype(np.uint8), np.asarray(counts, dtype=np.int64))
    assert flat.size == H * W, (flat.size, H, W)
    return flat.reshape((H, W), order='F')


def to_bbox(counts, H, W):
    """rleToBbox: [x, y, w, h] with w = xmax - xmin + 1; [0, 0, 0, 0] for an empty mask"""
    m = len(counts) // 2 * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye = W, H, 0, 0
    cc = 0
    xp = 0
    for j in range(m):
        cc += int(counts[j])
        t = cc - j % 2
        y, x = t % H, (t - t % H) // H
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, H - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]


def encode(mask):
    """{'size': [H, W], 'counts': str}, pycocotools.mask.encode's result (its counts are bytes)"""
    H, W = mask.shape
    return {'size': [int(H), int(W)], 'counts': rle_to_string(rle_encode(mask))}


def runs_of(label_map):
    """(run_start uint32, run_key uint16) of an integer [H, W] map: a run starts at Fortran position 0 and wherever the label differs
    from the one before"""
    flat = np.asarray(label_map).ravel(order='F')
    start = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1))
    return start.astype(np.uint32), flat[start].astype(np.uint16)


def key_map(pan_2ch, id_channel=2):
    return pan_2ch[..., 0].astype(np.int64) * 256 + pan_2ch[..., id_channel]
