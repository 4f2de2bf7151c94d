"""NumPy restatement of the boundary band and of boundary PQ / boundary VPQ (vps_amd/boundary.py), for tests/test_boundary.py and
tests/test_boundary_gpu.py.

`mask_to_boundary` is written literally as the published Boundary IoU code states it (from memory; `cv2` is not installed): pad the
mask with a ring of zeros, erode d times with a 3 x 3 kernel of ones (here a 3 x 3 minimum built from nine shifted slices), crop,
subtract. It runs per segment over boolean masks and is deliberately NOT the window formulation of the kernel, so the two pin each
other. The evaluators below count per pixel with boolean masks per segment and share no code with vps_amd/boundary.py."""
import math

import numpy as np

VOID = 0
FILL = 0xFFFFFF


def dilation(H, W, ratio=0.02):
    return max(1, int(round(ratio * math.sqrt(H * H + W * W))))


def ids_of(pan):
    q = np.asarray(pan).astype(np.int64)
    return q[:, :, 0] + 256 * q[:, :, 1] + 65536 * q[:, :, 2]


def pan_of(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def erode3x3(padded):
    """one iteration of a 3 x 3 erosion of a 0/1 array whose outer ring is zero; the ring stays zero"""
    out = np.zeros_like(padded)
    core = padded[1:-1, 1:-1].copy()
    H, W = padded.shape
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            core = np.minimum(core, padded[dy:H - 2 + dy, dx:W - 2 + dx])
    out[1:-1, 1:-1] = core
    return out


def mask_to_boundary(mask, d):
    """the band of one boolean mask: mask - erode(pad(mask), 3 x 3, iterations = d)"""
    mask = np.asarray(mask).astype(np.uint8)
    padded = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), dtype=np.uint8)
    padded[1:-1, 1:-1] = mask
    eroded = padded
    for _ in range(int(d)):
        eroded = erode3x3(eroded)
        if not eroded.any():
            break
    return (mask - eroded[1:-1, 1:-1]).astype(bool)


def band_map(pan, d):
    """what vps_boundary_band writes: per segment (id != 0) the band keeps the id and the rest of the segment becomes FILL"""
    ids = ids_of(pan)
    out = np.zeros_like(ids)
    for s in np.unique(ids):
        if s == VOID:
            continue
        m = ids == s
        b = mask_to_boundary(m, d)
        out[m] = FILL
        out[b] = s
    return pan_of(out)


class Stat:
    def __init__(self):
        self.cat = {}

    def __getitem__(self, c):
        return self.cat.setdefault(c, dict(tp=0, fp=0, fn=0, iou=0.0, biou=0.0))


def _merge(ann):
    segms = {}
    for el in ann['segments_info']:
        if el['id'] in segms:
            segms[el['id']]['area'] += el['area']
        else:
            segms[el['id']] = dict(el)
    return segms


def window_stat(frames, stat, ratio=0.02):
    """One window (1 frame = an image): `frames` are (gt_ann, pred_ann, gt_pan, pred_pan, ...). Every count is taken per pixel from
    boolean masks and summed over the frames; then the definition of the module docstring of vps_amd/boundary.py. Ground-truth areas
    come from the JSON (summed over the frames), predicted areas from the maps, as in the reference's evaluators."""
    gt_segms, pred_segms = {}, {}
    inter, binter, bg, bp = {}, {}, {}, {}
    for gt_ann, pred_ann, gt_pan, pred_pan in (f[:4] for f in frames):
        g, p = ids_of(gt_pan), ids_of(pred_pan)
        d = dilation(g.shape[0], g.shape[1], ratio) if ratio is not None else None
        for k, el in _merge(gt_ann).items():
            if k in gt_segms:
                gt_segms[k]['area'] += el['area']
            else:
                gt_segms[k] = el
        for k, el in _merge(pred_ann).items():
            el['area'] = int((p == k).sum())
            if k in pred_segms:
                pred_segms[k]['area'] += el['area']
            else:
                pred_segms[k] = el
        cut = (lambda m: mask_to_boundary(m, d)) if d is not None else (lambda m: m)      # no band: the whole mask, b_iou == mask_iou
        gb = {k: cut(g == k) for k in np.unique(g) if k != VOID}
        pb = {k: cut(p == k) for k in np.unique(p) if k != VOID}
        for k, b in gb.items():
            bg[int(k)] = bg.get(int(k), 0) + int(b.sum())
        for k, b in pb.items():
            bp[int(k)] = bp.get(int(k), 0) + int(b.sum())
        for gk in np.unique(g):
            gm = g == gk
            for pk in np.unique(p[gm]):
                key = (int(gk), int(pk))
                inter[key] = inter.get(key, 0) + int((gm & (p == pk)).sum())
                if pk != VOID:
                    both = (gm if gk == VOID else gb[gk]) & pb[pk]       # over ground-truth VOID: the band pixels of p that lie on it
                    binter[key] = binter.get(key, 0) + int(both.sum())
    gt_matched, pred_matched = set(), set()
    for (gk, pk) in sorted(inter):
        if gk not in gt_segms or pk not in pred_segms:
            continue
        if gt_segms[gk]['iscrowd'] == 1:
            continue
        if gt_segms[gk]['category_id'] != pred_segms[pk]['category_id']:
            continue
        union = pred_segms[pk]['area'] + gt_segms[gk]['area'] - inter[(gk, pk)] - inter.get((VOID, pk), 0)
        mask_iou = inter[(gk, pk)] / union
        bi = binter.get((gk, pk), 0)
        b_iou = bi / (bg[gk] + bp[pk] - bi - binter.get((VOID, pk), 0))
        iou = min(mask_iou, b_iou)
        if iou > 0.5:
            c = stat[gt_segms[gk]['category_id']]
            c['tp'] += 1; c['iou'] += iou; c['biou'] += b_iou
            gt_matched.add(gk); pred_matched.add(pk)
    crowd = {}
    for gk, info in gt_segms.items():
        if gk in gt_matched:
            continue
        if info['iscrowd'] == 1:
            crowd[info['category_id']] = gk
            continue
        stat[info['category_id']]['fn'] += 1
    for pk, info in pred_segms.items():
        if pk in pred_matched:
            continue
        over = inter.get((VOID, pk), 0)
        if info['category_id'] in crowd:
            over += inter.get((crowd[info['category_id']], pk), 0)
        if over / info['area'] > 0.5:
            continue
        stat[info['category_id']]['fp'] += 1
    return stat


def boundary_pq(frames, ratio=0.02):
    """boundary PQ statistics of images, each a window of its own"""
    stat = Stat()
    for f in frames:
        window_stat([f], stat, ratio)
    return stat


def boundary_vpq(frames, nframes, ratio=0.02):
    """boundary VPQ statistics of one clip over all windows of `nframes` frames"""
    stat = Stat()
    for i in range(len(frames) - nframes + 1):
        window_stat(frames[i:i + nframes], stat, ratio)
    return stat


def mask_pq(frames):
    """plain PQ statistics of images (the whole mask in place of the band): to show where the two measures part"""
    stat = Stat()
    for f in frames:
        window_stat([f], stat, ratio=None)
    return stat
