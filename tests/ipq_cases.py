"""Inputs shared by tests/golden/make_ipq_golden.py (which runs the reference's real functions on them), tests/test_ipq.py and
tests/test_ipq_gpu.py: built with fixed seeds, so the generator and the tests see the same arrays without storing them twice."""
import functools

import numpy as np


class Colors:
    """deterministic stand-in for panopticapi's IdGenerator (which draws random shades of the category colour): distinct colours in
    call order, with one deliberate repeat (the 7th call returns the 3rd colour) so that two segments can share a colour id"""

    def __init__(self):
        self.n = 0

    def get_color(self, cat_id):
        self.n += 1
        k = self.n if self.n != 7 else 3
        return [int(cat_id) * 7 % 256, k % 256, (k * 37) % 256]


class DistinctColors:
    """as `Colors` without the repeat: every segment gets its own id (what the PQ consistency checks need)"""

    def __init__(self):
        self.n = 0

    def get_color(self, cat_id):
        self.n += 1
        return [int(cat_id) * 7 % 256, self.n % 256, 1 + self.n // 256]


def _blocks(rng, H, W, C, bs):
    m = rng.integers(0, C, size=((H + bs - 1) // bs, (W + bs - 1) // bs)).astype(np.uint8)
    return np.ascontiguousarray(m.repeat(bs, 0).repeat(bs, 1)[:H, :W])


@functools.lru_cache(maxsize=None)
def confusion_inputs(C):
    """{name: (label uint8 [Hg,Wg], prediction uint8 [Hp,Wp])} for class_num C (19 or 23)"""
    rng = np.random.default_rng(100 + C)
    c = {}

    def pair(gh, gw, ph, pw, bs=6):
        gt = _blocks(rng, gh, gw, C, bs)
        gt[rng.random((gh, gw)) < 0.03] = 255                         # ignored pixels
        gt[: gh // 5, : gw // 7] = 255
        pred = _blocks(rng, ph, pw, C, max(2, bs * ph // gh))
        noise = rng.random((ph, pw)) < 0.1
        pred[noise] = rng.integers(0, C, size=int(noise.sum()))
        return gt, pred
    c['ragged'] = pair(37, 53, 19, 27)                                # width no multiple of a vector, non-integer ratio
    c['ident'] = pair(64, 128, 64, 128)
    c['half'] = pair(64, 128, 32, 64)
    c['down'] = pair(48, 64, 96, 160)
    c['uniform'] = (np.full((64, 128), 5, np.uint8), np.full((64, 128), 5, np.uint8))        # every count goes to one bin
    c['noise'] = (rng.integers(0, C, size=(64, 128)).astype(np.uint8), rng.integers(0, C, size=(48, 96)).astype(np.uint8))
    c['void'] = (np.full((37, 53), 255, np.uint8), _blocks(rng, 19, 27, C, 4))              # nothing counted
    gt, pred = pair(40, 72, 40, 72)
    gt[:10, :30] = 3; pred[:10, :30] = 25                             # C 19: idx 82 -> cell (4, 6); C 23: idx 94 -> cell (4, 2)
    gt[10:20, 20:60] = C - 1; pred[10:20, 20:60] = 255                # idx past the matrix: dropped
    gt[30:, 50:] = 40                                                 # a label value that is no class and not 255: dropped
    gt[20:30, :9] = 0; pred[20:30, :9] = C + 2                        # row 0 aliases into row 1
    c['alias'] = (gt, pred)
    return c


CATEGORIES = {c: {'id': c, 'name': 'c%d' % c, 'isthing': 1 if c >= 11 else 0} for c in range(19)}


def _rgb(m):
    return np.stack([m % 256, (m // 256) % 256, m // 65536], -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pq_images():
    H, W = 48, 160
    rng = np.random.default_rng(11)
    images = []

    def info(m, cats, crowd=()):
        return [{'id': int(k), 'category_id': int(cats[k]), 'iscrowd': 1 if k in crowd else 0, 'area': int((m == k).sum())}
                for k in cats if (m == k).any()]

    # image 0: hand-made pairs around IoU 0.5, a crowd region, a prediction over VOID
    gt = np.zeros((H, W), np.int64); pr = np.zeros((H, W), np.int64)
    gt[:, :80] = 1002; gt[:, 80:] = 1005; pr[:, :76] = 2002; pr[:, 76:] = 2005             # stuff, borders moved
    gcat = {1002: 2, 1005: 5}; pcat = {2002: 2, 2005: 5}
    for j, (dx, extra) in enumerate(((5, 0), (5, 1), (5, -1), (2, 0))):                    # 10 x 15 boxes: IoU 100/200, 101/200, 99/200, 130/170
        y, x = 2 + 11 * j, 4
        gid, pid = 5000 + j, 9000 + j
        gt[y:y + 10, x:x + 15] = gid; pr[y:y + 10, x + dx:x + dx + 15] = pid
        if extra == 1:
            pr[y, x + dx - 1] = pid                                                        # one more pixel inside the gt box
        if extra == -1:
            pr[y, x + dx] = 2002                                                           # one pixel of the intersection given away
        gcat[gid] = 11 + j % 2; pcat[pid] = 11 + j % 2
    gt[4:30, 100:150] = 6000; gcat[6000] = 13                                              # crowd region of category 13
    pr[6:20, 105:130] = 9100; pcat[9100] = 13                                              # inside the crowd: ignored
    pr[32:44, 100:120] = 9101; pcat[9101] = 13                                             # outside: a false positive
    gt[34:46, 130:158] = 0                                                                 # VOID
    pr[35:45, 128:156] = 9102; pcat[9102] = 14                                             # mostly over VOID: ignored
    pr[30:46, 121:127] = 9103; pcat[9103] = 14                                             # beside it: a false positive
    gt[40:47, 60:75] = 5100; gcat[5100] = 15; pr[40:47, 60:75] = 9104; pcat[9104] = 16    # same place, another class
    images.append(({'segments_info': info(gt, gcat, crowd=(6000,))}, {'segments_info': info(pr, pcat)}, _rgb(gt), _rgb(pr), {'id': 'a'}))

    # image 1: no predictions at all
    gt = np.zeros((H, W), np.int64); gt[:, :100] = 1001; gt[10:20, 10:40] = 5200
    images.append(({'segments_info': info(gt, {1001: 1, 5200: 12})}, {'segments_info': []}, _rgb(gt), _rgb(np.zeros((H, W), np.int64)), {'id': 'b'}))

    # images 2, 3: many moved boxes, several matches per category (the IoU sums are real float additions)
    for n in range(2):
        st = rng.integers(0, 11, size=(H // 16, W // 16)).repeat(16, 0).repeat(16, 1)
        gt = 1000 + st.astype(np.int64); pr = 2000 + st.astype(np.int64)
        gcat = {1000 + c: c for c in range(11)}; pcat = {2000 + c: (c if c != 4 else 5) for c in range(11)}
        for i in range(12):
            h, w = int(rng.integers(6, 12)), int(rng.integers(8, 20))
            y, x = int(rng.integers(0, H - h - 3)), int(rng.integers(0, W - w - 4))
            gid, pid = 5300 + i, 9300 + i
            gt[y:y + h, x:x + w] = gid; gcat[gid] = 11 + i % 4
            if i % 5 == 3:
                continue
            dy, dx = int(rng.integers(0, 3)), int(rng.integers(0, 4))
            pr[y + dy:y + dy + h, x + dx:x + dx + w] = pid; pcat[pid] = 11 + i % 4 if i % 7 != 6 else 16
        gt[:3, :7] = 0; pr[H - 2:, :5] = 0
        images.append(({'segments_info': info(gt, gcat)}, {'segments_info': info(pr, pcat)}, _rgb(gt), _rgb(pr), {'id': 'r%d' % n}))
    return images


def pq_images():
    """[(gt_json, pred_json, gt_pan uint8 [H,W,3], pred_pan, gt_image_json)]: fresh copies (the functions write into the JSON)"""
    import copy
    return copy.deepcopy(_pq_images())
