"""Plain per-pixel restatement of the temporal-consistency definition (the contract in the docstring of vps_amd/tc.py), sharing no code
with vps_amd/tc.py: the warp in float32 NumPy (float32 adds, np.floor), the counting as one Python loop over the pixels. The definition
itself is restated from memory of the publication and extended to track ids; what pins it are the hand-derived answers of
tests/test_tc.py.

    warp(flow)                                  -> (in view [H,W] bool, qx, qy int64 [H,W])
    pair_tables(prev, cur, flow, ...)           -> the five integer tables of one pair and its inconsistency map
    video_tables(maps, flows, ...)              -> the tables of a video (the sum over its pairs) and the per-pair list
    terms(tables)                               -> TC, TC_sem, TC_track, per-class and per-track IoU
    evaluate(videos_tables)                     -> the set's figures
"""
import math

import numpy as np


def warp(flow):
    """flow float32 [H,W,2] (x, y) -> in view, qx, qy; sx = float(x) + u, qx = floor(sx + 0.5), compared as floats"""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    H, W = flow.shape[:2]
    xs = np.arange(W, dtype=np.int64).astype(np.float32)[None, :]
    ys = np.arange(H, dtype=np.int64).astype(np.float32)[:, None]
    with np.errstate(all='ignore'):
        sx = (xs + flow[:, :, 0]).astype(np.float32)
        sy = (ys + flow[:, :, 1]).astype(np.float32)
        qx = np.floor((sx + np.float32(0.5)).astype(np.float32))
        qy = np.floor((sy + np.float32(0.5)).astype(np.float32))
        inview = (qx >= np.float32(0)) & (qx <= np.float32(W - 1)) & (qy >= np.float32(0)) & (qy <= np.float32(H - 1))
    ix = np.where(inview, qx, 0).astype(np.int64)
    iy = np.where(inview, qy, 0).astype(np.int64)
    return inview, ix, iy


def pair_tables(prev, cur, flow, seg_class, C, id_channel, keys):
    """{'conf' [C+1][C+1], 'prev_size', 'cur_size', 'same' [n], 'misc' [2] = (in view, outside), 'map' uint8 [H,W]}, int64"""
    prev, cur = np.asarray(prev), np.asarray(cur)
    assert prev.shape == cur.shape and prev.dtype == cur.dtype == np.uint8 and prev.shape[2] == 3
    H, W = cur.shape[:2]
    assert np.asarray(flow).shape[:2] == (H, W) and id_channel in (1, 2)
    index = {int(k): i for i, k in enumerate(keys)}
    assert len(index) == len(keys) and list(keys) == sorted(keys)
    n = len(keys)
    conf = np.zeros((C + 1, C + 1), dtype=np.int64)
    prev_size, cur_size, same = (np.zeros(n, dtype=np.int64) for _ in range(3))
    misc = np.zeros(2, dtype=np.int64)
    out = np.zeros((H, W), dtype=np.uint8)
    inview, ix, iy = warp(flow)
    seg_class = [int(v) for v in seg_class]
    cur_l, prev_l = cur.tolist(), prev.tolist()
    inview_l, ix_l, iy_l = inview.tolist(), ix.tolist(), iy.tolist()
    for y in range(H):
        for x in range(W):
            if not inview_l[y][x]:
                misc[1] += 1
                out[y, x] = 3
                continue
            misc[0] += 1
            a, b = cur_l[y][x], prev_l[iy_l[y][x]][ix_l[y][x]]
            ca, cb = min(seg_class[a[0]], C), min(seg_class[b[0]], C)
            conf[cb][ca] += 1
            ka, kb = index.get(a[0] * 256 + a[id_channel]), index.get(b[0] * 256 + b[id_channel])
            if ka is not None:
                cur_size[ka] += 1
            if kb is not None:
                prev_size[kb] += 1
            if ka is not None and kb is not None and ka == kb:
                same[ka] += 1
            if ca != cb:
                out[y, x] = 1
            elif ka is not None and kb is not None and ka != kb:
                out[y, x] = 2
    return {'conf': conf, 'prev_size': prev_size, 'cur_size': cur_size, 'same': same, 'misc': misc, 'map': out}


NAMES = ('conf', 'prev_size', 'cur_size', 'same', 'misc')


def flat(tab):
    """the five tables in the order they lie in one block"""
    return np.concatenate([np.asarray(tab[k]).reshape(-1) for k in NAMES])


def video_tables(maps, flows, seg_class, C, id_channel, keys):
    """(the video's tables = the sum over its pairs, [the tables of pair 1, 2, ..]); flows[t] belongs to (maps[t-1], maps[t])"""
    pairs = [pair_tables(maps[t - 1], maps[t], flows[t], seg_class, C, id_channel, keys) for t in range(1, len(maps))]
    n = len(keys)
    total = {'conf': np.zeros((C + 1, C + 1), dtype=np.int64), 'prev_size': np.zeros(n, dtype=np.int64), 'cur_size': np.zeros(n, dtype=np.int64),
             'same': np.zeros(n, dtype=np.int64), 'misc': np.zeros(2, dtype=np.int64)}
    for p in pairs:
        for k in NAMES:
            total[k] = total[k] + p[k]
    return total, pairs


def class_ious(conf):
    C = len(conf) - 1
    rows = []
    for c in range(C):
        inter = int(conf[c][c])
        union = sum(int(conf[c][k]) for k in range(C + 1)) + sum(int(conf[r][c]) for r in range(C + 1)) - inter
        rows.append((inter, union, inter / union if union > 0 else 0.0))
    return rows


def track_ious(tab):
    rows = []
    for k in range(len(tab['same'])):
        s = int(tab['same'][k])
        union = int(tab['prev_size'][k]) + int(tab['cur_size'][k]) - s
        rows.append((s, union, s / union if union > 0 else 0.0))
    return rows


def _mean_present(rows):
    present = [r[2] for r in rows if r[1] > 0]
    return (sum(present) / len(present) if present else 0.0), len(present)


def terms(tab):
    """{'tc', 'tc_sem', 'tc_track', 'n_classes', 'n_tracks', 'class_rows', 'track_rows' [(inter, union, iou)], 'in_view', 'outside'}"""
    crow, trow = class_ious(tab['conf']), track_ious(tab)
    sem, nc = _mean_present(crow)
    trk, nt = _mean_present(trow)
    return {'tc': math.sqrt(sem * trk), 'tc_sem': sem, 'tc_track': trk, 'n_classes': nc, 'n_tracks': nt, 'class_rows': crow, 'track_rows': trow,
            'in_view': int(tab['misc'][0]), 'outside': int(tab['misc'][1])}


def evaluate(videos):
    """videos: the tables of every video -> the set's (tc, tc_sem, tc_track): the matrices summed, the tracks of all videos together"""
    conf = sum(np.asarray(v['conf']) for v in videos)
    trow = [r for v in videos for r in track_ious(v)]
    sem, _ = _mean_present(class_ious(conf))
    trk, nt = _mean_present(trow)
    return {'tc': math.sqrt(sem * trk), 'tc_sem': sem, 'tc_track': trk, 'n_tracks': nt}
