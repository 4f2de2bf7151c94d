"""Plain per-pixel restatement of the STQ definition (the contract in the docstring of vps_amd/stq.py), from the maps and the JSON
annotations, sharing no code with vps_amd/stq.py: Python dictionaries and one loop over the pixels. The definition itself is restated
from memory of the published implementation (deeplab2); what pins it are the hand-derived answers of tests/test_stq.py.

    video_tables(frames, categories)  -> the four integer tables of one video (+ the id lists)
    video_terms(tables)               -> aq_sum, n, per-class tp / fp / fn, per-track rows
    evaluate(videos, categories)      -> the whole result dict
    stq_txt(result)                   -> the text of stq.txt
"""
import math

import numpy as np


def _ids(pan):
    pan = np.asarray(pan).astype(np.int64)
    return (pan[..., 0] + 256 * pan[..., 1] + 65536 * pan[..., 2]).reshape(-1)


def id_lists(frames, categories):
    """({gt id: (class index, isthing, iscrowd)}, {pred id: (class index, isthing)}) over all frames of the video"""
    order = sorted(categories.keys())
    gt, pred = {}, {}
    for frame in frames:
        for el in frame[0]['segments_info']:
            if el['category_id'] not in categories:
                raise KeyError(el['category_id'])
            entry = (order.index(el['category_id']), int(categories[el['category_id']]['isthing'] == 1), int(el.get('iscrowd', 0) == 1))
            if el['id'] in gt and gt[el['id']] != entry:
                raise ValueError(el['id'])
            gt[el['id']] = entry
        for el in frame[1]['segments_info']:
            if el['category_id'] not in categories:
                raise KeyError(el['category_id'])
            entry = (order.index(el['category_id']), int(categories[el['category_id']]['isthing'] == 1))
            if el['id'] in pred and pred[el['id']] != entry:
                raise ValueError(el['id'])
            pred[el['id']] = entry
    return gt, pred


def video_tables(frames, categories):
    """{'gt_ids', 'pred_ids' (ascending lists), 'conf' [C][C+1], 'gt_size' [ngt], 'pred_size' [npred+1] (last cell: pixels of unlisted
    non-zero predicted ids), 'inter' [ngt][npred], 'unlisted' (sorted unlisted predicted ids)}, int64, one pixel at a time"""
    C = len(categories)
    gt, pred = id_lists(frames, categories)
    gt_ids, pred_ids = sorted(gt), sorted(pred)
    grow = {v: i for i, v in enumerate(gt_ids)}
    pcol = {v: i for i, v in enumerate(pred_ids)}
    conf = np.zeros((C, C + 1), dtype=np.int64)
    gt_size = np.zeros(len(gt_ids), dtype=np.int64)
    pred_size = np.zeros(len(pred_ids) + 1, dtype=np.int64)
    inter = np.zeros((len(gt_ids), len(pred_ids)), dtype=np.int64)
    unlisted = set()
    for frame in frames:
        G_all, P_all = _ids(frame[2]), _ids(frame[3])
        assert G_all.shape == P_all.shape
        for G, P in zip(G_all.tolist(), P_all.tolist()):
            cg, g_thing, g_crowd = C, 0, 0
            if G != 0 and G in gt:
                cg, g_thing, g_crowd = gt[G]
            cp, p_thing = C, 0
            if P != 0:
                if P in pred:
                    cp, p_thing = pred[P]
                else:
                    unlisted.add(P)
                    pred_size[len(pred_ids)] += 1
            crowd = cg != C and g_thing == 1 and g_crowd == 1
            gt_track = cg != C and g_thing == 1 and not crowd
            pred_track = cp != C and p_thing == 1 and not crowd
            if cg != C:
                conf[cg][cp] += 1
            if gt_track:
                gt_size[grow[G]] += 1
            if pred_track:
                pred_size[pcol[P]] += 1
            if gt_track and pred_track:
                inter[grow[G]][pcol[P]] += 1
    return {'gt_ids': gt_ids, 'pred_ids': pred_ids, 'gt': gt, 'conf': conf, 'gt_size': gt_size, 'pred_size': pred_size, 'inter': inter,
            'unlisted': sorted(unlisted)}


def class_counts(conf):
    C = conf.shape[0]
    tp, fp, fn = [], [], []
    for c in range(C):
        t = int(conf[c][c])
        tp.append(t)
        fp.append(sum(int(conf[r][c]) for r in range(C)) - t)
        fn.append(sum(int(conf[c][k]) for k in range(C + 1)) - t)
    return tp, fp, fn


def sq_of(conf):
    tp, fp, fn = class_counts(conf)
    ious, total, present = [], 0.0, 0
    for t, p, n in zip(tp, fp, fn):
        u = t + p + n
        ious.append(t / max(u, 1e-15))
        total += ious[-1]
        present += 1 if u > 0 else 0
    return (total / present if present else 0.0), ious


def video_terms(tab):
    """aq_sum, n, per-class counts and the per-track rows (gt id, size, score, overlapping predicted ids, best predicted id)"""
    aq_sum, n, rows = 0.0, 0, []
    for g, gid in enumerate(tab['gt_ids']):
        size = int(tab['gt_size'][g])
        if size <= 0:
            continue
        inner, overlaps, best, best_i = 0.0, 0, None, 0
        for p, pid in enumerate(tab['pred_ids']):
            i = int(tab['inter'][g][p])
            if i <= 0:
                continue
            inner += float(i) * float(i) / float(size + int(tab['pred_size'][p]) - i)
            overlaps += 1
            if i > best_i:
                best, best_i = pid, i
        aq_sum += (1.0 / size) * inner
        n += 1
        rows.append((gid, size, inner / size, overlaps, best))
    tp, fp, fn = class_counts(tab['conf'])
    return {'aq_sum': aq_sum, 'n': n, 'tp': tp, 'fp': fp, 'fn': fn, 'rows': rows}


def evaluate(videos, categories, video_ids=None):
    """videos: list of frame lists. The result dict of StqEvaluator.result(), computed independently."""
    order = sorted(categories.keys())
    C = len(order)
    conf = np.zeros((C, C + 1), dtype=np.int64)
    aq_sum, n, per_video, tracks = 0.0, 0, [], []
    for v, frames in enumerate(videos):
        vid = v if video_ids is None else video_ids[v]
        tab = video_tables(frames, categories)
        if tab['unlisted']:
            raise KeyError('Segment with ID {} is presented in PNG and not presented in JSON.'.format(tab['unlisted'][0]))
        t = video_terms(tab)
        aq_sum += t['aq_sum']
        n += t['n']
        conf += tab['conf']
        aq_v = t['aq_sum'] / max(t['n'], 1e-15)
        sq_v, _ = sq_of(tab['conf'])
        per_video.append({'video': vid, 'stq': math.sqrt(aq_v * sq_v), 'aq': aq_v, 'sq': sq_v, 'n': t['n']})
        for gid, size, score, overlaps, best in t['rows']:
            tracks.append({'video': vid, 'gt_id': gid, 'category_id': order[tab['gt'][gid][0]], 'size': size, 'score': score, 'n_pred': overlaps,
                           'best_pred_id': best})
    aq = aq_sum / max(n, 1e-15)
    sq, ious = sq_of(conf)
    tp, fp, fn = class_counts(conf)
    return {'stq': math.sqrt(aq * sq), 'aq': aq, 'sq': sq, 'n': n, 'per_video': per_video,
            'per_class_iou': {cid: ious[c] for c, cid in enumerate(order)},
            'per_class': {cid: {'iou': ious[c], 'tp': tp[c], 'fp': fp[c], 'fn': fn[c]} for c, cid in enumerate(order)}, 'tracks': tracks}


def stq_txt(result):
    """the layout of stq.txt, written out independently of vps_amd.stq.stq_text"""
    lines = ['=' * 48]
    lines.append('%-10s| %5s  %5s  %5s %5s' % ('', 'STQ', 'AQ', 'SQ', 'N'))
    lines.append('-' * 38)
    lines.append('%-10s| %5.1f  %5.1f  %5.1f %5d' % ('All', 100 * result['stq'], 100 * result['aq'], 100 * result['sq'], result['n']))
    lines.append('%-4s| %5s %9s %9s %9s' % ('IDX', 'IoU', 'TP', 'FP', 'FN'))
    for cid, r in result['per_class'].items():
        lines.append('%4d| %5.1f %9d %9d %9d' % (cid, 100 * r['iou'], r['tp'], r['fp'], r['fn']))
    lines.append('%-10s| %5s  %5s  %5s %5s' % ('VIDEO', 'STQ', 'AQ', 'SQ', 'N'))
    for r in result['per_video']:
        lines.append('%-10s| %5.1f  %5.1f  %5.1f %5d' % (str(r['video']), 100 * r['stq'], 100 * r['aq'], 100 * r['sq'], r['n']))
    return '\n'.join(lines) + '\n'
