"""STQ (Segmentation and Tracking Quality; Weber et al., "STEP: Segmenting and Tracking Every Pixel", NeurIPS 2021 datasets track)
from the files `eval_vpq` reads, with the per-pixel counting on the device.

The reference has no STQ. The definition below is RESTATED FROM MEMORY of the published implementation (deeplab2
`segmentation_and_tracking_quality.py`), which is not available where this was written; it is pinned only by five hand-derived
answers (tests/test_stq.py) and by an independent per-pixel restatement (tests/stq_restate.py), not by a run of the original.

Input, per video: the frames `(gt_json_ann, pred_json_ann, gt_pan, pred_pan[, ...])` of `evaluate.vpq_compute_single_core`; maps are
uint8 [H,W,3], segment id = R + 256 G + 65536 B. Class index c = position of the category id in the ascending list of ids, 0 .. C-1;
index C is void; C <= 63.

Video-level id tables (host, from ALL frames): the sorted unique ids of every `segments_info` entry with (class index, isthing,
iscrowd) - `iscrowd` for the ground truth only.

Per pixel, G = gt id, P = predicted id:
    cg = class of G, void if G == 0 or G is not listed;  cp = class of P, void if P == 0
    a non-zero P that is not listed is an error: the device counts it in an overflow cell (and as void in the confusion matrix),
    `add_video` raises KeyError for the smallest such id once the video is counted
    crowd = cg is a thing class and G has iscrowd == 1;  gt_track = cg thing and not crowd;  pred_track = cp thing and not crowd
    cg != void: conf[cg][cp] += 1   (cp may be C; crowd pixels count under their class)
    gt_track:   gt_size[G] += 1;    pred_track: pred_size[P] += 1;    both: inter[G][P] += 1   (the classes need not agree)

Result, float64, sums over ascending g then ascending p, videos in the order they were added:
    aq_sum_v = sum_{g: gt_size[g] > 0} (1 / gt_size[g]) sum_{p: inter[g][p] > 0} inter[g][p]^2 / (gt_size[g] + pred_size[p] - inter[g][p])
    n_v = #{g: gt_size[g] > 0};  AQ_v = aq_sum_v / max(n_v, 1e-15);  AQ = sum_v aq_sum_v / max(sum_v n_v, 1e-15)
    per class c < C: tp = conf[c][c], fp = sum_{r<C} conf[r][c] - tp, fn = sum_{k<=C} conf[c][k] - tp, u = tp + fp + fn
    SQ = (sum_c tp / max(u, 1e-15)) / #{c: u > 0}   (SQ_v on the video's matrix, SQ on the sum of all videos' matrices)
    STQ = sqrt(AQ SQ), STQ_v = sqrt(AQ_v SQ_v)

`stq_from_tables`, `StqStats` and `stq_text` are NumPy / Python only. The counting (`StqEvaluator`) is `vps_stq_accumulate`
(csrc/stq_ops.hip): no CPU path, the HIP library must load and a device must be present; host maps are uploaded."""
import math

import numpy as np
import torch

from . import hip

VOID = 0
MAX_CLASSES = 63
INFO_THING, INFO_CROWD = 64, 128


def class_indices(categories):
    """{category id: class index}: the position of the id in the ascending list of ids"""
    ids = sorted(categories)
    if not 1 <= len(ids) <= MAX_CLASSES:
        raise ValueError('STQ takes 1..%d categories, got %d' % (MAX_CLASSES, len(ids)))
    return {cid: i for i, cid in enumerate(ids)}


def build_id_tables(frames, categories):
    """The video-level id tables of `frames` (tuples whose first two entries are the gt and the predicted annotation).
    Returns (gt_ids uint32 [ngt], gt_info uint8 [ngt], pred_ids uint32 [npred], pred_info uint8 [npred]), ids ascending; info byte:
    bits 0-5 class index, bit 6 thing, bit 7 crowd (gt only). ValueError: an id listed with two categories or two `iscrowd` values in
    one video (or outside 0 .. 2^24-1); KeyError: a `category_id` that `categories` does not have."""
    cls = class_indices(categories)

    def table(which, with_crowd):
        seen = {}
        for frame in frames:
            for el in frame[which]['segments_info']:
                sid, cat = int(el['id']), el['category_id']
                if cat not in categories:
                    raise KeyError('Segment with ID {} has unknown category_id {}.'.format(sid, cat))
                if not 0 <= sid < (1 << 24):
                    raise ValueError('segment id {} is outside 0 .. 2^24-1'.format(sid))
                info = cls[cat] | (INFO_THING if categories[cat]['isthing'] == 1 else 0)
                if with_crowd and int(el.get('iscrowd', 0)) == 1:
                    info |= INFO_CROWD
                if seen.setdefault(sid, (info, cat)) != (info, cat):
                    raise ValueError('Segment with ID {} is listed with two different categories or iscrowd values in one video.'.format(sid))
        ids = sorted(seen)
        return np.array(ids, dtype=np.uint32), np.array([seen[i][0] for i in ids], dtype=np.uint8)

    gt_ids, gt_info = table(0, True)
    pred_ids, pred_info = table(1, False)
    return gt_ids, gt_info, pred_ids, pred_info


def stq_from_tables(conf, gt_size, pred_size, inter):
    """One video's (or one set's) tables -> {'aq_sum', 'n', 'tp', 'fp', 'fn', 'track_scores', 'track_overlaps', 'track_best'}.
    conf [C][C+1], gt_size [ngt], pred_size [npred] (a trailing overflow cell is ignored), inter [ngt][npred], integers.
    tp / fp / fn: int64 [C]. track_scores: float64 [ngt], the inner sum divided by the size (0 where the size is 0); track_overlaps:
    how many predicted ids intersect the track; track_best: column of the largest intersection (the lowest on a tie), -1 if none."""
    conf = np.asarray(conf, dtype=np.int64)
    gt_size = np.asarray(gt_size, dtype=np.int64).reshape(-1)
    inter = np.asarray(inter, dtype=np.int64).reshape(len(gt_size), -1)
    pred_size = np.asarray(pred_size, dtype=np.int64).reshape(-1)[:inter.shape[1]]
    C = conf.shape[0]
    assert conf.shape == (C, C + 1) and len(pred_size) == inter.shape[1]
    scores = np.zeros(len(gt_size), dtype=np.float64)
    overlaps = np.zeros(len(gt_size), dtype=np.int64)
    best = np.full(len(gt_size), -1, dtype=np.int64)
    aq_sum, n = 0.0, 0
    for g in np.nonzero(gt_size > 0)[0]:                       # ascending g, then ascending p
        gs = float(gt_size[g])
        inner = 0.0
        cols = np.nonzero(inter[g] > 0)[0]
        for p in cols:
            i = float(inter[g, p])
            inner += i * i / (gs + float(pred_size[p]) - i)
        scores[g] = inner / gs
        overlaps[g] = len(cols)
        if len(cols):
            best[g] = int(np.argmax(inter[g]))
        aq_sum += scores[g]
        n += 1
    tp = np.diag(conf[:, :C]).copy()
    fp = conf[:, :C].sum(0) - tp
    fn = conf.sum(1) - tp
    return {'aq_sum': aq_sum, 'n': n, 'tp': tp, 'fp': fp, 'fn': fn, 'track_scores': scores, 'track_overlaps': overlaps, 'track_best': best}


def sq_from_counts(tp, fp, fn):
    """(SQ, per-class IoU float64 [C]) of the per-class counts"""
    ious = np.zeros(len(tp), dtype=np.float64)
    total, classes = 0.0, 0
    for c in range(len(tp)):
        u = int(tp[c]) + int(fp[c]) + int(fn[c])
        ious[c] = float(tp[c]) / max(float(u), 1e-15)
        total += ious[c]
        classes += u > 0
    return (total / classes if classes else 0.0), ious


class StqStats:
    """Host side of the evaluation: collects the downloaded tables of every video and turns them into the result. No device."""

    def __init__(self, categories):
        self.categories = categories
        self.class_of = class_indices(categories)
        self.cat_ids = sorted(categories)
        self.num_classes = len(self.cat_ids)
        self.videos = []

    def add_tables(self, video_id, gt_ids, gt_info, pred_ids, conf, gt_size, pred_size, inter):
        C = self.num_classes
        conf = np.asarray(conf, dtype=np.int64).reshape(C, C + 1)
        inter = np.asarray(inter, dtype=np.int64).reshape(len(gt_ids), len(pred_ids))
        st = stq_from_tables(conf, gt_size, pred_size, inter)
        st.update(video=len(self.videos) if video_id is None else video_id, conf=conf, gt_ids=np.asarray(gt_ids), gt_info=np.asarray(gt_info),
                  pred_ids=np.asarray(pred_ids), gt_size=np.asarray(gt_size, dtype=np.int64),
                  pred_size=np.asarray(pred_size, dtype=np.int64)[:len(pred_ids)], inter=inter)
        self.videos.append(st)
        return st

    def result(self):
        """{'stq', 'aq', 'sq', 'per_video': [{'video', 'stq', 'aq', 'sq', 'n'}], 'per_class_iou': {category id: IoU},
        'per_class': {category id: {'iou', 'tp', 'fp', 'fn'}}, 'tracks': [{'video', 'gt_id', 'category_id', 'size', 'score',
        'n_pred', 'best_pred_id'}]}; `tracks` lists every ground-truth track with pixels, per video in ascending id"""
        C = self.num_classes
        conf = np.zeros((C, C + 1), dtype=np.int64)
        aq_sum, n, per_video, tracks = 0.0, 0, [], []
        for st in self.videos:
            aq_sum += st['aq_sum']; n += st['n']; conf += st['conf']
            aq_v = st['aq_sum'] / max(st['n'], 1e-15)
            sq_v, _ = sq_from_counts(st['tp'], st['fp'], st['fn'])
            per_video.append({'video': st['video'], 'stq': math.sqrt(aq_v * sq_v), 'aq': aq_v, 'sq': sq_v, 'n': st['n']})
            for g in np.nonzero(st['gt_size'] > 0)[0]:
                b = int(st['track_best'][g])
                tracks.append({'video': st['video'], 'gt_id': int(st['gt_ids'][g]), 'category_id': self.cat_ids[int(st['gt_info'][g]) & 63],
                               'size': int(st['gt_size'][g]), 'score': float(st['track_scores'][g]), 'n_pred': int(st['track_overlaps'][g]),
                               'best_pred_id': int(st['pred_ids'][b]) if b >= 0 else None})
        aq = aq_sum / max(n, 1e-15)
        tp = np.diag(conf[:, :C]).copy()
        fp = conf[:, :C].sum(0) - tp
        fn = conf.sum(1) - tp
        sq, ious = sq_from_counts(tp, fp, fn)
        return {'stq': math.sqrt(aq * sq), 'aq': aq, 'sq': sq, 'n': n, 'per_video': per_video,
                'per_class_iou': {cid: float(ious[c]) for c, cid in enumerate(self.cat_ids)},
                'per_class': {cid: {'iou': float(ious[c]), 'tp': int(tp[c]), 'fp': int(fp[c]), 'fn': int(fn[c])} for c, cid in enumerate(self.cat_ids)},
                'tracks': tracks}


def stq_text(result):
    """the text of stq.txt: the set's STQ / AQ / SQ x100 with the number of tracks, the per-class IoU rows, the per-video rows"""
    out = []
    out.append('=' * 48 + '\n')
    out.append('{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}\n'.format('', 'STQ', 'AQ', 'SQ', 'N'))
    out.append('-' * (10 + 7 * 4) + '\n')
    out.append('{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n'.format('All', 100 * result['stq'], 100 * result['aq'], 100 * result['sq'], result['n']))
    out.append('{:4s}| {:>5s} {:>9s} {:>9s} {:>9s}\n'.format('IDX', 'IoU', 'TP', 'FP', 'FN'))
    for idx, r in result['per_class'].items():
        out.append('{:4d}| {:5.1f} {:9d} {:9d} {:9d}\n'.format(idx, 100 * r['iou'], r['tp'], r['fp'], r['fn']))
    out.append('{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}\n'.format('VIDEO', 'STQ', 'AQ', 'SQ', 'N'))
    for r in result['per_video']:
        out.append('{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n'.format(str(r['video']), 100 * r['stq'], 100 * r['aq'], 100 * r['sq'], r['n']))
    return ''.join(out)


class StqEvaluator(StqStats):
    """The device side: `add_video` counts one video into tables that stay on the device until its last frame is enqueued
    (`vps_stq_accumulate` per frame, no synchronisation between frames, one download per video); `result` is `StqStats.result`."""

    def __init__(self, categories, device='cuda'):
        super().__init__(categories)
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise hip.VpsHipError('StqEvaluator counts on the device (vps_stq_accumulate); there is no CPU path and no device is present')
        self.lib = hip.load()

    def _map(self, m):
        t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
        t = t.to(self.device).contiguous()
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, 'panoptic PNG as uint8 [H,W,3]'
        return t

    def count_video(self, frames):
        """the id tables and the DEVICE tables of one video, all frames enqueued, nothing downloaded:
        ((gt_ids, gt_info, pred_ids, pred_info), int64 tensor conf | gt_size | pred_size | inter, the uploaded prediction maps)"""
        dev, C = self.device, self.num_classes
        ids = build_id_tables(frames, self.categories)
        gt_ids, gt_info, pred_ids, pred_info = ids
        ngt, npred = len(gt_ids), len(pred_ids)
        # (ids are below 2^24: the int32 view of the uint32 arrays holds the same bits)
        d_ids = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in ids]
        sizes = [C * (C + 1), ngt, npred + 1, ngt * npred]
        tables = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)              # the video's tables, zeroed once
        conf, gsz, psz, inter = torch.split(tables, sizes)
        preds = []
        for frame in frames:                                                         # no synchronisation between frames
            g, p = self._map(frame[2]), self._map(frame[3])
            assert g.shape == p.shape
            hip.check(self.lib.vps_stq_accumulate(hip.ptr(g), hip.ptr(p), g.shape[0] * g.shape[1], hip.ptr(d_ids[0]) if ngt else None,
                                                  hip.ptr(d_ids[1]) if ngt else None, ngt, hip.ptr(d_ids[2]) if npred else None,
                                                  hip.ptr(d_ids[3]) if npred else None, npred, C, hip.ptr(conf), hip.ptr(gsz) if ngt else None,
                                                  hip.ptr(psz), hip.ptr(inter) if ngt and npred else None, hip.stream_ptr()),
                      'vps_stq_accumulate')
            preds.append(p)
        return ids, tables, preds

    def add_video(self, frames, video_id=None):
        """frames: [(gt_json_ann, pred_json_ann, gt_pan, pred_pan, ...)] of one video, maps as uint8 [H,W,3] host arrays or device
        tensors. Returns the video's entry (its tables and `stq_from_tables` of them)."""
        C = self.num_classes
        (gt_ids, gt_info, pred_ids, pred_info), tables, preds = self.count_video(frames)
        ngt, npred = len(gt_ids), len(pred_ids)
        host = tables.cpu().numpy()                                                  # the one download (and synchronisation) of the video
        conf, gsz, psz, inter = np.split(host, np.cumsum([C * (C + 1), ngt, npred + 1]))
        if psz[npred] > 0:                                                           # a predicted id that is neither listed nor VOID
            listed = set(int(v) for v in pred_ids)
            bad = set()
            for p in preds:
                q = p.cpu().numpy().astype(np.int64)
                bad.update(int(v) for v in np.unique(q[:, :, 0] + q[:, :, 1] * 256 + q[:, :, 2] * 65536) if v != VOID and int(v) not in listed)
            raise KeyError('Segment with ID {} is presented in PNG and not presented in JSON.'.format(min(bad)))
        return self.add_tables(video_id, gt_ids, gt_info, pred_ids, conf, gsz, psz, inter)
