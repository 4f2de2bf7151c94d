"""Boundary PQ and boundary VPQ: panoptic quality that scores a matched pair by min(mask IoU, boundary IoU), with the boundary band
of every segment cut on the device (csrc/boundary_ops.hip).

The reference has no boundary measure. What follows is THIS REPOSITORY'S definition, RESTATED FROM MEMORY of the published Boundary
IoU / Boundary PQ code (Cheng, Girshick, Dollar, Berg, Kirillov, "Boundary IoU: Improving Object-Centric Image Segmentation
Evaluation", CVPR 2021; `boundary_iou_api`). Neither that code nor `cv2` nor `panopticapi` is installed where this was written: the
definition is pinned by hand-derived answers (tests/test_boundary.py) and by an independent per-segment erosion and per-pixel
restatement (tests/boundary_restate.py), not by a run of the original.

Band. d = max(1, int(round(ratio * sqrt(H^2 + W^2)))), ratio 0.02 (46 at 1024 x 2048), taken per frame from that frame's size. The band of
a segment is `mask_to_boundary(mask, d)` of the published code: the mask padded with one ring of zeros, eroded d times with a 3 x 3
kernel of ones, cropped, and subtracted from the mask. The zero ring never erodes away, so the image border always erodes. For all
segments of a map at once (`boundary_band` -> `vps_boundary_band`): a pixel of id s != 0 is INTERIOR when the whole (2d+1) x (2d+1)
window centred on it lies inside the image and holds s alone; interior pixels become FILL = 0xFFFFFF, every other pixel (the band) keeps
its id, VOID (0) stays 0 and is never banded. The id 0xFFFFFF is therefore reserved: a JSON that lists it is refused (ValueError).

Boundary PQ (`pq_compute_single_core`, the twin of `ipq.pq_compute_single_core`). Per image `vps_pair_count` runs twice with the same id
lists: on the two maps and on the two band maps; in the band table FILL is unlisted and lands in the extra row / column. For a
candidate pair (g, p) that passes the existing filters (both listed, g not crowd, same category), visited in ascending (g, p):
    mask_iou = the reference's: inter / (area_p + area_g - inter - |p over gt VOID|)
    bi = band pixels of g that are band pixels of p;  bg, bp = band sizes of g and of p (all of the segment's band pixels in the map);
    bv = band pixels of p over ground-truth VOID;  b_iou = bi / (bg + bp - bi - bv)
    iou = min(mask_iou, b_iou);  true positive when iou > 0.5, and that iou is what is summed into SQ
FN, FP and the crowd / void rule for FP are unchanged and use mask areas. The mean b_iou of the matched pairs is reported beside.

Boundary VPQ (`vpq_compute_single_core`, the twin of `evaluate.vpq_compute_single_core`). Every count above - bi, bg, bp, bv like the
mask counts - is summed over the frames of the window before the divisions: a tube boundary IoU. NO PUBLICATION DEFINES IT; it is the
natural extension of tube matching and is this repository's own.

`dilation`, the statistics classes and the text writers are Python only. The band and the counts have no CPU path: the HIP library
must load and a device must be present; host maps are uploaded."""
import copy
import math
import os
from collections import defaultdict

import numpy as np
import torch

from . import hip
from .evaluate import VOID, FrameCounts, PQStat, PQStatCat

FILL = 0xFFFFFF
MAX_D = 255


def dilation(H, W, ratio=0.02):
    """the published rule: the band's width in pixels from the image diagonal"""
    return max(1, int(round(ratio * math.sqrt(H * H + W * W))))


def check_reserved(*anns):
    """ValueError when an annotation lists the fill id"""
    for ann in anns:
        for el in ann['segments_info']:
            if int(el['id']) == FILL:
                raise ValueError('segment id 0xFFFFFF (16777215) is reserved for the interior fill of the boundary band')


def _up(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = t.to(dev).contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, 'panoptic PNG as uint8 [H,W,3]'
    return t


def band_workspace_bytes(H, W, d):
    n = hip.c_int64(0)
    hip.check(hip.load().vps_boundary_band_ws(int(H), int(W), int(d), hip.byref(n)), 'vps_boundary_band_ws')
    return int(n.value)


def boundary_band(pan, d=None, ratio=0.02, device='cuda'):
    """The band map of a panoptic map (device or NumPy uint8 [H,W,3]): a device uint8 [H,W,3] tensor in which the interior of every
    segment is FILL. `d` defaults to `dilation(H, W, ratio)`. Enqueued on the current stream, no synchronisation."""
    dev = pan.device if torch.is_tensor(pan) and pan.is_cuda else torch.device(device)
    t = _up(pan, dev)
    H, W = int(t.shape[0]), int(t.shape[1])
    d = dilation(H, W, ratio) if d is None else int(d)
    if not 1 <= d <= MAX_D:
        raise ValueError('boundary band width d = %d is outside 1..%d' % (d, MAX_D))
    ws = torch.empty(band_workspace_bytes(H, W, d), dtype=torch.uint8, device=dev)
    out = torch.empty_like(t)
    hip.check(hip.load().vps_boundary_band(hip.ptr(t), H, W, d, hip.ptr(out), hip.ptr(ws), ws.numel(), hip.stream_ptr()), 'vps_boundary_band')
    return out


class BPQStatCat(PQStatCat):
    """PQStatCat plus `biou`, the sum of the boundary IoU of the matched pairs"""

    def __init__(self):
        super().__init__()
        self.biou = 0.0

    def __iadd__(self, other):
        super().__iadd__(other)
        self.biou += getattr(other, 'biou', 0.0)
        return self


class BPQStat(PQStat):
    def __init__(self):
        self.pq_per_cat = defaultdict(BPQStatCat)


def _pair_table(g, p, gt_ids, pred_ids, dev):
    """`vps_pair_count` of two maps over the id lists -> int64 [ngt+1][npred+1] on the host"""
    gi = torch.from_numpy(gt_ids.astype(np.int32)).to(dev); pi = torch.from_numpy(pred_ids.astype(np.int32)).to(dev)   # ids < 2^24
    counts = torch.empty((len(gt_ids) + 1) * (len(pred_ids) + 1), dtype=torch.int32, device=dev)
    hip.check(hip.load().vps_pair_count(hip.ptr(g), hip.ptr(p), g.shape[0] * g.shape[1], hip.ptr(gi), len(gt_ids), hip.ptr(pi), len(pred_ids),
                                        hip.ptr(counts), hip.stream_ptr()), 'vps_pair_count')
    return counts.view(len(gt_ids) + 1, len(pred_ids) + 1).cpu().numpy().astype(np.int64)


def band_counts(g, p, gt_ids, pred_ids, ratio, dev):
    """The band table of one frame: (bpairs {(gt id, pred id): band pixels of both}, bg {gt id: band size}, bp {pred id: band size})
    over the listed ids. A band size counts ALL band pixels of the segment: the row / column sum with the extra column / row, where
    the other map's fill and unlisted ids land."""
    d = dilation(int(g.shape[0]), int(g.shape[1]), ratio)
    tab = _pair_table(boundary_band(g, d), boundary_band(p, d), gt_ids, pred_ids, dev)
    bpairs = {}
    rows, cols = np.nonzero(tab[:-1, :-1])
    for r, c in zip(rows, cols):
        bpairs[(int(gt_ids[r]), int(pred_ids[c]))] = int(tab[r, c])
    bg = {int(i): int(v) for i, v in zip(gt_ids, tab[:-1].sum(1))}
    bp = {int(i): int(v) for i, v in zip(pred_ids, tab[:, :-1].sum(0))}
    return bpairs, bg, bp


def _boundary_iou(gt_label, pred_label, bpairs, bg, bp):
    bi = bpairs.get((gt_label, pred_label), 0)
    return bi / (bg[gt_label] + bp[pred_label] - bi - bpairs.get((VOID, pred_label), 0))


# ------------------------------------------------------------------------------------------------------------------
# Boundary PQ of images
# ------------------------------------------------------------------------------------------------------------------
def pq_compute_single_core(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons, categories, device='cuda', boundary_ratio=0.02):
    """The boundary twin of `ipq.pq_compute_single_core`: same arguments, a `BPQStat`. The bookkeeping statements are that function's;
    a pair is scored with min(mask IoU, boundary IoU) (module docstring)."""
    gt_jsons, pred_jsons = list(gt_jsons), list(pred_jsons)
    check_reserved(*gt_jsons, *pred_jsons)
    hip.load()
    dev = torch.device(device)
    pq_stat = BPQStat()
    for gt_json, pred_json, gt_pan, pred_pan, gt_image_json in zip(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons):
        g, p = _up(gt_pan, dev), _up(pred_pan, dev)
        assert g.shape == p.shape
        image_id = gt_image_json.get('id') if isinstance(gt_image_json, dict) else None
        gt_segms = {el['id']: el for el in gt_json['segments_info']}
        pred_segms = {el['id']: copy.copy(el) for el in pred_json['segments_info']}
        gt_ids = np.unique(np.array([VOID] + list(gt_segms), dtype=np.int64))
        pred_ids = np.unique(np.array([VOID] + list(pred_segms), dtype=np.int64))
        tab = _pair_table(g, p, gt_ids, pred_ids, dev)
        if tab[:, -1].sum() > 0:                               # a predicted id that is neither listed nor VOID
            ids = (lambda q: q[:, :, 0] + q[:, :, 1] * 256 + q[:, :, 2] * 65536)(p.cpu().numpy().astype(np.int64))
            bad = [int(v) for v in np.unique(ids) if v not in pred_segms and v != VOID]
            raise KeyError('In the image with ID {} segment with ID {} is presented in PNG and not presented in JSON.'.format(image_id, bad[0]))
        col = tab.sum(0)
        pred_labels_set = set(el['id'] for el in pred_json['segments_info'])
        for j, label in enumerate(pred_ids):
            label = int(label)
            if col[j] == 0 or label not in pred_segms:
                continue
            pred_segms[label]['area'] = int(col[j])
            pred_labels_set.remove(label)
            if pred_segms[label]['category_id'] not in categories:
                raise KeyError('In the image with ID {} segment with ID {} has unknown category_id {}.'.format(
                    image_id, label, pred_segms[label]['category_id']))
        if len(pred_labels_set) != 0:
            raise KeyError('In the image with ID {} the following segment IDs {} are presented in JSON and not presented in PNG.'.format(
                image_id, list(pred_labels_set)))
        gt_pred_map = {}
        rows, cols = np.nonzero(tab[:-1, :-1])                 # row-major: ascending gt id, then pred id
        for r, c in zip(rows, cols):
            gt_pred_map[(int(gt_ids[r]), int(pred_ids[c]))] = int(tab[r, c])
        bpairs, bg, bp = band_counts(g, p, gt_ids, pred_ids, boundary_ratio, dev)

        gt_matched, pred_matched = set(), set()
        for (gt_label, pred_label), intersection in gt_pred_map.items():
            if gt_label not in gt_segms:
                continue
            if pred_label not in pred_segms:
                continue
            if gt_segms[gt_label]['iscrowd'] == 1:
                continue
            if gt_segms[gt_label]['category_id'] != pred_segms[pred_label]['category_id']:
                continue
            union = pred_segms[pred_label]['area'] + gt_segms[gt_label]['area'] - intersection - gt_pred_map.get((VOID, pred_label), 0)
            b_iou = _boundary_iou(gt_label, pred_label, bpairs, bg, bp)
            iou = min(intersection / union, b_iou)
            if iou > 0.5:
                cat = pq_stat[gt_segms[gt_label]['category_id']]
                cat.tp += 1
                cat.iou += iou
                cat.biou += b_iou
                gt_matched.add(gt_label)
                pred_matched.add(pred_label)

        crowd_labels_dict = {}
        for gt_label, gt_info in gt_segms.items():
            if gt_label in gt_matched:
                continue
            if gt_info['iscrowd'] == 1:
                crowd_labels_dict[gt_info['category_id']] = gt_label
                continue
            pq_stat[gt_info['category_id']].fn += 1

        for pred_label, pred_info in pred_segms.items():
            if pred_label in pred_matched:
                continue
            intersection = gt_pred_map.get((VOID, pred_label), 0)
            if pred_info['category_id'] in crowd_labels_dict:
                intersection += gt_pred_map.get((crowd_labels_dict[pred_info['category_id']], pred_label), 0)
            if intersection / pred_info['area'] > 0.5:
                continue
            pq_stat[pred_info['category_id']].fp += 1
    return pq_stat


# ------------------------------------------------------------------------------------------------------------------
# Boundary VPQ of a clip
# ------------------------------------------------------------------------------------------------------------------
def vpq_compute_single_core(gt_pred_set, categories, nframes=2, device='cuda', _cache=None, boundary_ratio=0.02):
    """The boundary twin of `evaluate.vpq_compute_single_core`: same arguments, a `BPQStat`. Every frame is counted once (`_cache` as
    there): `FrameCounts.count` for the masks, `band_counts` for the bands; a window sums both before the divisions."""
    check_reserved(*[a for item in gt_pred_set for a in item[:2]])
    fc = FrameCounts(device)
    dev = torch.device(device)
    cache = {} if _cache is None else _cache
    stat = BPQStat()
    clip_gt_ids = sorted({el['id'] for item in gt_pred_set for el in item[0]['segments_info']})
    for idx in range(0, len(gt_pred_set) - nframes + 1):
        gts, preds, gt_pred_map, bpairs, bg, bp = [], [], {}, {}, {}, {}
        for off, (gt_json, pred_json, gt_pan, pred_pan, _) in enumerate(gt_pred_set[idx:idx + nframes]):
            key = (id(gt_pred_set), idx + off, 'boundary', float(boundary_ratio))
            ent = cache.get(key)
            if ent is None or ent[0] is not gt_pred_set:       # keyed by the clip OBJECT, as in evaluate.vpq_compute_single_core
                g, p = _up(gt_pan, dev), _up(pred_pan, dev)
                # the id lists of FrameCounts.count
                gt_ids = np.unique(np.array([VOID] + [el['id'] for el in gt_json['segments_info']] + list(clip_gt_ids), dtype=np.int64))
                pred_ids = np.unique(np.array([VOID] + [el['id'] for el in pred_json['segments_info']], dtype=np.int64))
                ent = cache[key] = (gt_pred_set, fc.count(gt_json, pred_json, g, p, categories, clip_gt_ids),
                                    band_counts(g, p, gt_ids, pred_ids, boundary_ratio, dev))
            gs, ps, pairs = ent[1]
            gts.append(copy.deepcopy(gs)); preds.append(copy.deepcopy(ps))
            for k, v in pairs.items():
                gt_pred_map[k] = gt_pred_map.get(k, 0) + v
            for src, dst in zip(ent[2], (bpairs, bg, bp)):
                for k, v in src.items():
                    dst[k] = dst.get(k, 0) + v
        vid_gt, vid_pred = {}, {}
        for segms, vid in [(s, vid_gt) for s in gts] + [(s, vid_pred) for s in preds]:
            for k in segms.keys():
                if k not in vid:
                    vid[k] = segms[k]
                else:
                    vid[k]['area'] += segms[k]['area']
        gt_pred_map = dict(sorted(gt_pred_map.items()))        # ascending gt id, then pred id
        gt_matched, pred_matched = set(), set()
        for (gt_label, pred_label), intersection in gt_pred_map.items():
            if gt_label not in vid_gt or pred_label not in vid_pred:
                continue
            if vid_gt[gt_label]['iscrowd'] == 1:
                continue
            if vid_gt[gt_label]['category_id'] != vid_pred[pred_label]['category_id']:
                continue
            union = vid_pred[pred_label]['area'] + vid_gt[gt_label]['area'] - intersection - gt_pred_map.get((VOID, pred_label), 0)
            mask_iou = intersection / union
            assert mask_iou <= 1.0, 'INVALID IOU VALUE : %d' % (gt_label)
            b_iou = _boundary_iou(gt_label, pred_label, bpairs, bg, bp)
            iou = min(mask_iou, b_iou)
            if iou > 0.5:
                cat = stat[vid_gt[gt_label]['category_id']]
                cat.tp += 1
                cat.iou += iou
                cat.biou += b_iou
                gt_matched.add(gt_label); pred_matched.add(pred_label)
        crowd = {}
        for gt_label, info in vid_gt.items():
            if gt_label in gt_matched:
                continue
            if info['iscrowd'] == 1:
                crowd[info['category_id']] = gt_label
                continue
            stat[info['category_id']].fn += 1
        for pred_label, info in vid_pred.items():
            if pred_label in pred_matched:
                continue
            inter = gt_pred_map.get((VOID, pred_label), 0)
            if info['category_id'] in crowd:
                inter += gt_pred_map.get((crowd[info['category_id']], pred_label), 0)
            if inter / info['area'] > 0.5:
                continue
            stat[info['category_id']].fp += 1
    return stat


# ------------------------------------------------------------------------------------------------------------------
# Results, text, files
# ------------------------------------------------------------------------------------------------------------------
METRICS = [("All", None), ("Things", True), ("Stuff", False)]


def bpq_results(pq_stat, categories, exclude=()):
    """`ipq.pq_results` plus `biou`: per class the mean boundary IoU of its matched pairs (0 without a match), per group the mean of
    that over the categories with support - averaged as SQ is"""
    results = {}
    for name, isthing in METRICS:
        results[name], per_class = pq_stat.pq_average(categories, isthing=isthing, exclude=exclude)
        total = 0.0
        for label, row in per_class.items():
            c = pq_stat[label]
            row['biou'] = getattr(c, 'biou', 0.0) / c.tp if c.tp else 0.0
            if c.tp + c.fp + c.fn:
                total += row['biou']
        results[name]['biou'] = total / results[name]['n']
        if name == 'All':
            results['per_class'] = per_class
    return results


def bpq_text(results):
    """the layout of pq.txt / vpq-<k>.txt with one more column, BIoU: the mean boundary IoU of the matched pairs, in percent"""
    out = []
    out.append("================================================\n")
    out.append("{:10s}| {:>5s}  {:>5s}  {:>5s}  {:>5s} {:>5s}".format("", "PQ", "SQ", "RQ", "BIoU", "N\n"))
    out.append("-" * (10 + 7 * 5) + '\n')
    for name, _isthing in METRICS:
        r = results[name]
        out.append("{:10s}| {:5.1f}  {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n".format(name, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'], 100 * r['biou'], r['n']))
    out.append("{:4s}| {:>5s} {:>5s} {:>5s} {:>5s} {:>6s} {:>7s} {:>7s} {:>7s}\n".format("IDX", "PQ", "SQ", "RQ", "BIoU", "IoU", "TP", "FP", "FN"))
    for idx, r in results['per_class'].items():
        out.append("{:4d} | {:5.1f} {:5.1f} {:5.1f} {:5.1f} {:6.1f} {:7d} {:7d} {:7d}\n".format(idx, 100 * r['pq'], 100 * r['sq'], 100 * r['rq'],
                                                                                              100 * r['biou'], r['iou'], r['tp'], r['fp'], r['fn']))
    return ''.join(out)


def bpq_compute(gt_jsons, pred_jsons, gt_pans, pred_pans, categories, output_dir, device='cuda', boundary_ratio=0.02):
    """The boundary twin of `ipq.pq_compute`: `(BPQStat, results)`, writes `output_dir/bpq.txt`."""
    stat = pq_compute_single_core(gt_jsons['annotations'], pred_jsons['annotations'], gt_pans, pred_pans, gt_jsons['images'], categories,
                                  device, boundary_ratio)
    results = bpq_results(stat, categories)
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'bpq.txt'), 'w') as f:
        f.write(bpq_text(results))
    print("BPQ_All:", 100 * results['All']['pq'])
    print("BPQ_Thing:", 100 * results['Things']['pq'])
    print("BPQ_Stuff:", 100 * results['Stuff']['pq'])
    return stat, results


def bvpq_compute(videos, categories, output_dir=None, device='cuda', boundary_ratio=0.02, windows=(1, 2, 3, 4)):
    """Boundary VPQ over the window lengths of eval_vpq.py (k = 5 (nframes - 1)): `videos` is a list of clips as
    `vpq_compute_single_core` takes them. Writes `bvpq-<k>.txt` per window length and `bvpq-final.txt` under `output_dir` (when given)
    and returns {'All' / 'Things' / 'Stuff': mean over the windows of 100 PQ, 'per_window': {nframes: results}}."""
    caches = [dict() for _ in videos]
    vpq = {name: [] for name, _ in METRICS}
    per_window = {}
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
    for nframes in windows:
        stat = BPQStat()
        for v, clip in enumerate(videos):
            stat += vpq_compute_single_core(clip, categories, nframes=nframes, device=device, _cache=caches[v], boundary_ratio=boundary_ratio)
        results = per_window[nframes] = bpq_results(stat, categories)
        if output_dir is not None:
            with open(os.path.join(output_dir, 'bvpq-%d.txt' % ((nframes - 1) * 5)), 'w') as f:
                f.write(bpq_text(results))
        for name, _ in METRICS:
            vpq[name].append(100 * results[name]['pq'])
    out = {name: sum(v) / len(v) for name, v in vpq.items()}
    if output_dir is not None:
        with open(os.path.join(output_dir, 'bvpq-final.txt'), 'w') as f:
            f.write('bvpq_all:%.4f\n' % out['All'])
            f.write('bvpq_thing:%.4f\n' % out['Things'])
            f.write('bvpq_stuff:%.4f\n' % out['Stuff'])
    out['per_window'] = per_window
    return out
