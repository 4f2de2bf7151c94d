"""Tube-matching VPQ statistics with the confusion counts taken on the device.

`vpq_compute_single_core(gt_pred_set, categories, nframes)` has the reference's signature and return value
(`tools/eval_vpq.py:74-209`, a `PQStat`). The reference stacks the id maps of every window of `nframes` frames and calls
`np.unique` on nframes x H x W uint64 keys — for every window and again for every window length (k = 1, 2, 3, 4 in
`eval_vpq.py:main`). Here `FrameCounts` counts every frame ONCE on the device (`vps_pair_count`: dense table over the segment
ids the two JSONs list for that frame) and a window's confusion map is the sum of its frames' sparse tables; the segment
bookkeeping and the matching rules are the reference's statements on the host. No CPU path for the counting.

The image evaluator (vps_amd/ipq.py) and the boundary ones (vps_amd/boundary.py) count, check, match and print with the functions of
this module: `count_frame` (over `pair_table`, the one caller of the kernel), `match`, `window_sums`, `pq_results`, `pq_text`."""
import copy
from collections import defaultdict

import numpy as np
import torch

from . import hip

VOID = 0


class PQStatCat:
    """eval_vpq.py:20-32"""

    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0

    def __iadd__(self, other):
        self.iou += other.iou; self.tp += other.tp; self.fp += other.fp; self.fn += other.fn
        return self


class PQStat:
    """eval_vpq.py:34-71"""

    def __init__(self):
        self.pq_per_cat = defaultdict(PQStatCat)

    def __getitem__(self, i):
        return self.pq_per_cat[i]

    def __iadd__(self, other):
        for label, cat in other.pq_per_cat.items():
            self.pq_per_cat[label] += cat
        return self

    def pq_average(self, categories, isthing, exclude=()):
        """tools/eval_vpq.py:40-71; `exclude`: category ids left out of the average - tools/dataset/viper.py:64-90 is the same
        function with `if label == 11: continue` (VIPER's "mobilebarrier"): `postprocess.DATASETS['viper']['pq_exclude']`"""
        pq, sq, rq, n = 0, 0, 0, 0
        per_class = {}
        for label, info in categories.items():
            if isthing is not None and isthing != (info['isthing'] == 1):
                continue
            if label in exclude:
                continue
            c = self.pq_per_cat[label]
            if c.tp + c.fp + c.fn == 0:
                per_class[label] = {'pq': 0.0, 'sq': 0.0, 'rq': 0.0, 'iou': 0.0, 'tp': 0, 'fp': 0, 'fn': 0}
                continue
            n += 1
            pq_c = c.iou / (c.tp + 0.5 * c.fp + 0.5 * c.fn)
            sq_c = c.iou / c.tp if c.tp != 0 else 0
            rq_c = c.tp / (c.tp + 0.5 * c.fp + 0.5 * c.fn)
            per_class[label] = {'pq': pq_c, 'sq': sq_c, 'rq': rq_c, 'iou': c.iou, 'tp': c.tp, 'fp': c.fp, 'fn': c.fn}
            pq += pq_c; sq += sq_c; rq += rq_c
        return {'pq': pq / n, 'sq': sq / n, 'rq': rq / n, 'n': n}, per_class


def _merged(json_entry):
    segms = {}
    for el in json_entry['segments_info']:                     # eval_vpq.py:93-104
        if el['id'] in segms:
            segms[el['id']]['area'] += el['area']
        else:
            segms[el['id']] = copy.deepcopy(el)
    return segms


def pan_tensor(a, dev):
    """a panoptic PNG (NumPy array or tensor) as a contiguous uint8 [H,W,3] tensor on `dev`; a host map is uploaded"""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = t.to(dev).contiguous()
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, 'panoptic PNG as uint8 [H,W,3]'
    return t


def pair_table(g, p, gt_ids, pred_ids, dev):
    """`vps_pair_count` of two device maps over sorted unique id lists -> int64 [ngt+1][npred+1] on the host; the extra row / column
    collects the ids that are not listed. The only caller of the kernel in the package and the only download of a frame's counts:
    the CPU tests of the host logic replace this one function with its NumPy definition."""
    gi = torch.from_numpy(gt_ids.astype(np.int32)).to(dev); pi = torch.from_numpy(pred_ids.astype(np.int32)).to(dev)   # ids < 2^24
    counts = torch.empty((len(gt_ids) + 1) * (len(pred_ids) + 1), dtype=torch.int32, device=dev)
    hip.check(hip.load().vps_pair_count(hip.ptr(g), hip.ptr(p), g.shape[0] * g.shape[1], hip.ptr(gi), len(gt_ids), hip.ptr(pi), len(pred_ids),
                                        hip.ptr(counts), hip.stream_ptr()), 'vps_pair_count')
    return counts.view(len(gt_ids) + 1, len(pred_ids) + 1).cpu().numpy().astype(np.int64)


def frame_ids(gt_json, pred_json, extra_gt_ids=None):
    """(gt_ids, pred_ids) counted in a frame, sorted unique int64: VOID and the ids its two JSONs list. `extra_gt_ids` (VPQ: the ids
    any frame of the clip lists) join the ground-truth ones: the reference takes np.unique over the WINDOW's pixel pairs
    (eval_vpq.py:150-157), so an id painted in this frame's PNG but listed only by another frame of the window still takes part in
    the matching."""
    gt_ids = np.unique(np.array([VOID] + [el['id'] for el in gt_json['segments_info']] + list(extra_gt_ids or ()), dtype=np.int64))
    pred_ids = np.unique(np.array([VOID] + [el['id'] for el in pred_json['segments_info']], dtype=np.int64))
    return gt_ids, pred_ids


def in_image(gt_image_json):
    """what the image evaluators put in front of the KeyError texts of `check_pred_areas`"""
    return 'In the image with ID {} '.format(gt_image_json.get('id') if isinstance(gt_image_json, dict) else None)


def check_pred_areas(tab, pred_ids, pred_json, pred_segms, p, categories, where=''):
    """eval_vpq.py:105-119 == base_dataset.py:352-366 on the pair table of a frame: the `area` of every entry of `pred_segms` becomes
    its pixel count in the PNG `p` (a column sum), and the PNG and the JSON must list the same segments of known categories
    (KeyError, after `where` when given)."""
    def error(text):
        return KeyError(where + text if where else text[0].upper() + text[1:])
    if tab[:, -1].sum() > 0:                                   # a predicted id that is neither listed nor VOID: name it like the reference
        ids = (lambda q: q[:, :, 0] + q[:, :, 1] * 256 + q[:, :, 2] * 65536)(p.cpu().numpy().astype(np.int64))
        bad = [int(v) for v in np.unique(ids) if v not in pred_segms and v != VOID]
        raise error('segment with ID {} is presented in PNG and not presented in JSON.'.format(bad[0]))
    col = tab.sum(0)
    pred_labels_set = set(el['id'] for el in pred_json['segments_info'])
    for j, label in enumerate(pred_ids):
        label = int(label)
        if col[j] == 0 or label not in pred_segms:             # not in the PNG / VOID that the JSON does not list
            continue
        pred_segms[label]['area'] = int(col[j])
        pred_labels_set.remove(label)
        if pred_segms[label]['category_id'] not in categories:
            raise error('segment with ID {} has unknown category_id {}.'.format(label, pred_segms[label]['category_id']))
    if len(pred_labels_set) != 0:
        raise error('the following segment IDs {} are presented in JSON and not presented in PNG.'.format(list(pred_labels_set)))


def sparse_pairs(tab, gt_ids, pred_ids):
    """{(gt id, pred id): pixels} of the listed ids of a pair table, row-major: ascending gt id, then pred id (unlisted ids never
    take part in the matching)"""
    rows, cols = np.nonzero(tab[:-1, :-1])
    return {(int(gt_ids[r]), int(pred_ids[c])): int(tab[r, c]) for r, c in zip(rows, cols)}


def count_frame(gt_json, pred_json, gt_pan, pred_pan, pred_segms, categories, dev, extra_gt_ids=None, where=''):
    """The device work of one frame or image, one launch and one download: (pairs, g, p, gt_ids, pred_ids) - the sparse pair table,
    the two maps on the device and the id lists that were counted. The entries of `pred_segms` (the caller's choice: the JSON's own,
    copies, or merged) get their `area` from the PNG, with the consistency checks of `check_pred_areas`."""
    g, p = pan_tensor(gt_pan, dev), pan_tensor(pred_pan, dev)
    assert g.shape == p.shape
    gt_ids, pred_ids = frame_ids(gt_json, pred_json, extra_gt_ids)
    tab = pair_table(g, p, gt_ids, pred_ids, dev)
    check_pred_areas(tab, pred_ids, pred_json, pred_segms, p, categories, where)
    return sparse_pairs(tab, gt_ids, pred_ids), g, p, gt_ids, pred_ids


class FrameCounts:
    """Per-frame device work, done once per frame whatever the window length: the (gt id, pred id) -> pixels table and the
    per-frame segment tables of eval_vpq.py:89-119 (with its consistency checks between PNG and JSON)."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)

    def count_maps(self, gt_json, pred_json, gt_pan, pred_pan, categories, extra_gt_ids=None):
        """`count` and what it counted on: ((gt_segms, pred_segms, pairs), (g, p, gt_ids, pred_ids)), for a second table over the
        same maps and id lists"""
        gt_segms, pred_segms = _merged(gt_json), _merged(pred_json)
        pairs, *maps = count_frame(gt_json, pred_json, gt_pan, pred_pan, pred_segms, categories, self.device, extra_gt_ids)
        return (gt_segms, pred_segms, pairs), tuple(maps)

    def count(self, gt_json, pred_json, gt_pan, pred_pan, categories, extra_gt_ids=None):
        return self.count_maps(gt_json, pred_json, gt_pan, pred_pan, categories, extra_gt_ids)[0]


def match(stat, gt_segms, pred_segms, gt_pred_map, tube=False, boundary_iou=None):
    """The matching rules of eval_vpq.py:166-213 == base_dataset.py:377-430 for one image or one tube window, added into `stat`:
    `gt_pred_map` {(gt id, pred id): pixels} in ascending (gt id, pred id) order, as `np.unique` gives it, so the IoU sums are the
    same float64 additions. `tube`: the VPQ evaluator's assertion on the mask IoU (the image evaluator has none).
    `boundary_iou(gt_label, pred_label)`, asked only for a candidate pair (both listed, not crowd, same category - for any other
    its denominator may be 0): the pair scores min(mask IoU, boundary IoU) and a match adds the boundary IoU to `biou`."""
    gt_matched, pred_matched = set(), set()
    for (gt_label, pred_label), intersection in gt_pred_map.items():
        if gt_label not in gt_segms or pred_label not in pred_segms:
            continue
        if gt_segms[gt_label]['iscrowd'] == 1:
            continue
        if gt_segms[gt_label]['category_id'] != pred_segms[pred_label]['category_id']:
            continue
        union = pred_segms[pred_label]['area'] + gt_segms[gt_label]['area'] - intersection - gt_pred_map.get((VOID, pred_label), 0)
        iou = intersection / union
        if tube:
            assert iou <= 1.0, 'INVALID IOU VALUE : %d' % (gt_label)
        if boundary_iou is not None:
            b_iou = boundary_iou(gt_label, pred_label)
            iou = min(iou, b_iou)
        if iou > 0.5:
            cat = stat[gt_segms[gt_label]['category_id']]
            cat.tp += 1
            cat.iou += iou
            if boundary_iou is not None:
                cat.biou += b_iou
            gt_matched.add(gt_label); pred_matched.add(pred_label)
    crowd_labels_dict = {}
    for gt_label, gt_info in gt_segms.items():                 # false negatives
        if gt_label in gt_matched:
            continue
        if gt_info['iscrowd'] == 1:                            # crowd segments are ignored
            crowd_labels_dict[gt_info['category_id']] = gt_label
            continue
        stat[gt_info['category_id']].fn += 1
    for pred_label, pred_info in pred_segms.items():           # false positives
        if pred_label in pred_matched:
            continue
        intersection = gt_pred_map.get((VOID, pred_label), 0)
        if pred_info['category_id'] in crowd_labels_dict:
            intersection += gt_pred_map.get((crowd_labels_dict[pred_info['category_id']], pred_label), 0)
        if intersection / pred_info['area'] > 0.5:             # mostly over VOID and CROWD regions: ignored
            continue
        stat[pred_info['category_id']].fp += 1


def window_sums(gt_pred_set, nframes, cache, tag, count):
    """eval_vpq.py:121-161 with every frame counted once: for each window of `nframes` frames of the clip, (vid_gt, vid_pred,
    gt_pred_map, *more) - the tube segment tables (areas summed over the window) and the summed tables of its frames, the first of
    them sorted. `count(gt_json, pred_json, gt_pan, pred_pan, clip_gt_ids)` -> (gt_segms, pred_segms, pairs, *more dicts) is what
    a frame costs; `cache` (a dict or None) keeps it across calls, under a key that ends in `tag`, so that callers with different
    `count`s can share one dict."""
    cache = {} if cache is None else cache
    clip_gt_ids = sorted({el['id'] for item in gt_pred_set for el in item[0]['segments_info']})
    for idx in range(0, len(gt_pred_set) - nframes + 1):
        gts, preds, sums = [], [], None
        for off, (gt_json, pred_json, gt_pan, pred_pan, _) in enumerate(gt_pred_set[idx:idx + nframes]):
            # keyed by the clip OBJECT: the entry keeps a reference to it and a hit is accepted only for the same object, so an
            # id() recycled by CPython for another (freed and re-allocated) clip list can never return stale counts
            key = (id(gt_pred_set), idx + off) + tuple(tag)
            ent = cache.get(key)
            if ent is None or ent[0] is not gt_pred_set:
                ent = cache[key] = (gt_pred_set, count(gt_json, pred_json, gt_pan, pred_pan, clip_gt_ids))
            g, p, *tables = ent[1]
            gts.append(copy.deepcopy(g)); preds.append(copy.deepcopy(p))        # the reference rebuilds them per window
            sums = [{} for _ in tables] if sums is None else sums
            for src, dst in zip(tables, sums):
                for k, v in src.items():
                    dst[k] = dst.get(k, 0) + v
        vid_gt, vid_pred = {}, {}
        for segms, vid in [(s, vid_gt) for s in gts] + [(s, vid_pred) for s in preds]:      # eval_vpq.py:129-141
            for k in segms.keys():
                if k not in vid:
                    vid[k] = segms[k]
                else:
                    vid[k]['area'] += segms[k]['area']
        yield (vid_gt, vid_pred, dict(sorted(sums[0].items()))) + tuple(sums[1:])      # np.unique order: ascending gt id, then pred id


def vpq_compute_single_core(gt_pred_set, categories, nframes=2, device='cuda', _cache=None):
    """eval_vpq.py:74-209, same arguments and result. `_cache` (optional dict) keeps the per-frame device results across
    calls with different `nframes`; entries are keyed by the clip object as well, so one dict may serve several videos."""
    fc = FrameCounts(device)
    stat = PQStat()

    def count(gt_json, pred_json, gt_pan, pred_pan, clip_gt_ids):
        return fc.count(gt_json, pred_json, gt_pan, pred_pan, categories, clip_gt_ids)
    for vid_gt, vid_pred, gt_pred_map in window_sums(gt_pred_set, nframes, _cache, (), count):
        match(stat, vid_gt, vid_pred, gt_pred_map, tube=True)
    return stat


METRICS = [("All", None), ("Things", True), ("Stuff", False)]


def pq_results(pq_stat, categories, exclude=(), biou=False):
    """base_dataset.py:189-194 == eval_vpq.py:224-231: the averages over all / thing / stuff categories, `per_class` from the first.
    `biou` (the statistics of vps_amd/boundary.py): per class the mean boundary IoU of its matched pairs (0 without a match), per
    group the mean of that over the categories with support - averaged as SQ is."""
    results = {}
    for name, isthing in METRICS:
        results[name], per_class = pq_stat.pq_average(categories, isthing=isthing, exclude=exclude)
        if biou:
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


def pq_text(results, biou=False):
    """the text of pq.txt (base_dataset.py:202-209) == vpq-<k>.txt (eval_vpq.py:233-244); `biou`: one more column after RQ, the
    mean boundary IoU of the matched pairs in percent"""
    heads, keys = (["PQ", "SQ", "RQ", "BIoU"], ['pq', 'sq', 'rq', 'biou']) if biou else (["PQ", "SQ", "RQ"], ['pq', 'sq', 'rq'])
    out = []
    out.append("================================================\n")
    out.append("{:10s}| ".format("") + "  ".join("{:>5s}".format(h) for h in heads) + " {:>5s}".format("N\n"))
    out.append("-" * (10 + 7 * (len(heads) + 1)) + '\n')
    for name, _isthing in METRICS:
        r = results[name]
        out.append("{:10s}| ".format(name) + "  ".join("{:5.1f}".format(100 * r[k]) for k in keys) + " {:5d}\n".format(r['n']))
    out.append("{:4s}| ".format("IDX") + " ".join("{:>5s}".format(h) for h in heads) + " {:>6s} {:>7s} {:>7s} {:>7s}\n".format("IoU", "TP", "FP", "FN"))
    for idx, r in results['per_class'].items():
        out.append("{:4d} | ".format(idx) + " ".join("{:5.1f}".format(100 * r[k]) for k in keys) +
                   " {:6.1f} {:7d} {:7d} {:7d}\n".format(r['iou'], r['tp'], r['fp'], r['fn']))
    return ''.join(out)
