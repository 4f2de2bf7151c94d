"""Plain-NumPy restatements of the reference's image-level evaluation (tools/dataset/base_dataset.py, tools/dataset/cityscapes.py),
the CPU twins of `vps_amd/ipq.py`: written statement by statement after the functions they restate and checked against goldens of
the REAL functions (tests/golden/make_ipq_golden.py -> ipq_cases.npz) in tests/test_ipq.py. The GPU tests compare the device path with
both. No file I/O, no device."""
from collections import defaultdict

import numpy as np


# ---------------------------------------------------------------------------------------------- semantic mIoU
def confusion_matrix(seg_gt, seg_pred, class_num, ytab=None, xtab=None):
    """cityscapes.py:122-135 + base_dataset.py:449-467 for one image. `seg_pred` is resampled to the label's size through the index
    tables of the NEAREST resize (None: equal sizes), label 255 is dropped, idx = gt * class_num + pred is counted by an int32
    bincount of which the first class_num^2 cells are kept. Returns float64 [class_num][class_num]."""
    seg_gt = np.asarray(seg_gt).astype('float32')
    seg_pred = np.asarray(seg_pred)
    if ytab is not None:
        seg_pred = seg_pred[np.asarray(ytab)[:, None], np.asarray(xtab)[None, :]]
    assert seg_pred.shape == seg_gt.shape
    keep = seg_gt != 255
    gt_label, pred_label = seg_gt[keep], seg_pred[keep]
    index = (gt_label * class_num + pred_label).astype('int32')
    label_count = np.bincount(index)
    cm = np.zeros((class_num, class_num))
    n = min(len(label_count), class_num * class_num)
    cm.reshape(-1)[:n] = label_count[:n]
    return cm


def miou(cm):
    """cityscapes.py:137-146"""
    pos = cm.sum(1)
    res = cm.sum(0)
    tp = np.diag(cm)
    IU_array = (tp / np.maximum(1.0, pos + res - tp))
    return {'meanIU': IU_array.mean(), 'IU_array': IU_array, 'confusion_matrix': cm}


# ---------------------------------------------------------------------------------------------- unify
def get_unified_pan_result(segs, pans, cls_inds, stuff_area_limit=4 * 64 * 64, names=None, id_last_stuff=10):
    """base_dataset.py:232-273"""
    out = {}
    for seg, pan, cls_ind, name in zip(segs, pans, cls_inds, names):
        pan_seg = pan.copy()
        pan_ins = pan.copy()
        ids = np.unique(pan)
        ids_ins = ids[ids > id_last_stuff]
        pan_ins[pan_ins <= id_last_stuff] = 0
        for idx, id_ in enumerate(ids_ins):
            region = pan_ins == id_
            if id_ == 255:
                pan_seg[region] = 255
                pan_ins[region] = 0
                continue
            cls, cnt = np.unique(seg[region], return_counts=True)
            inst_cls = cls_ind[int(id_) - id_last_stuff - 1] + id_last_stuff            # IndexError when the id has no entry
            top = cls[np.argmax(cnt)]
            if top != inst_cls and np.max(cnt) / np.sum(cnt) >= 0.5 and top <= id_last_stuff:
                pan_seg[region] = top
                pan_ins[region] = 0
            else:
                pan_seg[region] = inst_cls
                pan_ins[region] = idx + 1
        for c in np.unique(pan_seg):
            if c <= id_last_stuff:
                area = pan_seg == c
                if area.sum() < stuff_area_limit:
                    pan_seg[area] = 255
        pan_2ch = np.zeros((pan.shape[0], pan.shape[1], 3), dtype=np.uint8)
        pan_2ch[:, :, 0] = pan_seg
        pan_2ch[:, :, 1] = pan_ins
        out[name] = pan_2ch
    return out


# ---------------------------------------------------------------------------------------------- converter
def rgb2id(color):
    return int(color[0]) + 256 * int(color[1]) + 256 * 256 * int(color[2])


def converter_2ch_single_core(pan_2ch_set, color_generator):
    """base_dataset.py:288-335 with vis_panoptic False"""
    OFFSET, VOID = 1000, 255
    annotations, pan_all = [], []
    for pan_2ch in pan_2ch_set:
        pan_2ch = np.uint32(pan_2ch)
        pan = OFFSET * pan_2ch[:, :, 0] + pan_2ch[:, :, 1]
        pan_format = np.zeros((pan_2ch.shape[0], pan_2ch.shape[1], 3), dtype=np.uint8)
        segm_info = []
        for el in np.unique(pan):
            sem = int(el // OFFSET)
            if sem == VOID:
                continue
            mask = pan == el
            color = color_generator.get_color(sem)
            pan_format[mask] = color
            ys, xs = np.where(mask)
            x, y = int(xs.min()), int(ys.min())
            segm_info.append({"category_id": sem, "iscrowd": 0, "id": rgb2id(color), "bbox": [x, y, int(xs.max()) - x, int(ys.max()) - y],
                              "area": int(mask.sum())})
        annotations.append({"segments_info": segm_info})
        pan_all.append(pan_format)
    return annotations, pan_all


# ---------------------------------------------------------------------------------------------- PQ
class PQStatCat:
    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0


def pq_compute_single_core(gt_jsons_set, pred_jsons_set, gt_pans_set, pred_pans_set, gt_image_jsons_set, categories):
    """base_dataset.py:338-431; returns {category: PQStatCat}. The consistency checks raise the KeyError they were written to raise."""
    OFFSET, VOID = 256 * 256 * 256, 0
    pq_stat = defaultdict(PQStatCat)
    for gt_json, pred_json, gt_pan, pred_pan, gt_image_json in zip(gt_jsons_set, pred_jsons_set, gt_pans_set, pred_pans_set, gt_image_jsons_set):
        gt_pan, pred_pan = np.uint32(gt_pan), np.uint32(pred_pan)
        pan_gt = gt_pan[:, :, 0] + gt_pan[:, :, 1] * 256 + gt_pan[:, :, 2] * 256 * 256
        pan_pred = pred_pan[:, :, 0] + pred_pan[:, :, 1] * 256 + pred_pan[:, :, 2] * 256 * 256
        gt_segms = {el['id']: dict(el) for el in gt_json['segments_info']}
        pred_segms = {el['id']: dict(el) for el in pred_json['segments_info']}
        pred_labels_set = set(el['id'] for el in pred_json['segments_info'])
        labels, labels_cnt = np.unique(pan_pred, return_counts=True)
        for label, label_cnt in zip(labels.tolist(), labels_cnt.tolist()):
            if label not in pred_segms:
                if label == VOID:
                    continue
                raise KeyError('segment with ID {} is presented in PNG and not presented in JSON.'.format(label))
            pred_segms[label]['area'] = label_cnt
            pred_labels_set.remove(label)
            if pred_segms[label]['category_id'] not in categories:
                raise KeyError('segment with ID {} has unknown category_id {}.'.format(label, pred_segms[label]['category_id']))
        if len(pred_labels_set) != 0:
            raise KeyError('segment IDs {} are presented in JSON and not presented in PNG.'.format(list(pred_labels_set)))
        pan_gt_pred = pan_gt.astype(np.uint64) * OFFSET + pan_pred.astype(np.uint64)
        gt_pred_map = {}
        labels, labels_cnt = np.unique(pan_gt_pred, return_counts=True)
        for label, intersection in zip(labels.tolist(), labels_cnt.tolist()):
            gt_pred_map[(label // OFFSET, label % OFFSET)] = intersection
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
            if iou > 0.5:
                pq_stat[gt_segms[gt_label]['category_id']].tp += 1
                pq_stat[gt_segms[gt_label]['category_id']].iou += iou
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


def stat_rows(pq_stat, categories):
    """(int64 [ncat][4] = category, tp, fp, fn; float64 [ncat] iou) in ascending category order: how the goldens store a PQStat"""
    cats = sorted(categories)
    return (np.array([[c, pq_stat[c].tp, pq_stat[c].fp, pq_stat[c].fn] for c in cats], dtype=np.int64),
            np.array([pq_stat[c].iou for c in cats], dtype=np.float64))
