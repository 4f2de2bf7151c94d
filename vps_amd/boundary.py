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

import torch

from . import evaluate, hip
from .evaluate import METRICS, VOID, FrameCounts, PQStat, PQStatCat, count_frame, in_image, match, pan_tensor, sparse_pairs, window_sums

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


def band_workspace_bytes(H, W, d):
    n = hip.c_int64(0)
    hip.check(hip.load().vps_boundary_band_ws(int(H), int(W), int(d), hip.byref(n)), 'vps_boundary_band_ws')
    return int(n.value)


def boundary_band(pan, d=None, ratio=0.02, device='cuda'):
    """The band map of a panoptic map (device or NumPy uint8 [H,W,3]): a device uint8 [H,W,3] tensor in which the interior of every
    segment is FILL. `d` defaults to `dilation(H, W, ratio)`. Enqueued on the current stream, no synchronisation."""
    dev = pan.device if torch.is_tensor(pan) and pan.is_cuda else torch.device(device)
    t = pan_tensor(pan, dev)
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


def band_counts(g, p, gt_ids, pred_ids, ratio, dev):
    """The band table of one frame: (bpairs {(gt id, pred id): band pixels of both}, bg {gt id: band size}, bp {pred id: band size})
    over the listed ids. A band size counts ALL band pixels of the segment: the row / column sum with the extra column / row, where
    the other map's fill and unlisted ids land."""
    d = dilation(int(g.shape[0]), int(g.shape[1]), ratio)
    tab = evaluate.pair_table(boundary_band(g, d), boundary_band(p, d), gt_ids, pred_ids, dev)      # looked up per call: the tests' seam
    bg = {int(i): int(v) for i, v in zip(gt_ids, tab[:-1].sum(1))}
    bp = {int(i): int(v) for i, v in zip(pred_ids, tab[:, :-1].sum(0))}
    return sparse_pairs(tab, gt_ids, pred_ids), bg, bp


def _boundary_iou(bpairs, bg, bp):
    """the `boundary_iou` of `evaluate.match` over the band counts of an image or of a window"""
    def boundary_iou(gt_label, pred_label):
        bi = bpairs.get((gt_label, pred_label), 0)
        return bi / (bg[gt_label] + bp[pred_label] - bi - bpairs.get((VOID, pred_label), 0))
    return boundary_iou


# ------------------------------------------------------------------------------------------------------------------
# Boundary PQ of images
# ------------------------------------------------------------------------------------------------------------------
def pq_compute_single_core(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons, categories, device='cuda', boundary_ratio=0.02):
    """The boundary twin of `ipq.pq_compute_single_core`: same arguments, a `BPQStat`, and the caller's entries keep their `area`. A
    pair is scored with min(mask IoU, boundary IoU) (module docstring)."""
    gt_jsons, pred_jsons = list(gt_jsons), list(pred_jsons)
    check_reserved(*gt_jsons, *pred_jsons)
    dev = torch.device(device)
    pq_stat = BPQStat()
    for gt_json, pred_json, gt_pan, pred_pan, gt_image_json in zip(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons):
        gt_segms = {el['id']: el for el in gt_json['segments_info']}
        pred_segms = {el['id']: copy.copy(el) for el in pred_json['segments_info']}
        gt_pred_map, g, p, gt_ids, pred_ids = count_frame(gt_json, pred_json, gt_pan, pred_pan, pred_segms, categories, dev,
                                                          where=in_image(gt_image_json))
        match(pq_stat, gt_segms, pred_segms, gt_pred_map, boundary_iou=_boundary_iou(*band_counts(g, p, gt_ids, pred_ids, boundary_ratio, dev)))
    return pq_stat


# ------------------------------------------------------------------------------------------------------------------
# Boundary VPQ of a clip
# ------------------------------------------------------------------------------------------------------------------
def vpq_compute_single_core(gt_pred_set, categories, nframes=2, device='cuda', _cache=None, boundary_ratio=0.02):
    """The boundary twin of `evaluate.vpq_compute_single_core`: same arguments, a `BPQStat`. Every frame is counted once (`_cache` as
    there, under keys of its own): `FrameCounts` for the masks, `band_counts` for the bands; a window sums both before the divisions."""
    check_reserved(*[a for item in gt_pred_set for a in item[:2]])
    fc = FrameCounts(device)
    stat = BPQStat()

    def count(gt_json, pred_json, gt_pan, pred_pan, clip_gt_ids):
        counts, (g, p, gt_ids, pred_ids) = fc.count_maps(gt_json, pred_json, gt_pan, pred_pan, categories, clip_gt_ids)
        return counts + band_counts(g, p, gt_ids, pred_ids, boundary_ratio, fc.device)
    for vid_gt, vid_pred, gt_pred_map, bpairs, bg, bp in window_sums(gt_pred_set, nframes, _cache, ('boundary', float(boundary_ratio)), count):
        match(stat, vid_gt, vid_pred, gt_pred_map, tube=True, boundary_iou=_boundary_iou(bpairs, bg, bp))
    return stat


# ------------------------------------------------------------------------------------------------------------------
# Results, text, files
# ------------------------------------------------------------------------------------------------------------------
def bpq_results(pq_stat, categories, exclude=()):
    """`ipq.pq_results` plus `biou`, the mean boundary IoU of the matched pairs"""
    return evaluate.pq_results(pq_stat, categories, exclude, biou=True)


def bpq_text(results):
    """the layout of pq.txt / vpq-<k>.txt with one more column, BIoU"""
    return evaluate.pq_text(results, biou=True)


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
