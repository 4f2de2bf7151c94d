"""Image-level evaluation on the device: the path of the reference's `tools/test_eval_ipq.py`, which scores `PanopticFuse` per
image with no tracking.

    Cityscapes.evaluate_ssegs            tools/dataset/cityscapes.py:112-189      -> SemanticEvaluator
    BaseDataset.get_unified_pan_result   tools/dataset/base_dataset.py:232-273    -> ImagePanopticUnifier
    _converter_2ch_single_core           :288-335                                 -> ImageConverter
    _pq_compute_single_core / pq_compute :338-431, :169-219                       -> pq_compute_single_core / pq_compute
    evaluate_panoptic                    :104-229                                 -> evaluate_panoptic

Same names, arguments and results; maps may be numpy arrays or device tensors. The per-pixel work (`np.unique` per instance, one
boolean mask per segment, `np.bincount` per image) runs in `csrc/ipq_ops.hip` and `csrc/post_ops.hip`; the host keeps the
reference's bookkeeping statements. No CPU path: the HIP library must load and the maps are uploaded if they are host arrays."""
import json
import os
import re
import time

import numpy as np
import torch

from . import hip
from .evaluate import PQStat, count_frame, in_image, match
from .evaluate import pq_results, pq_text      # noqa: F401  `ipq.pq_results`, `ipq.pq_text`: the shared writers under this module's names
from .postprocess import DevicePngWriter, PanopticUnifier, _rgb2id


# ------------------------------------------------------------------------------------------------------------------
# Semantic segmentation: mIoU
# ------------------------------------------------------------------------------------------------------------------
def nearest_tables(src_hw, dst_hw):
    """(ytab int32 [Hd], xtab int32 [Wd]): source row / column of every row / column of `Image.resize((Wd, Hd), Image.NEAREST)`
    applied to an Hs x Ws image. Pillow steps a floating-point source coordinate from pixel to pixel, which is not
    floor((x + 0.5) * Ws / Wd) for every x; the tables are therefore taken from Pillow itself, by resizing one int32 ramp per
    axis (the mapping is separable). Equal sizes give the identity."""
    from PIL import Image
    (hs, ws), (hd, wd) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
    assert min(hs, ws, hd, wd) > 0
    if (hs, ws) == (hd, wd):
        return np.arange(hd, dtype=np.int32), np.arange(wd, dtype=np.int32)
    xramp = Image.fromarray(np.arange(ws, dtype=np.int32)[None, :])          # mode 'I', 1 row
    yramp = Image.fromarray(np.arange(hs, dtype=np.int32)[:, None])          # mode 'I', 1 column
    xtab = np.array(xramp.resize((wd, 1), Image.NEAREST), dtype=np.int32).reshape(wd)
    ytab = np.array(yramp.resize((1, hd), Image.NEAREST), dtype=np.int32).reshape(hd)
    return ytab, xtab


def get_pallete():
    """cityscapes.py:66-109: 256 x 3 uint8, flattened; the 19 train ids carry the Cityscapes label colours, the rest is black"""
    train_colors = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
                    (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
                    (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32)]
    pallete = np.zeros((256, 3), dtype=np.uint8)
    pallete[:len(train_colors)] = np.array(train_colors, dtype=np.uint8)
    return pallete.reshape(-1)


def segm_png_name(res_file_folder, pred_segm_name):
    """cityscapes.py:184"""
    return os.path.join(res_file_folder, pred_segm_name.replace('_leftImg8bit.png', '.png')).replace('_newImg8bit.png', '.png')


def _dev_u8(m, device, squeeze=False):
    t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
    t = t.to(device)
    if squeeze:
        t = t.squeeze()
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)
    return t.contiguous()


class SemanticEvaluator:
    """The confusion matrix of `evaluate_ssegs` kept on the device: `add` enqueues one image (`vps_sseg_confusion` adds into one
    int64 matrix, no synchronisation between images), `result` reads the matrix once."""

    def __init__(self, num_seg_classes=19, device='cuda'):
        self.num_seg_classes = int(num_seg_classes)
        self.device = torch.device(device)
        self.counts = torch.zeros(self.num_seg_classes * self.num_seg_classes, dtype=torch.int64, device=self.device)
        self._tables = {}

    def tables(self, src_hw, dst_hw):
        """device index tables of one (prediction size, label size) pair, built once; (None, None) for equal sizes"""
        key = (tuple(src_hw), tuple(dst_hw))
        if key not in self._tables:
            if key[0] == key[1]:
                self._tables[key] = (None, None)
            else:
                ytab, xtab = nearest_tables(*key)
                assert 0 <= ytab.min() and ytab.max() < key[0][0] and 0 <= xtab.min() and xtab.max() < key[0][1]
                self._tables[key] = (torch.from_numpy(ytab).to(self.device), torch.from_numpy(xtab).to(self.device))
        return self._tables[key]

    def add(self, seg_gt, seg_pred):
        """cityscapes.py:122-135 for one image: `seg_pred` resized to the label's size (NEAREST), label 255 dropped, counted"""
        g, p = _dev_u8(seg_gt, self.device), _dev_u8(seg_pred, self.device, squeeze=True)
        assert g.dim() == 2 and p.dim() == 2, 'label and prediction are [H,W] maps'
        ytab, xtab = self.tables(p.shape, g.shape)
        hip.check(hip.load().vps_sseg_confusion(hip.ptr(g), g.shape[0], g.shape[1], hip.ptr(p), p.shape[0], p.shape[1], hip.ptr(ytab),
                                                hip.ptr(xtab), self.num_seg_classes, hip.ptr(self.counts), hip.stream_ptr()),
                  'vps_sseg_confusion')

    def result(self):
        """cityscapes.py:137-146 on the float64 matrix"""
        n = self.num_seg_classes
        confusion_matrix = self.counts.cpu().numpy().reshape(n, n).astype(np.float64)
        pos = confusion_matrix.sum(1)
        res = confusion_matrix.sum(0)
        tp = np.diag(confusion_matrix)
        IU_array = (tp / np.maximum(1.0, pos + res - tp))
        mean_IU = IU_array.mean()
        return {'meanIU': mean_IU, 'IU_array': IU_array, 'confusion_matrix': confusion_matrix}

    def write_segmentation_result(self, segmentation_results, res_file_folder, pred_segm_names, writer=None):
        """cityscapes.py:169-189: palette PNGs of the predictions; device maps are encoded on the device"""
        os.makedirs(res_file_folder, exist_ok=True)
        own = writer is None
        writer = DevicePngWriter(self.device) if own else writer
        pallete = get_pallete().reshape(256, 3)
        maps = []
        for i, pred_segm_name in enumerate(pred_segm_names):
            m = _dev_u8(segmentation_results[i], self.device, squeeze=True)
            writer.submit(m, segm_png_name(res_file_folder, pred_segm_name), palette=pallete)
            maps.append(m)
        if own:
            writer.close()
        return maps

    def evaluate_ssegs(self, pred_segmentations, res_file_folder, pred_segm_names, gt_paths, writer=None):
        """`Cityscapes.evaluate_ssegs` (cityscapes.py:112-166): writes the palette PNGs, counts every image against its label file
        `gt_paths[i]` and prints what the reference prints. The reference reads each map back from the PNG it has just written
        before scoring it; that only round-trips the uint8 map, so the device tensors are counted directly."""
        from PIL import Image
        maps = self.write_segmentation_result(pred_segmentations, res_file_folder, pred_segm_names, writer)
        for m, gt_path in zip(maps, gt_paths):
            self.add(np.array(Image.open(gt_path)), m)
        evaluation_results = self.result()

        def convert_confusion_matrix(confusion_matrix):
            cls_sum = confusion_matrix.sum(axis=1)
            return confusion_matrix / cls_sum.reshape((-1, 1))

        print('evaluate segmentation:')
        meanIU = evaluation_results['meanIU']
        IU_array = evaluation_results['IU_array']
        with np.errstate(divide='ignore', invalid='ignore'):
            confusion_matrix = convert_confusion_matrix(evaluation_results['confusion_matrix'])
        print('IU_array:')
        for i in range(len(IU_array)):
            print('%.5f' % IU_array[i])
        print('meanIU:%.5f' % meanIU)
        with np.printoptions(precision=3, suppress=True, linewidth=200):
            confusion_matrix = re.sub(r'[\[\]]', '', np.array2string(confusion_matrix, separator='\t'))
        print('confusion_matrix:')
        print(confusion_matrix)
        return evaluation_results


def evaluate_ssegs(pred_segmentations, res_file_folder, pred_segm_names, gt_paths, num_seg_classes=19, device='cuda'):
    return SemanticEvaluator(num_seg_classes, device).evaluate_ssegs(pred_segmentations, res_file_folder, pred_segm_names, gt_paths)


# ------------------------------------------------------------------------------------------------------------------
# Unify: (semantic map, panoptic map, class indices) -> 2-channel map
# ------------------------------------------------------------------------------------------------------------------
class ImagePanopticUnifier(PanopticUnifier):
    """`BaseDataset.get_unified_pan_result` (base_dataset.py:232-273): the decisions of the video unifier without object ids, and
    channel 2 of the result is 0 (the video one, called without object ids, leaves the raw panoptic id there)."""

    def unify_frame(self, seg, pan, cls_ind, stuff_area_limit=4 * 64 * 64):
        """one image. Returns a device uint8 tensor [H,W,3]."""
        lib = hip.load()
        seg, pan = self._map(seg), self._map(pan)
        assert seg.shape == pan.shape and pan.dim() == 2
        npix = pan.numel()
        cls_t = torch.as_tensor(np.asarray(cls_ind.cpu() if torch.is_tensor(cls_ind) else cls_ind), dtype=torch.int32).to(self.device)
        out = torch.empty(pan.shape[0], pan.shape[1], 3, dtype=torch.uint8, device=self.device)
        s = hip.stream_ptr()
        hip.check(lib.vps_unify_hist(hip.ptr(pan), hip.ptr(seg), npix, self.id_last_stuff, hip.ptr(self.hist), hip.ptr(self.pan_count), s),
                  'vps_unify_hist')
        hip.check(lib.vps_unify_tables_image(hip.ptr(self.hist), hip.ptr(self.pan_count), hip.ptr(cls_t) if cls_t.numel() else None,
                                             cls_t.numel(), self.id_last_stuff, int(stuff_area_limit), hip.ptr(self.tables),
                                             hip.ptr(self.status), s), 'vps_unify_tables_image')
        hip.check(lib.vps_unify_write(hip.ptr(pan), npix, hip.ptr(self.tables), hip.ptr(out), s), 'vps_unify_write')
        self._keep = (seg, pan, cls_t)                   # alive until the stream has consumed them
        return out

    def get_unified_pan_result_device(self, segs, pans, cls_inds, stuff_area_limit=4 * 64 * 64, names=None):
        """as `get_unified_pan_result`, the maps stay on the device"""
        results = {}
        for seg, pan, cls_ind, name in zip(segs, pans, cls_inds, names):
            out = self.unify_frame(seg, pan, cls_ind, stuff_area_limit)
            if int(self.status.item()):                  # also orders the reuse of hist / tables by the next image
                raise IndexError('instance id without cls_ind entry (base_dataset.py:251)')
            results[name] = out
        return results

    def get_unified_pan_result(self, segs, pans, cls_inds, stuff_area_limit=4 * 64 * 64, names=None):
        return {k: v.cpu().numpy() for k, v in self.get_unified_pan_result_device(segs, pans, cls_inds, stuff_area_limit, names).items()}


# ------------------------------------------------------------------------------------------------------------------
# Converter: 2-channel map -> panoptic PNG colours + segments_info
# ------------------------------------------------------------------------------------------------------------------
class ImageConverter:
    """Device-side body of `_converter_2ch_single_core(proc_id, pan_2ch_set, color_generator)` (base_dataset.py:288-335, with
    `vis_panoptic` False): one statistics pass and one painting pass per image instead of a boolean mask per segment. A segment is
    a (pan_seg, pan_ins) pair. Every non-void segment of every image draws a fresh colour from the caller's generator, in ascending
    order of 1000 * seg + ins; `area` is the pixel count of that pair, `bbox` [xmin, ymin, xmax - xmin, ymax - ymin]."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        self.stats = torch.empty(65536 * 5, dtype=torch.int32, device=self.device)
        self.lut = torch.zeros(65536 * 3, dtype=torch.uint8, device=self.device)

    def convert(self, pan_2ch_set, color_generator):
        annotations, pan_dev, _ = self.convert_device(pan_2ch_set, color_generator)
        return annotations, [p.cpu().numpy() for p in pan_dev]

    def convert_device(self, pan_2ch_set, color_generator):
        """as `convert`, but the painted maps stay on the device: (annotations, pan device tensors, pan_2ch device tensors)"""
        lib = hip.load()
        annotations, pan_all, two_all = [], [], []
        for pan_2ch in pan_2ch_set:
            t = torch.from_numpy(np.ascontiguousarray(pan_2ch)) if isinstance(pan_2ch, np.ndarray) else pan_2ch
            t = t.to(self.device).contiguous()
            assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
            H, W = int(t.shape[0]), int(t.shape[1])
            hip.check(lib.vps_segment_stats_ch(hip.ptr(t), H, W, 1, hip.ptr(self.stats), hip.stream_ptr()), 'vps_segment_stats_ch')
            st = self.stats.view(65536, 5)
            keys = torch.nonzero(st[:, 0] > 0).flatten()
            rows = st[keys].cpu().numpy()
            keys = keys.cpu().numpy()                            # ascending seg * 256 + ins == ascending 1000 * seg + ins (ins < 256)
            lut = np.zeros((65536, 3), dtype=np.uint8)
            segm_info = []
            for key, row in zip(keys, rows):
                sem = int(key) >> 8
                if sem == 255:
                    continue
                color = color_generator.get_color(sem)
                lut[key] = color
                cnt, x0, y0, x1, y1 = (int(v) for v in row)
                segm_info.append({"category_id": sem, "iscrowd": 0, "id": _rgb2id(color), "bbox": [x0, y0, x1 - x0, y1 - y0], "area": cnt})
            self.lut.copy_(torch.from_numpy(lut.reshape(-1)), non_blocking=False)
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
            hip.check(lib.vps_segment_paint_ch(hip.ptr(t), H * W, 1, hip.ptr(self.lut), hip.ptr(out), hip.stream_ptr()), 'vps_segment_paint_ch')
            pan_all.append(out)
            two_all.append(t)
            annotations.append({"segments_info": segm_info})
        return annotations, pan_all, two_all


# ------------------------------------------------------------------------------------------------------------------
# Image PQ
# ------------------------------------------------------------------------------------------------------------------
def pq_compute_single_core(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons, categories, device='cuda'):
    """`BaseDataset._pq_compute_single_core` (base_dataset.py:338-431) without its `proc_id`: a `PQStat` over the images. The pixel
    pairs of an image come from `vps_pair_count` (`evaluate.count_frame`); the matching is the reference's (`evaluate.match`), visited
    in ascending (gt id, pred id) order as `np.unique` gives it, so the IoU sums are the same float64 additions. Like the reference,
    the predicted segments' `area` is overwritten with the pixel count of the PNG.
    One deliberate difference: where the reference's PNG / JSON consistency checks (:359, :363, :366) would die with a NameError on
    their undefined `gt_ann`, this raises the KeyError those lines were written to raise (with the image id of `gt_image_jsons`)."""
    dev = torch.device(device)
    pq_stat = PQStat()
    for gt_json, pred_json, gt_pan, pred_pan, gt_image_json in zip(gt_jsons, pred_jsons, gt_pans, pred_pans, gt_image_jsons):
        gt_segms = {el['id']: el for el in gt_json['segments_info']}
        pred_segms = {el['id']: el for el in pred_json['segments_info']}       # the caller's entries: their `area` is overwritten
        gt_pred_map = count_frame(gt_json, pred_json, gt_pan, pred_pan, pred_segms, categories, dev, where=in_image(gt_image_json))[0]
        match(pq_stat, gt_segms, pred_segms, gt_pred_map)
    return pq_stat


def pq_compute(gt_jsons, pred_jsons, gt_pans, pred_pans, categories, output_dir, device='cuda'):
    """the `pq_compute` closure (base_dataset.py:169-219): returns `(PQStat, results)` and writes `output_dir/pq.txt`. One pass over
    the images instead of one worker process per CPU: the per-category IoU is summed image by image, which is what the reference
    computes when its pool has one worker (with more it adds per-worker partial sums, so its last bits depend on the CPU count)."""
    start_time = time.time()
    gt_image_jsons = gt_jsons['images']
    gt_anns, pred_anns = gt_jsons['annotations'], pred_jsons['annotations']
    pq_stat = pq_compute_single_core(gt_anns, pred_anns, gt_pans, pred_pans, gt_image_jsons, categories, device)
    results = pq_results(pq_stat, categories)
    pq_all = 100 * results['All']['pq']
    pq_thing = 100 * results['Things']['pq']
    pq_stuff = 100 * results['Stuff']['pq']
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'pq.txt'), 'w') as f:
        f.write(pq_text(results))
    t_delta = time.time() - start_time
    print("PQ_All:", pq_all)
    print("PQ_Thing:", pq_thing)
    print("PQ_Stuff:", pq_stuff)
    print("Time elapsed: {:0.2f} seconds".format(t_delta))
    return pq_stat, results


def ipq_png_name(save_folder, file_name):
    """base_dataset.py:159 (save_image): output file name of a ground-truth image entry"""
    return os.path.join(save_folder, file_name.replace('_leftImg8bit', '').replace('jpg', 'png').replace('jpeg', 'png'))


def evaluate_panoptic(pred_pans_2ch, output_dir, gt_json, gt_pans, categories=None, color_generator=None, device='cuda', writer=None):
    """`BaseDataset.evaluate_panoptic` (base_dataset.py:104-229) without its hard-coded dataset paths: the caller passes what `get_gt`
    loads - `gt_json` (the panoptic ground-truth JSON as a dict, or its path), `gt_pans` (the ground-truth PNGs as uint8 [H,W,3] maps
    in the order of `gt_json['images']`, or the folder that holds them), `categories` ({id: entry}, default: from `gt_json`) and the
    colour generator (default: panopticapi's `IdGenerator(categories)`). Converts the 2-channel predictions, writes `pan_2ch/`,
    `pan/`, `gt.json`, `pred.json` and `pq.txt` under `output_dir` and returns the results dict."""
    from PIL import Image
    if isinstance(gt_json, str):
        with open(gt_json, 'r') as f:
            gt_json = json.load(f)
    if categories is None:
        categories = {el['id']: el for el in gt_json['categories']}
    if isinstance(gt_pans, str):
        gt_pans = [np.array(Image.open(os.path.join(gt_pans, item['file_name']))) for item in gt_json['images']]
    if color_generator is None:
        from panopticapi.utils import IdGenerator
        color_generator = IdGenerator(categories)
    own = writer is None
    writer = DevicePngWriter(device) if own else writer
    ann, pans_dev, twos_dev = ImageConverter(device).convert_device(pred_pans_2ch, color_generator)
    pred_json = {'annotations': ann}
    on_device = bool(getattr(writer, 'accepts_device', False))
    for item, two, pan in zip(gt_json['images'], twos_dev, pans_dev):
        for folder, m in (('pan_2ch', two), ('pan', pan)):
            writer.submit(m if on_device else m.cpu().numpy(), ipq_png_name(os.path.join(output_dir, folder), item['file_name']))
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'gt.json'), 'w') as f:
        json.dump(gt_json, f)
    with open(os.path.join(output_dir, 'pred.json'), 'w') as f:
        json.dump(pred_json, f)
    _, results = pq_compute(gt_json, pred_json, gt_pans, pans_dev, categories, output_dir, device)
    if own:
        writer.close()
    return results
