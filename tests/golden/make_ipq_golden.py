"""Generates tests/golden/ipq_cases.npz by running the REAL image-level evaluation functions of the reference
(/root/reference/tools/dataset/base_dataset.py: BaseDataset.get_unified_pan_result, _converter_2ch_single_core,
_pq_compute_single_core, get_confusion_matrix, evaluate_panoptic; tools/dataset/cityscapes.py: Cityscapes.evaluate_ssegs) in the
build container, on synthetic inputs. Inputs and outputs only are stored.

Only import shims are installed: the stub loader of make_unify_golden.py for the third-party modules the dataset package imports at
module level, `panopticapi.utils` (absent here; rgb2id = R + 256 G + 65536 B, IdGenerator = the deterministic stand-in `Colors` of
tests/ipq_cases.py) and, for evaluate_panoptic, an in-process stand-in for the multiprocessing pool with one worker. The function
bodies that run are the reference's own. Run from the repo root:
    python tests/golden/make_ipq_golden.py
The GPU box has no /root/reference: tests read the committed .npz only."""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_unify_golden as U  # noqa: E402
from ipq_cases import Colors, confusion_inputs, pq_images, CATEGORIES  # noqa: E402


def _jbytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def _py(obj):
    """numpy scalars -> Python numbers, recursively (the reference leaves np.int64 areas in its dicts)"""
    if isinstance(obj, dict):
        return {(_py(k)): _py(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_py(v) for v in obj]
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


class _Result:
    def __init__(self, v):
        self.v = v

    def get(self):
        return self.v


class _Pool:
    """one worker, run in this process: `apply_async` calls the function at once"""

    def __init__(self, processes=None):
        pass

    def apply_async(self, fn, args):
        return _Result(fn(*args))

    def close(self):
        pass

    def join(self):
        pass


def main():
    warnings.simplefilter('ignore')
    out = {}
    # ------------------------------------------------------------------ unify, both class tables
    unify_fn = {}
    for tag, nseg, ncls in (('c19', 19, 9), ('c23', 23, 11)):
        unify_fn[tag] = U.load_reference_function('tools.dataset.base_dataset', nseg, ncls)
    base = sys.modules['tools.dataset.base_dataset']
    cfg = sys.modules['tools.config.config'].config
    assert base.vis_panoptic is False
    pm = types.ModuleType('panopticapi'); pu = types.ModuleType('panopticapi.utils')
    pu.rgb2id = lambda color: int(color[0]) + 256 * int(color[1]) + 256 * 256 * int(color[2])
    pu.IdGenerator = lambda categories: Colors()
    pm.utils = pu
    sys.modules['panopticapi'] = pm; sys.modules['panopticapi.utils'] = pu
    BD = base.BaseDataset
    clips = [
        dict(H=64, W=128, ks=[6, 9, 12], void=True, limit=4 * 64 * 64),
        dict(H=64, W=128, ks=[5, 0, 7], void=False, limit=200),
        dict(H=96, W=160, ks=[20, 33], void=False, limit=1500),
        dict(H=48, W=64, ks=[8], void=True, limit=100),
    ]
    unified = {}
    for tag, nseg, ncls, seed in (('c19', 19, 9, 0), ('c23', 23, 11, 7)):
        cfg.dataset.num_seg_classes, cfg.dataset.num_classes = nseg, ncls
        nstuff, nthing = nseg - ncls + 1, ncls - 1
        rng = np.random.default_rng(seed)
        for ci, c in enumerate(clips):
            segs, pans, clss, names = [], [], [], []
            for fi, k in enumerate(c['ks']):
                seg, pan, cls_ind, _ = U.make_case(rng, c['H'], c['W'], k, False, False, c['void'], False, nstuff, nthing)
                segs.append(seg); pans.append(pan); clss.append(cls_ind); names.append('f%d' % fi)
            res = unify_fn[tag](None, [s.copy() for s in segs], [p.copy() for p in pans], [c_.copy() for c_ in clss], c['limit'], names)
            out['unify_%s_clip%d_limit' % (tag, ci)] = np.int64(c['limit'])
            out['unify_%s_clip%d_n' % (tag, ci)] = np.int64(len(names))
            for fi, n in enumerate(names):
                pre = 'unify_%s_clip%d_f%d_' % (tag, ci, fi)
                out[pre + 'seg'], out[pre + 'pan'], out[pre + 'cls'], out[pre + 'out'] = segs[fi], pans[fi], clss[fi], res[n]
                assert not res[n][..., 2].any()
                unified[(tag, ci, fi)] = res[n]
        out['unify_%s_nclips' % tag] = np.int64(len(clips))
        out['unify_%s_id_last_stuff' % tag] = np.int64(nseg - ncls)

    # ------------------------------------------------------------------ converter
    two = unified[('c19', 3, 0)].copy()
    two[5:15, 5:20] = (13, 1, 0); two[25:40, 30:50] = (13, 2, 0)            # two segments of one class in one image
    conv_set = [unified[('c19', 0, 0)], unified[('c19', 0, 2)], unified[('c19', 1, 1)]]
    ann, pans = BD._converter_2ch_single_core(0, [c.copy() for c in conv_set], Colors())
    out['conv_a_in'] = np.stack(conv_set); out['conv_a_pan'] = np.stack(pans); out['conv_a_ann'] = _jbytes(_py(ann))
    ann, pans = BD._converter_2ch_single_core(0, [two.copy(), unified[('c19', 2, 1)].copy()[:48, :64]], Colors())
    out['conv_b_in'] = np.stack([two, unified[('c19', 2, 1)][:48, :64]]); out['conv_b_pan'] = np.stack(pans); out['conv_b_ann'] = _jbytes(_py(ann))

    # ------------------------------------------------------------------ PQ
    imgs = pq_images()
    stat = BD._pq_compute_single_core(0, *[[copy.deepcopy(im[j]) for im in imgs] for j in range(5)], CATEGORIES)
    cats = sorted(CATEGORIES)
    out['pq_counts'] = np.array([[c, stat[c].tp, stat[c].fp, stat[c].fn] for c in cats], dtype=np.int64)
    out['pq_iou'] = np.array([stat[c].iou for c in cats], dtype=np.float64)
    assert out['pq_counts'][:, 1].sum() >= 6 and out['pq_counts'][:, 2].sum() >= 2 and out['pq_counts'][:, 3].sum() >= 4

    # ------------------------------------------------------------------ evaluate_panoptic (whole closure, one in-process worker)
    cfg.dataset.num_seg_classes, cfg.dataset.num_classes = 19, 9
    pred_2ch = [unified[('c19', ci, fi)] for ci, fi in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2))]
    gt_2ch = []
    for i, p in enumerate(pred_2ch):                      # ground truth: the prediction moved by a few pixels, one image unchanged
        g = np.roll(p, (i, 2 * i), (0, 1)).copy()
        if i == 1:
            g[:6, :9] = (255, 0, 0)                       # a void corner
        gt_2ch.append(g)
    gt_ann, gt_pans = BD._converter_2ch_single_core(0, [g.copy() for g in gt_2ch], Colors())
    gt_ann = _py(gt_ann)
    gt_ann[2]['segments_info'][-1]['iscrowd'] = 1
    images = [{'id': 'img%d' % i, 'file_name': 'img%d_leftImg8bit.png' % i, 'height': 64, 'width': 128} for i in range(len(pred_2ch))]
    categories = [{'id': c, 'name': 'c%d' % c, 'isthing': 1 if c >= 11 else 0, 'color': [c, c, c]} for c in range(19)]
    gt_json = {'images': images, 'annotations': gt_ann, 'categories': categories}
    with tempfile.TemporaryDirectory() as tmp:
        folder = os.path.join(tmp, 'panoptic'); os.makedirs(folder)
        for item, g in zip(images, gt_pans):
            Image.fromarray(g).save(os.path.join(folder, item['file_name']))
        with open(os.path.join(tmp, 'gt.json'), 'w') as f:
            json.dump(gt_json, f)
        base.multiprocessing = types.SimpleNamespace(cpu_count=lambda: 1, Pool=_Pool)
        this = types.SimpleNamespace(panoptic_json_file=os.path.join(tmp, 'gt.json'), panoptic_gt_folder=folder)
        outdir = os.path.join(tmp, 'out')
        with contextlib.redirect_stdout(io.StringIO()):
            results = BD.evaluate_panoptic(this, [p.copy() for p in pred_2ch], outdir)
        out['eval_pq_txt'] = np.frombuffer(open(os.path.join(outdir, 'pq.txt'), 'rb').read(), dtype=np.uint8)
        out['eval_pred_json'] = np.frombuffer(open(os.path.join(outdir, 'pred.json'), 'rb').read(), dtype=np.uint8)
        out['eval_pan'] = np.stack([np.array(Image.open(os.path.join(outdir, 'pan', 'img%d.png' % i))) for i in range(len(images))])
        two_back = np.stack([np.array(Image.open(os.path.join(outdir, 'pan_2ch', 'img%d.png' % i))) for i in range(len(images))])
        assert np.array_equal(two_back, np.stack(pred_2ch))
    out['eval_2ch'] = np.stack(pred_2ch); out['eval_gt_pan'] = np.stack(gt_pans); out['eval_gt_json'] = _jbytes(gt_json)
    out['eval_results'] = _jbytes(_py(results))
    assert results['All']['n'] > 3 and 0 < results['All']['pq'] < 1

    # ------------------------------------------------------------------ semantic confusion matrix + evaluate_ssegs
    for C in (19, 23):
        for name, (gt, pred) in confusion_inputs(C).items():
            seg_gt = gt.astype('float32')                                                   # cityscapes.py:122
            seg_pred = np.array(Image.fromarray(pred).resize((seg_gt.shape[1], seg_gt.shape[0]), Image.NEAREST))      # :128
            ignore_index = seg_gt != 255
            cm = BD.get_confusion_matrix(None, seg_gt[ignore_index], seg_pred[ignore_index], C)
            out['cm_c%d_%s' % (C, name)] = cm.astype(np.int64)
            assert np.array_equal(cm, cm.astype(np.int64))
    city = __import__('importlib').import_module('tools.dataset.cityscapes')
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'images')); os.makedirs(os.path.join(tmp, 'labels'))
        ins = confusion_inputs(19)
        names, preds, roidb = [], [], []
        for i, k in enumerate(('ragged', 'half', 'down', 'alias')):
            gt, pred = ins[k]
            stem = 'city_%06d_000019' % i
            Image.fromarray(gt).save(os.path.join(tmp, 'labels', stem + '_gtFine_labelTrainIds.png'))
            roidb.append({'image': os.path.join(tmp, 'images', stem + '_leftImg8bit.png')})
            names.append(stem + '_leftImg8bit.png'); preds.append(pred[None])
        this = types.SimpleNamespace(roidb=roidb)
        for m in ('write_segmentation_result', 'get_pallete', 'get_confusion_matrix'):
            setattr(this, m, types.MethodType(getattr(city.Cityscapes, m), this))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            city.Cityscapes.evaluate_ssegs(this, preds, os.path.join(tmp, 'ssegs'), names)
        np.set_printoptions()
        out['ssegs_stdout'] = np.frombuffer(buf.getvalue().encode(), dtype=np.uint8)
        with Image.open(os.path.join(tmp, 'ssegs', 'city_000000_000019.png')) as im:
            assert im.mode == 'P'
            out['ssegs_palette'] = np.array(im.getpalette(), dtype=np.uint8)
            assert np.array_equal(np.asarray(im), ins['ragged'][1])
    path = os.path.join(HERE, 'ipq_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
