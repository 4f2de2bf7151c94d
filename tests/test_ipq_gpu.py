"""Image-level evaluation on the device (vps_amd/ipq.py over csrc/ipq_ops.hip) against goldens of the REAL reference functions
(tests/golden/ipq_cases.npz) and the NumPy restatements (tests/ipq_restate.py). Every comparison is exact."""
import contextlib
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ipq_cases
import ipq_restate as R
from test_ipq import TABLES, gold, jload, unify_clips
from vps_amd import hip, ipq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _restated(C, name):
    gt, pred = ipq_cases.confusion_inputs(C)[name]
    return R.confusion_matrix(gt, pred, C, *ipq.nearest_tables(pred.shape, gt.shape))


@pytest.mark.parametrize('C', [19, 23])
def test_confusion_matrix_equals_the_reference(dev, C):
    """each case on its own evaluator: ragged 37x53 <- 19x27, identity, 2x up, down, one class everywhere, per-pixel noise, all-255
    labels, predictions 25 / 255 (aliased / dropped)"""
    z = gold()
    for name, (gt, pred) in ipq_cases.confusion_inputs(C).items():
        ev = ipq.SemanticEvaluator(C, dev)
        ev.add(gt, torch.from_numpy(pred).to(dev))
        cm = ev.result()['confusion_matrix']
        assert cm.dtype == np.float64 and cm.shape == (C, C)
        assert np.array_equal(cm, z['cm_c%d_%s' % (C, name)]), name
        assert np.array_equal(cm, _restated(C, name)), name
    alias = ipq.SemanticEvaluator(C, dev)
    alias.add(*ipq_cases.confusion_inputs(C)['alias'])
    cm = alias.result()['confusion_matrix']
    assert cm[{19: (4, 6), 23: (4, 2)}[C]] >= 300                     # gt 3, pred 25
    assert cm[C - 1].sum() == z['cm_c%d_alias' % C][C - 1].sum()      # gt C-1, pred 255: dropped


@pytest.mark.parametrize('C', [19, 23])
def test_confusion_accumulates_without_synchronisation_and_carries_into_64_bits(dev, C):
    ev = ipq.SemanticEvaluator(C, dev)
    want = np.zeros((C, C))
    for name in ('ragged', 'half', 'noise'):                          # three images, no synchronisation between the calls
        ev.add(*ipq_cases.confusion_inputs(C)[name])
        want += _restated(C, name)
    res = ev.result()
    assert np.array_equal(res['confusion_matrix'], want)
    ref = R.miou(want)
    assert res['meanIU'] == ref['meanIU'] and np.array_equal(res['IU_array'], ref['IU_array'])
    # one call into a buffer pre-loaded with 2^31 - 5 in the cell every pixel of the uniform map goes to
    ev = ipq.SemanticEvaluator(C, dev)
    ev.counts[5 * C + 5] = 2 ** 31 - 5
    ev.add(*ipq_cases.confusion_inputs(C)['uniform'])
    got = ev.counts.cpu().numpy()
    assert got.dtype == np.int64 and got[5 * C + 5] == 2 ** 31 - 5 + 64 * 128 and got.sum() == got[5 * C + 5]


def test_confusion_refuses_more_than_32_classes(dev):
    gt, pred = ipq_cases.confusion_inputs(19)['ident']
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    counts = torch.full((33 * 33,), 7, dtype=torch.int64, device=dev)
    rc = hip.load().vps_sseg_confusion(hip.ptr(g), 64, 128, hip.ptr(p), 64, 128, None, None, 33, hip.ptr(counts), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1001 and bool((counts == 7).all())
    with pytest.raises(hip.VpsHipError):
        ipq.SemanticEvaluator(33, dev).add(gt, pred)
    # 32 is the last size served: against the restatement
    ev = ipq.SemanticEvaluator(32, dev)
    ev.add(gt, pred)
    assert np.array_equal(ev.result()['confusion_matrix'], R.confusion_matrix(gt, pred, 32))


def test_evaluate_ssegs_prints_what_the_reference_prints_and_writes_palette_pngs(dev, tmp_path):
    from PIL import Image
    z = gold()
    ins = ipq_cases.confusion_inputs(19)
    names, preds, gt_paths = [], [], []
    for i, k in enumerate(('ragged', 'half', 'down', 'alias')):
        gt, pred = ins[k]
        stem = 'city_%06d_000019' % i
        gt_paths.append(str(tmp_path / (stem + '_gtFine_labelTrainIds.png')))
        Image.fromarray(gt).save(gt_paths[-1])
        names.append(stem + '_leftImg8bit.png')
        preds.append(torch.from_numpy(pred[None]).to(dev))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ipq.SemanticEvaluator(19, dev).evaluate_ssegs(preds, str(tmp_path / 'ssegs'), names, gt_paths)
    assert buf.getvalue() == z['ssegs_stdout'].tobytes().decode()
    for i, k in enumerate(('ragged', 'half', 'down', 'alias')):
        with Image.open(tmp_path / 'ssegs' / ('city_%06d_000019.png' % i)) as im:
            assert im.mode == 'P' and np.array_equal(np.array(im.getpalette(), dtype=np.uint8), z['ssegs_palette'])
            assert np.array_equal(np.asarray(im), ins[k][1])


@pytest.mark.parametrize('tag', sorted(TABLES))
def test_image_unify_equals_the_reference(dev, tag):
    z = gold()
    nseg, ncls = TABLES[tag]
    for ci, segs, pans, clss, limit, names, outs in unify_clips(z, tag):
        u = ipq.ImagePanopticUnifier(dev, num_seg_classes=nseg, num_classes=ncls)
        res = u.get_unified_pan_result([torch.from_numpy(s).to(dev) for s in segs], pans, clss, limit, names)
        for n, o in zip(names, outs):
            assert res[n].dtype == np.uint8 and np.array_equal(res[n], o), (ci, n)
            assert not res[n][..., 2].any()


def test_image_unify_raises_indexerror_without_a_cls_ind_entry(dev):
    z = gold()
    ci, segs, pans, clss, limit, names, outs = next(unify_clips(z, 'c19'))
    with pytest.raises(IndexError):
        ipq.ImagePanopticUnifier(dev).get_unified_pan_result(segs[:1], pans[:1], [clss[0][:2]], limit, names[:1])
    with pytest.raises(IndexError):
        R.get_unified_pan_result(segs[:1], pans[:1], [clss[0][:2]], limit, names[:1])


def test_image_converter_equals_the_reference(dev):
    z = gold()
    conv = ipq.ImageConverter(dev)
    for s in ('a', 'b'):
        ann, pans = conv.convert([torch.from_numpy(m).to(dev) for m in z['conv_%s_in' % s]], ipq_cases.Colors())
        assert ann == jload(z, 'conv_%s_ann' % s)                       # ids follow the order of the colour draws
        assert np.array_equal(np.stack(pans), z['conv_%s_pan' % s])
    info = [el for el in ann[0]['segments_info'] if el['category_id'] == 13]
    assert len(info) == 2 and info[0]['id'] != info[1]['id'] and [el['area'] for el in info] == [150, 300]
    # a ragged size against the restatement
    m = z['conv_a_in'][0][:37, :53].copy()
    ann, pans = conv.convert([m], ipq_cases.Colors())
    ann_r, pans_r = R.converter_2ch_single_core([m], ipq_cases.Colors())
    assert ann == ann_r and np.array_equal(pans[0], pans_r[0])


def test_pq_single_core_equals_the_reference(dev):
    z = gold()
    imgs = ipq_cases.pq_images()
    args = [[im[j] for im in imgs] for j in range(5)]
    args[2] = [torch.from_numpy(a).to(dev) for a in args[2]]            # maps may be device tensors or arrays
    stat = ipq.pq_compute_single_core(*args, ipq_cases.CATEGORIES, dev)
    counts, iou = R.stat_rows(stat, ipq_cases.CATEGORIES)
    assert np.array_equal(counts, z['pq_counts'])
    assert iou.tobytes() == z['pq_iou'].tobytes()


def test_pq_single_core_raises_keyerror_for_a_png_id_missing_from_the_json(dev):
    imgs = ipq_cases.pq_images()[:1]
    imgs[0][1]['segments_info'] = imgs[0][1]['segments_info'][:-1]
    with pytest.raises(KeyError, match='presented in PNG and not presented in JSON'):
        ipq.pq_compute_single_core(*[[im[j] for im in imgs] for j in range(5)], ipq_cases.CATEGORIES, dev)
    imgs = ipq_cases.pq_images()[:1]
    imgs[0][1]['segments_info'].append({'id': 77, 'category_id': 12, 'iscrowd': 0, 'area': 1})
    with pytest.raises(KeyError, match='presented in JSON and not presented in PNG'):
        ipq.pq_compute_single_core(*[[im[j] for im in imgs] for j in range(5)], ipq_cases.CATEGORIES, dev)


def test_evaluate_panoptic_writes_the_reference_files(dev, tmp_path):
    from PIL import Image
    z = gold()
    gt_json = jload(z, 'eval_gt_json')
    want = jload(z, 'eval_results')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        results = ipq.evaluate_panoptic([torch.from_numpy(m).to(dev) for m in z['eval_2ch']], str(tmp_path), copy.deepcopy(gt_json),
                                        list(z['eval_gt_pan']), None, ipq_cases.Colors(), device=dev)
    assert sorted(os.listdir(tmp_path)) == ['gt.json', 'pan', 'pan_2ch', 'pq.txt', 'pred.json']
    assert (tmp_path / 'pq.txt').read_text() == z['eval_pq_txt'].tobytes().decode()
    assert json.load(open(tmp_path / 'pred.json')) == jload(z, 'eval_pred_json')
    assert json.load(open(tmp_path / 'gt.json')) == gt_json
    for i in range(len(gt_json['images'])):
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'pan' / ('img%d.png' % i))), z['eval_pan'][i])
        assert np.array_equal(np.asarray(Image.open(tmp_path / 'pan_2ch' / ('img%d.png' % i))), z['eval_2ch'][i])
    for k in ('All', 'Things', 'Stuff'):
        assert results[k] == want[k]                                     # floats equal to the last bit
    assert {str(k): v for k, v in results['per_class'].items()} == want['per_class']
    assert buf.getvalue().startswith('PQ_All: %s\n' % repr(100 * want['All']['pq']))


def test_run_ipq_dry_run_scores_itself_at_pq_100(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_ipq.py'), '--dry-run', '--height', '128', '--width', '256',
                          '--work-dir', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'PQ_All: 100.0' in out.stdout and 'meanIU over the classes present: 1.00000' in out.stdout
