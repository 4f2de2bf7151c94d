"""The code that PQ, VPQ, boundary PQ and boundary VPQ share (vps_amd/evaluate.py: `pair_table`, `count_frame`, `match`, `window_sums`,
`pq_results`, `pq_text`), on the CPU through the NumPy pair table of tests/numpy_seam.py, and `pair_table` itself on the device."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import boundary_restate as R
import ipq_cases
import ipq_restate
import test_boundary as TB
import test_evaluate as TE
from numpy_seam import numpy_device, numpy_pair_table          # noqa: F401 (fixture)
from test_ipq import gold, jload
from vps_amd import boundary, ipq
from vps_amd import evaluate as ev


def _columns(images):
    return [[im[j] for im in images] for j in range(5)]


# ---------------------------------------------------------------------------------------------- image PQ: the host half of ipq.py
def test_image_pq_host_logic_equals_the_reference(numpy_device):
    z = gold()
    imgs = ipq_cases.pq_images()
    for im in imgs:
        for el in im[1]['segments_info']:
            el['area'] = -1
    args = _columns(imgs)
    args[2] = [torch.from_numpy(a) for a in args[2]]                       # maps may be tensors or arrays
    stat = ipq.pq_compute_single_core(*args, ipq_cases.CATEGORIES, 'cpu')
    counts, iou = ipq_restate.stat_rows(stat, ipq_cases.CATEGORIES)
    assert np.array_equal(counts, z['pq_counts'])
    assert iou.tobytes() == z['pq_iou'].tobytes()                          # bitwise-equal float64 sums
    for im in imgs:                                                        # the caller's entries carry the PNG's pixel counts
        ids = R.ids_of(im[3])
        assert all(el['area'] == int((ids == el['id']).sum()) > 0 for el in im[1]['segments_info'])
    assert sum(len(im[1]['segments_info']) for im in imgs) > 20


def test_image_pq_keyerrors_name_the_image(numpy_device):
    def run(change):
        imgs = ipq_cases.pq_images()[:1]
        change(imgs[0][1]['segments_info'])
        ipq.pq_compute_single_core(*_columns(imgs), ipq_cases.CATEGORIES, 'cpu')
    with pytest.raises(KeyError, match=re.escape('In the image with ID a segment with ID 9104 is presented in PNG and not presented in JSON.')):
        run(lambda info: info.pop())
    with pytest.raises(KeyError, match=re.escape('In the image with ID a the following segment IDs [77] are presented in JSON and not presented in PNG.')):
        run(lambda info: info.append({'id': 77, 'category_id': 12, 'iscrowd': 0, 'area': 1}))
    with pytest.raises(KeyError, match=re.escape('In the image with ID a segment with ID 9104 has unknown category_id 40.')):
        run(lambda info: info[-1].update(category_id=40))


# ---------------------------------------------------------------------------------------------- FrameCounts.count through the seam
def test_frame_counts_through_the_seam_equal_the_numpy_count(numpy_device):
    fc = ev.FrameCounts('cpu')
    nframes = 0
    for ci in range(4):
        frames = next(f for c, nf, f, _, _ in TE._clips() if c == ci)
        clip_ids = sorted({el['id'] for f in frames for el in f[0]['segments_info']})
        for gt_json, pred_json, gt_pan, pred_pan, _ in frames:
            got = fc.count(gt_json, pred_json, gt_pan, pred_pan, TE.CATS, clip_ids)
            assert got == TE._numpy_count(None, gt_json, pred_json, gt_pan, pred_pan, TE.CATS, clip_ids)
            assert list(got[2]) == sorted(got[2])                          # ascending gt id, then pred id
            nframes += 1
    assert nframes >= 12
    # an id that the frame's PNG paints and its own JSON does not list: counted only when `extra_gt_ids` brings it
    gt_json, pred_json, gt_pan, pred_pan, _ = frames[0]
    painted = [el for el in gt_json['segments_info'] if (R.ids_of(gt_pan) == el['id']).any()]
    gone = painted[-1]['id']
    short = {'segments_info': [el for el in gt_json['segments_info'] if el['id'] != gone]}
    with_extra = fc.count(short, pred_json, gt_pan, pred_pan, TE.CATS, [gone])
    assert with_extra == TE._numpy_count(None, short, pred_json, gt_pan, pred_pan, TE.CATS, [gone])
    assert gone not in with_extra[0] and any(g == gone for g, _ in with_extra[2])
    without = fc.count(short, pred_json, gt_pan, pred_pan, TE.CATS)
    assert without == TE._numpy_count(None, short, pred_json, gt_pan, pred_pan, TE.CATS) and not any(g == gone for g, _ in without[2])
    # the VPQ wording of the consistency errors: no image id
    bad = {'segments_info': pred_json['segments_info'][1:]}
    with pytest.raises(KeyError, match=re.escape('Segment with ID %d is presented in PNG and not presented in JSON.' % pred_json['segments_info'][0]['id'])):
        fc.count(gt_json, bad, gt_pan, pred_pan, TE.CATS)
    extra = {'segments_info': pred_json['segments_info'] + [{'id': 12345, 'category_id': 3, 'iscrowd': 0, 'area': 1}]}
    with pytest.raises(KeyError, match=re.escape('The following segment IDs [12345] are presented in JSON and not presented in PNG.')):
        fc.count(gt_json, extra, gt_pan, pred_pan, TE.CATS)


# ---------------------------------------------------------------------------------------------- one cache dict for both VPQ evaluators
def _rows(stat, cats):
    return [(c, stat[c].tp, stat[c].fp, stat[c].fn, stat[c].iou, getattr(stat[c], 'biou', None)) for c in cats]


def test_one_cache_dict_never_hands_one_evaluators_entry_to_the_other(numpy_device):
    clip = TB._clip()
    shared = {}
    for nf in (1, 2, 3):
        plain = ev.vpq_compute_single_core(clip, TB.CATS, nframes=nf, device='cpu', _cache=shared)
        band = boundary.vpq_compute_single_core(clip, TB.CATS, nframes=nf, device='cpu', _cache=shared)
        assert _rows(plain, TB.CATS) == _rows(ev.vpq_compute_single_core(clip, TB.CATS, nframes=nf, device='cpu', _cache={}), TB.CATS)
        assert _rows(band, TB.CATS) == _rows(boundary.vpq_compute_single_core(clip, TB.CATS, nframes=nf, device='cpu', _cache={}), TB.CATS)
        assert plain[TB.CAR].tp > 0 and band[TB.CAR].biou > 0
    assert len(shared) == 2 * len(clip)                                    # every frame once per evaluator, whatever the window length
    other = boundary.vpq_compute_single_core(clip, TB.CATS, nframes=1, device='cpu', _cache=shared, boundary_ratio=0.05)
    assert len(shared) == 3 * len(clip) and _rows(other, TB.CATS) == _rows(
        boundary.vpq_compute_single_core(clip, TB.CATS, nframes=1, device='cpu', boundary_ratio=0.05), TB.CATS)


# ---------------------------------------------------------------------------------------------- mask IoU above 1
def test_iou_above_one_is_refused_by_the_tube_evaluators_and_matched_by_the_image_ones(numpy_device):
    """6 x 6, d = 1. Ground truth and prediction paint the same 3 x 4 block (rows 1..3, columns 1..4: 12 pixels), the rest is void, but the
    ground-truth JSON says area 6. Mask: intersection 12, prediction over void 0, union 12 + 6 - 12 - 0 = 6, IoU 12 / 6 = 2.
    Band: only (2, 2) and (2, 3) have their 3 x 3 window inside the block, so each band has 10 pixels, all common: 10 / (10 + 10 - 10 - 0) = 1.
    The reference's image evaluator has no check: a true positive with IoU 2 (PQ) or min(2, 1) = 1 (boundary PQ). Its tube evaluator asserts."""
    m = np.zeros((6, 6), dtype=np.int64); m[1:4, 1:5] = 5
    gt_json = {'segments_info': [TB.seg(5, TB.CAR, 6)]}
    pred_json = {'segments_info': [{'id': 5, 'category_id': TB.CAR, 'area': 12}]}
    pan = R.pan_of(m)
    assert boundary.dilation(6, 6) == 1 and R.mask_to_boundary(m == 5, 1).sum() == 10
    one = ([gt_json], [pred_json], [pan], [pan], [{}])
    car = ipq.pq_compute_single_core(*copy.deepcopy(one), TB.CATS, 'cpu')[TB.CAR]
    assert (car.tp, car.fp, car.fn, car.iou) == (1, 0, 0, 2.0)
    car = boundary.pq_compute_single_core(*copy.deepcopy(one), TB.CATS, 'cpu')[TB.CAR]
    assert (car.tp, car.fp, car.fn, car.iou, car.biou) == (1, 0, 0, 1.0, 1.0)
    clip = [(gt_json, pred_json, pan, pan, {})]
    for fn in (ev.vpq_compute_single_core, boundary.vpq_compute_single_core):
        with pytest.raises(AssertionError, match='INVALID IOU VALUE : 5'):
            fn(clip, TB.CATS, nframes=1, device='cpu')


# ---------------------------------------------------------------------------------------------- the table text
def test_shared_writer_and_eval_vpq_device_write_the_reference_layout(numpy_device, monkeypatch, tmp_path):
    z = gold()
    results = jload(z, 'eval_results')
    results['per_class'] = {int(k): v for k, v in results['per_class'].items()}
    want = z['eval_pq_txt'].tobytes().decode()
    assert ev.pq_text(results) == want
    # the tool writes what `pq_results` hands it through the same writer: with the golden results, the golden file
    monkeypatch.setattr(ev, 'pq_results', lambda stat, categories: results)
    submit, truth, gj, _ = TE._write_dataset(tmp_path, (0, 3))
    TE._load_cli().main(['--submit_dir', submit, '--truth_dir', truth, '--pan_gt_json_file', gj, '--nframes_per_video', '5', '--device', 'cpu'])
    for k in (0, 5, 10, 15):
        assert open(os.path.join(submit, 'vpq-%d.txt' % k)).read() == want
    assert open(os.path.join(submit, 'vpq-final.txt')).read() == ''.join('vpq_%s:%.4f\n' % (n, 100 * results[k]['pq'])
                                                                         for n, k in (('all', 'All'), ('thing', 'Things'), ('stuff', 'Stuff')))


# ---------------------------------------------------------------------------------------------- the device seam itself
@pytest.mark.gpu
def test_pair_table_on_the_device_equals_its_numpy_definition(dev):
    """7 x 13 maps: 91 pixels, no multiple of the kernel's 8 pixels per thread or of its block. Ids in every byte of the colour, the
    largest 24-bit one among them; 77 and 300 are painted and not listed, so the extra row, the extra column and their corner fill."""
    listed = np.array([0, 1, 255, 256, 65536, (1 << 24) - 1], dtype=np.int64)
    yy, xx = np.mgrid[0:7, 0:13]
    gt = np.concatenate([listed, [77]])[(yy * 13 + xx) % 7]
    pr = np.concatenate([listed, [300]])[(3 * yy + xx // 2) % 7]
    cases = [(gt, pr, listed, listed), (gt, pr, np.array([0], dtype=np.int64), np.array([0], dtype=np.int64)),
             (gt, pr, listed[:3], listed), (np.zeros_like(gt), pr, listed, listed[1:])]
    for g, p, gt_ids, pred_ids in cases:
        g_host, p_host = torch.from_numpy(R.pan_of(g)), torch.from_numpy(R.pan_of(p))
        want = numpy_pair_table(g_host, p_host, gt_ids, pred_ids, None)
        got = ev.pair_table(ev.pan_tensor(R.pan_of(g), dev), ev.pan_tensor(p_host.to(dev), dev), gt_ids, pred_ids, dev)
        assert got.dtype == np.int64 and got.shape == (len(gt_ids) + 1, len(pred_ids) + 1) and np.array_equal(got, want)
        assert got.sum() == 91
    full = numpy_pair_table(torch.from_numpy(R.pan_of(gt)), torch.from_numpy(R.pan_of(pr)), listed, listed, None)
    assert full[-1, -1] > 0 and full[-1, :-1].sum() > 0 and full[:-1, -1].sum() > 0 and (full[:-1, :-1].sum(1) > 0).all()
