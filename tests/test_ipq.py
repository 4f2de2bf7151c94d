"""Image-level evaluation, CPU side (the path of the reference's tools/test_eval_ipq.py): the NEAREST index tables against Pillow,
the NumPy restatements (tests/ipq_restate.py) against goldens of the REAL reference functions (tests/golden/make_ipq_golden.py ->
ipq_cases.npz), the palette PNG container, and the new C symbols' argument checks. The device path: tests/test_ipq_gpu.py."""
import io
import json
import os

import numpy as np
import pytest

import ipq_cases
import ipq_restate as R
import png_cases
import png_restate
from vps_amd import hip, ipq
from vps_amd import postprocess as pp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ipq_cases.npz')
TABLES = {'c19': (19, 9), 'c23': (23, 11)}


def gold():
    return np.load(GOLD)


def unify_clips(z, tag):
    for ci in range(int(z['unify_%s_nclips' % tag])):
        n = int(z['unify_%s_clip%d_n' % (tag, ci)])
        get = lambda k: [z['unify_%s_clip%d_f%d_%s' % (tag, ci, f, k)] for f in range(n)]      # noqa: E731
        yield ci, get('seg'), get('pan'), get('cls'), int(z['unify_%s_clip%d_limit' % (tag, ci)]), ['f%d' % f for f in range(n)], get('out')


def jload(z, key):
    return json.loads(z[key].tobytes().decode())


# (src w x h -> dst w x h); pairs five and six break floor((x + 0.5) * Wi / Wo)
SIZES = [((27, 19), (53, 37)), ((64, 32), (128, 64)), ((160, 96), (64, 48)), ((128, 64), (128, 64)), ((100, 50), (333, 167)),
         ((1000, 7), (17, 5)), ((17, 5), (1000, 3))]


@pytest.mark.parametrize('src,dst', SIZES, ids=['%dx%d-%dx%d' % (s + d) for s, d in SIZES])
def test_nearest_tables_equal_pillow(src, dst):
    from PIL import Image
    (ws, hs), (wd, hd) = src, dst
    index = np.arange(hs * ws, dtype=np.int32).reshape(hs, ws)
    want = np.asarray(Image.fromarray(index).resize((wd, hd), Image.NEAREST))
    ytab, xtab = ipq.nearest_tables((hs, ws), (hd, wd))
    assert ytab.dtype == np.int32 and xtab.dtype == np.int32 and ytab.shape == (hd,) and xtab.shape == (wd,)
    assert np.array_equal(index[ytab[:, None], xtab[None, :]], want)
    if src == dst:
        assert np.array_equal(ytab, np.arange(hd)) and np.array_equal(xtab, np.arange(wd))


def test_the_naive_formula_is_not_pillows_rule():
    """the reason the tables come from Pillow: pairs five and six differ from floor((x + 0.5) * Wi / Wo) somewhere"""
    for (ws, hs), (wd, hd) in SIZES[4:6]:
        ytab, xtab = ipq.nearest_tables((hs, ws), (hd, wd))
        ny = np.floor((np.arange(hd) + 0.5) * hs / hd).astype(np.int32)
        nx = np.floor((np.arange(wd) + 0.5) * ws / wd).astype(np.int32)
        assert not (np.array_equal(ytab, ny) and np.array_equal(xtab, nx))


@pytest.mark.parametrize('C', [19, 23])
def test_restated_confusion_matrix_equals_the_reference(C):
    z = gold()
    cases = ipq_cases.confusion_inputs(C)
    assert set(cases) == {'ragged', 'ident', 'half', 'down', 'uniform', 'noise', 'void', 'alias'}
    for name, (gt, pred) in cases.items():
        ytab, xtab = ipq.nearest_tables(pred.shape, gt.shape)
        cm = R.confusion_matrix(gt, pred, C, ytab, xtab)
        assert cm.dtype == np.float64 and np.array_equal(cm, z['cm_c%d_%s' % (C, name)]), name
    assert z['cm_c%d_void' % C].sum() == 0
    assert z['cm_c%d_uniform' % C][5, 5] == 64 * 128 and z['cm_c%d_uniform' % C].sum() == 64 * 128
    # a prediction >= class_num lands in a later cell; an index past the matrix is dropped
    alias = z['cm_c%d_alias' % C]
    cell = divmod(3 * C + 25, C)
    assert cell == {19: (4, 6), 23: (4, 2)}[C] and alias[cell] >= 300
    gt, pred = cases['alias']
    assert alias.sum() < ((gt != 255) & (gt < C)).sum()


def test_restated_miou_and_palette_equal_what_evaluate_ssegs_prints():
    z = gold()
    text = z['ssegs_stdout'].tobytes().decode()
    cases = ipq_cases.confusion_inputs(19)
    cm = np.zeros((19, 19))
    for k in ('ragged', 'half', 'down', 'alias'):
        gt, pred = cases[k]
        cm += R.confusion_matrix(gt, pred, 19, *ipq.nearest_tables(pred.shape, gt.shape))
    res = R.miou(cm)
    lines = text.splitlines()
    assert lines[0] == 'evaluate segmentation:' and lines[1] == 'IU_array:'
    assert lines[2:21] == ['%.5f' % v for v in res['IU_array']]
    assert lines[21] == 'meanIU:%.5f' % res['meanIU']
    assert np.array_equal(ipq.get_pallete(), z['ssegs_palette']) and ipq.get_pallete().dtype == np.uint8


@pytest.mark.parametrize('tag', sorted(TABLES))
def test_restated_unify_equals_the_reference(tag):
    z = gold()
    nseg, ncls = TABLES[tag]
    assert int(z['unify_%s_id_last_stuff' % tag]) == nseg - ncls
    ncase = absent = void = small = 0
    for ci, segs, pans, clss, limit, names, outs in unify_clips(z, tag):
        res = R.get_unified_pan_result(segs, pans, clss, limit, names, id_last_stuff=nseg - ncls)
        for n, o, pan, seg in zip(names, outs, pans, segs):
            assert res[n].dtype == np.uint8 and np.array_equal(res[n], o), (ci, n)
            assert not o[..., 2].any()                                             # channel 2 all zero
            ids = np.unique(pan); ids = ids[(ids > nseg - ncls) & (ids != 255)]
            absent += int(len(ids) and ids.max() - (nseg - ncls) != len(ids))      # an absent instance id: idx != id - 11
            void += int((pan == 255).any() and (o[..., 0][pan == 255] == 255).all())
            small += int(((o[..., 0] == 255) & (pan <= nseg - ncls)).any())        # stuff below the area limit
            ncase += 1
    assert ncase == 9 and absent >= 3 and void >= 2 and small >= 3


def test_restated_converter_equals_the_reference():
    z = gold()
    for s in ('a', 'b'):
        ann, pans = R.converter_2ch_single_core(list(z['conv_%s_in' % s]), ipq_cases.Colors())
        assert ann == jload(z, 'conv_%s_ann' % s)
        assert np.array_equal(np.stack(pans), z['conv_%s_pan' % s])
    # two segments of one class in one image: two colours, separate areas
    info = [el for el in jload(z, 'conv_b_ann')[0]['segments_info'] if el['category_id'] == 13]
    assert len(info) == 2 and info[0]['id'] != info[1]['id'] and [el['area'] for el in info] == [150, 300]
    assert info[0]['bbox'] == [5, 5, 14, 9] and info[1]['bbox'] == [30, 25, 19, 14]


def test_restated_pq_equals_the_reference():
    z = gold()
    imgs = ipq_cases.pq_images()
    stat = R.pq_compute_single_core(*[[im[j] for im in imgs] for j in range(5)], ipq_cases.CATEGORIES)
    counts, iou = R.stat_rows(stat, ipq_cases.CATEGORIES)
    assert np.array_equal(counts, z['pq_counts'])
    assert iou.tobytes() == z['pq_iou'].tobytes()                                  # bitwise-equal float64 sums
    # the cases the inputs were built for
    gt_json, pred_json, gt_pan, pred_pan, _ = imgs[0]
    assert sum(el['iscrowd'] for el in gt_json['segments_info']) == 1              # a crowd segment
    assert imgs[1][1]['segments_info'] == []                                       # an image with no predictions
    first = R.pq_compute_single_core(*[[im[j] for im in imgs[:1]] for j in range(5)], ipq_cases.CATEGORIES)
    assert first[13].fp == 1 and first[14].fp == 1                                 # 9100 (in the crowd) and 9102 (over VOID) are no false positives
    assert (first[11].tp, first[11].fn, first[12].tp, first[12].fn) == (0, 2, 2, 0)     # IoU 100/200 and 99/200 miss, 101/200 and 130/170 match


def test_restated_pq_raises_keyerror_for_a_png_id_missing_from_the_json():
    imgs = ipq_cases.pq_images()[:1]
    imgs[0][1]['segments_info'] = imgs[0][1]['segments_info'][:-1]
    with pytest.raises(KeyError):
        R.pq_compute_single_core(*[[im[j] for im in imgs] for j in range(5)], ipq_cases.CATEGORIES)


def test_pq_text_equals_the_reference_file():
    z = gold()
    results = jload(z, 'eval_results')
    results['per_class'] = {int(k): v for k, v in results['per_class'].items()}
    assert ipq.pq_text(results) == z['eval_pq_txt'].tobytes().decode()


def test_palette_png_container():
    from PIL import Image
    img = png_cases.cases()['ff_grey'].copy()
    img[::7, ::5] = 3; img[100:200, 50:400] = 18
    stream = png_restate.png_stream(img)
    pal = ipq.get_pallete().reshape(256, 3)
    data = pp.png_container(stream, img.shape[0], img.shape[1], 1, palette=pal)
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == 'P'
        assert np.array_equal(np.array(im.getpalette(), dtype=np.uint8), pal.reshape(-1))
        assert np.array_equal(np.asarray(im), img)
    with pytest.raises(AssertionError):
        pp.png_container(stream, img.shape[0], img.shape[1], 3, palette=pal)


@pytest.mark.parametrize('name', sorted(png_cases.cases()))
def test_container_without_a_palette_is_unchanged(name):
    img = png_cases.cases()[name]
    stream = png_restate.idat_of(png_cases.restated(name))
    assert pp.png_container(stream, img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3) == png_cases.restated(name)


def test_new_symbols_refuse_bad_arguments_without_a_gpu():
    lib = hip.load()
    assert lib.vps_abi_version() == 21
    assert lib.vps_sseg_confusion(None, 4, 4, None, 4, 4, None, None, 33, None, None) == -1001     # class_num first: nothing is launched
    assert lib.vps_sseg_confusion(None, 4, 4, None, 4, 4, None, None, 0, None, None) == -1001
    assert lib.vps_sseg_confusion(None, 4, 4, None, 4, 4, None, None, 19, None, None) <= -1000
    assert lib.vps_unify_tables_image(None, None, None, 0, 10, 100, None, None, None) <= -1000
    assert lib.vps_segment_stats_ch(None, 4, 4, 1, None, None) <= -1000
    assert lib.vps_segment_paint_ch(None, 16, 1, None, None, None) <= -1000
