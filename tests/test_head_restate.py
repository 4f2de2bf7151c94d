"""tests/head_restate.py (the numpy restatements the detection-head kernels are compared with on the GPU) pinned to the oracle
(oracle/fusetrack.py, the restatement of the reference's detector) on the CPU: whoever trusts the oracle can trust them."""
import copy

import numpy as np
import pytest
import torch

import head_restate as R
from oracle import fusetrack as OF
from oracle import ops as O


def _mask_roi_inputs(n, nc, seed, hot=0.35):
    """rois inside a 300 x 500 image, deltas as the box head scales them, probabilities WITHOUT ties (distinct float32 values)"""
    rg = np.random.default_rng(seed)
    x1 = rg.uniform(0, 400, n); y1 = rg.uniform(0, 220, n)
    rois = np.stack([np.zeros(n), x1, y1, x1 + rg.uniform(4, 120, n), y1 + rg.uniform(4, 90, n)], 1).astype(np.float32)
    delta = (rg.standard_normal((n, 4 * nc)) * 2.0).astype(np.float32)
    prob = rg.permutation(n * nc).reshape(n, nc).astype(np.float32) / np.float32(n * nc)       # distinct multiples of 1 / (n nc)
    prob = np.where(rg.random((n, nc)) < hot, 0.55 + 0.45 * prob, 0.5 * prob).astype(np.float32)
    assert np.unique(prob).size == prob.size
    return rois, delta, prob


@pytest.mark.parametrize('n,max_det,seed', [(60, 100, 0), (200, 100, 1), (200, 20, 2), (5, 100, 3)])
def test_maskroi_select_nms_finish_equals_oracle_mask_roi(n, max_det, seed):
    nc = 9
    rois, delta, prob = _mask_roi_inputs(n, nc, seed)
    cfg = dict(OF.CFG, max_det=max_det)
    im_info = np.array([[300., 500., 1.]], dtype=np.float32)
    sc, boxes, cls = OF.mask_roi(torch.from_numpy(rois), torch.from_numpy(delta), torch.from_numpy(prob), im_info, cfg, nc)
    dets, cand, m = R.maskroi_select(rois, delta, prob, None, nc, cfg['mask_roi']['score_thresh'], cfg['bbox_reg_weights'], (300., 500.))
    assert m[0] > 0 and m[1] == 0 and m[2] == n
    keep = O.nms_upsnet(dets, cfg['mask_roi']['nms_thresh'])
    assert len(keep) < m[0], 'the NMS suppresses something'
    head, rows = R.maskroi_finish(dets, cand, m, keep, len(keep), nc, max_det, 256)
    assert head.tolist() == [rows.shape[0], m[0], len(keep), 0, n]
    if max_det == 20:
        assert len(keep) > 20 and rows.shape[0] == 20
    assert np.array_equal(rows[:, 5], sc.numpy())
    assert np.array_equal(rows[:, 0:5], boxes.numpy())
    assert np.array_equal(rows[:, 6].astype(np.int64), cls.numpy())
    assert np.array_equal(rows[:, 7].astype(np.int64) % (nc - 1) + 1, cls.numpy())


def test_maskroi_empty_list_is_the_dummy_row():
    nc = 9
    rois, delta, prob = _mask_roi_inputs(12, nc, 5)
    prob = (prob * 0.5).astype(np.float32)
    im_info = np.array([[300., 500., 1.]], dtype=np.float32)
    sc, boxes, cls = OF.mask_roi(torch.from_numpy(rois), torch.from_numpy(delta), torch.from_numpy(prob), im_info, OF.CFG, nc)
    dets, cand, m = R.maskroi_select(rois, delta, prob, None, nc, 0.6, OF.CFG['bbox_reg_weights'], (300., 500.))
    assert m == [0, 0, 12] and dets.shape == (0, 5)
    head, rows = R.maskroi_finish(dets, cand, m, [], 0, nc, 100, 256)
    assert head.tolist() == [1, 0, 0, 0, 12]
    assert np.array_equal(rows[:, 5], sc.numpy()) and np.array_equal(rows[:, 0:5], boxes.numpy()) and np.array_equal(rows[:, 6], cls.numpy())


def test_maskroi_select_tie_order_and_strict_threshold():
    """equal scores: the larger candidate index first (a stable ascending argsort reversed); a probability equal to the threshold in
    float32 is no candidate; rows past n_valid are ignored"""
    nc = 3
    rois = np.array([[0, 0, 0, 9, 9]] * 4, dtype=np.float32)
    delta = np.zeros((4, 12), dtype=np.float32)
    prob = np.array([[0, .75, .6], [0, .875, .75], [0, .5, .75], [0, .99, .99]], dtype=np.float32)
    dets, cand, m = R.maskroi_select(rois, delta, prob, 3, nc, 0.6, (10., 10., 5., 5.), (20., 20.))
    assert cand.tolist() == [2, 5, 3, 0] and m == [4, 0, 3]
    ref = np.argsort(prob[:3, 1:].reshape(-1), kind='stable')[::-1]
    assert cand.tolist() == [q for q in ref if prob[:3, 1:].reshape(-1)[q] > np.float32(0.6)]
    assert dets[:, 4].tolist() == [.875, .75, .75, .75] and np.array_equal(dets[:, :4], np.array([[0, 0, 9, 9]] * 4, dtype=np.float32))


@pytest.mark.parametrize('K,M,seed', [(1, 1, 0), (30, 12, 1), (50, 5, 2), (8, 40, 3)])
def test_track_assign_ids_equal_greedy_assign(K, M, seed):
    rg = np.random.default_rng(seed)
    comp = rg.standard_normal((K, M + 1)).astype(np.float32)
    comp[:, 0] -= 0.5                                                       # most rows pick a memory entry: several per entry
    E = 5
    emb = rg.standard_normal((K, E)).astype(np.float32); box = rg.uniform(0, 100, (K, 5)).astype(np.float32)
    label = rg.integers(1, 9, K).astype(np.int64)
    pe = np.full((M + K, E), -7, np.float32); pb = np.full((M + K, 4), -7, np.float32); pl = np.full(M + K, -7, np.int64)
    ids, mem, ne, nb, nl = R.track_assign(comp, M, emb, box, label, pe, pb, pl)
    want, updates = OF.greedy_assign(torch.from_numpy(comp), M)
    assert np.array_equal(ids, want)
    assert mem == M + sum(u[0] == 'add' for u in updates) == max(int(ids.max()) + 1, M)
    assert sorted(ids.tolist()) == sorted(set(ids.tolist())), 'ids are unique'
    # a memory entry that some detection holds carries that detection's embedding and box; every id >= M is an appended row
    for i, d in enumerate(ids):
        assert np.array_equal(ne[d], emb[i]) and np.array_equal(nb[d], box[i, :4])
        assert nl[d] == (label[i] if d >= M else -7)
    assert (ne[mem:] == -7).all() and (nb[mem:] == -7).all() and (nl[mem:] == -7).all()
    assert pe.min() == -7 and pe.max() == -7, 'the inputs are copied, not written'


def test_track_assign_first_maximum_on_ties():
    comp = np.array([[1., 1., 0., 1.], [0., 2., 2., 2.], [0., 0., 0., 3.]], dtype=np.float32)
    assert torch.max(torch.from_numpy(comp), dim=1)[1].tolist() == np.argmax(comp, axis=1).tolist() == [0, 1, 3]


def test_rpn_collect_equals_the_tail_of_rpn_get_bboxes():
    """oracle.fusetrack.rpn_get_bboxes on three small levels; the per-level part (sort, top nms_pre, decode, NMS) is redone here to
    get the sorted box lists and kept positions the kernel is handed, the concatenation + top-k is the restatement's"""
    g = torch.Generator().manual_seed(3)
    cfg = copy.deepcopy(OF.CFG)
    cfg['anchor_strides'] = [4, 8, 16]
    cfg['rpn'] = dict(nms_pre=50, nms_post=50, max_num=40, nms_thr=0.7, min_bbox_size=0)
    shapes = [(8, 8), (4, 4), (2, 2)]                                       # 192 (> nms_pre), 48 and 12 anchors
    outs = [(torch.randn(1, 3, h, w, generator=g) * 2, torch.randn(1, 12, h, w, generator=g) * 0.3) for h, w in shapes]
    img_shape = (32, 32)
    want = OF.rpn_get_bboxes(outs, img_shape, cfg).numpy()
    nmax = cfg['rpn']['nms_pre']
    boxes = np.zeros((3, nmax, 5), np.float32); keep = np.zeros((3, nmax), np.int64); nkeep = []
    for l, (cls, reg) in enumerate(outs):
        scores = cls[0].permute(1, 2, 0).reshape(-1).sigmoid()
        assert scores.unique().numel() == scores.numel()
        anchors = OF.grid_anchors(OF.gen_base_anchors(cfg['anchor_strides'][l], cfg['anchor_scales'], cfg['anchor_ratios']), cls.shape[-2:],
                                  cfg['anchor_strides'][l])
        order = torch.sort(scores, descending=True)[1][:nmax]
        props = OF.delta2bbox(anchors[order], reg[0].permute(1, 2, 0).reshape(-1, 4)[order], (0., 0., 0., 0.), (1., 1., 1., 1.), img_shape)
        k = O._greedy_nms_sorted(props.numpy(), cfg['rpn']['nms_thr'])
        boxes[l, :len(order)] = torch.cat([props, scores[order, None]], 1).numpy()
        keep[l, :len(k)] = k; nkeep.append(len(k))
    assert sum(nkeep) > 40 and nkeep[0] < nmax
    out, n = R.rpn_collect(boxes, keep, nkeep, cfg['rpn']['nms_post'], cfg['rpn']['max_num'])
    assert n == 40 == want.shape[0] and np.array_equal(out, want)
    # fewer boxes than max_num: rows >= n are zero
    out, n = R.rpn_collect(boxes, keep, nkeep, 3, 60)
    assert n == 9 and (out[9:] == 0).all() and np.array_equal(out[:9, 4], np.sort(np.concatenate([boxes[l, keep[l, :3], 4] for l in range(3)]))[::-1])


def test_pan_instances_crop_is_the_seg_term_crop():
    """the crop oracle.fusetrack.seg_term copies (half-integer x2 / y2: numpy rounds half to even) and the nothing-kept record"""
    rows = np.zeros((5, 8), dtype=np.float32)
    rows[:, 1:5] = [[2.7, 3.2, 10.5, 11.5], [0., 0., 12.49, 12.51], [5.9, 1.1, 11.5, 10.5], [1., 1., 2.5, 3.5], [4., 4., 8., 8.]]
    rows[:, 6] = [1, 3, 8, 2, 0]
    seg = torch.zeros(1, 19, 24, 24)
    seg[0, 11:] = 1.0
    _, inst = OF.seg_term(torch.from_numpy(rows[:, 6]).long(), seg, torch.from_numpy(rows[:, 0:5] * 4.0))
    for i in range(5):
        nz = inst[0, i].nonzero()
        sx0, sy0, sx1, sy1 = R.seg_crop(rows[i])
        if rows[i, 6] == 0:
            assert nz.numel() == 0
            continue
        assert (int(nz[:, 1].min()), int(nz[:, 0].min()), int(nz[:, 1].max()) + 1, int(nz[:, 0].max()) + 1) == (sx0, sy0, sx1, sy1)
    assert [R.seg_crop(r)[2:] for r in rows[:4]] == [(11, 13), (13, 14), (13, 11), (3, 5)]
    cm = {c: 10 + c for c in range(1, 9)}
    inst, keep, k = R.pan_instances([3, 0, 4, 1, 2], [1, 0, 1, 0, 1], rows, np.arange(20).reshape(5, 4), cm)
    assert keep.tolist() == [3, 4, 2] and k == [3, 1]
    assert inst.tolist() == [[1, 1, 3, 5, 12, 0, 1, 2, 3, 3], [0, 0, 0, 0, 0, 8, 9, 10, 11, 4], [5, 1, 13, 11, 18, 16, 17, 18, 19, 2]]
    inst, keep, k = R.pan_instances([3, 0, 4, 1, 2], [0] * 5, rows, np.arange(20).reshape(5, 4), cm)
    assert keep.tolist() == [0] and k == [1, 0] and inst.tolist() == [[2, 3, 11, 13, 11, 0, 0, -1, -1, 0]]
    inst, keep, k = R.pan_instances(None, None, np.array([[0, 0, 0, 0, 0, 1, 0, 0]], np.float32), None, cm)
    assert keep.tolist() == [0] and k == [1, 0] and inst.tolist() == [[0, 0, 0, 0, 0, 0, 0, -1, -1, 0]]
