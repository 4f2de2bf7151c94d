"""tests/pan_restate.py (the numpy restatements the kernels of vps_amd/csrc/pan_ops.hip are compared with on the GPU) pinned to the
oracle (oracle/fusetrack.py, oracle/ops.py) on the CPU, on the inputs of tests/test_pan_ops_gpu.py - and the conditions those GPU
comparisons rely on: the exclusion cap of the margin rule and "every MaskRemoval list is decisive". A changed seed that breaks one
of them fails here, not on the GPU machine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pan_restate as R
from oracle import fusetrack as OF
from oracle import ops as O

EXCLUDED_CAP = 0.002                  # of a case's pixels: what the margin rule may take out of the exact comparison


def _fcn_output(case):
    s = torch.from_numpy(case['score'][:, :, :case['nclass']]).permute(2, 0, 1)[None].contiguous()
    return F.interpolate(s, None, case['up'], mode='bilinear', align_corners=False)


def _oracle_argmax(logits):
    """panoptic_fusetrack.py:590-593, torch.max(F.softmax(logits, 1), 1)[1] - but where the softmax rounds DIFFERENT logits to one
    largest probability, the arg-max of the logits"""
    p = F.softmax(logits, dim=1)
    by_p, by_l = torch.max(p, dim=1)[1], torch.max(logits, dim=1)[1]
    same_p = (p == p.max(dim=1, keepdim=True)[0]).sum(1)
    same_l = (logits == logits.max(dim=1, keepdim=True)[0]).sum(1)
    return torch.where(same_p != same_l, by_l, by_p)[0].numpy()


def _cfg(case):
    nthings = case['nclass'] - case['nstuff']
    return dict(OF.CFG, num_stuff=case['nstuff'], class_mapping={c: case['nstuff'] + c - 1 for c in range(1, nthings + 1)})


@pytest.mark.parametrize('name', R.EXACT_CASES)
def test_upsample_and_exact_cases_equal_the_oracle_composition(name):
    """family A: float32 upsample == F.interpolate bit for bit, float64 == float32 (the arithmetic is exact), and the restated maps equal
    SegTerm's crops (written into the instance channels as unary_logits.py:106 does) + zero mask energy + cat + softmax + max"""
    case = R.exact_case(name)
    fcn = _fcn_output(case)
    score = case['score'][:, :, :case['nclass']]
    assert np.array_equal(R.upsample(score, case['up'], np.float32), fcn[0].numpy())
    assert np.array_equal(R.upsample(score, case['up'], np.float64), fcn[0].numpy().astype(np.float64))
    a = (score, case['up'], case['nstuff'], case['insts'], case['masks'])
    pan, sem = R.combine(*a, np.float32)
    pan64, sem64 = R.combine(*a, np.float64)
    assert np.array_equal(pan, pan64) and np.array_equal(sem, sem64)
    inst = torch.zeros(1, len(case['insts']), fcn.shape[2], fcn.shape[3])
    for j, it in enumerate(case['insts']):
        x0, y0, x1, y1 = (int(v) for v in it[:4])
        inst[0, j, y0:y1, x0:x1] = fcn[0, int(it[R.SEG_CH]), y0:y1, x0:x1]
    logits = torch.cat([fcn[:, :case['nstuff']], inst + torch.zeros(1, 1, fcn.shape[2], fcn.shape[3])], dim=1)
    if logits.shape[1]:
        assert np.array_equal(pan, _oracle_argmax(logits))
    assert np.array_equal(sem, _oracle_argmax(fcn))
    ties = int((R.margins(R.pan_logits(*a, np.float64)) == 0).sum()) if logits.shape[1] > 1 else 0
    if name not in ('k0', 'k1_nothing'):
        assert ties >= 400, 'equal logits are common: first-maximum-wins is tested at %d pixels' % ties
    if name.startswith('chunk'):
        # the winner everywhere is an instance that adds exactly 0; in most tiles only the first-skipped rule lists it
        assert pan.min() >= case['nstuff'] + 5 and len(np.unique(pan)) >= 3


@pytest.mark.parametrize('name', list(R.RANDOM_CASES))
def test_random_cases_equal_the_oracle_composition_and_keep_the_exclusion_cap(name):
    """family B: the float32 restatement equals seg_term + mask_removal's mask_energy + cat + softmax + max of oracle/fusetrack.py bit for
    bit (on the instances whose mask the oracle pastes: a threshold of 2 keeps every box with a positive pixel), and the margin rule
    excludes at most 0.2 % of the case's pixels, with the float32 restatement itself passing it"""
    case = R.random_case(name)
    fcn = _fcn_output(case)
    H, W = fcn.shape[2:]
    k = len(case['insts'])
    mi = case['insts'][:, R.MASK_IDX]
    prob = np.linspace(0.9, 0.1, k).astype(np.float32)                            # the walk visits the instances in table order
    keep, energy = R.oracle_mask_removal(case['boxes'], prob, case['masks'][mi], case['cls'], (H, W), 2.0)
    assert max(1, k // 2 - 2) <= len(keep) <= k
    rois = torch.cat([torch.zeros(len(keep), 1), torch.from_numpy(case['clipped'][keep]) * 4.0], dim=1)
    stuff, inst = OF.seg_term(torch.from_numpy(case['cls'][keep]), fcn, rois, _cfg(case))
    want = _oracle_argmax(torch.cat([stuff, inst + energy], dim=1))
    score = case['score'][:, :, :case['nclass']]
    pan, sem = R.combine(score, case['up'], case['nstuff'], case['insts'][keep], case['masks'], np.float32)
    assert np.array_equal(pan, want)
    assert np.array_equal(sem, _oracle_argmax(fcn))
    # the bound and the cap, on the whole table
    bound, dist, p64, s64 = R.margin_bound(case)
    print('%s: float32 vs float64 %.3g, bound %.3g' % (name, dist, bound))
    assert 1e-7 < bound < 2e-5, 'a float32 rounding distance on logits of about 10'
    pan, sem = R.combine(score, case['up'], case['nstuff'], case['insts'], case['masks'], np.float32)
    ex = 0
    for got, l64 in ((pan, p64), (sem, s64)):
        wrong, wrong_excluded, excluded = R.margin_compare(got, l64, bound)
        assert wrong == 0 and wrong_excluded == 0
        ex += excluded
    print('%s: %d of %d pixels excluded' % (name, ex, H * W))
    assert ex <= EXCLUDED_CAP * H * W


def test_margin_compare_sees_a_wrong_pixel_a_tie_and_an_excluded_one():
    l64 = np.zeros((3, 1, 4))
    l64[:, 0, 0] = (1, 5, 2)           # clear
    l64[:, 0, 1] = (5, 5, 2)           # structural tie: the lowest index
    l64[:, 0, 2] = (5, 5 - 1e-7, 2)    # inside the bound: excluded, 0 or 1 pass
    l64[:, 0, 3] = (1, 2, 5)
    assert R.margin_compare(np.array([[1, 0, 1, 2]]), l64, 1e-6) == (0, 0, 1)
    assert R.margin_compare(np.array([[1, 1, 0, 2]]), l64, 1e-6) == (1, 0, 1)
    assert R.margin_compare(np.array([[2, 0, 2, 2]]), l64, 1e-6) == (1, 1, 1)
    assert R.margin_compare(np.array([[1, 0, 1, 90]]), l64, 1e-6) == (1, 0, 1)


@pytest.mark.parametrize('w,h', [(1, 1), (1, 40), (7, 3), (28, 28), (29, 27), (56, 56), (97, 13), (300, 5)])
def test_resize_linear_equals_the_oracle_resize(w, h):
    for S in (28, 7):
        m = (np.random.default_rng(w * 100 + h).standard_normal((S, S)) * 2 + 0.6).astype(np.float32)
        assert np.array_equal(R.resize_linear(m, w, h, np.float32), O.cv2_resize_linear(m, (w, h)))
        assert np.abs(R.resize_linear(m, w, h, np.float64) - O.cv2_resize_linear(m, (w, h))).max() < 1e-5
    b = (-3, 2, w - 4, h + 1)
    p = R.pasted_logit(m, b, 20, 30, np.float32)
    if p is not None:
        full = R.resize_linear(m, w, h, np.float32)
        assert np.array_equal(p[0], full[p[3] - b[1]:p[4] - b[1], p[1] - b[0]:p[2] - b[0]])


@pytest.mark.parametrize('name', list(R.REMOVAL_LISTS) + ['thr30', 'thr31'])
def test_mask_removal_walk_equals_the_oracle_and_every_list_is_decisive(name):
    rows, masks = R.removal_list(name)
    walk, unsure_bound, dist = R.removal_walk(rows, masks)
    print('%s: resized logits float32 vs float64 %.3g, unsure_bound %.3g' % (name, dist, unsure_bound))
    keep, _ = R.oracle_mask_removal(rows[:, 1:5], rows[:, 5], masks, rows[:, 6], R.REMOVAL_HW, R.REMOVAL_THR)
    assert np.array_equal(walk['keep_inds'], keep)
    assert walk['decisive'].all(), 'the kept list does not depend on pixels whose logit is within %g of zero' % unsure_bound
    walk64, _, _ = R.removal_walk(rows, masks, np.float64)
    assert np.array_equal(walk64['keep_inds'], keep)
    assert unsure_bound <= 7e-6 * float(np.abs(masks).max()), "inside the single-box test's 7e-6 max|m28|"
    n = len(rows)
    if name.startswith('n40'):
        assert 5 <= len(keep) <= n - 5 and (walk['ov'] > 0).sum() >= 10, 'crowded: boxes are dropped for their overlap'
    if name == 'thr30':
        assert walk['ms'].tolist() == [0, 100, 1, 100] and walk['ov'].tolist() == [0, 0, 0, 30] and keep.tolist() == [0, 1, 2]
    if name == 'thr31':
        assert walk['ms'].tolist() == [0, 100, 1, 100] and walk['ov'].tolist() == [0, 0, 0, 31] and keep.tolist() == [0, 1]


def test_walk_flags_a_list_that_is_not_decisive():
    """a box whose overlap ratio sits at the threshold with unsure pixels, and one whose positive pixels are all unsure"""
    m = np.ones((3, 4, 4), dtype=np.float32)
    m[1, :, 0] = 1e-7                                   # resized: the first column of box 1 (it lies on box 0) is unsure
    boxes = np.array([[0, 0, 9, 9], [7, 0, 16, 9], [40, 40, 41, 41]], dtype=np.int32)
    m[2] = 1e-7
    w = R.mask_removal_walk(boxes, np.zeros(3, np.int64), m, np.arange(3), 64, 96, 0.3, np.float32, 1e-6)
    assert w['u'][1] > 0 and not w['decisive'][1] and not w['decisive'][2] and w['decisive'][0]


def test_recorded_figures_are_the_measured_ones():
    """tests/tolerances.py PAN_OPS_MEASURED is a record of what the derived bounds came from: it follows the inputs"""
    from tolerances import PAN_OPS_MEASURED as M
    for name, want in M['combine_f32_vs_f64'].items():
        assert abs(R.margin_bound(R.random_case(name))[1] - want) <= 0.02 * want, name
    for name, want in M['removal_resized_f32_vs_f64'].items():
        assert abs(R.removal_walk(*R.removal_list(name))[2] - want) <= 0.02 * want, name
