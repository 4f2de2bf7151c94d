"""Kernel-level tests of vps_amd/csrc/pan_ops.hip: the fused panoptic combine (vps_panoptic_combine, vps_panoptic_combine_dev) through
the C ABI with instance tables built here, and the four MaskRemoval routes against the oracle's kept list. The yardstick is
tests/pan_restate.py (dense numpy restatements of the reference's host code, pinned to the oracle by tests/test_pan_restate.py, which
also asserts on the CPU what the comparisons here rely on: the exclusion cap and "every MaskRemoval list is decisive").

Family A compares whole maps exactly (exact arithmetic, thousands of tied pixels); family B compares under a margin rule whose
bound the test derives from the float32 restatement's own distance to float64 (figures in tests/tolerances.py). Every output map is
allocated with guard rows of 0x5a bytes before and after it and compared WHOLE, guards included."""
import ctypes

import numpy as np
import pytest
import torch

import pan_restate as R
from vps_amd import hip

pytestmark = pytest.mark.gpu

SENT, GUARD = 0x5a, 3
EXCLUDED_CAP = 0.002


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _table(dev, insts):
    """the vps_pan_inst table of insts [k, 10] (one spare sentinel entry behind it: the entry points want a pointer even for k = 0)"""
    assert ctypes.sizeof(hip.PanInst) == 40
    t = np.full((len(insts) + 1, 10), 0x5a5a5a5a, dtype=np.int32)
    t[:len(insts)] = insts
    return _up(dev, t)


def _combine(dev, case, entry, k=None, H=None, W=None):
    """-> (return code, pan buffer, sem buffer [GUARD + H + GUARD, W] uint8 as numpy, k_dev as a list or None)"""
    score = _up(dev, case['score'])
    Hs, Ws, ld = score.shape
    Ho, Wo = H or Hs * case['up'], W or Ws * case['up']
    inst = _table(dev, case['insts'])
    masks = _up(dev, case['masks'])
    k = len(case['insts']) if k is None else k
    bufs = [torch.full((GUARD + Ho + GUARD, Wo), SENT, dtype=torch.uint8, device=dev) for _ in range(2)]
    ptrs = [ctypes.c_void_p(b.data_ptr() + GUARD * Wo) for b in bufs]
    lib = hip.load()
    k_dev = None
    if entry == 'host':
        rc = lib.vps_panoptic_combine(hip.ptr(score), ld, Hs, Ws, case['nclass'], case['nstuff'], hip.ptr(inst), k, hip.ptr(masks),
                                      masks.shape[-1], ptrs[0], ptrs[1], Ho, Wo, hip.stream_ptr())
    else:
        k_dev = _up(dev, np.array([k, -7, 0, -7], dtype=np.int32))
        rc = lib.vps_panoptic_combine_dev(hip.ptr(score), ld, Hs, Ws, case['nclass'], case['nstuff'], hip.ptr(inst), hip.ptr(k_dev), hip.ptr(masks),
                                          masks.shape[-1], ptrs[0], ptrs[1], Ho, Wo, hip.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(score.cpu().numpy(), case['score']), 'the scores are read only'
    return rc, bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), None if k_dev is None else k_dev.cpu().tolist()


def _guarded(m):
    out = np.full((GUARD + m.shape[0] + GUARD, m.shape[1]), SENT, dtype=np.uint8)
    out[GUARD:GUARD + m.shape[0]] = m
    return out


def _diff(got, want):
    bad = np.argwhere(got != want)
    return '%d bytes differ, first (row, col, got, want): %s' % (len(bad), [(int(r) - GUARD, int(c), int(got[r, c]), int(want[r, c])) for r, c in bad[:6]])


# ------------------------------------------------------------------------------------------------ family A
@pytest.mark.parametrize('name', R.EXACT_CASES)
def test_combine_exact_cases_equal_the_restatement_everywhere(dev, name):
    """exact float32 arithmetic, zero mask logits: pan and sem equal the restatement at EVERY pixel - the per-tile instance list (ballot,
    popcount, 64-instance chunks), the first-skipped rule, first-maximum-wins at exactly tied pixels, the staged texels (up 2: 18 x 6 =
    the cap; up 8) and the unstaged reads (up 1, 33 classes), score_ld > nclass, nstuff = 0 and nstuff = nclass, ragged last tiles;
    both entry points give the same bytes"""
    case = R.exact_case(name)
    pan, sem = R.combine(case['score'][:, :, :case['nclass']], case['up'], case['nstuff'], case['insts'], case['masks'], np.float32)
    want_pan, want_sem = _guarded(pan), _guarded(sem)
    rc, gp, gs, _ = _combine(dev, case, 'host')
    assert rc == 0
    assert np.array_equal(gp, want_pan), 'pan: ' + _diff(gp, want_pan)
    assert np.array_equal(gs, want_sem), 'sem: ' + _diff(gs, want_sem)
    rc, dp, ds, k_dev = _combine(dev, case, 'dev')
    assert rc == 0 and k_dev == [len(case['insts']), -7, 0, -7]
    assert np.array_equal(dp, gp) and np.array_equal(ds, gs), 'vps_panoptic_combine_dev differs from vps_panoptic_combine'


# ------------------------------------------------------------------------------------------------ family B
@pytest.mark.parametrize('name', list(R.RANDOM_CASES))
def test_combine_random_cases_under_the_margin_rule(dev, name):
    """random scores, masks and boxes (overhanging every edge; a 1-pixel, an outside, an inverted and a whole-image box): per pixel, with
    m = the float64 margin between the two largest logits and bound = 4 x max|float32 - float64 restatement| of the case (at least one
    float32 ulp of the largest logit): m > bound or m == 0 (a structural tie, the lowest index wins) -> the float64 first arg-max;
    0 < m <= bound -> excluded, but a channel within bound of the maximum. At most 0.2 % of the pixels are excluded."""
    case = R.random_case(name)
    bound, dist, p64, s64 = R.margin_bound(case)
    H, W = p64.shape[1:]
    res = {}
    for entry in ('host', 'dev'):
        rc, gp, gs, k_dev = _combine(dev, case, entry)
        assert rc == 0 and (k_dev is None or k_dev == [len(case['insts']), -7, 0, -7])
        excluded = 0
        for what, got, l64 in (('pan', gp, p64), ('sem', gs, s64)):
            frame = got.copy(); frame[GUARD:GUARD + H] = SENT
            assert (frame == SENT).all(), '%s: guard rows written' % what
            wrong, wrong_excluded, ex = R.margin_compare(got[GUARD:GUARD + H], l64, bound)
            print('%s %s %s: float32 vs float64 %.3g, bound %.3g, %d wrong, %d excluded (%d of them out of range)' % (name, entry, what, dist, bound, wrong, ex, wrong_excluded))
            assert wrong == 0 and wrong_excluded == 0, (what, wrong, wrong_excluded)
            excluded += ex
        assert excluded <= EXCLUDED_CAP * H * W
        res[entry] = (gp, gs)
    assert np.array_equal(res['host'][0], res['dev'][0]) and np.array_equal(res['host'][1], res['dev'][1])


# ------------------------------------------------------------------------------------------------ refusals and bounds
def _many_nothing(k):
    """the 13 x 22 scores of family A with k instances that add nothing"""
    case = R.exact_case('k0')
    case['insts'] = np.array([R._inst((0, 0, 0, 0), 11) for _ in range(k)], dtype=np.int32)
    return case


def test_combine_refuses_more_instances_than_the_uint8_map_names(dev):
    """nstuff = 11: 244 instances are the most. The device-count entry raises bit 0 of k_dev[2] and writes NOTHING for 245, and
    writes every pixel for 244; the host-count entry returns -1002"""
    case = _many_nothing(245)
    rc, gp, gs, k_dev = _combine(dev, case, 'dev')
    assert rc == 0 and k_dev == [245, -7, 1, -7]
    assert (gp == SENT).all() and (gs == SENT).all()
    rc, gp, gs, _ = _combine(dev, case, 'host')
    assert rc == -1002 and (gp == SENT).all() and (gs == SENT).all()
    case = _many_nothing(244)
    pan, sem = R.combine(case['score'], case['up'], case['nstuff'], case['insts'], case['masks'], np.float32)
    for entry in ('dev', 'host'):
        rc, gp, gs, k_dev = _combine(dev, case, entry)
        assert rc == 0 and (k_dev is None or k_dev == [244, -7, 0, -7])
        assert np.array_equal(gp, _guarded(pan)) and np.array_equal(gs, _guarded(sem))
    assert (pan != SENT).all() and (sem != SENT).all(), 'every pixel is written with something else than the sentinel'


def test_combine_argument_checks(dev):
    """made before any launch: nothing is written"""
    case = R.exact_case('k5_borders')
    for entry in ('host', 'dev'):
        for H, W in ((53, 88), (52, 89), (52, 44), (26, 88)):                  # not a multiple of the score map; two different factors
            rc, gp, gs, _ = _combine(dev, case, entry, H=H, W=W)
            assert rc == -1003 and (gp == SENT).all() and (gs == SENT).all(), (entry, H, W, rc)
    lib = hip.load()
    score, inst, masks = _up(dev, case['score']), _table(dev, case['insts']), _up(dev, case['masks'])
    out = torch.full((52, 88), SENT, dtype=torch.uint8, device=dev)
    k_dev = _up(dev, np.array([5, -7, 0, -7], dtype=np.int32))
    for s, p, m in ((None, out, out), (score, None, out), (score, out, None)):
        assert lib.vps_panoptic_combine(hip.ptr(s), 19, 13, 22, 19, 11, hip.ptr(inst), 5, hip.ptr(masks), 28, hip.ptr(p), hip.ptr(m), 52, 88, hip.stream_ptr()) == -1001
        assert lib.vps_panoptic_combine_dev(hip.ptr(s), 19, 13, 22, 19, 11, hip.ptr(inst), hip.ptr(k_dev), hip.ptr(masks), 28, hip.ptr(p), hip.ptr(m), 52, 88,
                                            hip.stream_ptr()) == -1001
    torch.cuda.synchronize()
    assert (out == SENT).all() and k_dev.cpu().tolist() == [5, -7, 0, -7]


# ------------------------------------------------------------------------------------------------ MaskRemoval against the oracle
MODES = ('hist', 'dep', 'level', 'single')


def _removal_modes(dev, rows, masks):
    """P.MaskRemoval(0.3) on the list through each of its four routes -> {mode: (kept list, occupancy planes != 0 or None)}"""
    from vps_amd import nhwc
    from vps_amd import panoptic_ops as P
    H, W = R.REMOVAL_HW
    ncls = int(rows[:, 6].max())
    rows_d, masks_d = _up(dev, rows), _up(dev, masks)
    cm = {c: 10 + c for c in range(1, ncls + 1)}
    res = {}
    old = P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH, P.HIST_MAX_PAIRS
    P.HIST_MAX_PAIRS = 10 ** 9
    try:
        for mode in MODES:
            P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH = mode, mode == 'single'
            ws = nhwc.Workspace(dev)
            out = P.MaskRemoval(R.REMOVAL_THR)(rows, rows_d, masks_d, (H, W), ws, cm)
            torch.cuda.synchronize()
            kinfo = out['kinfo'].cpu().numpy()
            assert kinfo[2] == 0 and kinfo[1] == 1, (mode, kinfo)
            assert ('mr.hist' in ws.bufs) == (mode == 'hist'), 'the route that was asked for ran'
            occ = None if mode == 'hist' else ws.bufs['mr.occ'].ne(0).cpu().numpy().copy()
            res[mode] = (out['keep'][:int(kinfo[0])].cpu().numpy().astype(np.int64), occ)
    finally:
        P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH, P.HIST_MAX_PAIRS = old
    return res


@pytest.mark.parametrize('name', list(R.REMOVAL_LISTS) + ['thr30', 'thr31'])
def test_mask_removal_routes_equal_the_oracle_kept_list(dev, name):
    """every route's kept list equals oracle.fusetrack.mask_removal's keep_inds EXACTLY (legitimate: every list is decisive, asserted on the
    CPU and again here) and the occupancy planes equal the restatement's wherever the resized logit is further than unsure_bound from
    zero. thr30 / thr31: all-ones masks, 30 of 100 pixels overlap -> 30 / 100 > 0.3 is false, kept; 31 -> dropped; a box outside the
    image has mask_sum == 0 -> dropped."""
    rows, masks = R.removal_list(name)
    walk, unsure_bound, dist = R.removal_walk(rows, masks)
    assert walk['decisive'].all()
    want, _ = R.oracle_mask_removal(rows[:, 1:5], rows[:, 5], masks, rows[:, 6], R.REMOVAL_HW, R.REMOVAL_THR)
    assert np.array_equal(walk['keep_inds'], want)
    if name.startswith('thr'):
        assert want.tolist() == ([0, 1, 2] if name == 'thr30' else [0, 1])
    print('%s: resized logits float32 vs float64 %.3g, unsure_bound %.3g, %d unsure pixels' % (name, dist, unsure_bound, int(walk['unsure'].sum())))
    for mode, (keep, occ) in _removal_modes(dev, rows, masks).items():
        assert np.array_equal(keep, want), (mode, keep.tolist(), want.tolist())
        if occ is not None:
            sure = ~walk['unsure']
            assert occ.shape == walk['occ'].shape and np.array_equal(occ[sure], walk['occ'][sure]), (mode, int((occ != walk['occ'])[sure].sum()))
