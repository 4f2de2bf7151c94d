"""GPU: SURVEY.md 8(d) config 2 at the BASELINE frame size (1024x2048) — head-side inputs INJECTED at the operator boundaries
(`simple_test(..., inject=...)`: neck_out, fcn_score, proposals, cls_score, bbox_pred, mask_score), so that the order-defining
logic of the reference runs on controlled detection sets:

    K in {0 -> MaskROI dummy row, 32, 100, >100 with ties at the max_det cap, >244 -> refusal}, tracker memory M in {0, 32, 100},
    MaskRemoval keeping nothing / its overlap rule, SegTerm's cls==0 skip, the tracker's "undo" branch.

Checker: tests/golden/inject_cases.npz — the REAL reference functions (`MaskROI.forward`, the tracking block of
`simple_test_bboxes`, `MaskRemoval.forward`, `SegTerm.forward`, the logit concat / arg-max) run on the same tensors by
tests/golden/make_inject_golden.py. Everything integer must be identical (detections and their order, track ids, kept list,
returned vectors); maps may differ in < 0.1 % of the pixels (bilinear x4 + arg-max at logit ties). Run in BOTH split-operand
arithmetic modes (the track embeddings go through the conv kernels); tests/test_inject_golden.py pins the oracle on the same file.
"""
import os

import numpy as np
import pytest
import torch

import golden_npz
import inject_cases as IC
import vps_amd
from inject_cases import CASES, H, W
from oracle import fusetrack as OF
from test_inject_golden import check_against_golden
from vps_amd import hip, nhwc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'inject_cases.npz')


@pytest.fixture(scope='module', params=['f16x3', 'bf16x6'])
def model(dev, request):
    """f16x3 = the benchmarked arithmetic (bench.py default), bf16x6 = the unrestricted fp32-grade mode"""
    old = nhwc.DEFAULT_PREC
    nhwc.DEFAULT_PREC = {'f16x3': hip.PREC_F16X3, 'bf16x6': hip.PREC_BF16X6}[request.param]
    try:
        cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
        m = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        sd = synth.load_synth(m, 0)
        m.ensure_packed(dev)
    finally:
        nhwc.DEFAULT_PREC = old
    frames = [f.to(dev) for f in synth.synth_clip(H, W, 2, 0)]
    x = [l.to(dev) for l in IC.neck_features()]
    return m, sd, frames, x, golden_npz.load(GOLD)


@pytest.mark.parametrize('case', list(CASES))
def test_injected_heads_match_real_reference_at_full_size(dev, model, case):
    m, sd, frames, x, g = model
    m._cache = None; m.reset_tracker()
    for t, inj in enumerate(IC.frames_of(case)):
        pub = IC.public(inj)
        pub['neck_out'] = x
        out = m.simple_test(frames[t], [synth.img_meta(H, W, 10000 + t + 1)], ref_img=[frames[t - 1 if t else 0]], inject=pub)
        torch.cuda.synchronize()
        hd = m._aux['det']
        p = '%s.f%d.' % (case, t)
        r = {k: v.cpu().numpy() for k, v in out[2].items()}
        comp = None if hd['comp_scores'] is None else hd['comp_scores'].cpu().numpy()
        print('%s frame %d: K=%d (golden %d) kept %d' % (case, t, hd['cls_idx'].numel(), g[p + 'mask_roi_cls_idx'].shape[0], len(m._aux['keep_inds'])))
        check_against_golden(g, p, (hd['cls_prob'].cpu().numpy(), hd['det_rois'].cpu().numpy(), hd['cls_idx'].cpu().numpy()), comp,
                             np.asarray(hd['det_obj_ids']), m._aux['keep_inds'], r, [int(k) for k in out[0].keys()],
                             r['panoptic_outputs'], r['fcn_outputs'], score_tol=1e-6, comp_tol=2e-3, map_tol=1e-3)
        if IC.CASES[case][t].get('masks') == 'negative':
            assert not m._aux.get('masks_valid', True)                                                        # mask_removal.py:89-91


def test_more_than_244_instances_is_refused_loudly(dev, model):
    """the uint8 panoptic map names at most 244 instances (11 + k <= 255, 255 = VOID, test_vpq.py:51-56); the reference
    silently wraps, vps_panoptic_combine refuses"""
    m, sd, frames, x, g = model
    m._cache = None; m.reset_tracker()
    inj = IC.make_inject(5, 300, tie_from=10)
    o = OF.FuseTrackOracle(sd)
    x = [torch.zeros(1, 256, H // s, W // s) for s in (4, 8, 16, 32, 64)]
    with torch.no_grad():
        det = o.detect(x, (H, W), True, IC.public(inj))
    assert det['cls_idx'].numel() > 244, 'the case must produce more than 244 detections (got %d)' % det['cls_idx'].numel()
    with pytest.raises(hip.VpsHipError):
        m.simple_test(frames[0], [synth.img_meta(H, W, 10001)], ref_img=[frames[0]], inject=IC.public(inj))
        torch.cuda.synchronize()
    m._cache = None; m.reset_tracker()


@pytest.mark.parametrize('mode', ['dep', 'hist'])
def test_mask_removal_expired_dependency_wait_is_recovered_not_raised(dev, model, mode):
    """VERDICT r5 next #5 / ADVICE r5: when a box of the one-launch MaskRemoval gives up waiting for a box it depends on (status bit 2
    of vps_mask_removal_dep), the detector repeats MaskRemoval + combine through the per-level launches instead of raising. The expiry
    is forced (VPS_MR_SPIN_LIMIT=0: a box that finds a dependency unfinished at its first poll gives up) on the golden case with 20
    same-class overlapping detections; results must equal the golden of the REAL reference like the undisturbed run's. `hist` (round 6
    default): the same recovery after a full pattern table of vps_mask_removal_hist (forced: a table of one entry)."""
    from vps_amd import panoptic_ops as P
    m, sd, frames, x, g = model
    case = 'overlap_skip'
    old = os.environ.get('VPS_MR_SPIN_LIMIT')
    os.environ['VPS_MR_SPIN_LIMIT'] = '0'
    os.environ['VPS_MR_HIST_CAP'] = '1'         # ... or, in `hist` mode (round 6 default), finds its pattern table full
    before = P.MR_RECOVERIES[0]
    old_mode = P.MASK_REMOVAL_MODE
    P.MASK_REMOVAL_MODE = mode
    try:
        m._cache = None; m.reset_tracker()
        for t, inj in enumerate(IC.frames_of(case)):
            pub = IC.public(inj)
            pub['neck_out'] = x
            out = m.simple_test(frames[t], [synth.img_meta(H, W, 10000 + t + 1)], ref_img=[frames[t - 1 if t else 0]], inject=pub)
            torch.cuda.synchronize()
            hd = m._aux['det']
            p = '%s.f%d.' % (case, t)
            r = {k: v.cpu().numpy() for k, v in out[2].items()}
            comp = None if hd['comp_scores'] is None else hd['comp_scores'].cpu().numpy()
            check_against_golden(g, p, (hd['cls_prob'].cpu().numpy(), hd['det_rois'].cpu().numpy(), hd['cls_idx'].cpu().numpy()), comp,
                                 np.asarray(hd['det_obj_ids']), m._aux['keep_inds'], r, [int(k) for k in out[0].keys()],
                                 r['panoptic_outputs'], r['fcn_outputs'], score_tol=1e-6, comp_tol=2e-3, map_tol=1e-3)
    finally:
        P.MASK_REMOVAL_MODE = old_mode
        os.environ.pop('VPS_MR_HIST_CAP', None)
        if old is None:
            os.environ.pop('VPS_MR_SPIN_LIMIT', None)
        else:
            os.environ['VPS_MR_SPIN_LIMIT'] = old
    assert P.MR_RECOVERIES[0] > before, 'the forced failure did not happen: the test exercised nothing'
    m._cache = None; m.reset_tracker()
