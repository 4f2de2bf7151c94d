"""The two sibling detectors of the reference: PanopticFuse (no track head) and PanopticTrack (no FlowNet2 /
temporal fusion neck). CPU: the oracle with the branch switched off against golden vectors of the REAL reference classes
(tests/golden/make_golden.py fuse|track, which also asserts that the state_dict keys of our classes equal the reference's).
GPU: the HIP path against those vectors and the oracle."""
import os

import numpy as np
import pytest
import torch

import golden_npz
import vps_amd
from oracle.fusetrack import FuseTrackOracle
from vps_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {'fuse': dict(with_fusion=True, with_track=False), 'track': dict(with_fusion=False, with_track=True)}


def _gold(v):
    return golden_npz.load(os.path.join(ROOT, 'tests', 'golden', '%s_clip.npz' % v))


def _model(v):
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', '%s.py' % v))
    return vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)


def _close(a, b, rtol=1e-4, atol=1e-4):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b)
    assert (err <= atol + rtol * np.abs(b)).all(), 'max err %.3e (ref max %.3e)' % (err.max(), np.abs(b).max())


def _check_outputs(v, t, r, gold, pix_tol):
    p = 'f%d.' % t
    assert np.array_equal(np.asarray(r['panoptic_cls_inds']), gold[p + 'panoptic_cls_inds'])
    _close(np.asarray(r['panoptic_cls_prob']), gold[p + 'panoptic_cls_prob'], 1e-4, 1e-5)
    if VARIANTS[v]['with_track']:
        assert np.array_equal(np.asarray(r['panoptic_det_labels']), gold[p + 'panoptic_det_labels'])
        assert np.array_equal(np.asarray(r['panoptic_det_obj_ids']), gold[p + 'panoptic_det_obj_ids'])
    else:
        assert 'panoptic_det_obj_ids' not in r and 'panoptic_det_labels' not in r          # panoptic_fuse.py:467-472
    pan = np.asarray(r['panoptic_outputs']).astype(np.uint8); sem = np.asarray(r['fcn_outputs']).astype(np.uint8)
    assert (pan != gold[p + 'panoptic_outputs']).mean() < pix_tol and (sem != gold[p + 'fcn_outputs']).mean() < pix_tol


@pytest.mark.parametrize('v', ['fuse', 'track'])
def test_oracle_variant_matches_reference_class(v):
    gold = _gold(v)
    H, W, n, seed = [int(x) for x in gold['meta']]
    m = _model(v)
    assert type(m).__name__ == {'fuse': 'PanopticFuse', 'track': 'PanopticTrack'}[v]
    sd = synth.synth_state_dict({k: x.shape for k, x in m.state_dict().items()}, seed)
    o = FuseTrackOracle(sd, **VARIANTS[v])
    frames = synth.synth_clip(H, W, n, seed)
    with torch.no_grad():
        for t in range(n):
            r = o.simple_test(frames[t], frames[t - 1] if t else frames[0], t == 0, return_aux=True)
            p = 'f%d.' % t
            _close(r['pre_neck'][0][0, :8].numpy(), gold[p + 'fpn_p2'])
            _close(r['fcn_score'][0].numpy(), gold[p + 'fcn_score'], 5e-4, 5e-4)
            _close(r['det']['cls_score'].numpy(), gold[p + 'cls_score'], 5e-4, 5e-4)
            if VARIANTS[v]['with_fusion']:
                _close(r['feats'][0][0, :8].numpy(), gold[p + 'neck_out_p2'], 2e-4, 2e-4)
            _check_outputs(v, t, {k: (x.numpy() if torch.is_tensor(x) else x) for k, x in r.items() if k.startswith(('panoptic', 'fcn_outputs'))},
                           gold, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('v', ['fuse', 'track'])
def test_hip_variant_matches_reference_class(dev, v):
    gold = _gold(v)
    H, W, n, seed = [int(x) for x in gold['meta']]
    m = _model(v)
    synth.load_synth(m, seed)
    frames = synth.synth_clip(H, W, n, seed)
    for t in range(n):
        out = m(return_loss=False, rescale=True, img=[frames[t].to(dev)], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                ref_img=[frames[t - 1 if t else 0].to(dev)])
        torch.cuda.synchronize()
        r = {k: x.cpu().numpy() for k, x in out[2].items()}
        _check_outputs(v, t, r, gold, 1e-3)
        p = 'f%d.' % t
        a = m._aux
        _close(a['levels'][0].to_nchw().cpu().numpy()[0, :8], gold[p + 'fpn_p2'], 2e-3, 2e-3 * float(np.abs(gold[p + 'fpn_p2']).max()))
        _close(a['fcn_score'].to_nchw().cpu().numpy()[0], gold[p + 'fcn_score'], 2e-3, 2e-3 * float(np.abs(gold[p + 'fcn_score']).max()))
        if v == 'fuse':
            assert isinstance(out[0], list) and [len(b) for b in out[0]] == gold[p + 'bbox_counts'].tolist()   # per-class box lists
        else:
            assert sorted(int(k) for k in out[0].keys()) == gold[p + 'bbox_ids'].tolist()
            assert a['flow'] is None
