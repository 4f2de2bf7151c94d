"""GPU: STRICT parity at the BASELINE frame sizes on decidable fixtures (VERDICT r2 "Next round" #1, r3 #3).

Three fixtures, each a golden of the REAL reference detector (tests/golden/make_golden.py) on a synthetic clip whose box-classification
layer `bbox_head.fc_cls` was FITTED (a weighted ridge regression on the shared-FC features) so that every listing decision of the clip -
MaskROI's 0.6 threshold, the order of the kept scores, every IoU the class-agnostic NMS compares with 0.5 - has a margin well above the
measured score error of the HIP path; the margins are stored in the .npz next to the weights and asserted by CPU tests:

  separated  4 frames at 1024x2048, 4..14 detections per frame  (search_separated.py; margins 4.2e-2 / 2.5e-2 / 0.4)
  dense      6 frames at 1024x2048, 32..53 detections per frame, track ids to 180  (search_dense.py, oracle margins only: 2.3e-2 / 4.3e-3 / 0.21)
  config5    3 frames at 1088x1920, ResNet-101 (BASELINE config 5), objectness layer rescaled against tied RPN scores
             (VPS_SEP_CONFIG5=1 search_separated.py, oracle margins only: 4.3e-2 / 2.7e-2 / 0.25)

On such clips "identical instance-id assignment" is decidable, so it is asserted with `array_equal` - no bijection, no unmatched
detection - in ALL THREE fp32-grade arithmetic modes, the benchmarked f16x3 included:

  * panoptic_cls_inds, panoptic_det_labels, panoptic_det_obj_ids, the id keys of the box results: identical arrays;
  * panoptic_cls_prob and the stage tensors within the fixture's tolerance (2e-3 max|ref|; 1e-2 for the 101-layer model);
  * panoptic / semantic maps: < 0.1 % differing pixels (separated); the dense / config5 fixtures bound the boundary strip of single
    instances (0.5 % / 1 %) and print where the differing pixels sit.

tests/test_oracle_golden.py checks the oracle against the same files on the CPU.
"""
import os

import numpy as np
import pytest
import torch

import golden_npz
import tolerances as T
import vps_amd
from vps_amd import hip, nhwc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'fusetrack_fullsize_sep.npz')
HEAD = os.path.join(ROOT, 'tests', 'golden', 'separated_fc_cls.npz')
REPORT = os.path.join(ROOT, 'gpurun_out', 'fullsize_sep_report.txt')
# round 4: the DENSE strict fixture - 6 frames, 32..53 detections per frame (31..52 kept), track ids past 170, chosen by oracle margins
# only (tests/golden/search_dense.py; margins stored in dense_fc_cls.npz: threshold >= 1e-2, kept-score gap >= 2.5e-3, NMS IoU >= 2e-2
# from 0.5 against a measured score error <= 9e-4); golden from the REAL reference (make_golden.py fullsize_dense), maps at stride 2
# config5: BASELINE config 5 made strict the same way - the ResNet-101 model (configs/viper/fusetrack_r101.py) on 3 frames at 1088x1920,
# bbox_head.fc_cls fitted by VPS_SEP_CONFIG5=1 search_separated.py (first trial that passes the oracle's margin filter: threshold >= 4.3e-2,
# kept-score gap >= 2.7e-2, NMS IoU >= 0.25 from 0.5), golden from the REAL reference built with depth=101 (make_golden.py config5_sep)
FIXTURES = {
    'separated': (GOLD, HEAD, 4, (1024, 2048), os.path.join('configs', 'cityscapes', 'fusetrack.py')),
    'dense': (os.path.join(ROOT, 'tests', 'golden', 'fusetrack_fullsize_dense.npz'), os.path.join(ROOT, 'tests', 'golden', 'dense_fc_cls.npz'), 6,
              (1024, 2048), os.path.join('configs', 'cityscapes', 'fusetrack.py')),
    'config5': (os.path.join(ROOT, 'tests', 'golden', 'fusetrack_config5_sep.npz'), os.path.join(ROOT, 'tests', 'golden', 'config5_fc_cls.npz'), 3,
                (1088, 1920), os.path.join('configs', 'viper', 'fusetrack_r101.py')),
}


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(float(np.abs(b).max()), 1e-12))


@pytest.mark.parametrize('fixture', ['separated', 'dense', 'config5'])
@pytest.mark.parametrize('prec_name', ['f16x3', 'bf16x6', 'f32'])
def test_strict_full_size_parity_on_the_separated_fixture(dev, prec_name, fixture):
    gold, head, nfr, hw, cfg_path = FIXTURES[fixture]
    g = golden_npz.load(gold)
    H, W, n, seed = [int(v) for v in g['meta']]
    s1, s2, c5 = [int(v) for v in g['strides']]
    ms = int(g['map_stride']) if 'map_stride' in g.files else 1
    assert (H, W, n) == (hw[0], hw[1], nfr)
    old = nhwc.DEFAULT_PREC
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[prec_name]
    try:
        cfg = vps_amd.Config.fromfile(os.path.join(ROOT, cfg_path))
        m = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        synth.load_synth(m, seed, overrides=synth.separated_overrides(head))
        m.ensure_packed(dev)
    finally:
        nhwc.DEFAULT_PREC = old
    frames = [f.to(dev) for f in synth.synth_clip(H, W, n, seed)]
    lines = []
    for t in range(n):
        out = m(return_loss=False, rescale=True, img=[frames[t]], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                ref_img=[frames[t - 1 if t else 0]])
        torch.cuda.synchronize()
        p = 'f%d.' % t
        r = {k: v.cpu().numpy() for k, v in out[2].items()}
        a = m._aux
        stage = {
            'flow': _rel(a['flow'].to_nchw().cpu().numpy()[0][:, ::s1, ::s1], g[p + 'flow_full']),
            'fpn_p2': _rel(a['levels'][0].to_nchw().cpu().numpy()[0, :8, ::s2, ::s2], g[p + 'fpn_p2']),
            'neck_p2': _rel(a['neck_out'][0].to_nchw().cpu().numpy()[0, :8, ::s2, ::s2], g[p + 'neck_out_p2']),
            'fcn_score': _rel(a['fcn_score'].to_nchw().cpu().numpy()[0][:, ::s2, ::s2], g[p + 'fcn_score']),
        }
        strict = {k: bool(np.array_equal(r[k], g[p + k])) for k in ('panoptic_cls_inds', 'panoptic_det_labels', 'panoptic_det_obj_ids')}
        strict['bbox_ids'] = bool(np.array_equal(np.array(sorted(int(k) for k in out[0].keys()), dtype=np.int64), g[p + 'bbox_ids']))
        dprob = float(np.abs(r['panoptic_cls_prob'] - g[p + 'panoptic_cls_prob']).max()) if strict['panoptic_cls_inds'] else float('nan')
        dpan = float((r['panoptic_outputs'][..., ::ms, ::ms] != g[p + 'panoptic_outputs']).mean())
        dsem = float((r['fcn_outputs'][..., ::ms, ::ms] != g[p + 'fcn_outputs']).mean())
        # where the differing panoptic pixels sit: (golden value -> our value): count, the three largest groups
        pa, pg = r['panoptic_outputs'][..., ::ms, ::ms].reshape(-1).astype(np.int64), g[p + 'panoptic_outputs'].reshape(-1).astype(np.int64)
        pairs, cnt = np.unique(pg[pa != pg] * 1000 + pa[pa != pg], return_counts=True)
        top = ['%d->%d:%d' % (pairs[i] // 1000, pairs[i] % 1000, cnt[i]) for i in np.argsort(-cnt)[:3]]
        lines.append('%s %s frame %d: kept %d (golden %d) ids %s | strict %s | max |dprob| %.2e | pan mismatch %.5f%% %s sem mismatch %.5f%% | stage %s'
                     % (fixture, prec_name, t, len(r['panoptic_cls_inds']), len(g[p + 'panoptic_cls_inds']), r['panoptic_det_obj_ids'].tolist(), strict,
                        dprob, 100 * dpan, top, 100 * dsem, {k: '%.1e' % v for k, v in stage.items()}))
        print(lines[-1])
        assert all(strict.values()), lines[-1]
        # maps: 0.1 % of the pixels on the separated fixture. The dense fixture's margins cover every LISTING decision, not the choice of the
        # source proposal behind a detection: in every arithmetic mode - the exact-fp32 kernels included (profiles/r04_fullsize_dense_strict_report.txt:
        # f32 frame 1 0.26 %, f16x3 frame 2 0.19 %, bf16x6 <= 0.08 %) - one or two of the 31..52 instances of some frame come out with a
        # boundary strip of differing pixels (instance <-> the stuff class around it, a few hundred pixels each way; score differences of
        # 1e-3 on that frame), listing and ids unchanged. Bound for it: 0.5 % of the pixels, the pairs are printed.
        # config5: the 101-layer synthetic network amplifies fp32 summation-order differences ~5x more than the 50-layer one - in the
        # EXACT-fp32 kernels as much as in the split modes (profiles/r04_fullsize_config5_strict_report.txt: head inputs 0.9 .. 2.4e-3,
        # semantic logits 4.6 .. 7.3e-3 of max|ref|, scores 4 .. 6e-3 in f32 / f16x3 / bf16x6) - so its fixture was fitted with margins of
        # 4.3e-2 / 2.7e-2 and is compared within 1e-2 (maps: 1 % - the boundary strip of ONE large instance was 0.6 % of the map in bf16x6
        # frame 0, 0.05 .. 0.3 % elsewhere, f32 included); the listing is strict all the same
        depth = 101 if fixture == 'config5' else 50          # the stated tolerances: tests/tolerances.py
        assert dprob < T.stage_tol('score', depth) and dpan < T.MAP[{'separated': 'pan', 'dense': 'pan_dense', 'config5': 'pan_config5'}[fixture]] and dsem < T.MAP['sem'], lines[-1]
        assert all(v < T.stage_tol(k, depth) for k, v in stage.items()), lines[-1]
    if fixture == 'dense':
        ids = np.concatenate([g['f%d.panoptic_det_obj_ids' % t] for t in range(n)])
        assert min(len(g['f%d.panoptic_cls_inds' % t]) for t in range(n)) >= 20 and int(ids.max()) >= 59, 'the dense fixture is dense'
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, 'a') as f:
        f.write('\n'.join(lines) + '\n')
