"""tools/eval_flow_device.py with KITTI flow files: its argument and file-layout handling on the CPU (nothing there touches a device), and on
the GPU a directory of three 24x40 pairs end to end against tests/flow_err_restate.py on the decode of tests/kitti_flow_restate.py."""
import json
import os
import struct
import sys

import numpy as np
import pytest

import flow_err_restate as FE
import kitti_flow_restate as K
import png16_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
F = np.float32


def _flo(path, flow):
    with open(path, 'wb') as f:
        f.write(struct.pack('<fii', 202021.25, flow.shape[1], flow.shape[0]) + np.ascontiguousarray(flow, '<f4').tobytes())


def _kitti(path, flow, valid=None):
    with open(path, 'wb') as f:
        f.write(K.write_file(flow, valid, P.types_all_pairs(flow.shape[0])))


def _dirs(tmp_path, *names):
    for n in names:
        os.makedirs(tmp_path / n)
    return [str(tmp_path / n) for n in names]


def test_argument_and_file_layout_handling(tmp_path):
    import eval_flow_device as T
    pred, gt, noc, msk, empty = _dirs(tmp_path, 'pred', 'gt', 'noc', 'mask', 'empty')
    flow = np.zeros((4, 6, 2), F)
    _flo(os.path.join(pred, 'a.flo'), flow)
    _kitti(os.path.join(pred, 'b.png'), flow)
    _kitti(os.path.join(gt, 'a.png'), flow)
    _kitti(os.path.join(gt, 'b.png'), flow)
    _kitti(os.path.join(noc, 'a.png'), flow)
    _kitti(os.path.join(noc, 'b.png'), flow)
    # mixed extensions, matched by stem; the noc file beside a KITTI ground truth
    args = T.parse_args(['--pred', pred, '--gt', gt, '--gt-noc', noc])
    assert T.match_files(args) == [('a', os.path.join(pred, 'a.flo'), os.path.join(gt, 'a.png'), os.path.join(noc, 'a.png')),
                                   ('b', os.path.join(pred, 'b.png'), os.path.join(gt, 'b.png'), os.path.join(noc, 'b.png'))]
    assert [m[3] for m in T.match_files(T.parse_args(['--pred', pred, '--gt', gt]))] == [None, None]
    # --gt-noc together with --mask / --occ-mask: refused by the parser
    for extra in (['--mask', msk], ['--occ-mask', msk]):
        with pytest.raises(SystemExit):
            T.parse_args(['--pred', pred, '--gt', gt, '--gt-noc', noc] + extra)
        with pytest.raises(SystemExit):                            # and a mask with KITTI ground truth, without --gt-noc, by the matching
            T.match_files(T.parse_args(['--pred', pred, '--gt', gt] + extra))
    # a noc file missing; --gt-noc with .flo ground truth; a stem with both extensions; no ground truth; no files; no directory
    os.remove(os.path.join(noc, 'b.png'))
    with pytest.raises(SystemExit):
        T.match_files(args)
    _kitti(os.path.join(noc, 'b.png'), flow)
    os.remove(os.path.join(gt, 'a.png'))
    _flo(os.path.join(gt, 'a.flo'), flow)
    with pytest.raises(SystemExit):
        T.match_files(args)
    assert [os.path.basename(m[2]) for m in T.match_files(T.parse_args(['--pred', pred, '--gt', gt]))] == ['a.flo', 'b.png']
    _kitti(os.path.join(gt, 'a.png'), flow)
    with pytest.raises(SystemExit):
        T.match_files(T.parse_args(['--pred', pred, '--gt', gt]))
    os.remove(os.path.join(gt, 'a.png'))
    os.remove(os.path.join(gt, 'b.png'))
    with pytest.raises(SystemExit):
        T.match_files(T.parse_args(['--pred', pred, '--gt', gt]))
    with pytest.raises(SystemExit):
        T.match_files(T.parse_args(['--pred', empty, '--gt', gt]))
    with pytest.raises(SystemExit):
        T.match_files(T.parse_args(['--pred', pred, '--gt', str(tmp_path / 'nowhere')]))
    # an 8-bit PNG under a flow's name is no KITTI file
    from PIL import Image
    Image.fromarray(np.zeros((4, 6), np.uint8)).save(os.path.join(gt, 'b.png'))
    with pytest.raises(SystemExit):
        T.match_files(T.parse_args(['--pred', pred, '--gt', gt]))


def test_the_flow_format_option_of_the_tools_takes_kitti():
    from vps_amd import flowvis
    assert 'kitti' in flowvis.FORMATS and flowvis.flow_name('out', 'dir/frame_7.jpg', 'kitti') == os.path.join('out', 'frame_7.png')
    assert flowvis.flow_name('out', 'dir/frame_7.jpg', 'flo') == os.path.join('out', 'frame_7.flo')
    for tool in ('run_config3.py', 'run_vps_synthetic.py'):
        src = open(os.path.join(ROOT, 'tools', tool)).read()
        assert "choices=['jpg', 'png', 'flo', 'kitti']" in src, tool


@pytest.mark.gpu
def test_a_directory_of_three_pairs_end_to_end(dev, tmp_path):
    import eval_flow_device as T
    from vps_amd import floweval as fe
    H, W = 24, 40
    pred_d, gt_d, noc_d = _dirs(tmp_path, 'pred', 'occ', 'noc')
    rg = np.random.default_rng(77)
    wants = {}
    for k, stem in enumerate(('000001_10', '000002_10', '000003_10')):
        gt = (rg.standard_normal((H, W, 2)) * (5, 20, 60)[k]).astype(F)
        gt_valid = rg.random((H, W)) < 0.8
        noc_valid = gt_valid & (rg.random((H, W)) < 0.7)
        pred = (gt + rg.standard_normal((H, W, 2)) * np.where(rg.random((H, W, 1)) < 0.3, 6.0, 0.4)).astype(F)
        _kitti(os.path.join(gt_d, stem + '.png'), gt, gt_valid)
        _kitti(os.path.join(noc_d, stem + '.png'), gt, noc_valid)
        if k == 1:                                                 # one prediction as .flo, unquantised, with a NaN
            pred[3, 4, 0] = np.nan
            _flo(os.path.join(pred_d, stem + '.flo'), pred)
            rp = pred
        else:                                                      # the others KITTI-coded, some pixels invalid -> NaN
            pv = rg.random((H, W)) < 0.95
            _kitti(os.path.join(pred_d, stem + '.png'), pred, pv)
            rp, rpv = K.quantised(pred, pv)
            rp = np.where(rpv[..., None], rp, F(np.nan)).astype(F)
        rgt, rgv = K.quantised(gt, gt_valid)
        wants[stem] = FE.flow_error(rp, rgt, K.mask_codes(rgv, K.quantised(gt, noc_valid)[1]))
    out = str(tmp_path / 'out')
    res = T.main(['--pred', pred_d, '--gt', gt_d, '--gt-noc', noc_d, '--out', out, '--device', str(dev)])
    total_c, total_s = sum(w['counts'] for w in wants.values()), sum(w['sums'] for w in wants.values())
    assert res['counts'] == total_c.tolist() and res['n_occ'] > 0 and res['invalid'] > 0 and res['bad'] > 0
    fig = FE.figures(total_c, total_s)
    close = lambda a, b: abs(a - b) <= 1e-12 * max(1.0, abs(b))
    assert all(close(res[k], fig[k]) for k in fe.FIGURES)
    doc = json.load(open(os.path.join(out, 'flow-eval.json')))
    assert doc == res and [r['pair'] for r in doc['per_pair']] == sorted(wants)
    for r in doc['per_pair']:
        f = FE.figures(wants[r['pair']]['counts'], wants[r['pair']]['sums'])
        assert all(close(r[k], f[k]) for k in fe.FIGURES)
