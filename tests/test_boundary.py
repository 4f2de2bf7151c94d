"""Boundary PQ / boundary VPQ without a device: the dilation rule, the restatement (tests/boundary_restate.py) against hand-derived
answers, the host half of vps_amd/boundary.py fed with the restatement's bands and NumPy counts, the refusals of `vps_boundary_band`
and of the reserved id, the text layout and the new flags of the tools."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary_restate as R
from numpy_seam import numpy_device                            # noqa: F401 (fixture)
from vps_amd import boundary, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROAD, CAR = 7, 26
CATS = {ROAD: {'id': ROAD, 'name': 'road', 'isthing': 0}, CAR: {'id': CAR, 'name': 'car', 'isthing': 1}}


def seg(sid, cat, area, iscrowd=0):
    return {'id': int(sid), 'category_id': cat, 'iscrowd': iscrowd, 'area': int(area)}


def frame(g, p, gt_cats, pred_cats, crowd=()):
    """(gt_ann, pred_ann, gt_pan, pred_pan, image entry) of two id maps; the ground-truth areas are the maps' pixel counts"""
    gt = [seg(i, gt_cats[int(i)], (g == i).sum(), int(i in crowd)) for i in np.unique(g) if i]
    pred = [{k: v for k, v in seg(i, pred_cats[int(i)], (p == i).sum()).items() if k != 'iscrowd'} for i in np.unique(p) if i]
    return ({'segments_info': gt}, {'segments_info': pred}, R.pan_of(g), R.pan_of(p), {})


def square(H, W, y0, y1, x0, x1, sid=5):
    m = np.zeros((H, W), dtype=np.int64)
    m[y0:y1, x0:x1] = sid
    return m


# ---------------------------------------------------------------------------------------------- the dilation rule
def test_dilation_rule():
    # 0.02 * sqrt(1024^2 + 2048^2) = 0.02 * 2289.73 = 45.79 -> 46;  0.02 * sqrt(800) = 0.566 -> 1;  never below 1
    assert boundary.dilation(1024, 2048) == 46 == R.dilation(1024, 2048)
    assert boundary.dilation(20, 20) == 1 and boundary.dilation(1, 1) == 1 and boundary.dilation(2, 3, ratio=0.0) == 1
    assert boundary.dilation(64, 128) == 3                      # 0.02 * 143.1 = 2.86
    assert boundary.dilation(1024, 2048, ratio=0.01) == 23      # 22.897
    assert boundary.dilation(300, 400, 0.1) == 50
    for H, W in ((7, 9), (128, 256), (1080, 1920)):
        assert boundary.dilation(H, W) == R.dilation(H, W)


# ---------------------------------------------------------------------------------------------- mask_to_boundary by hand
def test_band_of_a_square_and_of_a_border_segment():
    m = square(20, 20, 5, 15, 5, 15) > 0
    b = R.mask_to_boundary(m, 1)
    ring = m.copy(); ring[6:14, 6:14] = False                   # one erosion removes the outer ring of a 10 x 10 square: 100 - 64 = 36
    assert np.array_equal(b, ring) and b.sum() == 36
    assert R.mask_to_boundary(m, 4).sum() == 100 - 4 and R.mask_to_boundary(m, 5).sum() == 100      # 2 x 2 left after 4; nothing after 5
    # a 5 x 5 segment in the image's corner: the zero ring erodes the image border too, so rows 0 and columns 0 are band; interior 1..3
    c = square(20, 20, 0, 5, 0, 5) > 0
    bc = R.mask_to_boundary(c, 1)
    assert bc.sum() == 25 - 9 and bc[0, :5].all() and bc[:5, 0].all() and not bc[1:4, 1:4].any()
    # a segment that fills the image: only the image border erodes
    full = np.ones((9, 11), dtype=bool)
    bf = R.mask_to_boundary(full, 2)
    assert bf.sum() == 99 - 5 * 7 and not bf[2:7, 2:9].any()
    # the band map: interior FILL, band keeps the id, void stays 0
    bm = R.ids_of(R.band_map(R.pan_of(square(20, 20, 5, 15, 5, 15, sid=70000)), 1))
    assert (bm == 70000).sum() == 36 and (bm == R.FILL).sum() == 64 and (bm == 0).sum() == 300


# ---------------------------------------------------------------------------------------------- boundary PQ by hand
def test_prediction_equal_to_ground_truth_scores_one():
    g = np.full((20, 20), 1, dtype=np.int64); g[5:15, 5:15] = 5; g[0, :4] = 0
    f = frame(g, g, {1: ROAD, 5: CAR}, {1: ROAD, 5: CAR})
    b, m = R.boundary_pq([f]), R.mask_pq([f])
    for c in (ROAD, CAR):                                       # every band equals itself: b_iou = 1 = mask_iou
        assert b[c] == dict(tp=1, fp=0, fn=0, iou=1.0, biou=1.0) and m[c]['iou'] == 1.0 and m[c]['tp'] == 1


def test_square_shifted_by_one_column_matches_under_pq_and_not_under_boundary_pq():
    """20 x 20, d = 1, over void. gt: rows and columns 5..14; prediction: columns 6..15.
    Bands (outer rings): 36 and 36. Common band pixels: rows 5 and 14, columns 6..14 = 9 + 9 = 18; the vertical sides do not meet
    (gt columns 5 and 14, predicted columns 6 and 15; column 14 is interior of the prediction, column 6 interior of the gt).
    Band of the prediction over gt void: column 15, rows 5..14 = 10. b_iou = 18 / (36 + 36 - 18 - 10) = 18 / 44 = 0.409.
    Masks: intersection 90, prediction over void 10, union 100 + 100 - 90 - 10 = 100, mask IoU 0.9."""
    f = frame(square(20, 20, 5, 15, 5, 15), square(20, 20, 5, 15, 6, 16), {5: CAR}, {5: CAR})
    assert R.dilation(20, 20) == 1
    gb, pb = R.mask_to_boundary(R.ids_of(f[2]) == 5, 1), R.mask_to_boundary(R.ids_of(f[3]) == 5, 1)
    assert (gb.sum(), pb.sum(), (gb & pb).sum(), (pb & (R.ids_of(f[2]) == 0)).sum()) == (36, 36, 18, 10)
    m = R.mask_pq([f])[CAR]
    assert (m['tp'], m['fp'], m['fn']) == (1, 0, 0) and m['iou'] == 90 / 100
    b = R.boundary_pq([f])[CAR]
    assert 18 / 44 < 0.5 and b == dict(tp=0, fp=1, fn=1, iou=0.0, biou=0.0)      # the prediction is 10 % over void: it counts as FP


def test_thin_segment_is_all_band():
    """a bar 2 rows thick with d = 1 (thinner than 2d + 1 = 3): no pixel has a full window inside it, the band is the bar, so every band
    count is the mask count and b_iou == mask_iou: 26 / (28 + 26 - 26 - 0) = 26 / 28"""
    f = frame(square(20, 20, 5, 7, 3, 17), square(20, 20, 5, 7, 4, 17), {5: CAR}, {5: CAR})
    assert R.mask_to_boundary(R.ids_of(f[2]) == 5, 1).sum() == 28
    b, m = R.boundary_pq([f])[CAR], R.mask_pq([f])[CAR]
    assert b['tp'] == 1 and b['iou'] == b['biou'] == m['iou'] == 26 / 28


def test_two_frame_tube_one_frame_matches_alone_and_the_summed_bands_do_not():
    """frame A: a 4 x 4 square predicted exactly (band 16 - 4 = 12, b_iou 1). frame B: the 10 x 10 square predicted 3 columns to the right
    (columns 8..17): common band rows 5 and 14, columns 8..14 = 14; prediction's band over void: rows 5 and 14 at columns 15..17 = 6 plus
    column 17, rows 6..13 = 8, 14 in all. Tube: bi = 12 + 14 = 26, bg = bp = 12 + 36 = 48, bv = 14: 26 / (96 - 26 - 14) = 26 / 56 = 0.464.
    Masks: intersection 16 + 70 = 86, areas 116 and 116, prediction over void 30: 86 / (232 - 86 - 30) = 86 / 116 = 0.741."""
    fa = frame(square(20, 20, 2, 6, 2, 6), square(20, 20, 2, 6, 2, 6), {5: CAR}, {5: CAR})
    fb = frame(square(20, 20, 5, 15, 5, 15), square(20, 20, 5, 15, 8, 18), {5: CAR}, {5: CAR})
    assert R.boundary_vpq([fa], 1)[CAR] == dict(tp=1, fp=0, fn=0, iou=1.0, biou=1.0)
    one = R.boundary_vpq([fa, fb], 1)[CAR]                      # frame by frame: A matches, B (b_iou 14 / 44) does not
    assert (one['tp'], one['fp'], one['fn']) == (1, 1, 1)
    tube = R.boundary_vpq([fa, fb], 2)[CAR]
    assert 26 / 56 < 0.5 < 86 / 116 and tube == dict(tp=0, fp=1, fn=1, iou=0.0, biou=0.0)      # 30 / 116 of the prediction over void: FP
    st = R.Stat(); R.window_stat([fa, fb], st, ratio=None)      # the mask tube of the same window does match
    assert st[CAR]['tp'] == 1 and st[CAR]['iou'] == 86 / 116


# ---------------------------------------------------------------------------------------------- the host half of vps_amd/boundary.py
def _same(stat, want, cats):
    for c in cats:
        got = stat[c]
        assert (got.tp, got.fp, got.fn) == (want[c]['tp'], want[c]['fp'], want[c]['fn']), c
        assert got.iou == want[c]['iou'] and got.biou == want[c]['biou'], c       # the same float64 divisions and additions in the same order


def _clip():
    """three 24 x 40 frames (d = 1): road / car / void, a car that drifts, a thin pole, a crowd region, an unmatched prediction"""
    frames = []
    for t in range(3):
        g = np.full((24, 40), 1, dtype=np.int64); g[0, :6] = 0
        p = g.copy(); p[0, :6] = 1
        g[4:14, 5:17] = 10; p[4:14, 5 + t:17 + t] = 20
        g[3:20, 30:32] = 11; p[3:19, 30:32] = 21
        g[16:22, 2:12] = 12; p[17:22, 3:11] = 22
        p[20:23, 34:39] = 23
        frames.append(frame(g, p, {1: ROAD, 10: CAR, 11: CAR, 12: CAR}, {1: ROAD, 20: CAR, 21: CAR, 22: CAR, 23: CAR}, crowd=(12,)))
    return frames


def test_host_logic_equals_the_restatement_with_numpy_counts(numpy_device):
    clip = _clip()
    stat = boundary.pq_compute_single_core([f[0] for f in clip], [f[1] for f in clip], [f[2] for f in clip], [f[3] for f in clip],
                                           [f[4] for f in clip], CATS, device='cpu')
    want = R.boundary_pq(clip)
    _same(stat, want, CATS)
    assert want[CAR]['tp'] > 0 and want[CAR]['fp'] > 0 and 0 < want[CAR]['biou'] < want[CAR]['tp']
    cache = {}
    for nf in (1, 2, 3):
        _same(boundary.vpq_compute_single_core(clip, CATS, nframes=nf, device='cpu', _cache=cache), R.boundary_vpq(clip, nf), CATS)
    # the hand-derived cases through the same host code
    fa = frame(square(20, 20, 2, 6, 2, 6), square(20, 20, 2, 6, 2, 6), {5: CAR}, {5: CAR})
    fb = frame(square(20, 20, 5, 15, 5, 15), square(20, 20, 5, 15, 8, 18), {5: CAR}, {5: CAR})
    tube = boundary.vpq_compute_single_core([fa, fb], CATS, nframes=2, device='cpu')[CAR]
    assert (tube.tp, tube.fp, tube.fn, tube.iou) == (0, 1, 1, 0.0)
    fs = frame(square(20, 20, 5, 15, 5, 15), square(20, 20, 5, 15, 6, 16), {5: CAR}, {5: CAR})
    one = boundary.pq_compute_single_core([fs[0]], [fs[1]], [fs[2]], [fs[3]], [fs[4]], CATS, device='cpu')[CAR]
    assert (one.tp, one.fp, one.fn) == (0, 1, 1)


def test_results_and_text_layout(numpy_device, tmp_path):
    clip = _clip()
    out = boundary.bvpq_compute([clip], CATS, str(tmp_path), device='cpu', windows=(1, 2))
    assert sorted(os.listdir(tmp_path)) == ['bvpq-0.txt', 'bvpq-5.txt', 'bvpq-final.txt']
    res = out['per_window'][1]
    want = R.boundary_pq(clip)
    assert res['per_class'][CAR]['biou'] == want[CAR]['biou'] / want[CAR]['tp'] and res['per_class'][ROAD]['biou'] == want[ROAD]['biou'] / want[ROAD]['tp']
    assert res['All']['biou'] == (res['per_class'][CAR]['biou'] + res['per_class'][ROAD]['biou']) / 2 and res['Things']['biou'] == res['per_class'][CAR]['biou']
    lines = open(tmp_path / 'bvpq-0.txt').read().splitlines()
    assert lines[0] == '=' * 48 and lines[1].split() == ['|', 'PQ', 'SQ', 'RQ', 'BIoU', 'N'] and lines[2] == '-' * 45
    assert [ln.split()[0] for ln in lines[3:6]] == ['All', 'Things', 'Stuff'] and lines[3].split()[5] == '%.1f' % (100 * res['All']['biou'])
    assert lines[6].split() == ['IDX', '|', 'PQ', 'SQ', 'RQ', 'BIoU', 'IoU', 'TP', 'FP', 'FN'] and len(lines) == 7 + len(CATS)
    fin = open(tmp_path / 'bvpq-final.txt').read().splitlines()
    assert [ln.split(':')[0] for ln in fin] == ['bvpq_all', 'bvpq_thing', 'bvpq_stuff'] and fin[0] == 'bvpq_all:%.4f' % out['All']
    stat = boundary.BPQStat(); stat[CAR].tp += 2; stat[CAR].biou += 1.5
    other = boundary.BPQStat(); other[CAR].tp += 1; other[CAR].biou += 0.25; other[CAR].iou += 0.2
    stat += other
    assert (stat[CAR].tp, stat[CAR].biou, stat[CAR].iou) == (3, 1.75, 0.2)


# ---------------------------------------------------------------------------------------------- refusals that need no GPU
def test_boundary_band_error_codes_before_any_launch():
    lib = hip.load()
    P = ctypes.c_void_p(4096)                                   # never dereferenced: every refusal comes before a launch
    call = lambda pan=P, H=8, W=8, d=1, out=P, ws=P, nbytes=4 * 64: lib.vps_boundary_band(pan, H, W, d, out, ws, nbytes, None)
    assert call(pan=None) == call(out=None) == call(ws=None) == -1001
    assert call(H=0) == call(W=0) == call(H=-3) == call(H=1 << 16, W=1 << 15) == -1002
    assert call(d=0) == call(d=256) == call(d=-1) == -1003
    assert call(nbytes=4 * 64 - 1) == call(nbytes=0) == call(ws=ctypes.c_void_p(4098)) == -1004
    assert call(pan=None, H=0, d=0) == -1001 and call(H=0, d=0) == -1002 and call(d=0, nbytes=0) == -1003      # in this order
    n = ctypes.c_int64(-1)
    assert lib.vps_boundary_band_ws(1024, 2048, 46, ctypes.byref(n)) == 0 and n.value == 4 * 1024 * 2048
    assert lib.vps_boundary_band_ws(1024, 2048, 46, None) == -1001
    assert lib.vps_boundary_band_ws(0, 8, 1, ctypes.byref(n)) == -1002 and n.value == 0
    assert lib.vps_boundary_band_ws(8, 8, 256, ctypes.byref(n)) == -1003
    tile = (ctypes.c_int32 * 2)()
    assert lib.vps_boundary_tile(tile) == 0 and tile[0] >= 1 and tile[1] >= 1 and lib.vps_boundary_tile(None) == -1001
    assert lib.vps_abi_version() == 21


def test_reserved_id_and_bad_width_are_refused():
    g = square(20, 20, 5, 15, 5, 15, sid=boundary.FILL)
    ok = frame(square(20, 20, 5, 15, 5, 15), square(20, 20, 5, 15, 5, 15), {5: CAR}, {5: CAR})
    bad = frame(g, g, {boundary.FILL: CAR}, {boundary.FILL: CAR})
    assert boundary.FILL == 0xFFFFFF == R.FILL
    with pytest.raises(ValueError, match='reserved'):
        boundary.pq_compute_single_core([bad[0]], [ok[1]], [bad[2]], [ok[3]], [{}], CATS)
    with pytest.raises(ValueError, match='reserved'):
        boundary.pq_compute_single_core([ok[0]], [bad[1]], [ok[2]], [bad[3]], [{}], CATS)
    with pytest.raises(ValueError, match='reserved'):
        boundary.vpq_compute_single_core([ok, bad], CATS, nframes=1)
    with pytest.raises(ValueError, match='outside 1..255'):
        boundary.boundary_band(torch.zeros(4, 4, 3, dtype=torch.uint8), d=256, device='cpu')
    with pytest.raises(hip.VpsHipError):                        # no CPU path: a host tensor never reaches the kernel
        boundary.boundary_band(torch.zeros(4, 4, 3, dtype=torch.uint8), d=1, device='cpu')


# ---------------------------------------------------------------------------------------------- the tools' flags
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('name', ['eval_vpq_device', 'run_ipq', 'run_vps_synthetic', 'run_config3', 'vpq_attribution'])
def test_boundary_flags_parse_and_default_off(name):
    mod = _tool(name)
    off = mod.parse_args([])
    assert off.boundary is False and off.boundary_ratio == 0.02
    on = mod.parse_args(['--boundary', '--boundary-ratio', '0.01'])
    assert on.boundary is True and on.boundary_ratio == 0.01
    assert {k: v for k, v in vars(on).items() if not k.startswith('boundary')} == {k: v for k, v in vars(off).items() if not k.startswith('boundary')}
