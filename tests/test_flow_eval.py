"""Optical-flow accuracy without a device: the hand-derived answers of the definition (vps_amd/floweval.py) through the per-pixel
restatement (tests/flow_err_restate.py, loop and array form held against each other), `flow_from_tables` / `FlowEvalStats` / `flow_text`
against the restated figures, and the argument checks of `vps_flow_error` and `vps_flow_error_ws_bytes`."""
import ctypes
import json
import math

import numpy as np
import pytest

import flow_err_restate as R
from vps_amd import floweval as fe
from vps_amd import hip

F = np.float32


def flow(H, W, u=0.0, v=0.0):
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def err(pred, gt, mask=None, occ_pred=None):
    """both restatements, which must agree in every cell, byte and bit"""
    a, b = R.flow_error(pred, gt, mask, occ_pred), R.flow_error_loop(pred, gt, mask, occ_pred)
    assert np.array_equal(a['counts'], b['counts']) and np.array_equal(a['rgb'], b['rgb'])
    assert a['sums'].tobytes() == b['sums'].tobytes() and a['abs'].tobytes() == b['abs'].tobytes()
    c = a['counts']
    assert int(c[0] + c[1] + c[12] + c[13] + c[24]) == a['n'] == pred.shape[0] * pred.shape[1]
    return a


def group(counts, g):
    return counts[12 * g:12 * g + 12].tolist()


def test_the_loop_and_the_array_restatement_agree_on_random_and_special_flows():
    rng = np.random.default_rng(7)
    H, W = 9, 13
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 1e9, -1e9], dtype=np.float32)
    for k in range(6):
        gt = (rng.standard_normal((H, W, 2)) * (0.5, 8, 30)[k % 3]).astype(np.float32)
        pred = (gt + rng.standard_normal((H, W, 2)) * (0.2, 2, 6)[k % 3]).astype(np.float32)
        if k >= 3:
            for f in (pred, gt):
                pick = rng.integers(0, 5 * len(vals), size=f.shape)
                f[pick < len(vals)] = vals[pick[pick < len(vals)]]
        mask = rng.integers(0, 4, size=(H, W)).astype(np.uint8) if k % 2 else None
        occ = rng.integers(0, 4, size=(H, W)).astype(np.uint8) if k >= 2 else None
        out = err(pred, gt, mask, occ)
        assert out['counts'][0] > 0 and (k < 3 or (out['counts'][1] > 0 and out['counts'][24] > 0))


def test_zero_error():
    gt = flow(3, 5, 2.5, -7)
    out = err(gt.copy(), gt)
    assert group(out['counts'], 0) == [15, 0, 0, 0, 0, 0, 15, 0, 0, 0, 0, 0] and not out['counts'][12:].any()
    assert not out['sums'].any() and (out['rgb'] == (49, 54, 149)).all()
    fig = fe.flow_from_tables(out['counts'], out['sums'])
    assert fig['epe_all'] == 0 and fig['fl_all'] == 0 and fig['acc_1px'] == 1 and fig['n'] == 15


def test_a_three_four_difference_has_an_end_point_error_of_exactly_five():
    gt = flow(2, 3, 1, 2)
    out = err(flow(2, 3, 4, 6), gt)                                             # du = 3, dv = 4
    assert out['sums'][0] == 30.0 and out['sums'][1] == 30.0                    # 6 pixels x 5.0, all below speed 10
    assert group(out['counts'], 0)[:6] == [6, 0, 6, 6, 6, 0]                     # outliers: 5 > 3 and 5 > 0.05 * sqrt(5); > 1, > 3, not > 5
    fig = fe.flow_from_tables(out['counts'], out['sums'])
    assert fig['epe_all'] == 5.0 == fig['epe_noc'] and fig['epe_occ'] == 0.0 and fig['fl_all'] == 100.0
    assert (fig['acc_1px'], fig['acc_3px'], fig['acc_5px']) == (0.0, 0.0, 1.0)


def test_exactly_three_and_exactly_five_percent_are_not_outliers():
    """epe = 3 against gt 0: 3 > 3 is false. gt = (60, 80), mag = 100, 0.05 * 100 = 5.0 in float64 (the product of the double next to 0.05
    and 100 rounds to 5.0), epe = 5: 5 > 3 but 5 > 5.0 is false. gt = (0, 96): 0.05 * 96 < 5, an outlier. The float above 3: an outlier."""
    assert 0.05 * 100.0 == 5.0
    gt = flow(1, 4)
    pred = flow(1, 4)
    pred[0, 0] = (3, 0)
    gt[0, 1] = (60, 80); pred[0, 1] = (63, 84)
    gt[0, 2] = (0, 96); pred[0, 2] = (3, 100)
    pred[0, 3] = (np.nextafter(F(3), F(4)), 0)
    out = err(pred, gt)
    c = group(out['counts'], 0)
    assert c[0] == 4 and c[2] == 2 and c[4] == 3                                 # epe > 3: the two fives and the float above 3
    for x, want in enumerate((0, 0, 1, 1)):
        assert group(err(pred[:, x:x + 1], gt[:, x:x + 1])['counts'], 0)[2] == want, x


def test_speeds_of_exactly_ten_and_forty_land_in_the_upper_bin():
    gt = flow(1, 5)
    gt[0, 0] = (6, 8)                                                           # mag 10 -> 10 <= mag < 40
    gt[0, 1] = (24, 32)                                                         # mag 40 -> mag >= 40
    gt[0, 2] = (0, 9.5)
    gt[0, 3] = (np.nextafter(F(10), F(0)), 0)                                   # just below 10
    gt[0, 4] = (0, np.nextafter(F(40), F(0)))                                   # just below 40
    pred = gt.copy()
    pred[..., 0] += F(0.5)
    pred[0, 1, 0] = 26                                                          # epe 2 in the top bin
    out = err(pred, gt)
    assert group(out['counts'], 0)[6:9] == [2, 2, 1]
    assert out['sums'].tolist()[:4] == [4.0, 1.0, 1.0, 2.0]
    fig = fe.flow_from_tables(out['counts'], out['sums'])
    assert (fig['s0_10'], fig['s10_40'], fig['s40plus']) == (0.5, 0.5, 2.0)


def test_zero_ground_truth_speed_with_an_error_divides_by_three_only():
    out = err(flow(1, 1, 6, 0), flow(1, 1))                                     # epe 6, mag 0: n_err = 2 -> the row below 3
    assert out['rgb'][0, 0].tolist() == [224, 243, 248] and group(out['counts'], 0)[:7] == [1, 0, 1, 1, 1, 1, 1]


def test_every_colour_row_with_each_boundary_on_its_upper_side():
    """gt = 0, pred = (3 hi, 0): epe / 3.0 is hi exactly (3 hi and hi are dyadic), which is not < hi: the next row. The float below 3 hi
    gives the row itself. The relative branch: gt = (60, 80), diff (4.5, 6): epe 7.5, min(2.5, 7.5 / 5.0) = 1.5, not < 1.5."""
    rows = [c for _, c in fe.ERROR_COLOURS]
    assert fe.ERROR_COLOURS == R.ROWS and len(rows) == 10
    his = [hi for hi, _ in fe.ERROR_COLOURS[:-1]]
    assert his == [0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48]
    W = 2 * len(his) + 2
    pred, gt = flow(1, W), flow(1, W)
    want = []
    for k, hi in enumerate(his):
        assert float(F(3 * hi)) == 3 * hi
        pred[0, 2 * k, 0] = 3 * hi; want.append(rows[k + 1])
        pred[0, 2 * k + 1, 0] = np.nextafter(F(3 * hi), F(0)); want.append(rows[k])
    pred[0, W - 2, 1] = -1e6; want.append(rows[9])
    gt[0, W - 1] = (60, 80); pred[0, W - 1] = (64.5, 86); want.append(rows[4])
    out = err(pred, gt)
    assert out['rgb'][0].tolist() == [list(c) for c in want]
    assert want[0] == (69, 117, 180) and want[1] == (49, 54, 149) and want[-3] == (215, 48, 39) and want[-4] == (165, 0, 38)


def test_unknown_ground_truth_bad_predictions_and_every_mask_value():
    gtv = [np.nan, 1e10, -1e10, np.inf, -np.inf, 1e9, -1e9]                     # the last two are known: |.| > 1e9 is strict
    gt = flow(2, len(gtv))
    for x, val in enumerate(gtv):
        gt[0, x, 0] = val
        gt[1, x, 1] = val
    pred = flow(2, len(gtv), 1, 1)
    out = err(pred, gt)
    assert out['counts'][24] == 10 and out['counts'][0] == 4 and (out['rgb'][:, :5] == 0).all() and out['rgb'][:, 5:].any(axis=2).all()
    pv = [np.nan, np.inf, -np.inf, 1e30, -1e30, 1e9, -1e9, -0.0]
    pred = flow(2, len(pv))
    for x, val in enumerate(pv):
        pred[0, x, 0] = val
        pred[1, x, 1] = val
    occ = np.ones((2, len(pv)), dtype=np.uint8)
    out = err(pred, flow(2, len(pv)), None, occ)
    c = group(out['counts'], 0)
    assert c[0] == 6 and c[1] == 10 and c[9:12] == [0, 16, 0] and (out['rgb'][:, :5] == (255, 0, 255)).all()
    assert out['sums'][0] == 4e9 and c[8] == 0                                  # the bad pixels touch no sum; 4 x 1e9 from the four known extremes
    mask = np.array([[0, 1, 2, 3, 255, 2]], dtype=np.uint8)
    pred, gt = flow(1, 6, 2, 0), flow(1, 6)
    pred[0, 5, 0] = np.nan
    out = err(pred, gt, mask, np.array([[1, 0, 2, 1, 1, 3]], dtype=np.uint8))
    assert out['counts'][24] == 3 and group(out['counts'], 0) == [1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    assert group(out['counts'], 1) == [1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1]      # the code 3 of the bad pixel is counted in no cell
    assert out['sums'].tolist() == [2, 2, 0, 0, 2, 2, 0, 0]
    assert out['rgb'][0].tolist() == [[0, 0, 0], [116, 173, 209], [116, 173, 209], [0, 0, 0], [0, 0, 0], [255, 0, 255]]


def test_occlusion_precision_and_recall_on_a_two_by_three_case():
    """mask: three occluded pixels (2), two visible (1), one invalid (0). occ_pred flags (codes 1 and 2) two of the occluded ones, one
    visible one and the invalid one: TP 2, FP 1, FN 1 -> precision 2/3, recall 2/3; 3 of 5 valid pixels predicted, 3 of 5 truly occluded."""
    mask = np.array([[2, 2, 2], [1, 1, 0]], dtype=np.uint8)
    occ = np.array([[1, 2, 0], [1, 0, 1]], dtype=np.uint8)
    out = err(flow(2, 3, 0.25), flow(2, 3), mask, occ)
    assert group(out['counts'], 0)[9:] == [1, 1, 0] and group(out['counts'], 1)[9:] == [1, 1, 1]
    for fig in (fe.flow_from_tables(out['counts'], out['sums'], with_occ=True), R.figures(out['counts'], out['sums'], with_occ=True)):
        assert fig['occ_precision'] == 2 / 3 and fig['occ_recall'] == 2 / 3 and math.isclose(fig['occ_f1'], 2 / 3, rel_tol=1e-15)
        assert fig['occ_pred_share'] == 0.6 and fig['occ_true_share'] == 0.6 and fig['invalid_share'] == 1 / 6
    assert 'occ_f1' not in fe.flow_from_tables(out['counts'], out['sums'])


def random_tables(seed, occ=True):
    rng = np.random.default_rng(seed)
    H, W = 11, 17
    gt = (rng.standard_normal((H, W, 2)) * 25).astype(np.float32)
    pred = (gt + rng.standard_normal((H, W, 2)) * 3).astype(np.float32)
    pred[0, :3] = np.nan
    gt[1, :2] = 2e9
    return err(pred, gt, rng.integers(0, 4, size=(H, W)).astype(np.uint8), rng.integers(0, 3, size=(H, W)).astype(np.uint8) if occ else None)


def test_the_figures_equal_the_restated_ones():
    for seed in (1, 2, 3):
        t = random_tables(seed)
        got, want = fe.flow_from_tables(t['counts'], t['sums'], with_occ=True), R.figures(t['counts'], t['sums'], with_occ=True)
        assert set(fe.FIGURES + fe.OCC_FIGURES) <= set(got)
        for k in fe.FIGURES + fe.OCC_FIGURES + ('n', 'bad', 'invalid'):
            assert math.isclose(got[k], want[k], rel_tol=1e-14, abs_tol=0), k   # a handful of float64 operations on the same tables
        assert got['n'] == got['n_noc'] + got['n_occ'] and 0 < got['fl_noc'] < 100 and got['epe_occ'] > 0
    empty = fe.flow_from_tables(np.zeros(25, dtype=np.int64), np.zeros(8), with_occ=True)
    assert all(empty[k] == 0 for k in fe.FIGURES + fe.OCC_FIGURES)               # no pixel: every quotient is 0


def test_stats_rows_sum_to_the_total_and_the_result_survives_json():
    a, b = random_tables(4), random_tables(5)
    st = fe.FlowEvalStats()
    st.add_tables(np.stack([a['counts'], b['counts']]), np.stack([a['sums'], b['sums']]), 2, ['a', 'b'], with_occ=True)
    res = st.result()
    assert res['pairs'] == 2 and [r['pair'] for r in res['per_pair']] == ['a', 'b'] and res['counts'] == (a['counts'] + b['counts']).tolist()
    assert res['sums'] == (a['sums'] + b['sums']).tolist() and res['n'] == sum(r['n'] for r in res['per_pair'])
    assert json.loads(json.dumps(res)) == res
    whole = fe.FlowEvalStats()
    whole.add_tables(a['counts'] + b['counts'], a['sums'] + b['sums'], 2, with_occ=True)
    w = whole.result()
    assert w['per_pair'] == [] and all(w[k] == res[k] for k in fe.FIGURES + fe.OCC_FIGURES)
    plain = fe.FlowEvalStats()
    t = random_tables(6, occ=False)
    plain.add_tables(t['counts'], t['sums'])
    assert not set(fe.OCC_FIGURES) & set(plain.result())


def test_flow_text_layout():
    a, b = random_tables(4), random_tables(5)
    st = fe.FlowEvalStats()
    st.add_tables(np.stack([a['counts'], b['counts']]), np.stack([a['sums'], b['sums']]), 2, ['frame_0001', 'frame_0002'], with_occ=True)
    res = st.result()
    lines = fe.flow_text(res).splitlines()
    assert lines[0] == '=' * 136 and lines[2] == '-' * 136 == lines[5] and len(lines) == 7
    assert lines[1].split() == ['PAIR', '|', 'EPE', 'EPE-noc', 'EPE-occ', 'Fl-all', 'Fl-noc', 's0-10', 's10-40', 's40+', '<=1px', '<=3px', '<=5px', 'BAD',
                                'INVAL', 'OCC-P', 'OCC-R', 'OCC-F1']
    assert lines[3].split()[0] == 'frame_0001' and lines[4].split()[0] == 'frame_0002'
    tot = lines[6].split()
    assert tot[:2] == ['All', '(2)'] and tot[3] == '%.3f' % res['epe_all'] and tot[6] == '%.2f' % res['fl_all'] and tot[-1] == '%.2f' % (100 * res['occ_f1'])
    assert tot[11] == '%.2f' % (100 * res['acc_1px']) and tot[14] == '%.2f' % (100 * res['bad_share'])
    plain = fe.FlowEvalStats()
    t = random_tables(6, occ=False)
    plain.add_tables(t['counts'], t['sums'])
    plines = fe.flow_text(plain.result()).splitlines()
    assert plines[0] == '=' * 112 and 'OCC-P' not in plines[1] and len(plines) == 5 and len(plines[4].split()) == 16


# ---------------------------------------------------------------------------------------------- the C entry points without a GPU
def test_ws_bytes_is_eight_doubles_per_workgroup_and_refuses_bad_sizes():
    lib = hip.load()
    assert lib.vps_flow_error_ws_bytes(1, 1) == 64 and lib.vps_flow_error_ws_bytes(1, 1024) == 64 and lib.vps_flow_error_ws_bytes(1, 1025) == 128
    big = lib.vps_flow_error_ws_bytes(1024, 2048)
    assert big % 64 == 0 and 64 < big <= 64 * 2048 and lib.vps_flow_error_ws_bytes(4096, 4096) == big     # capped: grid-stride beyond it
    assert lib.vps_flow_error_ws_bytes(0, 4) == -1002 and lib.vps_flow_error_ws_bytes(4, -1) == -1002
    assert lib.vps_flow_error_ws_bytes(1 << 16, 1 << 15) == -1002


def test_flow_error_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(pred=p, pld=2, pco=0, gt=p, gld=2, gco=0, mask=p, occ=p, H=4, W=4, counts=p, sums=p, rgb=p, ws=p, wsb=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_flow_error(a['pred'], a['pld'], a['pco'], a['gt'], a['gld'], a['gco'], a['mask'], a['occ'], a['H'], a['W'], a['counts'], a['sums'],
                                  a['rgb'], a['ws'], a['wsb'], None)
    for name in ('pred', 'gt', 'counts', 'sums', 'ws'):
        assert call(**{name: None}) == -1001, name
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(W=-3) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    for f in ('p', 'g'):
        assert call(**{f + 'ld': 1}) == -1003 and call(**{f + 'ld': 4, f + 'co': 3}) == -1003 and call(**{f + 'co': -1}) == -1003, f
    assert call(counts=ctypes.c_void_p(4100)) == -1004 and call(sums=ctypes.c_void_p(4100)) == -1004
    assert call(pred=ctypes.c_void_p(4098)) == -1004 and call(gt=ctypes.c_void_p(4097)) == -1004
    assert call(ws=ctypes.c_void_p(4100)) == -1005 and call(wsb=63) == -1005 and call(wsb=0) == -1005 and call(wsb=-64) == -1005
    assert call(H=1, W=1025, wsb=64) == -1005                                    # two workgroups need two slots


def test_the_device_entries_need_a_device():
    with pytest.raises(hip.VpsHipError):
        fe.flow_error(np.zeros((2, 2, 2), dtype=np.float32), np.zeros((2, 2, 2), dtype=np.float32), device='cpu')
    with pytest.raises(hip.VpsHipError):
        fe.FlowEvaluator(device='cpu')
