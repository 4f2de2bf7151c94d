"""CPU: the ternary census warp error - hand-derived answers for the restatement (tests/flow_census_restate.py), the
loop restatement against the array one, the host side of vps_amd/flowphoto.py (figures, text, JSON) against restated figures, and what
`vps_flow_census` refuses before any launch, through the C ABI. No device."""
import ctypes
import json
import os

import numpy as np
import pytest

import flow_census_restate as R
import flow_photo_restate as P
from vps_amd import flowphoto as fp
from vps_amd import hip, tc

F = np.float32


def flow(H, W, u=0.0, v=0.0):
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def frame(H, W, value=0):
    return np.full((H, W, 3), value, dtype=np.uint8)


def census(cur, prev, fl, mask=None, thr=25, eps=2000.0):
    """the array restatement, checked against the loop on the way"""
    a, b = R.flow_census(cur, prev, fl, mask, thr, eps), R.flow_census_loop(cur, prev, fl, mask, thr, eps)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    t = a['table']
    assert int(t[:, 0].sum() + t[:, 11].sum() + t[:, 12].sum()) == a['n']
    return a


def test_the_loop_and_the_array_restatement_agree_on_random_and_special_flows():
    H, W = 9, 11
    for seed in range(4):
        rng = np.random.default_rng(seed)
        prev = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        cur = np.clip(prev.astype(np.int64) + rng.integers(-6, 7, size=(H, W, 3)), 0, 255).astype(np.uint8) if seed % 2 else \
            rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        fl = (rng.standard_normal((H, W, 2)) * (0.7, 3.0, 0.2, 6.0)[seed]).astype(np.float32)
        fl[1, 2] = np.nan; fl[3, 4, 0] = np.inf; fl[5, 6, 1] = -1e30; fl[0, 0] = (-0.5, -0.5); fl[8, 10] = (0.5, 0.25)
        mask = np.where(rng.random((H, W)) < 0.4, rng.choice(np.array([1, 2, 3, 255], dtype=np.uint8), size=(H, W)), 0).astype(np.uint8)
        got = census(cur, prev, fl, mask if seed else None, thr=(25, 0, 50, 100)[seed], eps=(2000.0, 0.0, 500.0, 30000.0)[seed])
        assert got['table'][:, 11].sum() >= 3 and got['table'][:, 0].sum() > 0


def test_identical_frames_and_a_zero_flow_differ_nowhere():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(8, 10, 3), dtype=np.uint8)
    got = census(img, img, flow(8, 10))
    assert not got['d_w'].any() and not got['d_s'].any() and np.array_equal(got['n_w'], got['n_s'])
    t = got['table']
    assert t[0, 0] == 80 and t[0, 2] == t[0, 4] == got['n_s'].sum() and not t[0, [1, 3, 5, 6, 7, 8, 9, 10, 11, 12]].any() and not t[1].any()
    assert not got['residual'].any() and not got['mask_out'].any()


def test_a_brightness_step_of_20_cancels_in_the_census_and_flags_every_pixel_photometrically():
    """the case the feature exists for: cur = prev + 20 on every channel, nothing clipped, zero flow"""
    rng = np.random.default_rng(2)
    prev = rng.integers(0, 236, size=(9, 12, 3), dtype=np.uint8)
    cur = (prev + 20).astype(np.uint8)
    got = census(cur, prev, flow(9, 12))
    assert not got['d_w'].any() and not got['d_s'].any() and not got['residual'].any() and not (got['mask_out'] == 3).any()
    assert got['table'][0, 0] == 108 and got['table'][0, 10] == 0
    photo = P.flow_photo(cur, prev, flow(9, 12), None, 16.0)
    assert (photo['residual'] == 20).all() and photo['counts'][1] == 108 and (photo['mask_out'] == 3).all()


def test_a_whole_pixel_shift_with_the_matching_flow_differs_nowhere_and_counts_the_column_that_left():
    rng = np.random.default_rng(3)
    H, W = 9, 13
    prev = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    cur = np.roll(prev, 1, axis=1)                                               # cur(x) = prev(x - 1); column 0 holds what wrapped round
    got = census(cur, prev, flow(H, W, u=-1.0))
    assert not got['in_view'][:, 0].any() and got['in_view'][:, 1:].all()
    assert got['table'][0, 11] == H and got['table'][0, 0] == H * (W - 1) and got['table'][0, 1] == 0 and not got['d_w'].any()
    assert (got['mask_out'][:, 0] == 2).all() and not got['mask_out'][:, 1:].any() and got['d_s'].sum() > 0
    assert got['n_w'][4, 6] == 48 and got['n_w'][4, 3] == 6 * 7 - 1 and got['n_s'][4, 3] == 48           # the window of x = 3 reaches column 0


def test_a_single_bright_pixel_under_a_flow_that_is_wrong_by_one_pixel():
    """a static scene, flat 100 with one pixel of 200 at x = 5, y = 5, and a flow of u = +1 everywhere: Wg(x, y) = prev(x + 1, y) has
    the bright pixel at x = 4; the last column is not in view"""
    H = W = 12
    img = frame(H, W, 100)
    img[5, 5] = 200
    got = census(img, img, flow(H, W, u=1.0))
    at = lambda y, x: (int(got['d_w'][y, x]), int(got['n_w'][y, x]), int(got['d_s'][y, x]), int(got['n_s'][y, x]))
    assert not got['d_s'].any() and not got['in_view'][:, 11].any()
    assert at(5, 5) == (48, 48, 0, 48)            # cur: -1 against every neighbour; Wg: 0, and +1 against x = 4
    assert at(5, 4) == (48, 48, 0, 48)            # Wg: -1 against every neighbour; cur: 0, and +1 against x = 5
    assert at(5, 7) == (2, 48, 0, 48)             # both bright pixels in the window, at different neighbours
    assert at(5, 8) == (1, 41, 0, 48)             # x = 5 only; the 7 neighbours in column 11 have no Wg
    assert at(5, 1) == (1, 34, 0, 34)             # x = 4 only; 5 columns x 7 rows - 1 in the image
    assert at(0, 0) == (0, 15, 0, 15)             # the corner: 4 x 4 - 1
    assert at(9, 5) == (0, 41, 0, 41)             # out of reach of either; rows 6 .. 11 are 6 x 7 - 1
    assert got['residual'][5, 5] == 255 and got['residual'][5, 7] == (255 * 2 + 24) // 48 == 11 and got['mask_out'][5, 5] == 3
    assert got['mask_out'][5, 7] == 0 and got['mask_out'][0, 11] == 2
    t = got['table'][0]
    assert t[11] == H and t[0] == H * (W - 1) and t[10] == 2 and t[9] == (got['d_w'] > 0).sum() and t[8] == 0


def test_a_difference_of_exactly_eps_is_code_0_and_the_next_float_above_is_not():
    prev = frame(1, 2, 50)
    cur = frame(1, 2, 50)
    cur[0, 1] = 52                                                               # grey 52 000 against 50 000: a difference of 2000
    got = census(cur, prev, flow(1, 2), eps=2000.0)
    assert not got['d_w'].any() and not got['d_s'].any() and got['n_w'].tolist() == [[1, 1]]
    below = float(np.nextafter(F(2000.0), F(0)))                                 # 2000 is the next float above this eps
    got = census(cur, prev, flow(1, 2), eps=below)
    assert got['d_w'].tolist() == [[1, 1]] and got['d_s'].tolist() == [[1, 1]] and got['residual'].tolist() == [[255, 255]]
    got = census(prev, cur, flow(1, 2), eps=below)                               # the other sign, in prev and Wg
    assert got['d_w'].tolist() == [[1, 1]]


def test_a_share_equal_to_the_threshold_is_not_flagged_and_one_more_neighbour_is():
    H = W = 15
    prev = frame(H, W, 100)
    spots = [(7 + dy, 7 + dx) for dy in (-3, -1, 2) for dx in (-3, -2, 1, 3)] + [(7, 6)]
    for k, want in ((12, False), (13, True)):
        cur = prev.copy()
        for y, x in spots[:k]:
            cur[y, x] = 200
        got = census(cur, prev, flow(H, W), thr=25)
        assert (got['d_w'][7, 7], got['n_w'][7, 7]) == (k, 48) and (100 * k > 25 * 48) == want
        assert (got['mask_out'][7, 7] == 3) == want and got['residual'][7, 7] == (255 * k + 24) // 48
    assert census(cur, prev, flow(H, W), thr=100)['table'][0, 10] == 0           # 100 d_w > 100 n_w never holds
    assert census(cur, prev, flow(H, W), thr=0)['table'][0, 10] == (got['d_w'] > 0).sum()


def test_a_1x1_image_and_a_6x6_image():
    one = frame(1, 1, 7)
    got = census(one, one, flow(1, 1))
    assert got['table'][0, 12] == 1 and got['table'].sum() == 1 and got['mask_out'][0, 0] == 0 and got['residual'][0, 0] == 0
    got = census(one, one, flow(1, 1, u=2.0), mask=np.array([[1]], dtype=np.uint8))
    assert got['table'][1, 11] == 1 and got['table'].sum() == 1 and got['mask_out'][0, 0] == 2
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, size=(2, 6, 6, 3), dtype=np.uint8)
    got = census(a, b, flow(6, 6))
    assert got['n_s'].max() == 35 and got['n_s'][0, 0] == 15 and got['n_s'][2, 3] == 35 and got['n_s'][0, 2] == 6 * 4 - 1
    assert np.array_equal(got['n_w'], got['n_s']) and got['table'][0, 0] == 36


def test_both_groups_every_code_of_mask_out_and_in_place():
    rng = np.random.default_rng(6)
    H, W = 8, 9
    prev, cur = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)          # unrelated frames: most pixels are flagged
    fl = flow(H, W)
    fl[:, 0, 0] = -2.0                                                           # column 0 is not in view
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[2] = 1; mask[3] = 2; mask[4] = 255; mask[5, :4] = 3
    got = census(cur, prev, fl, mask, thr=10)
    plain = census(cur, prev, fl, None, thr=10)
    flagged = plain['mask_out'] == 3
    assert flagged[:, 1:].any() and (got['mask_out'][:, 0] == 2).all()
    want = np.where(mask != 0, mask, np.where(flagged, 3, 0)); want[:, 0] = 2
    assert np.array_equal(got['mask_out'], want) and np.array_equal(got['residual'], plain['residual'])
    assert np.array_equal(got['table'][0] + got['table'][1], plain['table'][0]) and got['table'][1, 11] == 4 and got['table'][0, 11] == H - 4
    assert got['table'][1, 0] == (mask[:, 1:] != 0).sum() and got['table'][1, 10] == (flagged & (mask != 0)).sum() > 0
    own = mask.copy()
    again = R.flow_census_loop(cur, prev, fl, own, thr=10, in_place=True)
    assert again['mask_out'] is own and np.array_equal(own, got['mask_out']) and np.array_equal(again['table'], got['table'])


def test_the_residual_is_255_where_every_neighbour_differs_whatever_their_number():
    prev = frame(5, 6, 100)
    cur = prev.copy()
    cur[0, 0] = 200                                                              # the corner: 15 neighbours
    cur[4, 3] = 200                                                              # the lower edge: 4 rows... 2 x 7 columns cut to the image
    got = census(cur, prev, flow(5, 6))
    assert (got['d_w'][0, 0], got['n_w'][0, 0]) == (15, 15) and got['residual'][0, 0] == 255
    n = got['n_w'][4, 3]
    assert n == 4 * 6 - 1 and got['d_w'][4, 3] == n and got['residual'][4, 3] == 255 and (255 * n + n // 2) // n == 255
    assert all((255 * k + k // 2) // k == 255 for k in range(1, 49))


# ---------------------------------------------------------------------------------------------- the host side of vps_amd/flowphoto.py
def random_table(seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 5000, size=(2, 13)).astype(np.int64)
    t[:, 2] += t[:, 1]; t[:, 4] += t[:, 3]
    return t


def same(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def test_the_figures_equal_the_restated_ones():
    for seed in range(3):
        t = random_table(seed)
        if seed == 2:
            t[1] = 0                                                             # an empty group: every quotient is 0
        got, want = fp.census_from_tables(t), R.figures(t)
        for grp in ('all', 'visible', 'masked'):
            assert got[grp]['n'] == want[grp]['n'] and got[grp]['outside'] == want[grp]['outside'] and got[grp]['alone'] == want[grp]['alone']
            assert all(same(got[grp][k], want[grp][k]) for k in fp.CENSUS_FIGURES), grp
    assert fp.census_from_tables(np.zeros((2, 13)))['all']['ratio'] == 0.0
    assert fp.CENSUS_THR == 25 and fp.CENSUS_EPS == 2000.0 and fp.CENSUS_CELLS == 13


def test_stats_rows_sum_to_the_video_text_and_files(tmp_path):
    st = fp.CensusStats(thr=30, eps=1500.0)
    rows = np.stack([random_table(s) for s in (5, 6, 7)])
    a = st.add_tables('clip-a', rows, 3)
    b = st.add_tables(None, random_table(8), 2)
    assert np.array_equal(a['table'], rows.sum(0)) and len(a['per_pair']) == 3 and b['per_pair'] is None and b['video'] == 1
    res = st.result()
    assert res['pairs'] == 5 and res['thr'] == 30 and res['eps'] == 1500.0 and res['table'] == (rows.sum(0) + random_table(8)).tolist()
    assert [r['pair'] for r in res['per_pair']] == [1, 2, 3] and json.loads(json.dumps(res)) == res
    want = R.figures(rows.sum(0) + random_table(8))
    assert all(same(res[g][k], want[g][k]) for g in ('all', 'visible', 'masked') for k in fp.CENSUS_FIGURES)
    text = fp.census_text(res)
    lines = text.splitlines()
    assert len(lines) == 3 + 6 + 1 + 3 + 1 and lines[3].startswith('clip-a') and 'CE-w' in lines[1] and lines[-1].startswith('thr 30 %  eps 1500')
    assert all(len(l) == len(lines[1]) for l in lines[3:9])
    fp.write_census_outputs(res, str(tmp_path))
    assert open(os.path.join(tmp_path, 'flow-census.txt')).read() == text
    assert json.load(open(os.path.join(tmp_path, 'flow-census.json'))) == res
    for bad in (dict(thr=-1), dict(thr=101), dict(thr=25.0), dict(eps=-1.0), dict(eps=float('nan')), dict(eps=float('inf'))):
        with pytest.raises(ValueError):
            fp.CensusStats(**bad)


# ---------------------------------------------------------------------------------------------- the C entry points without a GPU
def test_ws_bytes_the_tile_and_bad_sizes():
    lib = hip.load()
    assert lib.vps_flow_census_ws_bytes(1, 1) == 48 and lib.vps_flow_census_ws_bytes(1, 4) == 48 and lib.vps_flow_census_ws_bytes(3, 3) == 144
    assert lib.vps_flow_census_ws_bytes(1024, 2048) == 12 * 1024 * 2048
    assert lib.vps_flow_census_ws_bytes(0, 4) == -1002 and lib.vps_flow_census_ws_bytes(4, -1) == -1002
    assert lib.vps_flow_census_ws_bytes(1 << 16, 1 << 15) == -1002
    t = (ctypes.c_int32 * 2)()
    assert lib.vps_flow_census_tile(t) == 0 and t[0] >= 7 and t[1] >= 7 and t[1] % 4 == 0
    assert lib.vps_flow_census_tile(None) == -1001
    assert lib.vps_abi_version() == 21                                           # symbols are only added


def test_flow_census_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(cur=p, prev=p, H=4, W=4, flow=p, ld=2, co=0, mask=p, thr=25, eps=2000.0, table=p, mout=p, res=p, ws=p, wsb=192)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_flow_census(a['cur'], a['prev'], a['H'], a['W'], a['flow'], a['ld'], a['co'], a['mask'], a['thr'], a['eps'], a['table'], a['mout'],
                                   a['res'], a['ws'], a['wsb'], None)
    for name in ('cur', 'prev', 'flow', 'table', 'ws'):
        assert call(**{name: None}) == -1001, name
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(W=-3) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    assert call(ld=1) == -1003 and call(ld=4, co=3) == -1003 and call(co=-1) == -1003
    assert call(table=ctypes.c_void_p(4100)) == -1004 and call(flow=ctypes.c_void_p(4098)) == -1004
    assert call(ws=ctypes.c_void_p(4104)) == -1005 and call(wsb=191) == -1005 and call(wsb=0) == -1005 and call(wsb=-192) == -1005
    assert call(H=1, W=17, wsb=192) == -1005                                     # 17 pixels need 3 planes of 20 floats
    assert call(thr=-1) == -1006 and call(thr=101) == -1006
    assert call(eps=-0.5) == -1007 and call(eps=float('nan')) == -1007 and call(eps=float('inf')) == -1007 and call(eps=-float('inf')) == -1007


def test_the_device_entries_need_a_device():
    z, f = np.zeros((2, 2, 3), dtype=np.uint8), np.zeros((2, 2, 2), dtype=np.float32)
    with pytest.raises(hip.VpsHipError):
        fp.flow_census(z, z, f)
    with pytest.raises(hip.VpsHipError):
        fp.CensusEvaluator(device='cpu')


def test_the_census_option_of_the_tc_evaluator_refuses_what_it_cannot_do():
    seg = np.arange(256, dtype=np.uint8)
    with pytest.raises(ValueError):
        tc.TcEvaluator(seg, 6, census=25)                                        # not without occlusion=True
    for bad in (dict(census=-1), dict(census=101), dict(census=12.5), dict(census=25, census_eps=-1.0), dict(census=25, census_eps=float('nan'))):
        with pytest.raises(ValueError):
            tc.TcEvaluator(seg, 6, occlusion=True, **bad)
    z, f = np.zeros((2, 2, 3), dtype=np.uint8), np.zeros((2, 2, 2), dtype=np.float32)
    for census, photometric, frames in ((None, None, (z, z)), (25, None, None), (25, 16.0, None)):       # the first check of add_pair: it needs no device
        ev = tc.TcEvaluator.__new__(tc.TcEvaluator)
        ev.photometric, ev.census, ev.occlusion, ev._open = photometric, census, True, None
        with pytest.raises(ValueError):
            ev.add_pair(z, z, f, back_flow=f, frames=frames)
        with pytest.raises(ValueError):
            ev.add_video([z, z], [None, f], back_flows=[None, f], frames=None if frames is None else [z, z])
