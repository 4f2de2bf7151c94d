"""The photometric warp error without a device: the hand-derived answers of the definition (vps_amd/flowphoto.py) through the per-pixel
restatement (tests/flow_photo_restate.py, loop and array form held against each other), `photo_from_tables` / `PhotoStats` / `photo_text`
against the restated figures, the argument checks of `vps_flow_photo` and `vps_flow_photo_ws_bytes`, and the refusals of the
`photometric=` option of `tc.TcEvaluator`."""
import ctypes
import json
import math

import numpy as np
import pytest

import flow_photo_restate as R
from vps_amd import flowphoto as fp
from vps_amd import hip, tc

F = np.float32


def flow(H, W, u=0.0, v=0.0):
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def frame(H, W, value=0):
    return np.full((H, W, 3), value, dtype=np.uint8)


def photo(cur, prev, fl, mask=None, thr=16.0):
    """both restatements, which must agree in every cell, byte and bit; the loop also with the mask written in place"""
    a, b = R.flow_photo(cur, prev, fl, mask, thr), R.flow_photo_loop(cur, prev, fl, mask, thr)
    assert np.array_equal(a['counts'], b['counts']) and a['sums'].tobytes() == b['sums'].tobytes()
    assert np.array_equal(a['mask_out'], b['mask_out']) and np.array_equal(a['residual'], b['residual'])
    if mask is not None:
        own = mask.copy()
        c = R.flow_photo_loop(cur, prev, fl, own, thr, in_place=True)
        assert c['mask_out'] is own and np.array_equal(own, a['mask_out']) and np.array_equal(c['counts'], a['counts'])
    n = a['counts']
    assert int(n[0] + n[10] + n[20]) == a['n'] == fl.shape[0] * fl.shape[1]
    return a


def test_the_loop_and_the_array_restatement_agree_on_random_and_special_flows():
    rng = np.random.default_rng(7)
    H, W = 9, 13
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], dtype=np.float32)
    for k in range(6):
        cur, prev = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        if k % 2:
            cur = np.clip(prev.astype(np.int64) + rng.integers(-6, 7, size=prev.shape), 0, 255).astype(np.uint8)
        fl = (rng.standard_normal((H, W, 2)) * (0.4, 2, 6)[k % 3]).astype(np.float32)
        if k >= 3:
            pick = rng.integers(0, 5 * len(vals), size=fl.shape)
            fl[pick < len(vals)] = vals[pick[pick < len(vals)]]
        mask = rng.integers(0, 3, size=(H, W)).astype(np.uint8) if k % 3 else None
        out = photo(cur, prev, fl, mask, thr=(16.0, 3.0)[k % 2])
        assert out['counts'][0] > 0 and (k < 3 or out['counts'][20] > 0) and (mask is None or out['counts'][10] > 0)


def test_identical_frames_and_a_zero_flow_give_all_zeros():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(4, 6, 3), dtype=np.uint8)
    out = photo(img, img.copy(), flow(4, 6))
    assert out['counts'].tolist() == [24] + [0] * 20 and not out['sums'].any() and not out['mask_out'].any() and not out['residual'].any()
    fig = fp.photo_from_tables(out['counts'], out['sums'])
    assert fig['all']['mae_warp'] == 0 and fig['all']['psnr_warp'] == float('inf') == fig['all']['psnr_static'] and fig['all']['gain_db'] == 0
    assert fig['all']['ratio'] == 0 and fig['outside_share'] == 0 and fig['masked']['n'] == 0


def test_different_frames_and_a_zero_flow_give_the_static_error_exactly():
    """the weights are 0, so s_c is prev_c(p) itself: aw == as, qw == qs, and no pixel is helped or hurt"""
    rng = np.random.default_rng(2)
    cur, prev = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8), rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    out = photo(cur, prev, flow(5, 7))
    c = out['counts']
    d = prev.astype(np.int64) - cur.astype(np.int64)
    assert c[0] == 35 and c[2] == np.abs(d).sum() and c[3] == (d * d).sum() and c[8] == 0 and c[9] == 0 and c[20] == 0
    assert out['sums'][0] == float(c[2]) and out['sums'][1] == float(c[3])
    fig = fp.photo_from_tables(c, out['sums'])['all']
    assert fig['ratio'] == 1.0 and fig['gain_db'] == 0.0 and fig['helped'] == 0 and fig['hurt'] == 0 and fig['mae_warp'] == fig['mae_static'] > 0


def test_a_whole_pixel_shift_with_the_matching_flow_has_no_residual_in_view():
    """cur(x) = prev(x + 1) and u = 1: the sample is prev(x + 1) with weight 0 on its neighbour. The last column points outside."""
    rng = np.random.default_rng(3)
    H, W = 4, 9
    prev = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    cur = np.roll(prev, -1, axis=1)
    out = photo(cur, prev, flow(H, W, 1.0))
    c = out['counts']
    assert c[20] == H and c[0] == H * (W - 1) and not out['sums'].any() and not out['residual'].any() and c[2] > 0 and c[3] > 0
    assert c[8] > 0 and c[9] == 0 and c[1] == 0 and not c[4:8].any()
    assert (out['mask_out'][:, -1] == 2).all() and not out['mask_out'][:, :-1].any()
    fig = fp.photo_from_tables(c, out['sums'])
    assert fig['all']['ratio'] == 0 and fig['all']['mae_static'] > 0 and fig['outside_share'] == 1 / W and fig['all']['psnr_warp'] == float('inf')


def test_a_ramp_under_half_a_pixel_of_flow():
    """prev = cur = 10 x in every channel, u = 0.5: sx = x + 0.5, x0 = x, wx = 0.5, s = 10 x + 0.5 * 10 = 10 x + 5, so every dw is 5:
    aw = 15, qw = 75, e = 5, residual floor(5.5) = 5; static error 0, so every pixel is hurt. floorf(x + 1) <= W - 1 leaves the last
    column out of view. e = 5 == thr is not flagged; the float below 5 as thr flags them all."""
    H, W = 3, 8
    img = np.repeat((10 * np.arange(W, dtype=np.uint8))[None, :, None], H, axis=0).repeat(3, axis=2)
    n = H * (W - 1)
    out = photo(img, img.copy(), flow(H, W, 0.5), thr=5.0)
    assert out['counts'].tolist() == [n, 0, 0, 0, n, 0, 0, 0, 0, n] + [0] * 10 + [H]
    assert out['sums'].tolist() == [15.0 * n, 75.0 * n, 0, 0]
    assert (out['residual'][:, :-1] == 5).all() and (out['residual'][:, -1] == 0).all() and not out['mask_out'][:, :-1].any()
    fig = fp.photo_from_tables(out['counts'], out['sums'])['all']
    assert fig['mae_warp'] == 5.0 and fig['rms_warp'] == 5.0 and fig['above_4'] == 1.0 and fig['above_8'] == 0 and fig['hurt'] == 1.0 and fig['flagged_share'] == 0
    assert math.isclose(fig['psnr_warp'], 10 * math.log10(65025 / 25.0), rel_tol=1e-15)
    below = photo(img, img.copy(), flow(H, W, 0.5), thr=float(np.nextafter(F(5), F(0))))
    assert below['counts'][1] == n and (below['mask_out'][:, :-1] == 3).all() and (below['mask_out'][:, -1] == 2).all()


def test_an_error_equal_to_the_threshold_is_not_flagged_and_the_next_double_above_is():
    """cur = 0. Pixel 0: prev(0) = (48, 0, 0), prev(1) = (48, 1, 0), u = 2^-47: wx = 2^-47, s = (48, 2^-47, 0), aw = 48 + 2^-47 (one ulp of
    a double at 48), e = aw / 3 = 16 + 2^-47 / 3, which rounds to 16 + 2^-48: the next double above 16. The other pixels, zero flow, differ
    from cur by (48, 0, 0): e = 16 exactly."""
    prev, cur = frame(1, 4), frame(1, 4)
    prev[0, 0] = (48, 0, 0); prev[0, 1] = (48, 1, 0); prev[0, 2] = (48, 0, 0); prev[0, 3] = (48, 0, 0)
    cur[0, 1] = (0, 1, 0)
    fl = flow(1, 4)
    fl[0, 0, 0] = 2.0 ** -47
    out = photo(cur, prev, fl, thr=16.0)
    assert float(np.nextafter(16.0, 17.0)) == (48 + 2.0 ** -47) / 3.0 and 48 + 2.0 ** -47 > 48
    assert out['mask_out'][0].tolist() == [3, 0, 0, 0] and out['counts'][1] == 1 and out['counts'][6] == 1 and out['counts'][5] == 4
    assert out['counts'][9] == 1 and out['counts'][8] == 0 and out['residual'][0].tolist() == [16, 16, 16, 16]


def test_both_groups_and_every_code_of_mask_out():
    """a row of six pixels: in view with mask 0 and a small error (0), in view with mask 0 and a large error (3), mask 1 kept, mask 2 kept,
    mask 255 kept, and one that is not in view whose mask byte 1 becomes 2"""
    prev = frame(1, 6, 100)
    cur = frame(1, 6, 100)
    cur[0, 1] = (160, 100, 100)                                                  # aw 60, e 20 > 16
    cur[0, 2] = (190, 100, 100)                                                  # aw 90, e 30, masked
    cur[0, 3] = (101, 100, 100)
    mask = np.array([[0, 0, 1, 2, 255, 1]], dtype=np.uint8)
    fl = flow(1, 6)
    fl[0, 5, 0] = 4
    out = photo(cur, prev, fl, mask)
    assert out['mask_out'][0].tolist() == [0, 3, 1, 2, 255, 2] and out['residual'][0].tolist() == [0, 20, 30, 0, 0, 0]
    assert out['counts'].tolist() == [2, 1, 60, 3600, 1, 1, 1, 0, 0, 0] + [3, 1, 91, 8101, 1, 1, 1, 0, 0, 0] + [1]
    assert out['sums'].tolist() == [60.0, 3600.0, 91.0, 8101.0]
    fig = fp.photo_from_tables(out['counts'], out['sums'])
    assert fig['visible']['mae_warp'] == 10.0 and fig['masked']['n'] == 3 and fig['all']['n'] == 5 and fig['outside'] == 1 and fig['outside_share'] == 1 / 6
    assert fig['visible']['flagged_share'] == 0.5 and fig['masked']['flagged'] == 1          # flagged is counted in the masked group too
    none = photo(cur, prev, fl)                                                  # without a mask: one group
    assert none['mask_out'][0].tolist() == [0, 3, 3, 0, 0, 2] and none['counts'][0] == 5 and not none['counts'][10:20].any()


def test_the_residual_rounds_half_up_and_ends_at_255():
    prev, cur = frame(1, 4, 255), frame(1, 4)
    cur[0, 1] = (1, 1, 0)                                                        # aw 763, e 254.33 -> 254
    cur[0, 2] = (1, 0, 0)                                                        # aw 764, e 254.67 -> 255
    cur[0, 3] = (3, 0, 0)                                                        # aw 762, e 254 -> 254
    out = photo(cur, prev, flow(1, 4))
    assert out['residual'][0].tolist() == [255, 254, 255, 254] and out['counts'][7] == 4
    prev = frame(1, 2)
    prev[0, 0] = (1, 0, 0); prev[0, 1] = (2, 0, 0)                               # e 1/3 -> 0, e 2/3 -> 1
    prev2 = frame(1, 2)
    prev2[0, 0] = (1, 0, 1); prev2[0, 1] = (3, 3, 3)
    assert photo(frame(1, 2), prev, flow(1, 2))['residual'][0].tolist() == [0, 1] and photo(frame(1, 2), prev2, flow(1, 2))['residual'][0].tolist() == [1, 3]


def random_tables(seed, masked=True):
    rng = np.random.default_rng(seed)
    H, W = 11, 17
    prev = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    cur = np.clip(np.roll(prev, 1, axis=1).astype(np.int64) + rng.integers(-9, 10, size=prev.shape), 0, 255).astype(np.uint8)
    fl = (flow(H, W, -1.0) + rng.standard_normal((H, W, 2)) * 0.3).astype(np.float32)
    fl[0, :3] = np.nan
    return photo(cur, prev, fl, rng.integers(0, 3, size=(H, W)).astype(np.uint8) if masked else None)


def test_the_figures_equal_the_restated_ones():
    for seed in (1, 2, 3):
        t = random_tables(seed)
        got, want = fp.photo_from_tables(t['counts'], t['sums']), R.figures(t['counts'], t['sums'])
        assert got['outside'] == want['outside'] >= 3 and got['outside_share'] == want['outside_share']
        for grp in ('all',) + fp.GROUPS:
            assert set(fp.FIGURES) <= set(got[grp])
            for k in fp.FIGURES + ('n', 'flagged'):
                assert math.isclose(got[grp][k], want[grp][k], rel_tol=1e-14, abs_tol=0), (grp, k)     # a handful of float64 operations on the same tables
        assert got['all']['n'] == got['visible']['n'] + got['masked']['n'] and 0 < got['all']['ratio'] < 1 and got['all']['gain_db'] > 0
        assert got['all']['helped'] > 0.5
    empty = fp.photo_from_tables(np.zeros(21, dtype=np.int64), np.zeros(4))
    assert all(empty[g][k] == 0 for g in ('all',) + fp.GROUPS for k in fp.FIGURES if not k.startswith('psnr')) and empty['outside_share'] == 0
    assert empty['all']['psnr_warp'] == float('inf')                             # no pixel, no error


def test_stats_rows_sum_to_the_video_and_the_result_survives_json():
    a, b = random_tables(4), random_tables(5)
    st = fp.PhotoStats(thr=12.0)
    v = st.add_tables('clip', np.stack([a['counts'], b['counts']]), np.stack([a['sums'], b['sums']]), 2)
    assert np.array_equal(v['counts'], a['counts'] + b['counts']) and v['sums'].tobytes() == (a['sums'] + b['sums']).tobytes() and len(v['per_pair']) == 2
    st.add_tables(None, a['counts'], a['sums'])
    res = st.result()
    assert res['pairs'] == 3 and res['thr'] == 12.0 and res['counts'] == (2 * a['counts'] + b['counts']).tolist()
    assert [r['video'] for r in res['per_video']] == ['clip', 1] and [(r['video'], r['pair']) for r in res['per_pair']] == [('clip', 1), ('clip', 2)]
    assert res['all']['n'] == sum(r['all']['n'] for r in res['per_video']) and res['per_pair'][1]['all'] == fp.photo_from_tables(b['counts'], b['sums'])['all']
    assert json.loads(json.dumps(res)) == res
    zero = fp.PhotoStats()
    zero.add_tables('still', [4] + [0] * 20, [0.0] * 4)
    rz = zero.result()
    assert rz['all']['psnr_warp'] == float('inf') and json.loads(json.dumps(rz)) == rz          # inf survives as Infinity
    with pytest.raises(ValueError):
        fp.PhotoStats(thr=-1.0)
    with pytest.raises(ValueError):
        fp.PhotoStats(thr=float('nan'))


def test_photo_text_layout_and_the_files(tmp_path):
    a, b = random_tables(4), random_tables(5, masked=False)
    st = fp.PhotoStats()
    st.add_tables('clip_a', a['counts'], a['sums'])
    st.add_tables('clip_b', b['counts'], b['sums'])
    res = st.result()
    lines = fp.photo_text(res).splitlines()
    assert lines[0] == '=' * 122 and lines[2] == '-' * 122 == lines[9] and len(lines) == 14
    assert lines[1].split() == ['VIDEO', '|', 'GROUP', 'N', 'MAE-w', 'MAE-s', 'RATIO', 'PSNR-w', 'PSNR-s', 'GAIN', '>4', '>8', '>16', '>32', 'HELP', 'HURT', 'FLAG']
    assert [ln.split()[0] for ln in lines[3:9]] == ['clip_a'] * 3 + ['clip_b'] * 3 and [ln.split()[2] for ln in lines[3:6]] == ['all', 'visible', 'masked']
    tot = lines[10].split()
    assert tot[:2] == ['All', '(2)'] and tot[3] == 'all' and tot[4] == str(res['all']['n']) and tot[5] == '%.3f' % res['all']['mae_warp']
    assert tot[7] == '%.3f' % res['all']['ratio'] and tot[-1] == '%.2f' % (100 * res['all']['flagged_share'])
    assert lines[13] == 'thr 16  outside %d (%.2f %%)' % (res['outside'], 100 * res['outside_share']) and res['outside'] >= 6
    fp.write_outputs(res, str(tmp_path))
    assert open(str(tmp_path / 'flow-photo.txt')).read() == fp.photo_text(res) and json.load(open(str(tmp_path / 'flow-photo.json'))) == res


def test_the_residual_palette():
    assert fp.RESIDUAL_PALETTE.shape == (256, 3) and fp.RESIDUAL_PALETTE.dtype == np.uint8 and fp.RESIDUAL_PALETTE[0].tolist() == [0, 0, 0]
    assert fp.RESIDUAL_PALETTE[1:].any(axis=1).all()                             # only a zero residual keeps the frame
    assert fp.RESIDUAL_PALETTE[64:].tolist() == [[255, 255, 255]] * 192 and (np.diff(fp.RESIDUAL_PALETTE.astype(int).sum(1)) >= 0).all()
    assert fp.PHOTO_THR == 16.0 and fp.COUNT_CELLS == 21 and fp.SUM_CELLS == 4


# ---------------------------------------------------------------------------------------------- the C entry points without a GPU
def test_ws_bytes_is_four_doubles_per_workgroup_and_refuses_bad_sizes():
    lib = hip.load()
    assert lib.vps_flow_photo_ws_bytes(1, 1) == 32 and lib.vps_flow_photo_ws_bytes(1, 1024) == 32 and lib.vps_flow_photo_ws_bytes(1, 1025) == 64
    big = lib.vps_flow_photo_ws_bytes(1024, 2048)
    assert big == 32 * 1024 and lib.vps_flow_photo_ws_bytes(4096, 4096) == big  # capped: grid-stride beyond it
    assert lib.vps_flow_photo_ws_bytes(0, 4) == -1002 and lib.vps_flow_photo_ws_bytes(4, -1) == -1002
    assert lib.vps_flow_photo_ws_bytes(1 << 16, 1 << 15) == -1002
    assert lib.vps_abi_version() == 21


def test_flow_photo_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(cur=p, prev=p, H=4, W=4, flow=p, ld=2, co=0, mask=p, thr=16.0, counts=p, sums=p, mout=p, res=p, ws=p, wsb=32)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_flow_photo(a['cur'], a['prev'], a['H'], a['W'], a['flow'], a['ld'], a['co'], a['mask'], a['thr'], a['counts'], a['sums'], a['mout'],
                                  a['res'], a['ws'], a['wsb'], None)
    for name in ('cur', 'prev', 'flow', 'counts', 'sums', 'ws'):
        assert call(**{name: None}) == -1001, name
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(W=-3) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    assert call(ld=1) == -1003 and call(ld=4, co=3) == -1003 and call(co=-1) == -1003
    assert call(counts=ctypes.c_void_p(4100)) == -1004 and call(sums=ctypes.c_void_p(4100)) == -1004
    assert call(flow=ctypes.c_void_p(4098)) == -1004 and call(flow=ctypes.c_void_p(4097)) == -1004
    assert call(ws=ctypes.c_void_p(4100)) == -1005 and call(wsb=31) == -1005 and call(wsb=0) == -1005 and call(wsb=-32) == -1005
    assert call(H=1, W=1025, wsb=32) == -1005                                    # two workgroups need two slots
    assert call(thr=-0.5) == -1006 and call(thr=float('nan')) == -1006 and call(thr=-float('inf')) == -1006


def test_the_device_entries_need_a_device():
    z, f = np.zeros((2, 2, 3), dtype=np.uint8), np.zeros((2, 2, 2), dtype=np.float32)
    with pytest.raises(hip.VpsHipError):
        fp.flow_photometric(z, z, f)
    with pytest.raises(hip.VpsHipError):
        fp.PhotoEvaluator(device='cpu')


def test_the_photometric_option_of_the_tc_evaluator_refuses_what_it_cannot_do():
    seg = np.arange(256, dtype=np.uint8)
    with pytest.raises(ValueError):
        tc.TcEvaluator(seg, 6, photometric=16.0)                                 # not without occlusion=True
    with pytest.raises(ValueError):
        tc.TcEvaluator(seg, 6, occlusion=True, photometric=-1.0)
    with pytest.raises(ValueError):
        tc.TcEvaluator(seg, 6, occlusion=True, photometric=float('nan'))
    z, f = np.zeros((2, 2, 3), dtype=np.uint8), np.zeros((2, 2, 2), dtype=np.float32)
    for photometric, frames in ((None, (z, z)), (16.0, None)):                   # the first check of add_pair: it needs no device
        ev = tc.TcEvaluator.__new__(tc.TcEvaluator)
        ev.photometric, ev.occlusion, ev._open = photometric, True, None
        with pytest.raises(ValueError):
            ev.add_pair(z, z, f, back_flow=f, frames=frames)
        with pytest.raises(ValueError):
            ev.add_video([z, z], [None, f], back_flows=[None, f], frames=None if frames is None else [z, z])
