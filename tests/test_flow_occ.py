"""The occlusion option of temporal consistency without a device: the hand-derived answers of the forward-backward check through the
per-pixel restatement (tests/flow_occ_restate.py), `vps_amd.tc.table_sizes` / `tc_from_tables` / `TcStats` / `tc_text` with and without
the option (without it the text is today's), and the argument checks of `vps_flow_occlusion` and `vps_tc_accumulate_masked`."""
import ctypes
import json

import numpy as np
import pytest

import flow_occ_restate as O
import tc_restate as R
from test_tc import C3, SEG3, base_map, case_relabelled_half, case_swapped_ids, close, restated, stats_of
from vps_amd import hip, tc


def const_flow(H, W, u, v=0.0):
    f = np.zeros((H, W, 2), dtype=np.float32)
    f[..., 0], f[..., 1] = u, v
    return f


def occ(fwd, back, alpha=0.01, beta=0.5):
    """both restatements, the loop and the array form, which must agree"""
    codes, counts = O.occlusion(fwd, back, alpha, beta)
    lcodes, lcounts = O.occlusion_loop(fwd, back, alpha, beta)
    assert np.array_equal(codes, lcodes) and np.array_equal(counts, lcounts) and int(counts.sum()) == codes.size
    return codes, counts


def test_the_loop_and_the_array_restatement_agree_on_random_and_special_flows():
    rng = np.random.default_rng(5)
    H, W = 9, 13
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], dtype=np.float32)
    for k in range(6):
        fwd = (rng.standard_normal((H, W, 2)) * (0.5, 2, 6)[k % 3]).astype(np.float32)
        back = (-fwd + rng.standard_normal((H, W, 2)) * 0.4).astype(np.float32)
        if k >= 3:
            for f in (fwd, back):
                pick = rng.integers(0, 4 * len(vals), size=f.shape)
                f[pick < len(vals)] = vals[pick[pick < len(vals)]]
        codes, counts = occ(fwd, back, alpha=(0.01, 0.0, 0.3)[k % 3], beta=(0.5, 0.0, 2.0)[k % 3])
        assert len(np.unique(codes)) == (2 if k % 3 == 1 else 3)                  # alpha = beta = 0: nothing cancels exactly, no pixel is visible


def test_zero_flows_are_visible_everywhere():
    codes, counts = occ(const_flow(5, 7, 0), const_flow(5, 7, 0))
    assert not codes.any() and counts.tolist() == [35, 0, 0]


def test_a_unit_shift_and_its_inverse_cancel_except_in_the_column_that_leaves_the_view():
    """fwd = (+1, 0) reads back at x + 1, which holds (-1, 0): d2 = 0. Column W-1 points at x = W: not in view."""
    H, W = 4, 6
    codes, counts = occ(const_flow(H, W, 1), const_flow(H, W, -1))
    assert not codes[:, :W - 1].any() and (codes[:, W - 1] == 2).all() and counts.tolist() == [H * (W - 1), 0, H]


def test_a_whole_pixel_against_a_zero_backward_flow_is_occluded_and_seven_tenths_is_not():
    """fwd = (1, 0), back = 0: d2 = 1, m = 1, thr = 0.01 + 0.5 = 0.51 < 1: occluded.
    fwd = (0.7, 0), back = 0: d2 = 0.49, thr = 0.01 * 0.49 + 0.5 = 0.5049 >= 0.49: visible (fp32 rounding is far from deciding either)."""
    H, W = 3, 5
    codes, counts = occ(const_flow(H, W, 1), const_flow(H, W, 0))
    assert (codes[:, :W - 1] == 1).all() and (codes[:, W - 1] == 2).all() and counts.tolist() == [0, H * (W - 1), H]
    codes, counts = occ(const_flow(H, W, 0.7), const_flow(H, W, 0))
    assert not codes[:, :W - 1].any() and (codes[:, W - 1] == 2).all()       # x = W-1: sx = W - 0.3 rounds to W, not in view


def test_a_square_that_moves_two_pixels_uncovers_a_strip():
    """8 x 12, a static background and a 3 x 3 square that sits at rows 2..4, columns 2..4 in prev and at columns 4..6 in cur.
    fwd (grid of cur, into prev): (-2, 0) on the square's place in cur (columns 4..6), 0 elsewhere.
    back (grid of prev, into cur): (+2, 0) on the square's place in prev (columns 2..4), 0 elsewhere.
    A pixel of cur on the square reads back two columns to the left, on the square in prev: -2 + 2 = 0, visible. A background pixel of
    cur has fwd 0 and reads back where it stands: 0 everywhere but on the square's place in prev. Of those three columns, 4 is under
    the square in cur (handled above), 2 and 3 are background in cur: fwd 0 + back 2, d2 = 4 > 0.01 * 4 + 0.5. So the flagged set is
    rows 2..4 x columns 2..3, the strip the square has uncovered: background that was hidden in prev."""
    H, W = 8, 12
    fwd, back = const_flow(H, W, 0), const_flow(H, W, 0)
    fwd[2:5, 4:7, 0] = -2
    back[2:5, 2:5, 0] = 2
    codes, counts = occ(fwd, back)
    want = np.zeros((H, W), dtype=np.uint8)
    want[2:5, 2:4] = 1
    assert np.array_equal(codes, want) and counts.tolist() == [H * W - 6, 6, 0]


def test_a_nan_in_the_backward_flow_under_a_finite_forward_flow_is_occluded():
    """The four corners are always read, x1 = x0 + 1 and y1 = y0 + 1 also under a weight of 0, and 0 * NaN is NaN: a NaN at (1, 2)
    flags every pixel that has it among its corners - (1, 2) itself, (1, 1) through x1, (0, 2) through y1, (0, 1) through both - with a
    zero forward flow as with a sub-pixel one. 'A NaN anywhere gives occluded.'"""
    H, W = 3, 4
    back = const_flow(H, W, 0)
    back[1, 2, 1] = np.nan
    want = np.zeros((H, W), dtype=np.uint8); want[0:2, 1:3] = 1
    for fwd in (const_flow(H, W, 0), const_flow(H, W, 0.25, 0.25)):
        codes, counts = occ(fwd, back)
        assert np.array_equal(codes, want) and counts.tolist() == [H * W - 4, 4, 0]


def test_minus_one_half_is_in_view_and_reads_the_clamped_column_zero():
    """sx = -0.5: qx = floor(0) = 0, in view. x0 = floor(-0.5) = -1, wx = 0.5, x1 = 0: both corners are column 0 after the clamp, so
    bt = b + 0.5 * (b - b) = back(column 0). With back = (+0.5, 0) there the flows cancel; the other columns hold what would not."""
    H, W = 1, 4
    fwd = const_flow(H, W, 0); fwd[0, 0, 0] = -0.5
    back = const_flow(H, W, 9, 9); back[0, 0] = (0.5, 0)
    codes, _ = occ(fwd, back)
    assert codes.tolist() == [[0, 1, 1, 1]]
    back[0, 0] = (9, 9)
    assert occ(fwd, back)[0].tolist() == [[1, 1, 1, 1]]
    fwd[0, 0, 0] = np.nextafter(np.float32(-0.5), np.float32(-1))
    assert occ(fwd, back)[0][0, 0] == 2


def test_bad_forward_values_fall_out_of_view_whatever_the_backward_flow_holds():
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        fwd = const_flow(2, 3, 0); fwd[1, 1, 0] = bad
        codes, counts = occ(fwd, const_flow(2, 3, 0))
        assert codes[1, 1] == 2 and counts.tolist() == [5, 0, 1]


# ---------------------------------------------------------------------------------------------- the masked counting, restated
def test_the_masked_restatement_skips_exactly_the_masked_in_view_pixels():
    m = base_map()
    H, W = m.shape[:2]
    flow = const_flow(H, W, 3, -2)                                              # in view: rows 2.., columns ..W-4 (test_tc.case_shift)
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[:4, :] = 1                                                              # rows 0, 1 are not in view: they stay outside
    mask[6, 5] = 2
    keys = [2 * 256 + 7, 2 * 256 + 9]
    plain = R.pair_tables(m, m, flow, SEG3, C3, 2, keys)
    got = O.masked_pair_tables(m, m, flow, mask, SEG3, C3, 2, keys)
    nmask = 2 * (W - 3) + 1
    assert got['masked'].tolist() == [nmask] and got['misc'].tolist() == [plain['misc'][0] - nmask, plain['misc'][1]]
    assert int(got['misc'].sum() + got['masked'][0]) == H * W and got['conf'].sum() == got['misc'][0]
    assert (got['map'][:2] == 3).all() and (got['map'][2:4, :W - 3] == 4).all() and (got['map'][2:4, W - 3:] == 3).all() and got['map'][6, 5] == 4
    free = O.masked_pair_tables(m, m, flow, np.zeros((H, W), dtype=np.uint8), SEG3, C3, 2, keys)
    assert all(np.array_equal(free[k], plain[k]) for k in R.NAMES + ('map',)) and free['masked'].tolist() == [0]


# ---------------------------------------------------------------------------------------------- tables, results, text
def test_table_sizes_keep_their_value_and_the_option_appends_one_cell():
    assert tc.table_sizes(3, 5) == [16, 5, 5, 5, 2] == tc.table_sizes(3, 5, occlusion=False)
    assert tc.table_sizes(3, 5, occlusion=True) == [16, 5, 5, 5, 2, 1]


def test_tc_from_tables_reports_the_occluded_share_only_with_the_masked_cell():
    tab = restated(case_relabelled_half())
    plain = tc.tc_from_tables(*[tab[k] for k in R.NAMES])
    assert 'occluded' not in plain and 'occluded_share' not in plain
    occ = tc.tc_from_tables(*[tab[k] for k in R.NAMES], masked=[20])
    assert occ['occluded'] == 20 and close(occ['occluded_share'], 20.0 / 100.0)            # 80 pixels in view + 20 masked
    assert all(np.array_equal(occ[k], plain[k]) for k in plain)


def occ_stats(per_pair=True):
    st = tc.TcStats(SEG3, C3)
    for i, (case, nm) in enumerate(((case_relabelled_half(), 20), (case_swapped_ids(), 0))):
        tab = restated(case)
        row = np.concatenate([R.flat(tab), [nm]])
        st.add_tables('v%d' % i, case['keys'], *[tab[k] for k in R.NAMES], pairs=row[None] if per_pair else None, masked=[nm])
    return st


def test_the_result_and_the_files_gain_the_occluded_share_only_with_the_option():
    plain = stats_of([case_relabelled_half(), case_swapped_ids()], per_pair=True)[0].result()
    res = occ_stats().result()
    assert set(res) - set(plain) == {'occluded', 'occluded_share'} and 'occluded' not in tc.tc_tracks_json(plain)
    assert res['occluded'] == 20 and close(res['occluded_share'], 20.0 / 164.0) and close(res['in_view_share'], 144.0 / 164.0)
    assert [r['occluded_share'] for r in res['per_video']] == [0.2, 0.0] and [r['occluded_share'] for r in res['per_pair']] == [0.2, 0.0]
    assert all('occluded_share' not in r for r in plain['per_video'] + plain['per_pair'])
    assert all(res[k] == plain[k] for k in ('tc', 'tc_sem', 'tc_track', 'conf', 'tracks', 'in_view', 'outside'))
    doc = tc.tc_tracks_json(res)
    assert json.loads(json.dumps(doc)) == doc and doc['occluded'] == 20 and close(doc['occluded_share'], 20.0 / 164.0)
    assert json.loads(json.dumps(res)) == res
    with pytest.raises(ValueError):
        st = occ_stats()
        tab = restated(case_swapped_ids())
        st.add_tables('plain', case_swapped_ids()['keys'], *[tab[k] for k in R.NAMES])


def test_tc_text_has_the_occ_column_only_with_the_option():
    plain = stats_of([case_relabelled_half(), case_swapped_ids()])[0].result()
    lines = tc.tc_text(plain).splitlines()                                      # today's text (tests/test_tc.py::test_tc_text_layout)
    assert lines[0] == '=' * 56 and lines[1].split() == ['|', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW'] and len(lines[3].split()) == 7
    assert 'OCC' not in tc.tc_text(plain)
    res = occ_stats(per_pair=False).result()
    olines = tc.tc_text(res).splitlines()
    assert olines[0] == '=' * 64 and olines[2] == '-' * 64 and len(olines) == len(lines)
    assert olines[1].split() == ['|', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW', 'OCC']
    assert olines[3].split() == lines[3].split()[:6] + ['%.2f' % (100 * 144.0 / 164.0), '%.2f' % (100 * 20.0 / 164.0)]
    assert olines[4:8] == lines[4:8]                                            # the class rows are the same
    assert olines[8].split() == ['VIDEO', '|', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW', 'OCC']
    assert olines[9].split()[-2:] == ['80.00', '20.00'] and olines[10].split()[-2:] == ['100.00', '0.00']


def test_the_palette_has_a_grey_for_code_four_and_keeps_the_other_four():
    assert tc.FLICKER_PALETTE[:4] == ((0, 0, 0), (255, 0, 0), (255, 200, 0), (0, 90, 255)) and len(tc.FLICKER_PALETTE) == 5
    r, g, b = tc.FLICKER_PALETTE[4]
    assert r == g == b and 0 < r < 255


# ---------------------------------------------------------------------------------------------- the C entry points without a GPU
def test_flow_occlusion_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(fwd=p, fld=2, fco=0, back=p, bld=2, bco=0, H=4, W=4, alpha=0.01, beta=0.5, occ=p, counts=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_flow_occlusion(a['fwd'], a['fld'], a['fco'], a['back'], a['bld'], a['bco'], a['H'], a['W'], a['alpha'], a['beta'], a['occ'],
                                      a['counts'], None)
    assert call(fwd=None) == -1001 and call(back=None) == -1001 and call(occ=None, counts=None) == -1001
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(W=-3) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    for f in ('f', 'b'):
        assert call(**{f + 'ld': 1}) == -1003 and call(**{f + 'ld': 4, f + 'co': 3}) == -1003 and call(**{f + 'co': -1}) == -1003, f
    assert call(counts=ctypes.c_void_p(4100)) == -1004
    assert call(alpha=-0.01) == -1005 and call(beta=-1.0) == -1005 and call(alpha=float('nan')) == -1005 and call(beta=float('nan')) == -1005


def test_tc_accumulate_masked_refuses_bad_arguments_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    ok = dict(prev=p, cur=p, H=4, W=4, flow=p, ld=2, coff=0, idch=2, seg=p, C=5, keys=p, n=2, conf=p, psz=p, csz=p, same=p, misc=p, flick=None, mask=p,
              masked=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_tc_accumulate_masked(a['prev'], a['cur'], a['H'], a['W'], a['flow'], a['ld'], a['coff'], a['idch'], a['seg'], a['C'], a['keys'],
                                            a['n'], a['conf'], a['psz'], a['csz'], a['same'], a['misc'], a['flick'], a['mask'], a['masked'], None)
    for name in ('prev', 'cur', 'flow', 'seg', 'conf', 'misc', 'keys', 'psz', 'csz', 'same', 'mask', 'masked'):
        assert call(**{name: None}) == -1001, name
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    assert call(C=0) == -1003 and call(C=64) == -1003
    assert call(n=-1) == -1004 and call(n=65537) == -1004
    assert call(idch=0) == -1005 and call(idch=3) == -1005
    for name in ('conf', 'psz', 'csz', 'same', 'misc', 'masked'):
        assert call(**{name: ctypes.c_void_p(4100)}) == -1006, name
    assert call(ld=1) == -1007 and call(ld=4, coff=3) == -1007 and call(coff=-1) == -1007


def test_the_device_entries_need_a_device():
    import torch
    with pytest.raises(hip.VpsHipError):
        tc.flow_occlusion(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2))
    with pytest.raises(hip.VpsHipError):
        tc.TcEvaluator(SEG3, C3, device='cpu', occlusion=True)
