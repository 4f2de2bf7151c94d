"""Temporal consistency without a device: the definition's hand-derived answers through the per-pixel restatement
(tests/tc_restate.py) and through `vps_amd.tc.tc_from_tables` / `TcStats` on the restatement's tables (integers exact; floats to 1e-12
relative: both are float64 means of at most a few dozen quotients of the same integers), the argument checks of `vps_tc_accumulate`,
the layout of tc.txt and the JSON round trip."""
import ctypes
import json
import math

import numpy as np
import pytest

import tc_restate as R
from vps_amd import hip, tc

RTOL = 1e-12
C3 = 3                                                      # classes 0, 1 stuff, 2 thing; every other pan_seg value is void
SEG3 = np.full(256, 255, dtype=np.uint8); SEG3[:3] = [0, 1, 2]


def close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b), 1e-300)


def umap(H, W, seg=0, ins=0, obj=0):
    m = np.zeros((H, W, 3), dtype=np.uint8)
    m[..., 0], m[..., 1], m[..., 2] = seg, ins, obj
    return m


def zero_flow(H, W):
    return np.zeros((H, W, 2), dtype=np.float32)


def base_map(H=12, W=16):
    """stuff 0 above stuff 1, a thing (2, obj 7) and a thing (2, obj 9), a void corner"""
    m = umap(H, W, 0)
    m[H // 2:, :, 0] = 1
    m[2:6, 3:8] = (2, 1, 7)
    m[5:10, 10:14] = (2, 2, 9)
    m[:2, :2] = (255, 0, 0)
    return m


def case_identical():
    m = base_map()
    return dict(prev=m, cur=m.copy(), flow=zero_flow(12, 16), keys=[2 * 256 + 7, 2 * 256 + 9],
                want=dict(tc=1.0, tc_sem=1.0, tc_track=1.0, in_view=192, outside=0, n_tracks=2, n_classes=3))


def case_shift():
    """cur(x, y) = prev(x + 3, y - 2) with flow (+3, -2): every in-view pixel agrees; the 3 right columns and 2 top rows are uncovered"""
    H, W = 12, 16
    prev = base_map(H, W)
    cur = umap(H, W, 1)                                      # the uncovered strip holds anything
    cur[2:, :W - 3] = prev[:H - 2, 3:]
    flow = zero_flow(H, W); flow[..., 0] = 3.0; flow[..., 1] = -2.0
    return dict(prev=prev, cur=cur, flow=flow, keys=[2 * 256 + 7, 2 * 256 + 9],
                want=dict(tc=1.0, tc_sem=1.0, tc_track=1.0, in_view=(H - 2) * (W - 3), outside=H * W - (H - 2) * (W - 3), n_tracks=2, n_classes=3))


def case_swapped_ids():
    """two tracks of one class exchange their ids: the classes agree everywhere, no track pixel keeps its id"""
    prev, cur = umap(8, 8, 2, 1, 1), umap(8, 8, 2, 1, 2)
    prev[:, 4:, 2], cur[:, 4:, 2] = 2, 1
    return dict(prev=prev, cur=cur, flow=zero_flow(8, 8), keys=[2 * 256 + 1, 2 * 256 + 2],
                want=dict(tc=0.0, tc_sem=1.0, tc_track=0.0, in_view=64, outside=0, n_tracks=2, n_classes=1))


def case_relabelled_half():
    """8 x 10: class 0 holds 32 pixels of prev and keeps 16 of them, the other 16 become class 1; class 1 keeps its 32; a thing of 16
    pixels stays. conf[0][0] = 16, conf[0][1] = 16, conf[1][1] = 32, conf[2][2] = 16:
    IoU_0 = 16 / (32 + 16 - 16) = 1/2, IoU_1 = 32 / (32 + 48 - 32) = 2/3, IoU_2 = 1; TC_sem = (1/2 + 2/3 + 1) / 3 = 13/18; TC_track = 1"""
    prev, cur = umap(8, 10, 0), umap(8, 10, 0)
    prev[4:, :, 0] = 1
    cur[2:, :, 0] = 1
    prev[:, 8:] = cur[:, 8:] = (2, 1, 5)
    return dict(prev=prev, cur=cur, flow=zero_flow(8, 10), keys=[2 * 256 + 5],
                want=dict(tc=math.sqrt(13.0 / 18.0), tc_sem=13.0 / 18.0, tc_track=1.0, in_view=80, outside=0, n_tracks=1, n_classes=3))


def case_all_void():
    m = umap(5, 7, 255)
    return dict(prev=m, cur=m.copy(), flow=zero_flow(5, 7), keys=[2 * 256 + 5],
                want=dict(tc=0.0, tc_sem=0.0, tc_track=0.0, in_view=35, outside=0, n_tracks=0, n_classes=0))


def case_no_keys():
    m = base_map()
    return dict(prev=m, cur=m.copy(), flow=zero_flow(12, 16), keys=[],
                want=dict(tc=0.0, tc_sem=1.0, tc_track=0.0, in_view=192, outside=0, n_tracks=0, n_classes=3))


CASES = dict(identical=case_identical, shift=case_shift, swapped_ids=case_swapped_ids, relabelled_half=case_relabelled_half,
             all_void=case_all_void, no_keys=case_no_keys)


def restated(case, id_channel=2):
    return R.pair_tables(case['prev'], case['cur'], case['flow'], SEG3, C3, id_channel, case['keys'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_derived_cases_through_the_restatement(name):
    case = CASES[name]()
    t = R.terms(restated(case))
    for k, v in case['want'].items():
        assert close(t[k], v) if isinstance(v, float) else t[k] == v, (k, t[k], v)


@pytest.mark.parametrize('name', sorted(CASES))
def test_hand_derived_cases_through_tc_from_tables(name):
    case = CASES[name]()
    tab = restated(case)
    t = tc.tc_from_tables(*[tab[k] for k in R.NAMES])
    for k, v in case['want'].items():
        assert close(t[k], v) if isinstance(v, float) else t[k] == v, (k, t[k], v)
    want = R.terms(tab)
    assert all(close(a, r[2]) for a, r in zip(t['class_iou'], want['class_rows']))
    assert all(close(a, r[2]) for a, r in zip(t['track_iou'], want['track_rows']))


def test_the_relabelled_case_has_the_confusion_matrix_worked_out_by_hand():
    conf = restated(case_relabelled_half())['conf']
    want = np.zeros((4, 4), dtype=np.int64)
    want[0][0], want[0][1], want[1][1], want[2][2] = 16, 16, 32, 16
    assert np.array_equal(conf, want)


def test_the_inconsistency_map_of_the_hand_cases():
    assert not restated(case_identical())['map'].any()
    m = restated(case_shift())['map']
    assert (m[:2] == 3).all() and (m[:, 13:] == 3).all() and not m[2:, :13].any()
    assert (restated(case_swapped_ids())['map'] == 2).all()
    m = restated(case_relabelled_half())['map']
    assert (m[2:4, :8] == 1).all() and m.sum() == 16
    no = case_swapped_ids(); no['keys'] = [2 * 256 + 1]                         # one key unlisted: not a track disagreement
    assert not restated(no)['map'].any()


def test_the_halves_round_to_the_next_pixel_and_bad_values_fall_out():
    """floor(s + 0.5): s = -0.5 is pixel 0 and the next float below it is outside; s = W - 0.5 is outside, the float below is W - 1"""
    W = 6
    flow = np.zeros((6, W, 2), dtype=np.float32)                                 # column 0 of every row: sx is the flow itself
    flow[0, 0, 0] = -0.5
    flow[1, 0, 0] = np.nextafter(np.float32(-0.5), np.float32(-1))
    flow[2, 0, 0] = np.float32(W - 0.5)
    flow[3, 0, 0] = np.nextafter(np.float32(W - 0.5), np.float32(0))
    flow[4, 0, 0] = np.nan
    flow[5, 0, 1] = np.inf
    inview, ix, _ = R.warp(flow)
    assert inview[:, 0].tolist() == [True, False, False, True, False, False] and inview[:, 1:].all()
    assert ix[0, 0] == 0 and ix[3, 0] == W - 1
    for bad in (-np.inf, 1e30, -1e30):
        flow[0, 0, 0] = bad
        assert not R.warp(flow)[0][0, 0]
    flow[0, 0, 0] = -0.0
    assert R.warp(flow)[0][0, 0]


def test_id_channel_one_reads_pan_ins():
    case = case_swapped_ids()                                                    # pan_ins is 1 everywhere: with channel 1 nothing is swapped
    case['keys'] = [2 * 256 + 1]
    t = R.terms(restated(case, id_channel=1))
    assert t['tc'] == 1.0 and t['n_tracks'] == 1


def stats_of(cases, per_pair=False):
    st = tc.TcStats(SEG3, C3)
    tabs = []
    for i, case in enumerate(cases):
        tab = restated(case)
        tabs.append(tab)
        st.add_tables('v%d' % i, case['keys'], *[tab[k] for k in R.NAMES], pairs=R.flat(tab)[None] if per_pair else None)
    return st, tabs


def test_the_set_result_equals_the_restatement():
    st, tabs = stats_of([case_identical(), case_swapped_ids(), case_relabelled_half(), case_shift()], per_pair=True)
    got, want = st.result(), R.evaluate(tabs)
    for k in ('tc', 'tc_sem', 'tc_track'):
        assert close(got[k], want[k]), (k, got[k], want[k])
    assert got['n_tracks'] == want['n_tracks'] == 7
    assert [r['video'] for r in got['per_video']] == ['v0', 'v1', 'v2', 'v3']
    for r, tab in zip(got['per_video'], tabs):
        w = R.terms(tab)
        assert all(close(r[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track'))
    assert [(r['video'], r['pair']) for r in got['per_pair']] == [('v0', 1), ('v1', 1), ('v2', 1), ('v3', 1)]
    assert [r['tc'] for r in got['per_pair']] == [r['tc'] for r in got['per_video']]       # one pair each
    swapped = [r for r in got['tracks'] if r['video'] == 'v1']
    assert [(r['key'], r['pan_seg'], r['id'], r['same'], r['prev_size'], r['cur_size'], r['iou']) for r in swapped] == \
        [(513, 2, 1, 0, 32, 32, 0.0), (514, 2, 2, 0, 32, 32, 0.0)]
    assert got['in_view'] == 192 + 64 + 80 + 130 and got['outside'] == 62
    assert close(got['in_view_share'], 466.0 / 528.0)


def test_stats_refuse_bad_tables():
    with pytest.raises(ValueError):
        tc.TcStats(SEG3[:100], 3)
    with pytest.raises(ValueError):
        tc.TcStats(SEG3, 64)
    with pytest.raises(ValueError):
        tc.TcStats(SEG3, 0)


# ---------------------------------------------------------------------------------------------- the C entry point without a GPU
def test_bad_arguments_return_error_codes_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(prev=p, cur=p, H=4, W=4, flow=p, ld=2, coff=0, idch=2, seg=p, C=5, keys=p, n=2, conf=p, psz=p, csz=p, same=p, misc=p, flick=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_tc_accumulate(a['prev'], a['cur'], a['H'], a['W'], a['flow'], a['ld'], a['coff'], a['idch'], a['seg'], a['C'], a['keys'], a['n'],
                                     a['conf'], a['psz'], a['csz'], a['same'], a['misc'], a['flick'], None)
    for name in ('prev', 'cur', 'flow', 'seg', 'conf', 'misc', 'keys', 'psz', 'csz', 'same'):
        assert call(**{name: None}) == -1001, name
    assert call(H=0) == -1002 and call(W=0) == -1002 and call(H=-1) == -1002 and call(H=1 << 16, W=1 << 15) == -1002
    assert call(C=0) == -1003 and call(C=64) == -1003 and call(C=-1) == -1003
    assert call(n=-1) == -1004 and call(n=65537) == -1004
    assert call(idch=0) == -1005 and call(idch=3) == -1005
    for name in ('conf', 'psz', 'csz', 'same', 'misc'):
        assert call(**{name: ctypes.c_void_p(4100)}) == -1006, name
    assert call(ld=1) == -1007 and call(ld=4, coff=3) == -1007 and call(coff=-1) == -1007


def test_the_evaluator_needs_a_device():
    import torch
    with pytest.raises(hip.VpsHipError):
        tc.TcEvaluator(SEG3, C3, device='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(hip.VpsHipError):
            tc.TcEvaluator(SEG3, C3)
    with pytest.raises(ValueError):
        tc.TcEvaluator(SEG3, C3, id_channel=0)


# ---------------------------------------------------------------------------------------------- the files
def test_tc_text_layout():
    st, _ = stats_of([case_relabelled_half(), case_swapped_ids()])
    res = st.result()
    lines = tc.tc_text(res).splitlines()
    assert lines[0] == '=' * 56 and lines[2] == '-' * 56
    assert lines[1].split() == ['|', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW']
    assert lines[3].split() == ['All', '|', '%.1f' % (100 * res['tc']), '%.1f' % (100 * res['tc_sem']), '%.1f' % (100 * res['tc_track']), '3', '100.00']
    assert lines[4].split() == ['IDX', '|', 'IoU', 'INTER', 'UNION']
    assert [l.split()[0] for l in lines[5:8]] == ['0|', '1|', '2|']
    assert lines[5].split()[1:] == ['50.0', '16', '32'] and lines[6].split()[1:] == ['66.7', '32', '48']
    assert lines[8].split()[0] == 'VIDEO' and lines[9].split()[0] == 'v0' and lines[10].split()[0] == 'v1' and len(lines) == 11
    assert lines[10].split()[2:5] == ['0.0', '100.0', '0.0']


def test_the_result_survives_json_unchanged():
    st, _ = stats_of([case_relabelled_half(), case_swapped_ids(), case_no_keys()], per_pair=True)
    res = st.result()
    assert json.loads(json.dumps(res)) == res
    tracks = tc.tc_tracks_json(res)
    back = json.loads(json.dumps(tracks))
    assert back == tracks and len(back['tracks']) == 3 and len(back['per_pair']) == 3
    assert set(back['tracks'][0]) == {'video', 'key', 'pan_seg', 'id', 'iou', 'same', 'prev_size', 'cur_size'}
