"""STQ without a device: the definition's five hand-derived answers through the per-pixel restatement (tests/stq_restate.py),
`vps_amd.stq.stq_from_tables` / `StqStats` against that restatement on its own tables (integers exact; floats to 1e-12 relative: both
are float64 sums of fewer than 10^4 terms in the same fixed order, which differ by the rounding of a / b against (1 / b) * a only),
the errors of the id-table builder, the argument checks of `vps_stq_accumulate`, and the layout of the tool's stq.txt."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import stq_cases as K
import stq_restate as R
from vps_amd import hip, stq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b))


def same_result(got, want):
    """a result dict of vps_amd.stq against the restatement's"""
    for k in ('stq', 'aq', 'sq'):
        assert close(got[k], want[k]), (k, got[k], want[k])
    assert got['n'] == want['n'] and len(got['per_video']) == len(want['per_video'])
    for a, b in zip(got['per_video'], want['per_video']):
        assert a['video'] == b['video'] and a['n'] == b['n']
        assert all(close(a[k], b[k]) for k in ('stq', 'aq', 'sq')), (a, b)
    assert list(got['per_class_iou']) == list(want['per_class_iou'])
    for c in want['per_class_iou']:
        assert close(got['per_class_iou'][c], want['per_class_iou'][c])
        assert {k: got['per_class'][c][k] for k in ('tp', 'fp', 'fn')} == {k: want['per_class'][c][k] for k in ('tp', 'fp', 'fn')}
    assert len(got['tracks']) == len(want['tracks'])
    for a, b in zip(got['tracks'], want['tracks']):
        assert {k: a[k] for k in a if k != 'score'} == {k: b[k] for k in b if k != 'score'}, (a, b)
        assert close(a['score'], b['score'])


def stats_from_restated_tables(videos, cats, video_ids=None):
    """StqStats fed with the tables the restatement counts: the host half of the evaluator without a device"""
    st = stq.StqStats(cats)
    for v, frames in enumerate(videos):
        tab = R.video_tables(frames, cats)
        gt_ids, gt_info, pred_ids, _ = stq.build_id_tables(frames, cats)
        assert list(gt_ids) == tab['gt_ids'] and list(pred_ids) == tab['pred_ids']
        st.add_tables(None if video_ids is None else video_ids[v], gt_ids, gt_info, pred_ids, tab['conf'], tab['gt_size'], tab['pred_size'], tab['inter'])
    return st


# ---------------------------------------------------------------------------------------------- the hand-derived answers
@pytest.mark.parametrize('name', ['equal', 'split', 'merged', 'crowd', 'stuff'])
def test_hand_derived_cases_through_the_restatement(name):
    frames, want = K.hand_cases()[name]
    res = R.evaluate([frames], K.CATS2)
    for k, v in want.items():
        if v is not None:
            assert res[k] == v, (name, k, res[k], v)
    assert res['per_video'][0]['stq'] == res['stq'] and res['per_video'][0]['aq'] == res['aq']      # one video: the set is the video
    tab = R.video_tables(frames, K.CATS2)
    if name == 'crowd':
        assert tab['pred_size'].tolist() == [2, 0] and tab['inter'].tolist() == [[0], [2]] and tab['conf'][1][1] == 4
        assert tab['gt_size'].tolist() == [0, 2]
    if name == 'stuff':
        assert res['n'] == 0 and res['per_class_iou'] == {K.ROAD: 0.75, K.CAR: 0.0}
    if name == 'split':
        assert res['tracks'] == [{'video': 0, 'gt_id': 5, 'category_id': K.CAR, 'size': 4, 'score': 0.5, 'n_pred': 2, 'best_pred_id': 8}]


@pytest.mark.parametrize('name', ['equal', 'split', 'merged', 'crowd', 'stuff'])
def test_hand_derived_cases_through_stq_from_tables(name):
    frames, want = K.hand_cases()[name]
    res = stats_from_restated_tables([frames], K.CATS2).result()
    for k, v in want.items():
        if v is not None:
            assert res[k] == v, (name, k, res[k], v)
    same_result(res, R.evaluate([frames], K.CATS2))


# ---------------------------------------------------------------------------------------------- stq_from_tables against the restatement
@pytest.mark.parametrize('seed', range(6))
def test_stq_from_tables_equals_the_restatement_on_random_small_videos(seed):
    frames = K.random_video(seed)
    tab = R.video_tables(frames, K.CATS5)
    want = R.video_terms(tab)
    got = stq.stq_from_tables(tab['conf'], tab['gt_size'], tab['pred_size'], tab['inter'])
    assert got['n'] == want['n'] and close(got['aq_sum'], want['aq_sum'])
    assert got['tp'].tolist() == want['tp'] and got['fp'].tolist() == want['fp'] and got['fn'].tolist() == want['fn']
    rows = [(tab['gt_ids'][g], int(tab['gt_size'][g]), got['track_scores'][g], int(got['track_overlaps'][g]),
             tab['pred_ids'][got['track_best'][g]] if got['track_best'][g] >= 0 else None) for g in np.nonzero(tab['gt_size'] > 0)[0]]
    assert len(rows) == len(want['rows'])
    for a, b in zip(rows, want['rows']):
        assert a[:2] == b[:2] and a[3:] == b[3:] and close(a[2], b[2])
    assert want['n'] > 0 or seed                                       # the first seed has tracks


def test_the_set_result_equals_the_restatement():
    videos = [K.random_video(s) for s in (1, 2, 3)] + K.two_videos()
    ids = ['a', 'b', 'c', 'd', 'e']
    got = stats_from_restated_tables(videos, K.CATS5, ids).result()
    want = R.evaluate(videos, K.CATS5, ids)
    same_result(got, want)
    assert 0 < got['aq'] < 1 and 0 < got['sq'] < 1 and got['n'] == sum(v['n'] for v in got['per_video'])
    # the set's AQ is the track-weighted mean of the videos', not the mean of the per-video values
    assert close(got['aq'], sum(v['aq'] * v['n'] for v in got['per_video']) / got['n'])


def test_a_self_scored_set_is_exactly_one():
    videos = K.self_scored(K.two_videos())
    got = stats_from_restated_tables(videos, K.CATS5).result()
    assert got['stq'] == 1.0 and got['aq'] == 1.0 and got['sq'] == 1.0
    assert all(v['stq'] == 1.0 for v in got['per_video']) and all(t['score'] == 1.0 and t['n_pred'] == 1 for t in got['tracks'])


def test_an_id_switch_and_a_merged_pair_show_in_the_track_report():
    got = stats_from_restated_tables(K.two_videos(), K.CATS5).result()
    tr = {(t['video'], t['gt_id']): t for t in got['tracks']}
    assert sorted(tr) == [(0, 10), (0, 11), (0, 12), (1, 30)]          # the crowd segment 13 is no track
    assert tr[(0, 10)]['n_pred'] == 2 and tr[(0, 10)]['best_pred_id'] == 20 and tr[(0, 10)]['score'] < 0.6
    assert tr[(0, 11)]['best_pred_id'] == 22 and tr[(0, 12)]['best_pred_id'] == 22 and tr[(0, 11)]['score'] < 0.5
    assert tr[(1, 30)]['score'] > 0.9 and tr[(1, 30)]['category_id'] == 20


# ---------------------------------------------------------------------------------------------- the id tables
def test_id_tables_hold_class_thing_and_crowd_bits():
    gt_ids, gt_info, pred_ids, pred_info = stq.build_id_tables([K.rich_frame()], K.CATS5)
    assert gt_ids.dtype == np.uint32 and gt_info.dtype == np.uint8
    assert gt_ids.tolist() == sorted(s['id'] for s in K.RICH_GT) and pred_ids.tolist() == sorted(s['id'] for s in K.RICH_PRED)
    info = dict(zip(gt_ids.tolist(), gt_info.tolist()))
    assert info[1] == 0 and info[K.MAX_ID] == 3 | 64 and info[70000] == 2 | 64 | 128 and info[5] == 1 and info[77] == 4 | 64
    assert dict(zip(pred_ids.tolist(), pred_info.tolist()))[1] == 3 | 64
    assert all(v < 128 for v in pred_info)


def test_id_tables_refuse_contradictions_and_unknown_categories():
    f = K.rich_frame()
    two_cats = ({'segments_info': [K.seg(5, 3)]}, f[1], f[2], f[3])
    with pytest.raises(ValueError):
        stq.build_id_tables([f, two_cats], K.CATS5)                    # id 5 is sky in the first frame
    two_crowds = ({'segments_info': [K.seg(300, 11, 1)]}, f[1], f[2], f[3])
    with pytest.raises(ValueError):
        stq.build_id_tables([f, two_crowds], K.CATS5)
    pred_two = (f[0], {'segments_info': [{'id': 9, 'category_id': 12}]}, f[2], f[3])
    with pytest.raises(ValueError):
        stq.build_id_tables([f, pred_two], K.CATS5)
    for which in (0, 1):
        bad = list(f)
        bad[which] = {'segments_info': [K.seg(6, 99)]}
        with pytest.raises(KeyError):
            stq.build_id_tables([tuple(bad)], K.CATS5)
    same_again = stq.build_id_tables([f, f], K.CATS5)                  # the same entry in every frame is the normal case
    assert all(np.array_equal(a, b) for a, b in zip(same_again, stq.build_id_tables([f], K.CATS5)))
    with pytest.raises(ValueError):
        stq.class_indices({i: {'isthing': 0} for i in range(64)})
    with pytest.raises(ValueError):
        R.id_lists([f, two_cats], K.CATS5)
    with pytest.raises(KeyError):
        R.id_lists([(f[0], {'segments_info': [K.seg(6, 99)]}, f[2], f[3])], K.CATS5)


# ---------------------------------------------------------------------------------------------- the C entry point without a GPU
def test_bad_arguments_return_error_codes_without_a_gpu():
    lib = hip.load()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused before a launch
    ok = dict(gt=p, pred=p, npix=16, gt_ids=p, gt_info=p, ngt=2, pred_ids=p, pred_info=p, npred=2, C=5, conf=p, gsz=p, psz=p, inter=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vps_stq_accumulate(a['gt'], a['pred'], a['npix'], a['gt_ids'], a['gt_info'], a['ngt'], a['pred_ids'], a['pred_info'], a['npred'],
                                      a['C'], a['conf'], a['gsz'], a['psz'], a['inter'], None)
    for name in ('gt', 'pred', 'conf', 'psz', 'gt_ids', 'gt_info', 'gsz', 'pred_ids', 'pred_info', 'inter'):
        assert call(**{name: None}) == -1001, name
    assert call(npix=0) == -1002 and call(npix=-3) == -1002 and call(npix=1 << 31) == -1002
    assert call(C=0) == -1003 and call(C=64) == -1003 and call(C=-1) == -1003
    assert call(ngt=-1) == -1004 and call(npred=-1) == -1004
    assert call(ngt=8192, npred=8192) == -1005                         # 2^26 intersection cells + the rest: above the bound
    assert call(ngt=1 << 30, npred=1 << 30) == -1005
    assert call(conf=ctypes.c_void_p(4100)) == -1006 and call(inter=ctypes.c_void_p(4097)) == -1006
    assert lib.vps_stq_lds_cells() == 12288


def test_the_evaluator_needs_a_device():
    import torch
    with pytest.raises(hip.VpsHipError):
        stq.StqEvaluator(K.CATS5, device='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(hip.VpsHipError):
            stq.StqEvaluator(K.CATS5)


# ---------------------------------------------------------------------------------------------- the tool's files
def _tool():
    spec = importlib.util.spec_from_file_location('eval_stq_device', os.path.join(ROOT, 'tools', 'eval_stq_device.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_stq_txt_layout_from_injected_tables(tmp_path):
    videos = K.two_videos()
    res = stats_from_restated_tables(videos, K.CATS5).result()
    _tool().write_outputs(res, str(tmp_path))
    text = open(tmp_path / 'stq.txt').read()
    assert text == R.stq_txt(R.evaluate(videos, K.CATS5))
    lines = text.splitlines()
    assert lines[0] == '=' * 48 and lines[1].split() == ['|', 'STQ', 'AQ', 'SQ', 'N'] and lines[2] == '-' * 38
    assert lines[3].startswith('All       |') and lines[3].split()[-1] == '4'
    assert lines[3].split()[2:5] == ['%.1f' % (100 * res[k]) for k in ('stq', 'aq', 'sq')]
    assert lines[4].split() == ['IDX', '|', 'IoU', 'TP', 'FP', 'FN'] and [l.split('|')[0].strip() for l in lines[5:10]] == ['3', '8', '11', '12', '20']
    assert lines[10].split() == ['VIDEO', '|', 'STQ', 'AQ', 'SQ', 'N'] and len(lines) == 13
    assert lines[11].startswith('0         |') and lines[12].startswith('1         |')
    tracks = json.load(open(tmp_path / 'stq-tracks.json'))
    assert tracks['stq'] == res['stq'] and tracks['tracks'] == res['tracks'] and tracks['per_video'] == res['per_video']
    assert set(tracks['tracks'][0]) == {'video', 'gt_id', 'category_id', 'size', 'score', 'n_pred', 'best_pred_id'}


def test_the_tool_takes_the_command_line_of_eval_vpq_device():
    spec = importlib.util.spec_from_file_location('eval_vpq_device', os.path.join(ROOT, 'tools', 'eval_vpq_device.py'))
    vpq = importlib.util.module_from_spec(spec); spec.loader.exec_module(vpq)
    argv = ['--submit_dir', 'a', '--truth_dir', 'b', '--pan_gt_json_file', 'c', '--nframes_per_video', '3', '--device', 'cuda:0']
    assert vars(_tool().parse_args(argv)) == vars(vpq.parse_args(argv))
    assert vars(_tool().parse_args([])) == vars(vpq.parse_args([]))
