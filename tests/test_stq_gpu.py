"""GPU: `vps_stq_accumulate` (csrc/stq_ops.hip) and `vps_amd.stq.StqEvaluator` against the per-pixel restatement
(tests/stq_restate.py). Tables are compared with `array_equal`, results to 1e-12 relative (float64 sums of fewer than 10^4 terms in the
same order on both sides; see tests/test_stq.py)."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import stq_cases as K
import stq_restate as R
from test_stq import same_result
from vps_amd import hip, stq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
C5 = len(K.CATS5)
NAMES = ('conf', 'gt_size', 'pred_size', 'inter')


class Tables:
    """the id lists of `frames` on the device and one set of zeroed device tables"""

    def __init__(self, dev, frames, cats=K.CATS5):
        self.dev, self.C = dev, len(cats)
        self.ids = stq.build_id_tables(frames, cats)
        self.d_ids = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in self.ids]
        self.ngt, self.npred = len(self.ids[0]), len(self.ids[2])
        self.sizes = [self.C * (self.C + 1), self.ngt, self.npred + 1, self.ngt * self.npred]
        self.cells = sum(self.sizes)
        self.buf = torch.zeros(self.cells, dtype=torch.int64, device=dev)
        self.keep = []

    def views(self):
        return torch.split(self.buf, self.sizes)

    def add_ptr(self, gptr, pptr, npix):
        conf, gsz, psz, inter = self.views()
        code = hip.load().vps_stq_accumulate(ctypes.c_void_p(gptr), ctypes.c_void_p(pptr), npix, hip.ptr(self.d_ids[0]), hip.ptr(self.d_ids[1]), self.ngt,
                                             hip.ptr(self.d_ids[2]), hip.ptr(self.d_ids[3]), self.npred, self.C, hip.ptr(conf), hip.ptr(gsz), hip.ptr(psz),
                                             hip.ptr(inter), hip.stream_ptr())
        assert code == 0, code

    def add(self, frame):
        g, p = (torch.from_numpy(np.ascontiguousarray(m)).to(self.dev) for m in frame[2:4])
        self.keep += [g, p]
        self.add_ptr(g.data_ptr(), p.data_ptr(), g.shape[0] * g.shape[1])
        return self

    def host(self):
        C = self.C
        conf, gsz, psz, inter = (v.cpu().numpy() for v in self.views())
        return {'conf': conf.reshape(C, C + 1), 'gt_size': gsz, 'pred_size': psz, 'inter': inter.reshape(self.ngt, self.npred)}


def equal_tables(got, want):
    for k in NAMES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k


def by_id(tab, ids):
    """the non-zero cells keyed by segment ids: comparable between id lists of different lengths"""
    gt_ids, pred_ids = [int(v) for v in ids[0]], [int(v) for v in ids[2]] + [-1]
    out = {('c', r, c): int(v) for (r, c), v in np.ndenumerate(tab['conf']) if v}
    out.update({('g', gt_ids[i]): int(v) for i, v in enumerate(tab['gt_size']) if v})
    out.update({('p', pred_ids[i]): int(v) for i, v in enumerate(tab['pred_size']) if v})
    out.update({('i', gt_ids[r], pred_ids[c]): int(v) for (r, c), v in np.ndenumerate(tab['inter']) if v})
    return out


def cut(frame, npix, shape=None):
    """the first `npix` pixels of a frame's maps as a 1 x npix (or `shape`) frame"""
    shape = shape or (1, npix)
    return frame[0], frame[1], frame[2].reshape(-1, 3)[:npix].reshape(*shape, 3), frame[3].reshape(-1, 3)[:npix].reshape(*shape, 3)


def bound_sizes(C=C5):
    """(ngt, npred) whose tables hold exactly vps_stq_lds_cells() cells: C (C + 1) + ngt + npred + 1 + ngt npred = (ngt + 1) (npred + 1) + C (C + 1)"""
    prod = hip.load().vps_stq_lds_cells() - C * (C + 1)
    for ngt in range(40, 120):
        if prod % (ngt + 1) == 0:
            return ngt, prod // (ngt + 1) - 1
    raise AssertionError('no factorisation')


@pytest.fixture(scope='module')
def rich():
    f = K.rich_frame(unlisted_pred=True)
    return f, R.video_tables([f], K.CATS5)


# ---------------------------------------------------------------------------------------------- sizes, alignment, reads
@pytest.mark.parametrize('shape', [(1, 1), (1, 3), (1, 4), (1, 5), (1, 255), (1, 256), (1, 257), (37, 53)])
def test_sizes_around_the_lane_and_workgroup_steps(dev, rich, shape):
    f = cut(rich[0], shape[0] * shape[1], shape)
    equal_tables(Tables(dev, [f]).add(f).host(), R.video_tables([f], K.CATS5))


@pytest.mark.parametrize('offs', [(1, 1), (2, 2), (3, 3), (1, 3), (0, 2)])
def test_unaligned_maps_and_a_canary_behind_the_last_pixel(dev, rich, offs):
    """both maps as slices that start off a dword boundary, 3 * npix no multiple of 4; the bytes in front of and behind the slices hold
    0x00 in one run and 0xff in the other: nothing outside the 3 * npix bytes may reach the tables"""
    npix = 37 * 53
    f = cut(rich[0], npix, (37, 53))
    want = R.video_tables([f], K.CATS5)
    for canary in (0x00, 0xff):
        t = Tables(dev, [f])
        bufs = []
        for m, off in zip(f[2:4], offs):
            b = torch.full((4 + 3 * npix + 16,), canary, dtype=torch.uint8, device=dev)
            assert b.data_ptr() % 4 == 0
            b[off:off + 3 * npix] = torch.from_numpy(m.reshape(-1)).to(dev)
            bufs.append(b)
        t.add_ptr(bufs[0].data_ptr() + offs[0], bufs[1].data_ptr() + offs[1], npix)
        equal_tables(t.host(), want)
    for n in (1, 3, 5, 6):                                              # the first chunk is also the last one
        fs = cut(f, n)
        t = Tables(dev, [fs])
        bufs = [torch.full((32,), 0xff, dtype=torch.uint8, device=dev) for _ in range(2)]
        for b, m, off in zip(bufs, fs[2:4], offs):
            b[off:off + 3 * n] = torch.from_numpy(m.reshape(-1)).to(dev)
        t.add_ptr(bufs[0].data_ptr() + offs[0], bufs[1].data_ptr() + offs[1], n)
        equal_tables(t.host(), R.video_tables([fs], K.CATS5))


# ---------------------------------------------------------------------------------------------- every rule, both paths
def test_every_rule_on_random_label_maps(dev, rich):
    f, want = rich
    got = Tables(dev, [f]).add(f).host()
    equal_tables(got, want)
    assert want['unlisted'] == [K.RICH_PRED_UNLISTED] and got['pred_size'][-1] > 0                # the overflow cell
    assert got['conf'][:, C5].sum() > 0 and got['inter'].sum() > 0 and (got['gt_size'] > 0).sum() >= 3
    gt_ids = [int(v) for v in stq.build_id_tables([f], K.CATS5)[0]]
    assert got['gt_size'][gt_ids.index(70000)] == 0 and got['gt_size'][gt_ids.index(1)] == 0     # crowd and stuff are no tracks
    assert got['gt_size'][gt_ids.index(K.MAX_ID)] > 0
    ev = stq.StqEvaluator(K.CATS5, dev)
    with pytest.raises(KeyError, match='Segment with ID %d is presented in PNG and not presented in JSON' % K.RICH_PRED_UNLISTED):
        ev.add_video([f])
    with pytest.raises(KeyError):
        R.evaluate([[f]], K.CATS5)


def test_both_table_paths_give_identical_tables(dev):
    """the same 64x96 content with 8 x 8 listed ids, with tables exactly at the bound of the workgroup-private path, one column above it
    and 300 x 300: the restatement's tables each time, and the same counts per pair of ids"""
    ngt, npred = bound_sizes()
    bound = hip.load().vps_stq_lds_cells()
    seen = []
    for extra_gt, extra_pred, lds in ((0, 0, True), (ngt - 8, npred - 8, True), (ngt - 8, npred - 7, False), (292, 292, False)):
        f = K.rich_frame(extra_gt=extra_gt, extra_pred=extra_pred)
        t = Tables(dev, [f])
        assert (t.cells <= bound) == lds
        if (extra_gt, extra_pred) == (ngt - 8, npred - 8):
            assert t.cells == bound
        got = t.add(f).host()
        equal_tables(got, R.video_tables([f], K.CATS5))
        seen.append(by_id(got, t.ids))
    assert all(s == seen[0] for s in seen[1:]) and len(seen[0]) > 30


@pytest.mark.parametrize('extra', [0, 292])
def test_uniform_maps_and_a_checkerboard(dev, extra):
    """one pair for every pixel (every wavefront folds to one add) and two pairs alternating pixel by pixel (nothing folds)"""
    base = K.rich_frame(extra_gt=extra, extra_pred=extra)
    H, W = 64, 96
    yy, xx = np.mgrid[:H, :W]
    uni = (base[0], base[1], K.pan_of(np.full((H, W), K.MAX_ID)), K.pan_of(np.full((H, W), 65537)))
    odd = (yy + xx) & 1
    chk = (base[0], base[1], K.pan_of(np.where(odd, K.MAX_ID, 1)), K.pan_of(np.where(odd, 65537, 1)))
    for f in (uni, chk):
        got = Tables(dev, [f]).add(f).host()
        equal_tables(got, R.video_tables([f], K.CATS5))
    assert got['inter'].sum() == H * W // 2 and got['conf'].sum() == H * W


# ---------------------------------------------------------------------------------------------- accumulation, determinism
@pytest.mark.parametrize('extra', [0, 292])
def test_calls_add_to_the_tables_and_carry_past_32_bits(dev, extra):
    f = K.rich_frame(unlisted_pred=True, extra_gt=extra, extra_pred=extra)
    one = Tables(dev, [f]).add(f).host()
    two = Tables(dev, [f]).add(f).add(f).host()
    for k in NAMES:
        assert np.array_equal(two[k], 2 * one[k]) and one[k].sum() > 0, k
    t = Tables(dev, [f])
    r, c = (int(v) for v in np.argwhere(one['inter'] == one['inter'].max())[0])
    conf, gsz, psz, inter = t.views()
    inter[r * t.npred + c] = 2 ** 32 - 3
    conf[0] = 2 ** 32 - 3
    got = t.add(f).host()
    assert got['inter'][r, c] == 2 ** 32 - 3 + one['inter'][r, c] > 2 ** 32 and got['conf'][0, 0] == 2 ** 32 - 3 + one['conf'][0, 0]
    got['inter'][r, c] -= 2 ** 32 - 3
    got['conf'][0, 0] -= 2 ** 32 - 3
    equal_tables(got, one)


def test_two_runs_and_a_side_stream_give_identical_tables(dev):
    videos = K.two_videos()
    ev = stq.StqEvaluator(K.CATS5, dev)
    _, first, _ = ev.count_video(videos[0])
    _, again, _ = ev.count_video(videos[0])
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        _, other, _ = ev.count_video(videos[0])
        side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first, again) and torch.equal(first, other) and int(first.sum()) > 0
    want = R.video_tables(videos[0], K.CATS5)
    assert np.array_equal(first.cpu().numpy(), np.concatenate([want[k].reshape(-1) for k in NAMES]))


# ---------------------------------------------------------------------------------------------- the evaluator and the tools
def _write_set(tmp, videos, cats):
    """the files tools/eval_vpq_device.py reads: (submit_dir, truth_dir, gt json file)"""
    from PIL import Image
    submit, truth = tmp / 'submit', tmp / 'truth'
    os.makedirs(submit / 'pan_pred'); os.makedirs(truth)
    images, gt_ann, pred_ann = [], [], []
    for v, frames in enumerate(videos):
        for t, f in enumerate(frames):
            iid = '%04d_%04d_city' % (v, t)
            images.append({'id': iid, 'file_name': iid + '_newImg8bit.png'})
            gt_ann.append(f[0]); pred_ann.append(f[1])
            Image.fromarray(f[2]).save(truth / (iid + '_final_mask.png'))
            Image.fromarray(f[3]).save(submit / 'pan_pred' / (iid + '.png'))
    json.dump({'annotations': pred_ann}, open(submit / 'pred.json', 'w'))
    gt_file = tmp / 'gt.json'
    json.dump({'annotations': gt_ann, 'images': images, 'categories': list(cats.values())}, open(gt_file, 'w'))
    return str(submit), str(truth), str(gt_file)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_whole_set_through_the_evaluator_and_the_tool(dev, tmp_path):
    videos = K.two_videos()
    want = R.evaluate(videos, K.CATS5)
    ev = stq.StqEvaluator(K.CATS5, dev)
    for frames in videos:
        ev.add_video(frames)
    got = ev.result()
    same_result(got, want)
    for st, frames in zip(ev.videos, videos):
        tab = R.video_tables(frames, K.CATS5)
        assert np.array_equal(st['conf'], tab['conf']) and np.array_equal(st['gt_size'], tab['gt_size'])
    assert 0.3 < got['aq'] < 0.9 and 0.5 < got['sq'] < 1.0
    # the same set from files, through the tool
    submit, truth, gt_file = _write_set(tmp_path, videos, K.CATS5)
    res = _tool('eval_stq_device').main(['--submit_dir', submit, '--truth_dir', truth, '--pan_gt_json_file', gt_file, '--nframes_per_video', '3',
                                         '--device', str(dev)])
    same_result(res, want)
    assert open(os.path.join(submit, 'stq.txt')).read() == R.stq_txt(want)
    tracks = json.load(open(os.path.join(submit, 'stq-tracks.json')))['tracks']
    assert [(t['video'], t['gt_id'], t['size'], t['n_pred'], t['best_pred_id']) for t in tracks] == \
        [(t['video'], t['gt_id'], t['size'], t['n_pred'], t['best_pred_id']) for t in want['tracks']]
    # a device map is taken as it is
    ev2 = stq.StqEvaluator(K.CATS5, dev)
    ev2.add_video([(f[0], f[1], torch.from_numpy(f[2]).to(dev), torch.from_numpy(f[3]).to(dev)) for f in videos[0]])
    assert ev2.result()['per_video'][0] == got['per_video'][0]


def test_a_self_scored_set_is_exactly_one(dev, tmp_path):
    videos = K.self_scored(K.two_videos())
    ev = stq.StqEvaluator(K.CATS5, dev)
    for frames in videos:
        ev.add_video(frames)
    got = ev.result()
    assert got['stq'] == 1.0 and got['aq'] == 1.0 and got['sq'] == 1.0 and [v['stq'] for v in got['per_video']] == [1.0, 1.0]
    submit, truth, gt_file = _write_set(tmp_path, videos, K.CATS5)
    res = _tool('eval_stq_device').main(['--submit_dir', submit, '--truth_dir', truth, '--pan_gt_json_file', gt_file, '--nframes_per_video', '3',
                                         '--device', str(dev)])
    assert res['stq'] == 1.0 and open(os.path.join(submit, 'stq.txt')).read().splitlines()[3].split()[2:5] == ['100.0', '100.0', '100.0']


def test_run_vps_synthetic_stq_scores_100_and_leaves_the_other_outputs_alone(dev, tmp_path):
    """tools/run_vps_synthetic.py --stq on its smallest clip (one video, the four labelled frames of 21): STQ 100 against itself, and
    pred.json and the PNGs are the bytes of a run without the option"""
    import filecmp
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_vps_synthetic as S
    common = ['--videos', '1', '--frames', '21', '--height', '128', '--width', '256']
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'stq')
    ra = S.main(common + ['--out', a])
    rb = S.main(common + ['--out', b, '--stq'])
    assert 'stq' not in ra and rb['stq']['stq'] == 100.0 and rb['stq']['aq'] == 100.0 and rb['stq']['sq'] == 100.0
    assert {k: v for k, v in rb.items() if k not in ('stq', 'seconds', 'frames_per_s_upload_prep_model_sequential')} == \
        {k: v for k, v in ra.items() if k not in ('seconds', 'frames_per_s_upload_prep_model_sequential')}
    for sub in ('pan_pred', 'pan_2ch'):
        fa = sorted(os.listdir(os.path.join(a, 'pred', sub)))
        assert len(fa) == 4 and fa == sorted(os.listdir(os.path.join(b, 'pred', sub)))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(a, 'pred', sub), os.path.join(b, 'pred', sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    assert sorted(set(os.listdir(os.path.join(b, 'pred'))) - set(os.listdir(os.path.join(a, 'pred')))) == ['stq-tracks.json', 'stq.txt']
    assert open(os.path.join(b, 'pred', 'stq.txt')).read().splitlines()[3].split()[2:5] == ['100.0', '100.0', '100.0']
