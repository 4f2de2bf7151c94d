"""GPU: the run list of a panoptic map (`vps_rle_runs`, csrc/rle_ops.hip) against `runs_of` of tests/rle_restate.py, and the track
tubes built on it (vps_amd/tubes.py: `rle_runs`, `segment_rles`, `TubeCollector`, `inference_panoptic_video(tubes=...)`) against
the NumPy restatement of the COCO mask API. Every comparison is exact equality."""
import json
import os

import numpy as np
import pytest
import torch

import rle_restate as R
from vps_amd import hip, tubes
from vps_amd import postprocess as pp

pytestmark = pytest.mark.gpu

B = tubes.BAND_ROWS
SIZES = [(1, 1), (7, 5), (64, 64), (37, 129), (200, 300), (B - 1, 70), (B, 70), (B + 1, 70), (2 * B + 1, 131)]
PATTERNS = ['single', 'alternate', 'wrap', 'vstripes', 'hstripes', 'blobs']


def blobs(H, W, nkeys, seed):
    """[H,W] indices 0 .. nkeys-1 in blocks of 5 x 3 with some single pixels"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, nkeys, size=((H + 4) // 5, (W + 2) // 3)).repeat(5, 0).repeat(3, 1)[:H, :W].copy()
    noise = rng.random((H, W)) < 0.02
    m[noise] = rng.integers(0, nkeys, size=int(noise.sum()))
    return m


def make_map(pattern, H, W, seed=0):
    """uint8 [H,W,3]; channels 1 and 2 carry different ids, so that the two id channels give different lists"""
    y, x = np.mgrid[0:H, 0:W]
    if pattern == 'single':
        idx = np.zeros((H, W), np.int64)
    elif pattern == 'alternate':                     # every position differs from the one before it in column-major order, also from
        idx = (x * H + y) & 1                        # the bottom of a column to the top of the next: a checkerboard when H is odd
    elif pattern == 'wrap':                          # one segment: the bottom rows of a column and the top rows of the next one
        idx = np.zeros((H, W), np.int64)
        if H >= 2 and W >= 2:
            c = W // 2 - 1
            idx[H - (H + 2) // 3:, c] = 5
            idx[:(H + 1) // 2, c + 1] = 5
    elif pattern == 'vstripes':
        idx = x // 3
    elif pattern == 'hstripes':
        idx = y // 3
    else:
        idx = blobs(H, W, 40, seed + H * 7 + W)
    rng = np.random.default_rng(seed + 99)
    cls = rng.permutation(200)[:64]                  # index -> class (never 255), pan_ins, pan_obj
    ins = rng.integers(0, 256, size=64)
    obj = rng.integers(0, 256, size=64)
    idx = idx % 64
    cls[5], ins[5], obj[5] = 17, 3, 9
    if pattern == 'alternate':
        ins[1], obj[1] = ins[0] + 1 & 255, obj[0] + 1 & 255
    return np.stack([cls[idx], ins[idx], obj[idx]], -1).astype(np.uint8)


def check_runs(dev, m, cap=None):
    t = torch.from_numpy(m).to(dev)
    H, W = m.shape[:2]
    for idc in (1, 2):
        want_start, want_key = R.runs_of(R.key_map(m, idc))
        rs, rk, n = tubes.rle_runs(t, idc, cap=cap)
        assert n == want_start.size, (idc, n, want_start.size)
        got_start, got_key = tubes.runs_to_host(rs, rk)
        assert got_start.shape == (n,) and np.array_equal(got_start, want_start), idc
        assert np.array_equal(got_key, want_key), idc
    return want_start.size


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('H,W', SIZES)
def test_runs_equal_the_restatement(dev, H, W, pattern):
    m = make_map(pattern, H, W)
    n = check_runs(dev, m, cap=H * W if pattern == 'alternate' else None)
    if pattern == 'alternate':
        assert n == H * W
    if pattern == 'single':
        assert n == 1


def test_runs_at_full_size(dev):
    """1024 x 2048: the scan runs over 2048 columns x 32 bands, four steps of its block"""
    m = make_map('blobs', 1024, 2048, seed=3)
    assert check_runs(dev, m) > 100000


def test_a_segment_across_two_columns_is_one_run(dev):
    H, W = 2 * B + 5, 9
    m = make_map('wrap', H, W)
    t = torch.from_numpy(m).to(dev)
    key = 17 * 256 + 9
    rs, rk, n = tubes.rle_runs(t, 2)
    start, keys = tubes.runs_to_host(rs, rk)
    assert n == 3 and keys.tolist()[1] == key and int((keys == key).sum()) == 1
    rles = tubes.segment_rles(t, 2)
    mask = tubes.rle_decode(rles[key])
    assert np.array_equal(mask, R.key_map(m, 2) == key)
    col = tubes.TubeCollector(things_only=False, device=dev)
    col.add(0, 'f', t)
    (tr,) = [tr for tr in col.result()['videos'][0]['tracks'] if tr['track_id'] == 17009]
    c = W // 2 - 1
    assert tr['bboxes'][0] == [c, 0, 2, H] == R.to_bbox(R.rle_encode(mask), H, W) and tr['areas'][0] == int(mask.sum())


def _raw_call(dev, t, idc, cap, guard=16):
    """vps_rle_runs on lists with `guard` canary entries behind the capacity"""
    H, W = int(t.shape[0]), int(t.shape[1])
    rs = torch.full((cap + guard,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
    rk = torch.full((cap + guard,), -0x5A5B, dtype=torch.int16, device=dev)
    n = torch.full((1,), -77, dtype=torch.int32, device=dev)
    ws = torch.empty(tubes.rle_runs_ws(H, W), dtype=torch.uint8, device=dev)
    st = hip.load().vps_rle_runs(hip.ptr(t), H, W, idc, hip.ptr(rs), hip.ptr(rk), cap, hip.ptr(n), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    torch.cuda.synchronize()
    return st, rs.cpu().numpy(), rk.cpu().numpy(), int(n.item())


def test_capacity_below_the_count(dev):
    m = make_map('blobs', 37, 129)
    t = torch.from_numpy(m).to(dev)
    want_start, want_key = R.runs_of(R.key_map(m, 2))
    true_n = want_start.size
    for cap in (true_n - 1, 0):
        st, rs, rk, n = _raw_call(dev, t, 2, cap)
        assert st == 0 and n == true_n, cap
        assert np.array_equal(rs[:cap].view(np.uint32), want_start[:cap]) and np.array_equal(rk[:cap].view(np.uint16), want_key[:cap]), cap
        assert (rs[cap:] == -0x5A5A5A5B).all() and (rk[cap:] == -0x5A5B).all(), cap       # nothing at or behind index cap
        a, b, k = tubes.rle_runs(t, 2, cap=cap)                                               # calls once more with the exact size
        a, b = tubes.runs_to_host(a, b)
        assert k == true_n and np.array_equal(a, want_start) and np.array_equal(b, want_key), cap


def test_argument_errors_launch_nothing(dev):
    m = make_map('blobs', 16, 24)
    t = torch.from_numpy(m).to(dev)
    lib = hip.load()
    rs = torch.full((64,), -5, dtype=torch.int32, device=dev)
    rk = torch.full((64,), -5, dtype=torch.int16, device=dev)
    n = torch.full((1,), -77, dtype=torch.int32, device=dev)
    ws = torch.full((tubes.rle_runs_ws(16, 24),), 0xA5, dtype=torch.uint8, device=dev)
    s = hip.stream_ptr()
    good = dict(pan=hip.ptr(t), H=16, W=24, idc=2, rs=hip.ptr(rs), rk=hip.ptr(rk), cap=64, n=hip.ptr(n), ws=hip.ptr(ws), wsb=ws.numel())
    for bad in (dict(pan=None), dict(rs=None), dict(rk=None), dict(n=None), dict(ws=None), dict(idc=0), dict(idc=3), dict(cap=-1),
                dict(H=1 << 16, W=1 << 15), dict(H=0), dict(W=-3), dict(wsb=ws.numel() - 1)):
        a = dict(good, **bad)
        st = lib.vps_rle_runs(a['pan'], a['H'], a['W'], a['idc'], a['rs'], a['rk'], a['cap'], a['n'], a['ws'], a['wsb'], s)
        assert st <= -1000, bad
    torch.cuda.synchronize()
    assert int(n.item()) == -77 and (rs == -5).all() and (rk == -5).all() and (ws == 0xA5).all()
    with pytest.raises(hip.VpsHipError):
        tubes.rle_runs(torch.from_numpy(m))                                                   # a host map: no CPU path
    assert lib.vps_rle_band_rows() == tubes.BAND_ROWS


def test_segment_rles_and_collector_statistics(dev):
    H, W = 61, 83
    m = make_map('blobs', H, W, seed=5)
    m[:4, :9] = 255                                                                          # void: class 255
    m[30:40, 50:52, 0] = 255
    t = torch.from_numpy(m).to(dev)
    for idc in (1, 2):
        km = R.key_map(m, idc)
        rles = tubes.segment_rles(t, idc)
        present = [int(k) for k in np.unique(km) if k >> 8 != 255]
        assert sorted(rles) == present and len(present) >= 30
        for k, rle in rles.items():
            assert rle['size'] == [H, W] and rle['counts'] == R.encode(km == k)['counts'].encode('ascii'), k
            assert np.array_equal(tubes.rle_decode(rle), km == k), k
        some = [present[3], 60000, present[0]]                                               # a subset, unsorted, with an absent key
        sub = tubes.segment_rles(t, idc, keys=some)
        assert sorted(sub) == sorted(some) and all(sub[k] == rles[k] for k in some if k in rles)
        assert tubes.rle_counts(sub[60000]) == [H * W]
        col = tubes.TubeCollector(things_only=False, id_channel=idc, device=dev)
        col.add('v', 'frame.png', t)
        v = col.result()['videos'][0]
        assert (v['video_id'], v['file_names'], v['height'], v['width']) == ('v', ['frame.png'], H, W)
        assert sorted(tr['track_id'] for tr in v['tracks']) == sorted(1000 * (k >> 8) + (k & 255) for k in present)
        for tr in v['tracks']:
            mask = tubes.rle_decode(tr['segmentations'][0])
            assert tr['areas'][0] == int(mask.sum()) and tr['bboxes'][0] == R.to_bbox(R.rle_encode(mask), H, W), tr['track_id']
            assert tr['category_id'] == tr['track_id'] // 1000


def test_two_frames_back_to_back_on_a_side_stream(dev):
    ma, mb = make_map('blobs', 200, 300, seed=1), make_map('blobs', 200, 300, seed=2)
    ta, tb = torch.from_numpy(ma).to(dev), torch.from_numpy(mb).to(dev)
    alone = [tubes.runs_to_host(*tubes.rle_runs(t, 2)[:2]) for t in (ta, tb)]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ra = tubes.rle_runs_async(ta, 2, cap=200 * 300)
        rb = tubes.rle_runs_async(tb, 2, cap=200 * 300)                                       # no synchronisation in between
    side.synchronize()
    for (rs, rk, n), (want_start, want_key), m in ((ra, alone[0], ma), (rb, alone[1], mb)):
        k = int(n.item())
        got_start, got_key = tubes.runs_to_host(rs[:k], rk[:k])
        assert np.array_equal(got_start, want_start) and np.array_equal(got_key, want_key)
        ref_start, ref_key = R.runs_of(R.key_map(m, 2))
        assert np.array_equal(got_start, ref_start) and np.array_equal(got_key, ref_key)


def _expected_tubes(frames, names, per_video, id_last_stuff):
    videos = []
    for v in range(len(frames) // per_video):
        fr = [R.key_map(f, 2) for f in frames[v * per_video:(v + 1) * per_video]]
        H, W = fr[0].shape
        keys = sorted(set(int(k) for km in fr for k in np.unique(km) if k >> 8 != 255 and k >> 8 > id_last_stuff),
                      key=lambda k: 1000 * (k >> 8) + (k & 255))
        tracks = []
        for k in keys:
            masks = [km == k for km in fr]
            tracks.append({'track_id': 1000 * (k >> 8) + (k & 255), 'category_id': k >> 8,
                           'segmentations': [R.encode(mk) if mk.any() else None for mk in masks],
                           'bboxes': [R.to_bbox(R.rle_encode(mk), H, W) if mk.any() else None for mk in masks],
                           'areas': [int(mk.sum()) if mk.any() else None for mk in masks]})
        videos.append({'video_id': v, 'file_names': names[v * per_video:(v + 1) * per_video], 'height': H, 'width': W, 'tracks': tracks})
    return {'videos': videos}


def test_inference_panoptic_video_with_a_collector(dev, tmp_path):
    """two synthetic videos x three sampled frames at 128 x 256: without a collector nothing changes, with one tubes.json is the
    restatement's"""
    from test_postprocess import _Colors, _pan2ch_clip
    H, W, nvid, nfr, per = 128, 256, 2, 15, 3
    rng = np.random.default_rng(11)
    frames = []
    for v in range(nvid):
        frames += _pan2ch_clip(rng, H, W, nfr)
    names = ['%04d_%04d_city_%06d_newImg8bit.png' % (v, f, f) for v in range(nvid) for f in range(nfr)]
    snames = names[4::5]
    dev_frames = [torch.from_numpy(f).to(dev) for f in frames]
    a, b = tmp_path / 'plain', tmp_path / 'tubes'
    pans_a, pj_a = pp.inference_panoptic_video(dev_frames, str(a), None, snames, n_video=nvid, color_generator=_Colors(), device=dev, nframes_per_video=per)
    col = tubes.TubeCollector(device=dev, id_last_stuff=10)
    pans_b, pj_b = pp.inference_panoptic_video(dev_frames, str(b), None, snames, n_video=nvid, color_generator=_Colors(), device=dev, nframes_per_video=per,
                                               tubes=col)
    assert not os.path.exists(a / 'tubes.json') and sorted(os.listdir(a)) == ['pan_2ch', 'pan_pred', 'pred.json']
    assert sorted(os.listdir(b)) == ['pan_2ch', 'pan_pred', 'pred.json', 'tubes.json']
    assert open(a / 'pred.json', 'rb').read() == open(b / 'pred.json', 'rb').read() and pj_a == pj_b
    assert all(np.array_equal(x, y) for x, y in zip(pans_a, pans_b)) and len(pans_b) == nvid * per
    for sub in ('pan_2ch', 'pan_pred'):
        assert sorted(os.listdir(a / sub)) == sorted(os.listdir(b / sub)) and len(os.listdir(b / sub)) == nvid * per
        for fn in os.listdir(a / sub):
            assert open(a / sub / fn, 'rb').read() == open(b / sub / fn, 'rb').read(), (sub, fn)
    got = json.load(open(b / 'tubes.json'))
    want = _expected_tubes(frames[4::5], snames, per, 10)
    assert got == want
    assert got == json.loads(json.dumps(col.result()))
    # the clip moves its object ids from frame to frame: some track is absent somewhere, and a track that is there twice is one track
    tracks = [tr for v in got['videos'] for tr in v['tracks']]
    assert any(None in tr['segmentations'] for tr in tracks)
    assert any(sum(s is not None for s in tr['segmentations']) >= 2 for tr in tracks)
    for v in got['videos']:
        ids = [tr['track_id'] for tr in v['tracks']]
        assert ids == sorted(set(ids))
        for tr in v['tracks']:
            assert [x is None for x in tr['segmentations']] == [x is None for x in tr['bboxes']] == [x is None for x in tr['areas']]
