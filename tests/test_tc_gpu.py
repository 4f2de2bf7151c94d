"""GPU: `vps_tc_accumulate` (csrc/tc_ops.hip) and `vps_amd.tc.TcEvaluator` against the per-pixel restatement (tests/tc_restate.py).
Device tables are compared with `array_equal`, results to 1e-12 relative (float64 means of a few dozen quotients of the same integers;
see tests/test_tc.py), and one run of tools/run_vps_synthetic.py --tc."""
import ctypes
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import tc_restate as R
from test_tc import close
from vps_amd import hip, tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

C6 = 6                                                       # classes 0..3 stuff, 4 and 5 things
SEG6 = np.full(256, 255, dtype=np.uint8)
SEG6[:6] = np.arange(6)
SEG6[6] = 2                                                  # two pan_seg values of one class
SEG6[200] = 77                                               # a class index >= C: void
TILE = 256 * 4                                               # pixels of cur per workgroup and step
SIZES = [(1, 1), (1, 5), (5, 1), (37, 53), (64, 96), (3, TILE + 1)]      # the last: one pixel wider, one row taller than whole tiles


def rand_map(rng, H, W, nrect=12):
    """random rectangles with void; keys 0 and 65535, unlisted things, seg values of a void class among them"""
    m = np.zeros((H, W, 3), dtype=np.uint8)
    m[..., 0] = rng.integers(0, 4)
    segs = [0, 1, 2, 3, 4, 4, 5, 5, 6, 200, 255]
    for _ in range(nrect):
        y0, x0 = rng.integers(0, H), rng.integers(0, W)
        y1, x1 = y0 + 1 + rng.integers(0, max(H // 2, 1)), x0 + 1 + rng.integers(0, max(W // 2, 1))
        s = segs[rng.integers(0, len(segs))]
        m[y0:y1, x0:x1] = (s, rng.integers(0, 4), rng.integers(0, 6) if s in (4, 5) else (255 if s == 255 else 0))
    return m


def keys_of(maps, idch, rng=None, extra=(0, 65535, 4 * 256 + 250)):
    """the keys present in `maps` (every second one when `rng` is given: listed and unlisted ones) and `extra`"""
    present = np.unique(np.concatenate([(m[..., 0].astype(np.int64) * 256 + m[..., idch]).reshape(-1) for m in maps]))
    if rng is not None:
        present = present[rng.random(len(present)) < 0.6]
    return np.unique(np.concatenate([present, np.asarray(extra, dtype=np.int64)])).astype(np.uint16)


def flows_for(rng, H, W):
    """name -> float32 [H,W,2]"""
    out = {'zero': np.zeros((H, W, 2), dtype=np.float32)}
    for name, (u, v) in dict(right1=(1, 0), left1=(-1, 0), down1=(0, 1), up1=(0, -1), far_right=(W + 3, 0), far_left=(-W - 3, 0), far_down=(0, H + 2),
                             far_up=(0, -H - 2)).items():
        f = np.zeros((H, W, 2), dtype=np.float32); f[..., 0], f[..., 1] = u, v
        out[name] = f
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    # sx exactly -0.5 (in view), the float below (not), W - 0.5 (not), the float below (W - 1): in column 0, where sx is the flow itself,
    # and the same for sy in row 0; +-k.5 elsewhere
    half = np.where(rng.random((H, W, 2)) < 0.5, 0.5, -0.5).astype(np.float32) + rng.integers(-2, 3, size=(H, W, 2)).astype(np.float32)
    edge = [np.float32(-0.5), np.nextafter(np.float32(-0.5), np.float32(-1)), np.float32(W - 0.5), np.nextafter(np.float32(W - 0.5), np.float32(0))]
    for y in range(H):
        half[y, 0, 0] = edge[y % 4]
    edge = [np.float32(-0.5), np.nextafter(np.float32(-0.5), np.float32(-1)), np.float32(H - 0.5), np.nextafter(np.float32(H - 0.5), np.float32(0))]
    for x in range(1, W):
        half[0, x, 1] = edge[x % 4]
    out['halves'] = half
    special = (rng.standard_normal((H, W, 2)) * 2).astype(np.float32)
    vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], dtype=np.float32)
    pick = rng.integers(0, 3 * len(vals), size=(H, W, 2))
    special = np.where(pick < len(vals), vals[pick % len(vals)], special).astype(np.float32)
    out['special'] = special
    out['smooth'] = np.stack([3.5 * np.sin(xs / 9 + 0.3) + 0.02 * ys, 2.5 * np.cos(ys / 7) - 0.03 * xs], axis=-1).astype(np.float32)
    out['noise'] = (rng.standard_normal((H, W, 2)) * max(H, W) / 3).astype(np.float32)
    return out


class Tables:
    """the keys on the device and one set of zeroed device tables for C classes"""

    def __init__(self, dev, keys, C=C6):
        self.dev, self.C, self.keys, self.n = dev, C, np.asarray(keys, dtype=np.uint16), len(keys)
        self.d_keys = torch.from_numpy(self.keys.view(np.int16)).to(dev) if self.n else None
        self.sizes = tc.table_sizes(C, self.n)
        self.buf = torch.zeros(sum(self.sizes), dtype=torch.int64, device=dev)
        self.keep = []

    def add_ptr(self, prev, cur, H, W, flow, ld=2, coff=0, idch=2, seg=SEG6, flick=None):
        conf, psz, csz, same, misc = torch.split(self.buf, self.sizes)
        n = self.n
        code = hip.load().vps_tc_accumulate(ctypes.c_void_p(prev), ctypes.c_void_p(cur), H, W, ctypes.c_void_p(flow), ld, coff, idch,
                                            seg.ctypes.data_as(ctypes.c_void_p), self.C, hip.ptr(self.d_keys) if n else None, n, hip.ptr(conf),
                                            hip.ptr(psz) if n else None, hip.ptr(csz) if n else None, hip.ptr(same) if n else None, hip.ptr(misc),
                                            None if flick is None else ctypes.c_void_p(flick), hip.stream_ptr())
        assert code == 0, code

    def add(self, prev, cur, flow, idch=2, seg=SEG6, flick=None):
        p, c, f = (torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in (prev, cur, flow))
        self.keep += [p, c, f]
        self.add_ptr(p.data_ptr(), c.data_ptr(), cur.shape[0], cur.shape[1], f.data_ptr(), idch=idch, seg=seg, flick=None if flick is None else flick.data_ptr())
        return self

    def host(self):
        conf, psz, csz, same, misc = (v.cpu().numpy() for v in torch.split(self.buf, self.sizes))
        return {'conf': conf.reshape(self.C + 1, self.C + 1), 'prev_size': psz, 'cur_size': csz, 'same': same, 'misc': misc}


def equal_tables(got, want, scale=1):
    for k in R.NAMES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], scale * want[k]), k


@pytest.mark.parametrize('H,W', SIZES)
def test_every_flow_kind_equals_the_restatement(dev, H, W):
    rng = np.random.default_rng(100 * H + W)
    for i, (name, flow) in enumerate(sorted(flows_for(rng, H, W).items())):
        prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
        if i % 3 == 0:
            cur = prev.copy()
        idch = 1 + i % 2
        keys = keys_of([prev, cur], idch, rng)
        want = R.pair_tables(prev, cur, flow, SEG6, C6, idch, keys)
        flick = torch.full((H * W + 64,), 0xAB, dtype=torch.uint8, device=dev)
        got = Tables(dev, keys).add(prev, cur, flow, idch=idch, flick=flick).host()
        equal_tables(got, want)
        assert int(got['misc'].sum()) == H * W, name
        f = flick.cpu().numpy()
        assert np.array_equal(f[:H * W].reshape(H, W), want['map']), name
        assert (f[H * W:] == 0xAB).all(), name                                   # intact behind its end
        equal_tables(Tables(dev, keys).add(prev, cur, flow, idch=idch).host(), want)        # the same without the map pointer


def test_uniform_and_checkerboard_maps(dev):
    H, W = 37, 53
    rng = np.random.default_rng(7)
    uni = np.zeros((H, W, 3), dtype=np.uint8); uni[:] = (4, 1, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    chk = np.zeros((H, W, 3), dtype=np.uint8)
    chk[..., 0] = np.where((yy + xx) % 2 == 0, 4, 5); chk[..., 1] = 1; chk[..., 2] = np.where((yy + xx) % 2 == 0, 1, 2)
    fl = flows_for(rng, H, W)
    for prev, cur, flow in ((uni, uni, fl['zero']), (uni, uni, fl['smooth']), (chk, chk, fl['zero']), (chk, chk, fl['right1']), (uni, chk, fl['noise'])):
        keys = keys_of([prev, cur], 2)
        equal_tables(Tables(dev, keys).add(prev, cur, flow).host(), R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys))
    both = Tables(dev, keys_of([chk], 2)).add(chk, chk, fl['right1']).host()
    assert both['same'].sum() == 0 and both['conf'][4][5] + both['conf'][5][4] == H * (W - 1)       # every in-view pixel lands on the other colour


def test_the_padded_nhwc_layout_and_the_unaligned_flow(dev):
    H, W = 37, 53
    rng = np.random.default_rng(11)
    prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
    flow = flows_for(rng, H, W)['smooth']
    keys = keys_of([prev, cur], 2, rng)
    want = R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys)
    p, c = (torch.from_numpy(a).to(dev) for a in (prev, cur))
    for ld, coff, off in ((4, 2, 0), (4, 1, 0), (5, 3, 0), (2, 0, 1), (8, 6, 0), (3, 0, 0)):       # 8-byte pairs, 4-byte loads, a dense map off 16 bytes
        wide = torch.full((H * W * ld + 8,), float('nan'), dtype=torch.float32, device=dev)
        body = wide[off:off + H * W * ld].view(H * W, ld)
        body[:, coff:coff + 2] = torch.from_numpy(flow.reshape(-1, 2)).to(dev)
        t = Tables(dev, keys)
        t.add_ptr(p.data_ptr(), c.data_ptr(), H, W, wide.data_ptr() + 4 * off, ld=ld, coff=coff)
        equal_tables(t.host(), want)


def test_maps_off_a_dword_boundary_between_canaries(dev):
    H, W = 5, 13
    rng = np.random.default_rng(13)
    prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
    flow = flows_for(rng, H, W)['noise'] / 4
    keys = keys_of([prev, cur], 2, extra=(4 * 256 + 1,))
    want = R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys)
    f = torch.from_numpy(flow).to(dev)
    for op in range(4):
        for oc in range(4):
            bufs = []
            for o, m in ((op, prev), (oc, cur)):
                b = torch.zeros(64 + 3 * H * W + 64, dtype=torch.uint8, device=dev)
                b.view(-1)[:] = torch.tensor([4, 1, 1], dtype=torch.uint8, device=dev).repeat((len(b) + 2) // 3)[:len(b)]      # a listed key all round
                b[32 + o:32 + o + 3 * H * W] = torch.from_numpy(m.reshape(-1)).to(dev)
                assert (b.data_ptr() + 32) % 4 == 0
                bufs.append(b)
            t = Tables(dev, keys)
            t.add_ptr(bufs[0].data_ptr() + 32 + op, bufs[1].data_ptr() + 32 + oc, H, W, f.data_ptr())
            equal_tables(t.host(), want)
    flick = torch.full((H * W + 9,), 0xAB, dtype=torch.uint8, device=dev)         # the map itself off a dword boundary
    t = Tables(dev, keys)
    p, c = (torch.from_numpy(a).to(dev) for a in (prev, cur))
    t.add_ptr(p.data_ptr(), c.data_ptr(), H, W, f.data_ptr(), flick=flick.data_ptr() + 1)
    got = flick.cpu().numpy()
    assert got[0] == 0xAB and (got[1 + H * W:] == 0xAB).all() and np.array_equal(got[1:1 + H * W].reshape(H, W), want['map'])


def test_both_table_paths_give_the_same_tables_at_the_bound(dev):
    bound = hip.load().vps_stq_lds_cells()
    n_at = (bound - (C6 + 1) ** 2 - 2) // 3
    assert (C6 + 1) ** 2 + 3 * n_at + 2 == bound                                 # 49 + 3 * 4079 + 2 = 12288: exactly at the bound
    H, W = 64, 96
    rng = np.random.default_rng(17)
    prev, cur = rand_map(rng, H, W, 40), rand_map(rng, H, W, 40)
    flow = flows_for(rng, H, W)['smooth']
    present = keys_of([prev, cur], 2)
    filler = np.setdiff1d(np.arange(65536), present)
    seen = []
    for n in (n_at, n_at + 1, 3):
        keys = np.sort(np.concatenate([present, rng.choice(filler, n - len(present), replace=False)])).astype(np.uint16) if n > 3 else present[:3]
        assert len(keys) == n and (sum(tc.table_sizes(C6, n)) <= bound) == (n <= n_at)
        want = R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys)
        got = Tables(dev, keys).add(prev, cur, flow).host()
        equal_tables(got, want)
        by_key = {('c',) + rc: int(v) for rc, v in np.ndenumerate(got['conf']) if v}
        for name in ('prev_size', 'cur_size', 'same'):
            by_key.update({(name, int(keys[i])): int(v) for i, v in enumerate(got[name]) if v})
        seen.append(by_key)
    assert seen[0] == seen[1] and len(seen[0]) > 20                               # LDS image and global atomics: the same cells


def test_the_same_pair_twice_doubles_the_tables(dev):
    H, W = 37, 53
    rng = np.random.default_rng(19)
    prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
    flow = flows_for(rng, H, W)['smooth']
    keys = keys_of([prev, cur], 2)
    want = R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys)
    equal_tables(Tables(dev, keys).add(prev, cur, flow).add(prev, cur, flow).host(), want, scale=2)


def test_a_call_on_a_side_stream_is_ordered_after_the_upload_on_it(dev):
    H, W = 64, 96
    rng = np.random.default_rng(23)
    prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
    flow = flows_for(rng, H, W)['smooth']
    keys = keys_of([prev, cur], 2)
    want = R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys)
    t = Tables(dev, keys)
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (prev, cur, flow)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        p, c, f = (a.to(dev, non_blocking=True) for a in pinned)
        t.add_ptr(p.data_ptr(), c.data_ptr(), H, W, f.data_ptr())
    side.synchronize()
    equal_tables(t.host(), want)


def test_the_evaluator_per_pair_slices_sum_to_the_video_and_match_the_restatement(dev):
    H, W = 37, 53
    rng = np.random.default_rng(29)
    maps = [rand_map(rng, H, W)]
    for _ in range(3):
        m = maps[-1].copy()
        m[rng.integers(0, H - 8):, rng.integers(0, W - 8):] = rand_map(rng, H, W)[:1, :1]
        maps.append(np.roll(m, (1, 2), axis=(0, 1)))
    fl = flows_for(rng, H, W)
    flows = [None, fl['smooth'], (fl['smooth'] * 0 + np.float32([-2, -1])).astype(np.float32), fl['noise'] / 8]
    ev = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3)
    keys = ev.video_keys(maps)
    present = keys_of(maps, 2, extra=())
    assert keys.tolist() == [int(k) for k in present if 3 < (k >> 8) != 255]                # the thing keys: classes above id_last_stuff
    total, pairs = R.video_tables(maps, flows, SEG6, C6, 2, keys)
    # host arrays, device tensors and a flow that is a view of a wider NHWC map
    wide = torch.zeros(H, W, 4, dtype=torch.float32, device=dev)
    wide[..., 2:] = torch.from_numpy(flows[2]).to(dev)
    st = ev.add_video([maps[0], torch.from_numpy(maps[1]).to(dev), maps[2], maps[3]], [None, flows[1], wide[..., 2:], torch.from_numpy(flows[3]).to(dev)], 'clip')
    equal_tables({k: st[k] for k in R.NAMES[:4]} | {'misc': np.array([st['in_view'], st['outside']])}, total)
    assert len(st['pairs']) == 3
    for got, want in zip(st['pairs'], pairs):
        w = R.terms(want)
        assert all(close(got[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track')) and got['in_view'] == w['in_view'] and got['outside'] == w['outside']
    plain = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, id_last_stuff=3)
    st2 = plain.add_video(maps, flows, 'clip')
    equal_tables({k: st2[k] for k in R.NAMES[:4]} | {'misc': np.array([st2['in_view'], st2['outside']])}, total)
    w = R.terms(total)
    res = ev.result()
    assert all(close(res[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track')) and res['n_tracks'] == w['n_tracks'] and 0 < res['tc'] < 1
    assert [r['pair'] for r in res['per_pair']] == [1, 2, 3] and plain.result()['per_pair'] == []
    assert close(plain.result()['tc'], res['tc'])
    with pytest.raises(ValueError):
        ev.add_pair(maps[0], maps[1], flows[1][:, :-1])
    with pytest.raises(ValueError):
        ev.add_pair(maps[0][:-1], maps[1], flows[1])
    assert ev._open is None


def test_run_vps_synthetic_tc_equals_the_restatement_and_leaves_the_other_outputs_alone(dev, tmp_path, monkeypatch):
    """tools/run_vps_synthetic.py --tc on its smallest clip (one video of 21 frames, 20 pairs): tc.txt and tc-tracks.json hold the tables
    of the restatement run on the maps and flows downloaded as the tool hands them to the evaluator; pred.json and the PNGs are the bytes
    of a run without the option"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_vps_synthetic as S
    seen = []
    inner = tc.TcEvaluator.add_pair

    def recording(self, prev, cur, flow, keys=None, flicker=None):
        seen.append((prev.cpu().numpy(), cur.cpu().numpy(), flow.cpu().numpy(), np.asarray(keys).copy(), self.seg_class.copy(), self.num_classes))
        return inner(self, prev, cur, flow, keys=keys, flicker=flicker)
    monkeypatch.setattr(tc.TcEvaluator, 'add_pair', recording)
    common = ['--videos', '1', '--frames', '21', '--height', '128', '--width', '256']
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'tc')
    ra = S.main(common + ['--out', a])
    assert not seen
    rb = S.main(common + ['--out', b, '--tc', '--tc-map', os.path.join(b, 'tcmap')])
    assert 'tc' not in ra and rb['tc']['pairs'] == 20 == len(seen) and rb['tc']['map_files'] == 20
    assert {k: v for k, v in rb.items() if k not in ('tc', 'seconds', 'frames_per_s_upload_prep_model_sequential')} == \
        {k: v for k, v in ra.items() if k not in ('seconds', 'frames_per_s_upload_prep_model_sequential')}
    for sub in ('pan_pred', 'pan_2ch'):
        fa = sorted(os.listdir(os.path.join(a, 'pred', sub)))
        assert len(fa) == 4 and fa == sorted(os.listdir(os.path.join(b, 'pred', sub)))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(a, 'pred', sub), os.path.join(b, 'pred', sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    assert not os.path.exists(os.path.join(a, 'pred', 'tc.txt'))
    from PIL import Image
    jpgs = sorted(os.listdir(os.path.join(b, 'tcmap')))
    assert len(jpgs) == 20
    with Image.open(os.path.join(b, 'tcmap', jpgs[0])) as im:
        assert im.size == (256, 128)
    # ---- the tables behind the files
    keys, seg, C = seen[0][3], seen[0][4], seen[0][5]
    assert C == 19 and all(np.array_equal(s[3], keys) for s in seen)
    pairs = [R.pair_tables(p, c, f, seg, C, 2, keys) for p, c, f, _, _, _ in seen]
    total = {k: sum(p[k] for p in pairs) for k in R.NAMES}
    w = R.terms(total)
    doc = json.load(open(os.path.join(b, 'pred', 'tc-tracks.json')))
    assert np.array_equal(np.array(doc['conf']), total['conf']) and doc['in_view'] == w['in_view'] and doc['outside'] == w['outside']
    listed = {int(k): i for i, k in enumerate(keys)}
    assert len(doc['tracks']) == w['n_tracks']
    for r in doc['tracks']:
        i = listed[r['key']]
        assert (r['same'], r['prev_size'], r['cur_size']) == (int(total['same'][i]), int(total['prev_size'][i]), int(total['cur_size'][i]))
    assert all(close(doc[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track'))
    assert len(doc['per_pair']) == 20 and all(close(r['tc'], R.terms(p)['tc']) for r, p in zip(doc['per_pair'], pairs))
    text = open(os.path.join(b, 'pred', 'tc.txt')).read()
    row = text.splitlines()[3].split()
    assert row[0] == 'All' and row[2:6] == ['%.1f' % (100 * w['tc']), '%.1f' % (100 * w['tc_sem']), '%.1f' % (100 * w['tc_track']), '%d' % w['n_tracks']]
    assert rb['tc']['tc'] == round(100 * doc['tc'], 4) and rb['tc']['tracks'] == w['n_tracks']
