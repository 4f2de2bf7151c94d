"""GPU: `vps_flow_occlusion` (csrc/flow_occ_ops.hip), `vps_tc_accumulate_masked` (csrc/tc_ops.hip) and the occlusion option of
`vps_amd.tc.TcEvaluator` against the per-pixel restatements (tests/flow_occ_restate.py, tests/tc_restate.py): every pixel of every mask
and every cell of every table with `array_equal`, results to 1e-12 relative (see tests/test_tc.py), and one run of
tools/run_vps_synthetic.py --tc --tc-occlusion."""
import ctypes
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import flow_occ_restate as O
import tc_restate as R
from test_tc import close
from test_tc_gpu import C6, SEG6, SIZES, Tables, equal_tables, flows_for, keys_of, rand_map
from vps_amd import hip, tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NAN_BITS = 0x7fc00abc                                        # the canary word: a NaN as a float, so a read of it shows in the mask too


def pairs_for(rng, H, W):
    """name -> (fwd, back), float32 [H,W,2]: the flow kinds of tests/test_tc_gpu.py in either place, exact and near inverses"""
    f = flows_for(rng, H, W)
    sub = np.zeros((H, W, 2), dtype=np.float32); sub[..., 0], sub[..., 1] = 0.3125, -0.625       # bilinear weights other than 0 and 1
    wobble = (rng.standard_normal((H, W, 2)) * 0.3).astype(np.float32)
    return {'zero': (f['zero'], f['zero']), 'right1': (f['right1'], f['left1']), 'left1': (f['left1'], f['right1']), 'down1': (f['down1'], f['up1']),
            'up1_zero': (f['up1'], f['zero']), 'far_right': (f['far_right'], f['far_left']), 'far_up': (f['far_up'], f['far_down']),
            'halves': (f['halves'], f['smooth']), 'halves_back': (f['smooth'], f['halves']), 'special': (f['special'], f['noise']),
            'special_back': (f['smooth'], f['special']), 'special_both': (f['special'], f['special'][::-1, ::-1].copy()),
            'smooth': (f['smooth'], (-f['smooth'] + wobble).astype(np.float32)), 'noise': (f['noise'], (f['noise'][:, ::-1] / 3).copy()),
            'subpixel': (sub, -sub), 'subpixel_wobble': (sub, (-sub + wobble).astype(np.float32))}


def canaried(dev, nbytes, lead):
    """a device buffer of `lead` + nbytes + 64 bytes filled with the canary word -> (buffer as int32, address of the payload)"""
    words = (lead + nbytes + 64 + 3) // 4 + 1
    buf = torch.full((words,), NAN_BITS, dtype=torch.int32, device=dev)
    return buf, buf.data_ptr() + lead


def put(buf, at, arr):
    """copy the bytes of a NumPy array to byte offset `at` of an int32 device buffer"""
    raw = torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()).to(buf.device)
    buf.view(torch.uint8)[at:at + raw.numel()] = raw


def strided(flow, ld, coff):
    """the flow laid out with `ld` floats per pixel, the two channels at `coff`, NaN in the pad channels"""
    H, W = flow.shape[:2]
    wide = np.full((H * W, ld), np.nan, dtype=np.float32)
    wide[:, coff:coff + 2] = flow.reshape(-1, 2)
    return wide


def run_occ(dev, fwd, back, flay=(2, 0, 0), blay=(2, 0, 0), occ_off=0, want_occ=True, want_counts=True, alpha=0.01, beta=0.5, repeat=1):
    """one `vps_flow_occlusion` call with the flows at (ld, coff, base offset in floats) between canaries -> (codes or None, counts or
    None); asserts that nothing around back, occ and counts has changed"""
    H, W = fwd.shape[:2]
    bufs = []
    for flow, (ld, coff, off) in ((fwd, flay), (back, blay)):
        body = strided(flow, ld, coff)
        buf, addr = canaried(dev, body.nbytes, 64 + 4 * off)
        put(buf, 64 + 4 * off, body)
        bufs.append((buf, addr, buf.clone()))
    obuf, oaddr = canaried(dev, H * W, 64 + occ_off)
    cbuf, caddr = canaried(dev, 24, 64)
    put(cbuf, 64, np.zeros(3, dtype=np.int64))
    csnap = cbuf.clone()
    for _ in range(repeat):
        code = hip.load().vps_flow_occlusion(ctypes.c_void_p(bufs[0][1]), flay[0], flay[1], ctypes.c_void_p(bufs[1][1]), blay[0], blay[1], H, W, alpha, beta,
                                             ctypes.c_void_p(oaddr) if want_occ else None, ctypes.c_void_p(caddr) if want_counts else None, hip.stream_ptr())
        assert code == 0, code
    torch.cuda.synchronize()
    for buf, _, snap in bufs:
        assert torch.equal(buf, snap)                                            # the flows and what lies round them
    o = obuf.view(torch.uint8).cpu().numpy()
    lo, hi = 64 + occ_off, 64 + occ_off + H * W
    canary = np.frombuffer(np.full(len(o) // 4, NAN_BITS, dtype=np.int32).tobytes(), dtype=np.uint8)
    assert np.array_equal(o[:lo], canary[:lo]) and np.array_equal(o[hi:], canary[hi:])
    if not want_occ:
        assert np.array_equal(o, canary)
    c = cbuf.cpu().numpy()
    s = csnap.cpu().numpy()
    assert np.array_equal(c[:16], s[:16]) and np.array_equal(c[22:], s[22:])
    if not want_counts:
        assert np.array_equal(c, s)
    return (o[lo:hi].reshape(H, W).copy() if want_occ else None), (c[16:22].view(np.int64).copy() if want_counts else None)


@pytest.mark.parametrize('H,W', SIZES)
def test_mask_and_counts_equal_the_restatement_for_every_flow_kind(dev, H, W):
    rng = np.random.default_rng(300 * H + W)
    for name, (fwd, back) in sorted(pairs_for(rng, H, W).items()):
        assert not ((np.abs(fwd) < np.finfo(np.float32).tiny) & (fwd != 0)).any() and not ((np.abs(back) < np.finfo(np.float32).tiny) & (back != 0)).any()
        want, wcounts = O.occlusion(fwd, back)
        got, counts = run_occ(dev, fwd, back)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(counts, wcounts) and int(counts.sum()) == H * W, name


def test_other_thresholds(dev):
    H, W = 37, 53
    rng = np.random.default_rng(31)
    fwd, back = pairs_for(rng, H, W)['smooth']
    seen = set()
    for alpha, beta in ((0.0, 0.0), (0.0, 0.5), (0.3, 0.0), (0.05, 2.0)):
        want, wcounts = O.occlusion(fwd, back, alpha, beta)
        got, counts = run_occ(dev, fwd, back, alpha=alpha, beta=beta)
        assert np.array_equal(got, want) and np.array_equal(counts, wcounts)
        seen.add(tuple(wcounts.tolist()))
    assert len(seen) == 4                                                        # the thresholds decide differently on this pair


def test_layouts_of_either_flow_and_an_odd_mask_address(dev):
    H, W = 37, 53
    rng = np.random.default_rng(37)
    sub, back = pairs_for(rng, H, W)['subpixel_wobble']
    fwd = (sub - 0.8 * flows_for(rng, H, W)['smooth']).astype(np.float32)      # leaves the view along the top, sub-pixel everywhere
    back = (back + (sub - fwd)).astype(np.float32)                               # its negative where it stands, plus the wobble
    want, wcounts = O.occlusion(fwd, back)                                       # one reference for every layout
    assert (want == 0).any() and (want == 1).any() and (want == 2).any()
    dense, pad4, pad5 = (2, 0, 0), (4, 0, 0), (5, 3, 0)
    for flay, blay, occ_off in ((pad4, pad4, 0), (pad5, pad5, 0), (pad4, pad5, 0), (pad5, pad4, 0), (dense, pad4, 0), (pad4, dense, 0),
                                (dense, (2, 0, 1), 0), ((2, 0, 1), dense, 0), ((2, 0, 2), (4, 2, 1), 0), ((4, 2, 0), (3, 1, 0), 0),
                                (dense, dense, 1), (pad4, pad5, 3), (dense, (2, 0, 1), 2)):
        got, counts = run_occ(dev, fwd, back, flay, blay, occ_off)
        assert np.array_equal(got, want) and np.array_equal(counts, wcounts), (flay, blay, occ_off)


def test_special_flows_between_canaries_read_and_write_nothing_outside(dev):
    """the test of the clamp: NaN, inf and 1e30 in either flow, the maps between NaN canaries (a corner read outside `back` would turn
    a visible pixel into an occluded one, a store outside `occ` or `counts` would change a canary), at sizes with partial chunks"""
    for H, W in ((5, 13), (37, 53), (3, 1025)):
        rng = np.random.default_rng(41 * H + W)
        p = pairs_for(rng, H, W)
        edge = flows_for(rng, H, W)['halves']
        for name, (fwd, back) in (('special', p['special']), ('special_back', p['special_back']), ('special_both', p['special_both']),
                                  ('edges', (edge, (-edge).astype(np.float32)))):
            want, wcounts = O.occlusion(fwd, back)
            for flay, blay, occ_off in (((2, 0, 0), (2, 0, 0), 0), ((4, 0, 0), (5, 3, 1), 1)):
                got, counts = run_occ(dev, fwd, back, flay, blay, occ_off)
                assert np.array_equal(got, want) and np.array_equal(counts, wcounts), (H, W, name, flay)


def test_calling_twice_doubles_the_counts_and_either_output_alone_gives_the_same(dev):
    H, W = 37, 53
    rng = np.random.default_rng(43)
    fwd, back = pairs_for(rng, H, W)['smooth']
    want, wcounts = O.occlusion(fwd, back)
    got, counts = run_occ(dev, fwd, back, repeat=2)
    assert np.array_equal(got, want) and np.array_equal(counts, 2 * wcounts)
    got, none = run_occ(dev, fwd, back, want_counts=False)
    assert none is None and np.array_equal(got, want)
    none, counts = run_occ(dev, fwd, back, want_occ=False)
    assert none is None and np.array_equal(counts, wcounts)


def test_the_python_entry_takes_views_of_wider_maps_and_adds_to_counts(dev):
    H, W = 37, 53
    rng = np.random.default_rng(47)
    fwd, back = pairs_for(rng, H, W)['smooth']
    want, wcounts = O.occlusion(fwd, back)
    wide = torch.zeros(H, W, 4, dtype=torch.float32, device=dev)                 # FlowNet2's padded layout
    wide[..., :2] = torch.from_numpy(back).to(dev)
    counts = torch.tensor([5, 6, 7], dtype=torch.int64, device=dev)
    out = torch.full((H, W), 9, dtype=torch.uint8, device=dev)
    got = tc.flow_occlusion(torch.from_numpy(fwd).to(dev), wide[..., :2], out=out, counts=counts)
    assert got is out and np.array_equal(got.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), wcounts + [5, 6, 7])
    assert np.array_equal(tc.flow_occlusion(torch.from_numpy(fwd).to(dev), torch.from_numpy(back).to(dev), alpha=0.3, beta=0.0).cpu().numpy(),
                          O.occlusion(fwd, back, 0.3, 0.0)[0])
    with pytest.raises(ValueError):
        tc.flow_occlusion(torch.from_numpy(fwd).to(dev), torch.from_numpy(back[:-1]).to(dev))


# ---------------------------------------------------------------------------------------------- the masked counting
class MaskedTables(Tables):
    """tests/test_tc_gpu.py's tables with the masked cell behind them"""

    def __init__(self, dev, keys, C=C6):
        super().__init__(dev, keys, C)
        self.sizes = tc.table_sizes(C, self.n, occlusion=True)
        self.buf = torch.zeros(sum(self.sizes), dtype=torch.int64, device=dev)

    def add_masked(self, prev, cur, flow, mask, idch=2, flick=None, mask_ptr=None):
        p, c, f = (torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in (prev, cur, flow))
        m = torch.from_numpy(np.ascontiguousarray(mask)).to(self.dev)
        self.keep += [p, c, f, m]
        conf, psz, csz, same, misc, masked = torch.split(self.buf, self.sizes)
        n = self.n
        code = hip.load().vps_tc_accumulate_masked(hip.ptr(p), hip.ptr(c), cur.shape[0], cur.shape[1], hip.ptr(f), 2, 0, idch, SEG6.ctypes.data_as(ctypes.c_void_p),
                                                   self.C, hip.ptr(self.d_keys) if n else None, n, hip.ptr(conf), hip.ptr(psz) if n else None,
                                                   hip.ptr(csz) if n else None, hip.ptr(same) if n else None, hip.ptr(misc),
                                                   None if flick is None else hip.ptr(flick), ctypes.c_void_p(mask_ptr) if mask_ptr else hip.ptr(m),
                                                   hip.ptr(masked), hip.stream_ptr())
        assert code == 0, code
        return self

    def host(self):
        parts = [v.cpu().numpy() for v in torch.split(self.buf, self.sizes)]
        out = dict(zip(O.NAMES, parts))
        out['conf'] = out['conf'].reshape(self.C + 1, self.C + 1)
        return out


def equal_masked(got, want, scale=1):
    for k in O.NAMES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], scale * np.asarray(want[k])), k


def rand_mask(rng, H, W):
    """a third of the pixels masked, with the byte values 1, 2 and 255, in runs and alone"""
    m = np.where(rng.random((H, W)) < 0.2, rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=(H, W)), 0).astype(np.uint8)
    for _ in range(4):
        y, x = rng.integers(0, H), rng.integers(0, W)
        m[y:y + 1 + H // 4, x:x + 1 + W // 3] = 1
    return m


@pytest.mark.parametrize('H,W', SIZES)
def test_the_masked_tables_and_the_map_equal_the_restatement(dev, H, W):
    rng = np.random.default_rng(500 * H + W)
    fl = flows_for(rng, H, W)
    for i, name in enumerate(('zero', 'smooth', 'halves', 'special', 'noise', 'right1')):
        prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
        if i % 2 == 0:
            cur = prev.copy()                                                    # long runs of equal pairs, cut by the mask
        idch = 1 + i % 2
        keys = keys_of([prev, cur], idch, rng)
        mask = rand_mask(rng, H, W)
        want = O.masked_pair_tables(prev, cur, fl[name], mask, SEG6, C6, idch, keys)
        flick = torch.full((H * W + 64,), 0xAB, dtype=torch.uint8, device=dev)
        got = MaskedTables(dev, keys).add_masked(prev, cur, fl[name], mask, idch=idch, flick=flick).host()
        equal_masked(got, want)
        assert int(got['misc'].sum() + got['masked'][0]) == H * W, name
        f = flick.cpu().numpy()
        assert np.array_equal(f[:H * W].reshape(H, W), want['map']) and (f[H * W:] == 0xAB).all(), name
        inview = R.warp(fl[name])[0]
        assert np.array_equal(want['map'] == 4, inview & (mask != 0))           # code 4 exactly at the masked in-view pixels
        equal_masked(MaskedTables(dev, keys).add_masked(prev, cur, fl[name], mask, idch=idch).host(), want)      # the same without the map pointer


def test_both_table_paths_of_the_masked_entry_at_the_bound(dev):
    bound = hip.load().vps_stq_lds_cells()
    n_at = (bound - (C6 + 1) ** 2 - 3) // 3                                      # 49 + 3 * 4078 + 3 = 12286 <= 12288 < 12289
    assert sum(tc.table_sizes(C6, n_at, occlusion=True)) <= bound < sum(tc.table_sizes(C6, n_at + 1, occlusion=True))
    H, W = 64, 96
    rng = np.random.default_rng(53)
    prev, cur = rand_map(rng, H, W, 40), rand_map(rng, H, W, 40)
    flow = flows_for(rng, H, W)['smooth']
    mask = rand_mask(rng, H, W)
    present = keys_of([prev, cur], 2)
    filler = np.setdiff1d(np.arange(65536), present)
    seen = []
    for n in (n_at, n_at + 1):
        keys = np.sort(np.concatenate([present, rng.choice(filler, n - len(present), replace=False)])).astype(np.uint16)
        got = MaskedTables(dev, keys).add_masked(prev, cur, flow, mask).host()
        equal_masked(got, O.masked_pair_tables(prev, cur, flow, mask, SEG6, C6, 2, keys))
        by_key = {('c',) + rc: int(v) for rc, v in np.ndenumerate(got['conf']) if v}
        for name in ('prev_size', 'cur_size', 'same'):
            by_key.update({(name, int(keys[i])): int(v) for i, v in enumerate(got[name]) if v})
        by_key.update(misc=got['misc'].tolist(), masked=got['masked'].tolist())
        seen.append(by_key)
    assert seen[0] == seen[1] and len(seen[0]) > 20 and seen[0]['masked'][0] > 0  # LDS image and global atomics: the same cells


def test_all_zero_and_all_ones_masks_and_an_odd_mask_address(dev):
    H, W = 37, 53
    rng = np.random.default_rng(59)
    prev, cur = rand_map(rng, H, W), rand_map(rng, H, W)
    flow = flows_for(rng, H, W)['smooth']
    keys = keys_of([prev, cur], 2, rng)
    plain = Tables(dev, keys).add(prev, cur, flow).host()
    equal_tables(plain, R.pair_tables(prev, cur, flow, SEG6, C6, 2, keys))
    zero = MaskedTables(dev, keys).add_masked(prev, cur, flow, np.zeros((H, W), dtype=np.uint8)).host()
    equal_tables(zero, plain)                                                    # the tables of vps_tc_accumulate
    assert zero['masked'].tolist() == [0]
    ones = MaskedTables(dev, keys).add_masked(prev, cur, flow, np.ones((H, W), dtype=np.uint8)).host()
    assert not ones['conf'].any() and not ones['prev_size'].any() and not ones['cur_size'].any() and not ones['same'].any()
    assert ones['misc'].tolist() == [0, int(plain['misc'][1])] and ones['masked'].tolist() == [int(plain['misc'][0])]
    twice = MaskedTables(dev, keys)
    mask = rand_mask(rng, H, W)
    want = O.masked_pair_tables(prev, cur, flow, mask, SEG6, C6, 2, keys)
    equal_masked(twice.add_masked(prev, cur, flow, mask).add_masked(prev, cur, flow, mask).host(), want, scale=2)
    for off in (1, 2, 3):                                                        # the mask off a dword boundary, canaries of 7 round it
        buf = torch.full((64 + H * W + 64,), 7, dtype=torch.uint8, device=dev)
        buf[32 + off:32 + off + H * W] = torch.from_numpy(mask.reshape(-1)).to(dev)
        assert (buf.data_ptr() + 32) % 4 == 0
        t = MaskedTables(dev, keys)
        t.keep.append(buf)
        equal_masked(t.add_masked(prev, cur, flow, mask, mask_ptr=buf.data_ptr() + 32 + off).host(), want)


# ---------------------------------------------------------------------------------------------- the evaluator and the tool
RESULT_KEYS = {'tc', 'tc_sem', 'tc_track', 'n_classes', 'n_tracks', 'in_view', 'outside', 'in_view_share', 'conf', 'per_class', 'per_video', 'tracks',
               'per_pair'}                                                       # today's result object


def test_the_evaluator_with_occlusion_per_pair_slices_sum_to_the_video_and_match_the_restatement(dev):
    H, W = 37, 53
    rng = np.random.default_rng(61)
    maps = [rand_map(rng, H, W)]
    for _ in range(3):
        m = maps[-1].copy()
        m[rng.integers(0, H - 8):, rng.integers(0, W - 8):] = rand_map(rng, H, W)[:1, :1]
        maps.append(np.roll(m, (1, 2), axis=(0, 1)))
    p = pairs_for(rng, H, W)
    flows = [None, p['smooth'][0], p['subpixel_wobble'][0], p['special_back'][0]]
    backs = [None, p['smooth'][1], p['subpixel_wobble'][1], p['special_back'][1]]
    ev = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3, occlusion=True)
    keys = ev.video_keys(maps)
    total, pairs = O.masked_video_tables(maps, flows, backs, SEG6, C6, 2, keys)
    assert total['masked'][0] > 0 and total['misc'][0] > 0
    wide = torch.zeros(H, W, 4, dtype=torch.float32, device=dev)                 # a backward flow that is a view of a wider NHWC map
    wide[..., :2] = torch.from_numpy(backs[2]).to(dev)
    st = ev.add_video([maps[0], torch.from_numpy(maps[1]).to(dev), maps[2], maps[3]], [None, flows[1], torch.from_numpy(flows[2]).to(dev), flows[3]], 'clip',
                      back_flows=[None, backs[1], wide[..., :2], torch.from_numpy(backs[3]).to(dev)])
    equal_tables({k: st[k] for k in R.NAMES[:4]} | {'misc': np.array([st['in_view'], st['outside']])}, total)
    assert st['occluded'] == int(total['masked'][0]) and st['in_view'] + st['outside'] + st['occluded'] == 3 * H * W
    assert len(st['pairs']) == 3
    for got, want in zip(st['pairs'], pairs):
        w = R.terms(want)
        assert all(close(got[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track')) and got['in_view'] == w['in_view'] and got['outside'] == w['outside']
        assert got['occluded'] == int(want['masked'][0]) and got['in_view'] + got['outside'] + got['occluded'] == H * W
    assert sum(g['occluded'] for g in st['pairs']) == st['occluded'] and sum(g['in_view'] for g in st['pairs']) == st['in_view']
    res = ev.result()
    w = R.terms(total)
    assert all(close(res[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track')) and res['n_tracks'] == w['n_tracks']
    assert set(res) == RESULT_KEYS | {'occluded', 'occluded_share'} and close(res['occluded_share'], int(total['masked'][0]) / (3.0 * H * W))
    assert [r['pair'] for r in res['per_pair']] == [1, 2, 3] and all('occluded_share' in r for r in res['per_pair'] + res['per_video'])
    whole = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, id_last_stuff=3, occlusion=True)      # one row for the video
    st2 = whole.add_video(maps, flows, 'clip', back_flows=backs)
    equal_tables({k: st2[k] for k in R.NAMES[:4]} | {'misc': np.array([st2['in_view'], st2['outside']])}, total)
    assert st2['occluded'] == st['occluded'] and whole.result()['per_pair'] == []
    # ---- without the option: today's result object, key for key, and the backward flow is refused
    plain = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3)
    st3 = plain.add_video(maps, flows, 'clip')
    ptotal, ppairs = R.video_tables(maps, flows, SEG6, C6, 2, keys)
    equal_tables({k: st3[k] for k in R.NAMES[:4]} | {'misc': np.array([st3['in_view'], st3['outside']])}, ptotal)
    pres = plain.result()
    assert set(pres) == RESULT_KEYS and 'occluded' not in st3
    assert all(set(r) == {'video', 'pair', 'tc', 'tc_sem', 'tc_track', 'in_view_share'} for r in pres['per_pair'])
    assert all(set(r) == {'video', 'tc', 'tc_sem', 'tc_track', 'n_tracks', 'in_view_share'} for r in pres['per_video'])
    assert all(close(pres[k], R.terms(ptotal)[k]) for k in ('tc', 'tc_sem', 'tc_track'))
    with pytest.raises(ValueError):
        plain.add_pair(maps[0], maps[1], flows[1], back_flow=backs[1])
    with pytest.raises(ValueError):
        ev.add_pair(maps[0], maps[1], flows[1])
    with pytest.raises(ValueError):
        ev.add_video(maps, flows, 'clip')
    assert ev._open is None and plain._open is None


def test_run_vps_synthetic_tc_occlusion_equals_the_restatement_and_leaves_the_other_outputs_alone(dev, tmp_path, monkeypatch):
    """tools/run_vps_synthetic.py --tc --tc-occlusion on the clip of the --tc tool test (one video of 21 frames at 128 x 256, 20 pairs):
    tc.txt and tc-tracks.json hold the tables of the masked restatement run on the maps and the two flows as the tool hands them to the
    evaluator; `flow_between(ref, img)` ran once per frame but the first; pred.json, the PNGs and the VPQ figures are those of a run
    with --tc alone"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_vps_synthetic as S
    from vps_amd.detector import PanopticFuseTrack
    seen, between = [], []
    inner, inner_between = tc.TcEvaluator.add_pair, PanopticFuseTrack.flow_between

    def recording(self, prev, cur, flow, keys=None, flicker=None, **kw):
        back = kw.get('back_flow')
        seen.append((prev.cpu().numpy(), cur.cpu().numpy(), flow.cpu().numpy(), np.asarray(keys).copy(), self.seg_class.copy(), self.num_classes,
                     None if back is None else back.cpu().numpy()))
        return inner(self, prev, cur, flow, keys=keys, flicker=flicker, **kw)

    def counting(self, a, b, **kw):
        out = inner_between(self, a, b, **kw)
        between.append((a.clone(), b.clone(), out))
        return out
    monkeypatch.setattr(tc.TcEvaluator, 'add_pair', recording)
    monkeypatch.setattr(PanopticFuseTrack, 'flow_between', counting)
    common = ['--videos', '1', '--frames', '21', '--height', '128', '--width', '256']
    a, b = str(tmp_path / 'tc'), str(tmp_path / 'occ')
    ra = S.main(common + ['--out', a, '--tc'])
    assert len(seen) == 20 and not between and all(s[6] is None for s in seen) and 'occluded_share' not in ra['tc']
    plain_seen, seen[:] = list(seen), []
    rb = S.main(common + ['--out', b, '--tc-occlusion', '--tc-map', os.path.join(b, 'tcmap')])             # the flag implies --tc
    assert len(seen) == 20 == len(between) == rb['tc']['pairs'] and rb['tc']['map_files'] == 20
    for k in range(1, 20):
        assert torch.equal(between[k][0], between[k - 1][1])                     # (ref, img): the first image is the frame before
    for s, q, (_, _, back) in zip(seen, plain_seen, between):
        assert np.array_equal(s[6], back.cpu().numpy()) and s[6].shape == (128, 256, 2)
        assert all(np.array_equal(s[i], q[i]) for i in (0, 1, 3))                 # the same maps and keys as with --tc alone
    drop = ('tc', 'seconds', 'frames_per_s_upload_prep_model_sequential')
    assert {k: v for k, v in rb.items() if k not in drop} == {k: v for k, v in ra.items() if k not in drop}      # the VPQ figures among them
    for sub in ('pan_pred', 'pan_2ch'):
        fa = sorted(os.listdir(os.path.join(a, 'pred', sub)))
        assert len(fa) == 4 and fa == sorted(os.listdir(os.path.join(b, 'pred', sub)))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(a, 'pred', sub), os.path.join(b, 'pred', sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    vpq_txt = sorted(f for f in os.listdir(os.path.join(a, 'pred')) if f.startswith('vpq') and f.endswith('.txt'))
    assert vpq_txt == sorted(f for f in os.listdir(os.path.join(b, 'pred')) if f.startswith('vpq') and f.endswith('.txt'))
    for f in vpq_txt:
        assert open(os.path.join(a, 'pred', f), 'rb').read() == open(os.path.join(b, 'pred', f), 'rb').read(), f
    assert len(os.listdir(os.path.join(b, 'tcmap'))) == 20
    # ---- the tables behind the files
    keys, seg, C = seen[0][3], seen[0][4], seen[0][5]
    assert C == 19
    pairs = [O.masked_pair_tables(p, c, f, O.occlusion(f, back)[0], seg, C, 2, keys) for p, c, f, _, _, _, back in seen]
    total = {k: sum(p[k] for p in pairs) for k in O.NAMES}
    w = R.terms(total)
    doc = json.load(open(os.path.join(b, 'pred', 'tc-tracks.json')))
    assert np.array_equal(np.array(doc['conf']), total['conf']) and doc['in_view'] == w['in_view'] and doc['outside'] == w['outside']
    npix = 20 * 128 * 256
    assert doc['occluded'] == int(total['masked'][0]) and doc['in_view'] + doc['outside'] + doc['occluded'] == npix
    assert close(doc['occluded_share'], int(total['masked'][0]) / float(npix))
    listed = {int(k): i for i, k in enumerate(keys)}
    assert len(doc['tracks']) == w['n_tracks']
    for r in doc['tracks']:
        i = listed[r['key']]
        assert (r['same'], r['prev_size'], r['cur_size']) == (int(total['same'][i]), int(total['prev_size'][i]), int(total['cur_size'][i]))
    assert all(close(doc[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track'))
    assert len(doc['per_pair']) == 20 and all(close(r['tc'], R.terms(p)['tc']) and close(r['occluded_share'], int(p['masked'][0]) / (128.0 * 256.0))
                                              for r, p in zip(doc['per_pair'], pairs))
    text = open(os.path.join(b, 'pred', 'tc.txt')).read()
    lines = text.splitlines()
    assert lines[1].split()[-1] == 'OCC' and 'OCC' not in open(os.path.join(a, 'pred', 'tc.txt')).read()
    row = lines[3].split()
    assert row[0] == 'All' and row[2:6] == ['%.1f' % (100 * w['tc']), '%.1f' % (100 * w['tc_sem']), '%.1f' % (100 * w['tc_track']), '%d' % w['n_tracks']]
    assert row[7] == '%.2f' % (100 * doc['occluded_share'])
    assert rb['tc']['tc'] == round(100 * doc['tc'], 4) and rb['tc']['occluded_share'] == round(doc['occluded_share'], 6)
