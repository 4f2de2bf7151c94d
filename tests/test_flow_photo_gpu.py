"""GPU: `vps_flow_photo` (csrc/flow_photo_ops.hip), `vps_amd.flowphoto`, the `photometric=` option of `vps_amd.tc.TcEvaluator` and the
tool flags against the per-pixel restatement (tests/flow_photo_restate.py). `counts`, `mask_out` and `residual` with `array_equal`: the
sample is fp32 without contraction and the errors are correctly rounded fp64 on both sides, so no decision can differ. Each `sums` cell
within n * 2^-53 * sum|terms| of the `math.fsum` value, n the number of pixels: the worst-case bound of ANY summation order of at most n
terms (Higham, Accuracy and Stability, 4.2; derived in tests/test_flow_eval_gpu.py), not a measured tolerance."""
import ctypes
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import flow_occ_restate as O
import flow_photo_restate as R
import tc_restate as T
from test_flow_eval_gpu import canary_bytes, payload
from test_flow_occ_gpu import canaried, put, strided
from test_tc import close
from test_tc_gpu import C6, SEG6, SIZES, TILE, equal_tables, flows_for, rand_map
from vps_amd import flowphoto as fp
from vps_amd import hip, tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BIG = (513, 513)                                             # 258 workgroups of 1024 pixels: more slots than the finishing launch has lanes per cell
DENSE = (2, 0, 0)
ZERO_OFFS = dict(cur=0, prev=0, mask=0, mout=0, res=0)


def frames_for(rng, H, W):
    """name -> (cur, prev), uint8 [H,W,3]: uniform noise, a smooth ramp against itself shifted, constants, a 0 / 255 checkerboard"""
    ys, xs = np.mgrid[0:H, 0:W]
    noise = lambda: rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ramp = np.stack([(3 * xs + 2 * ys) % 256, (5 * ys + xs) % 256, (xs * 2) % 256], axis=-1).astype(np.uint8)
    check = np.repeat((((xs + ys) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    const = np.full((H, W, 3), 200, dtype=np.uint8)
    return {'noise': (noise(), noise()), 'ramp': (np.roll(ramp, 1, axis=1), ramp), 'const': (const, np.full((H, W, 3), 201, dtype=np.uint8)),
            'check': (check, 255 - check)}


def all_flows(rng, H, W):
    """the flow kinds of tests/test_tc_gpu.py (NaN / +-inf / +-1e30 / exact halves among them) and a sub-pixel field whose weights are
    neither 0 nor 1"""
    f = flows_for(rng, H, W)
    sub = np.zeros((H, W, 2), dtype=np.float32); sub[..., 0], sub[..., 1] = 0.3125, -0.625
    f['subpixel'] = sub
    f['subpixel_wobble'] = (sub + rng.standard_normal((H, W, 2)) * 0.3).astype(np.float32)
    return f


def rand_mask(rng, H, W):
    """the codes of vps_flow_occlusion and other bytes, in runs and alone"""
    m = np.where(rng.random((H, W)) < 0.3, rng.choice(np.array([1, 2, 3, 255], dtype=np.uint8), size=(H, W)), 0).astype(np.uint8)
    m[H // 3:H // 3 + 1 + H // 4, W // 4:W // 4 + 1 + W // 2] = 1
    return m


def run_photo(dev, cur, prev, flow, mask=None, thr=16.0, lay=DENSE, offs=ZERO_OFFS, want_mout=True, want_res=True, in_place=False, repeat=1,
              zero_between=False, stream=None):
    """`repeat` calls of `vps_flow_photo` with the flow at (ld, coff, base offset in floats), the frames and the byte maps 0..3 bytes off a
    dword boundary, the tables and a workspace of exactly ws_bytes, everything between canaries (NaN words) -> (counts int64 [21], sums
    float64 [4], mask_out or None, residual or None, the bytes of sums per call). in_place: mask_out is the mask's own buffer. Asserts that
    nothing around any buffer, and no input, changed."""
    lib = hip.load()
    H, W = flow.shape[:2]
    P = ctypes.c_void_p
    ld, coff, off = lay
    body = strided(flow, ld, coff)
    fbuf, faddr = canaried(dev, body.nbytes, 64 + 4 * off)
    put(fbuf, 64 + 4 * off, body)
    inputs = [(fbuf, fbuf.clone())]
    addr = {}
    for name, arr in (('cur', cur), ('prev', prev)):
        buf, a = canaried(dev, 3 * H * W, 64 + offs[name])
        put(buf, 64 + offs[name], arr)
        assert a % 4 == offs[name]
        addr[name] = a
        inputs.append((buf, buf.clone()))
    mbuf = None
    if mask is not None:
        mbuf, addr['mask'] = canaried(dev, H * W, 64 + offs['mask'])
        put(mbuf, 64 + offs['mask'], mask)
        if not in_place:
            inputs.append((mbuf, mbuf.clone()))
    obuf, addr['mout'] = canaried(dev, H * W, 64 + offs['mout'])
    rbuf, addr['res'] = canaried(dev, H * W, 64 + offs['res'])
    cbuf, caddr = canaried(dev, 168, 64)
    sbuf, saddr = canaried(dev, 32, 64)
    nws = int(lib.vps_flow_photo_ws_bytes(H, W))
    assert nws == 32 * min((H * W + TILE - 1) // TILE, 1024)
    wbuf, waddr = canaried(dev, nws, 64)
    put(cbuf, 64, np.zeros(21, dtype=np.int64))
    put(sbuf, 64, np.zeros(4))
    mout_addr = (addr['mask'] if in_place else addr['mout']) if want_mout else None
    per_call = []
    ctx = torch.cuda.stream(stream) if stream is not None else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        ctx.__enter__()
    try:
        for k in range(repeat):
            if k and zero_between:
                put(cbuf, 64, np.zeros(21, dtype=np.int64))
                put(sbuf, 64, np.zeros(4))
            if k and in_place:
                put(mbuf, 64 + offs['mask'], mask)
            code = lib.vps_flow_photo(P(addr['cur']), P(addr['prev']), H, W, P(faddr), ld, coff, P(addr['mask']) if mask is not None else None, thr, P(caddr),
                                      P(saddr), P(mout_addr) if mout_addr else None, P(addr['res']) if want_res else None, P(waddr), nws, hip.stream_ptr())
            assert code == 0, code
            if zero_between:
                per_call.append(payload(sbuf, 64, 96).tobytes())
    finally:
        if stream is not None:
            ctx.__exit__(None, None, None)
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for buf, snap in inputs:
        assert torch.equal(buf, snap)                                            # the inputs and what lies round them
    counts = payload(cbuf, 64, 64 + 168).view(np.int64)
    sums = payload(sbuf, 64, 96).view(np.float64)
    payload(wbuf, 64, 64 + nws)                                                  # the canary right behind a workspace of exactly ws_bytes
    mout = res = None
    if want_mout and in_place:
        mout = payload(mbuf, 64 + offs['mask'], 64 + offs['mask'] + H * W).reshape(H, W)
    elif want_mout:
        mout = payload(obuf, 64 + offs['mout'], 64 + offs['mout'] + H * W).reshape(H, W)
    if not want_mout or in_place:
        assert np.array_equal(obuf.view(torch.uint8).cpu().numpy(), canary_bytes(obuf.numel() * 4))
    if want_res:
        res = payload(rbuf, 64 + offs['res'], 64 + offs['res'] + H * W).reshape(H, W)
    else:
        assert np.array_equal(rbuf.view(torch.uint8).cpu().numpy(), canary_bytes(rbuf.numel() * 4))
    return counts, sums, mout, res, per_call


def check(got, want, scale=1, what=''):
    counts, sums, mout, res = got[:4]
    assert np.array_equal(counts, scale * want['counts']), (what, counts.tolist(), want['counts'].tolist())
    if mout is not None:
        assert np.array_equal(mout, want['mask_out']), (what, int((mout != want['mask_out']).sum()))
    if res is not None:
        assert np.array_equal(res, want['residual']), (what, int((res != want['residual']).sum()))
    bound = want['n'] * 2.0 ** -53 * want['abs']
    err = np.abs(sums - scale * want['sums'])
    assert (err <= scale * bound).all(), (what, err.tolist(), bound.tolist())
    assert int(counts[0] + counts[10] + counts[20]) == scale * want['n']


@pytest.mark.parametrize('H,W', SIZES)
def test_counts_maps_and_sums_equal_the_restatement_for_every_flow_and_frame_kind(dev, H, W):
    rng = np.random.default_rng(900 * H + W)
    frames = sorted(frames_for(rng, H, W).items())
    for i, (name, flow) in enumerate(sorted(all_flows(rng, H, W).items())):
        fname, (cur, prev) = frames[i % 4]
        mask = rand_mask(rng, H, W) if i % 3 else None
        thr = (16.0, 4.0, 0.0)[i % 3]
        want = R.flow_photo(cur, prev, flow, mask, thr)
        check(run_photo(dev, cur, prev, flow, mask, thr), want, what=(name, fname))


def test_several_hundred_workgroups_and_the_finishing_launch(dev):
    H, W = BIG
    assert (H * W + TILE - 1) // TILE > 256
    rng = np.random.default_rng(11)
    fl = all_flows(rng, H, W)
    fr = frames_for(rng, H, W)
    mask = rand_mask(rng, H, W)
    for name, fname in (('subpixel_wobble', 'noise'), ('special', 'ramp')):
        cur, prev = fr[fname]
        want = R.flow_photo(cur, prev, fl[name], mask)
        assert want['counts'][1] > 0 and want['counts'][10] > 0
        check(run_photo(dev, cur, prev, fl[name], mask), want, what=name)


def test_the_three_flow_layouts_and_every_byte_offset_of_the_five_maps(dev):
    H, W = 37, 53
    rng = np.random.default_rng(13)
    flow = (all_flows(rng, H, W)['subpixel_wobble'] - 0.8 * flows_for(rng, H, W)['smooth']).astype(np.float32)
    flow[5, 7] = np.nan; flow[9, :3, 1] = 1e30
    cur, prev = frames_for(rng, H, W)['noise']
    mask = rand_mask(rng, H, W)
    want = R.flow_photo(cur, prev, flow, mask)                                   # one reference for every layout
    assert want['counts'][20] > 0 and want['counts'][1] > 0 and want['counts'][11] > 0 and (want['mask_out'] == 3).any()
    modes = set()
    for lay, o in ((DENSE, (0, 0, 0, 0, 0)), ((4, 0, 0), (1, 1, 1, 1, 1)), ((5, 3, 0), (2, 3, 1, 0, 2)), ((2, 0, 1), (3, 2, 0, 3, 1)), ((2, 0, 2), (0, 1, 2, 2, 3)),
                   ((4, 2, 1), (1, 0, 3, 1, 0)), ((3, 1, 0), (2, 2, 2, 2, 2)), (DENSE, (3, 3, 3, 3, 3))):
        modes.add(2 if lay == DENSE else 1 if (lay[0] % 2 == 0 and (lay[1] + lay[2]) % 2 == 0) else 0)
        offs = dict(zip(('cur', 'prev', 'mask', 'mout', 'res'), o))
        check(run_photo(dev, cur, prev, flow, mask, lay=lay, offs=offs), want, what=(lay, o))
        got = run_photo(dev, cur, prev, flow, mask, lay=lay, offs=offs, in_place=True)           # mask_out is mask_in: the two-buffer result
        check(got, want, what=('in place', lay, o))
    assert modes == {0, 1, 2}


def test_special_values_at_sizes_with_partial_chunks_read_and_write_nothing_outside(dev):
    """NaN, inf, 1e30 and exact halves between NaN canaries, the maps off a dword boundary at sizes whose last chunk is partial and whose
    maps end inside a dword; a corner read outside `prev` would meet a canary byte and change a sum"""
    for H, W in ((1, 1), (1, 6), (5, 13), (3, TILE + 1), (2, TILE + 3)):
        rng = np.random.default_rng(17 * H + W)
        fl = all_flows(rng, H, W)
        cur, prev = frames_for(rng, H, W)['noise']
        mask = rand_mask(rng, H, W)
        for name in ('special', 'halves', 'noise'):
            want = R.flow_photo(cur, prev, fl[name], mask)
            for lay, o in ((DENSE, (0, 0, 0, 0, 0)), ((5, 3, 1), (1, 3, 2, 1, 3)), ((2, 0, 2), (3, 2, 1, 3, 2))):
                offs = dict(zip(('cur', 'prev', 'mask', 'mout', 'res'), o))
                check(run_photo(dev, cur, prev, fl[name], mask, lay=lay, offs=offs, in_place=(lay != DENSE)), want, what=(H, W, name, lay))


def test_without_the_optional_buffers(dev):
    H, W = 37, 53
    rng = np.random.default_rng(19)
    flow = all_flows(rng, H, W)['subpixel_wobble']
    cur, prev = frames_for(rng, H, W)['ramp']
    mask = rand_mask(rng, H, W)
    for m, want_mout, want_res in ((None, True, True), (mask, False, True), (mask, True, False), (None, False, False)):
        want = R.flow_photo(cur, prev, flow, m)
        got = run_photo(dev, cur, prev, flow, m, want_mout=want_mout, want_res=want_res)
        assert (got[2] is None) == (not want_mout) and (got[3] is None) == (not want_res)
        check(got, want)
        if m is None:
            assert not got[0][10:20].any() and not got[1][2:].any()              # every pixel is in group 0


def test_twice_gives_identical_bytes_and_without_zeroing_exactly_double(dev):
    for H, W in ((37, 53), (130, 257)):
        rng = np.random.default_rng(23 + H)
        flow = all_flows(rng, H, W)['subpixel_wobble']
        cur, prev = frames_for(rng, H, W)['noise']
        mask = rand_mask(rng, H, W)
        want = R.flow_photo(cur, prev, flow, mask)
        counts, sums, mout, res, per_call = run_photo(dev, cur, prev, flow, mask, repeat=2, zero_between=True)
        check((counts, sums, mout, res), want)
        assert per_call[0] == per_call[1] == sums.tobytes() and sums.all()       # the same bytes on every call
        counts2, sums2, mout2, res2, _ = run_photo(dev, cur, prev, flow, mask, repeat=2)
        assert np.array_equal(counts2, 2 * counts) and sums2.tobytes() == (2 * sums).tobytes() and np.array_equal(mout2, mout) and np.array_equal(res2, res)


def test_a_side_stream(dev):
    H, W = 64, 96
    rng = np.random.default_rng(29)
    flow = all_flows(rng, H, W)['smooth']
    cur, prev = frames_for(rng, H, W)['noise']
    mask = rand_mask(rng, H, W)
    want = R.flow_photo(cur, prev, flow, mask)
    got = run_photo(dev, cur, prev, flow, mask, stream=torch.cuda.Stream(dev))
    check(got, want)
    assert got[1].tobytes() == run_photo(dev, cur, prev, flow, mask)[1].tobytes()   # and the bytes of the default stream


def test_the_python_entry_validates_and_adds_to_caller_owned_tables(dev):
    H, W = 37, 53
    rng = np.random.default_rng(31)
    flow = all_flows(rng, H, W)['subpixel_wobble']
    cur, prev = frames_for(rng, H, W)['noise']
    mask = rand_mask(rng, H, W)
    want = R.flow_photo(cur, prev, flow, mask, 8.0)
    wide = torch.full((H, W, 4), float('nan'), dtype=torch.float32, device=dev)  # FlowNet2's padded layout, read in place
    wide[..., :2] = torch.from_numpy(flow).to(dev)
    dflow = torch.from_numpy(flow).to(dev)
    for f, c, m in ((wide[..., :2], cur, mask), (dflow, torch.from_numpy(cur).to(dev), torch.from_numpy(mask).to(dev))):
        mout, res = torch.empty(H, W, dtype=torch.uint8, device=dev), torch.empty(H, W, dtype=torch.uint8, device=dev)
        counts, sums = fp.flow_photometric(c, prev, f, mask=m, thr=8.0, mask_out=mout, residual=res)
        assert counts.is_cuda and sums.is_cuda and counts.dtype == torch.int64 and sums.dtype == torch.float64
        check((counts.cpu().numpy(), sums.cpu().numpy(), mout.cpu().numpy(), res.cpu().numpy()), want)
    dm = torch.from_numpy(mask).to(dev)
    c2, s2 = fp.flow_photometric(cur, prev, dflow, mask=dm, thr=8.0, counts=counts, sums=sums, mask_out=dm)   # in place, into the same tables
    assert c2 is counts and s2 is sums
    check((counts.cpu().numpy(), sums.cpu().numpy(), dm.cpu().numpy(), None), want, scale=2)
    for bad in (dict(cur=cur[:-1]), dict(prev=prev[:, :-1]), dict(mask=mask[:-1]), dict(thr=-1.0), dict(thr=float('nan')),
                dict(mask_out=torch.empty(H, W + 1, dtype=torch.uint8, device=dev)), dict(residual=torch.empty(H, W, dtype=torch.int32, device=dev)),
                dict(counts=torch.zeros(20, dtype=torch.int64, device=dev)), dict(sums=torch.zeros(4, dtype=torch.float32, device=dev))):
        kw = dict(dict(cur=cur, prev=prev, mask=mask, thr=8.0), **bad)
        with pytest.raises(ValueError):
            fp.flow_photometric(kw.pop('cur'), kw.pop('prev'), dflow, **kw)
    lut = fp.residual_colour(res)
    assert lut.shape == (H, W, 3) and np.array_equal(lut.cpu().numpy(), fp.RESIDUAL_PALETTE[want['residual']])


def same(a, b):
    return a == b or close(a, b)                                                 # inf == inf; otherwise a handful of float64 operations


def test_the_evaluator_with_and_without_per_pair_rows(dev):
    H, W = 37, 53
    rng = np.random.default_rng(37)
    fl, fr = all_flows(rng, H, W), frames_for(rng, H, W)
    pairs = [('smooth', 'noise', True), ('subpixel_wobble', 'ramp', False), ('special', 'check', True), ('zero', 'const', False)]
    masks = [rand_mask(rng, H, W) if m else None for _, _, m in pairs]
    wants = [R.flow_photo(fr[b][0], fr[b][1], fl[a], m, 12.0) for (a, b, _), m in zip(pairs, masks)]
    total_c, total_s = sum(w['counts'] for w in wants), sum(w['sums'] for w in wants)
    want_fig = R.figures(total_c, total_s)
    for per_pair in (True, False):
        ev = fp.PhotoEvaluator(dev, thr=12.0, per_pair=per_pair)
        for i, ((a, b, _), m) in enumerate(zip(pairs, masks)):
            flow = torch.from_numpy(fl[a]).to(dev) if i % 2 else fl[a]           # device flows are used as they are, host ones uploaded
            res = torch.empty(H, W, dtype=torch.uint8, device=dev) if i == 1 else None
            ev.add_pair(fr[b][1], fr[b][0], flow, mask=m, residual=res)
            assert res is None or np.array_equal(res.cpu().numpy(), wants[1]['residual'])
        st = ev.end_video('clip')
        assert np.array_equal(st['counts'], total_c) and st['pairs'] == 4
        res = ev.result()
        assert res['counts'] == total_c.tolist() and res['pairs'] == 4 and res['thr'] == 12.0
        # each pair's cell is within H W u of its fsum (above); the three adds of four non-negative rows cost at most 3 u more, on either side
        assert all(abs(a - b) <= (H * W + 6) * 2.0 ** -53 * abs(b) for a, b in zip(res['sums'], total_s.tolist()))
        for grp in ('all',) + fp.GROUPS:
            assert all(same(res[grp][k], want_fig[grp][k]) for k in fp.FIGURES), grp
        assert res['outside'] == want_fig['outside'] and json.loads(json.dumps(res)) == res
        if per_pair:
            assert [r['pair'] for r in res['per_pair']] == [1, 2, 3, 4] and sum(r['all']['n'] for r in res['per_pair']) == res['all']['n']
            for r, w in zip(res['per_pair'], wants):
                f = R.figures(w['counts'], w['sums'])
                assert all(same(r[g][k], f[g][k]) for g in ('all',) + fp.GROUPS for k in fp.FIGURES) and r['outside'] == f['outside']
        else:
            assert res['per_pair'] == []
    ev = fp.PhotoEvaluator(dev, per_pair=True)                                   # more pairs than one block of rows, through add_video
    n = 18
    st = ev.add_video(([fr['noise'][1], fr['noise'][0]] * (n // 2 + 1))[:n + 1], [None] + [fl['smooth']] * n, 'long')
    one = R.flow_photo(fr['noise'][0], fr['noise'][1], fl['smooth'])['counts'] + R.flow_photo(fr['noise'][1], fr['noise'][0], fl['smooth'])['counts']
    assert len(st['per_pair']) == n and np.array_equal(st['counts'], (n // 2) * one)
    with pytest.raises(ValueError):
        ev.add_pair(fr['noise'][1][:-1], fr['noise'][0], fl['smooth'])           # frames of another size than the flow's
    with pytest.raises(ValueError):
        ev.add_video([fr['noise'][1]] * 3, [None, fl['smooth']])
    assert ev._n == 0


def combined_tables(maps, frames, flows, backs, thr, keys):
    """the masked tables of tc_restate / flow_occ_restate fed the mask that flow_photo_restate makes of the occlusion mask"""
    pairs = []
    for t in range(1, len(maps)):
        occ = O.occlusion(flows[t], backs[t])[0]
        mask = R.flow_photo(frames[t], frames[t - 1], flows[t], occ, thr)['mask_out']
        assert np.array_equal(mask != 0, (occ != 0) | (mask == 3))
        pairs.append(O.masked_pair_tables(maps[t - 1], maps[t], flows[t], mask, SEG6, C6, 2, keys))
    return {k: sum(p[k] for p in pairs) for k in O.NAMES}, pairs


def test_the_photometric_option_of_the_tc_evaluator_equals_the_restated_combined_mask(dev):
    H, W = 37, 53
    rng = np.random.default_rng(61)
    maps = [rand_map(rng, H, W)]
    for _ in range(3):
        maps.append(np.roll(maps[-1], (1, 2), axis=(0, 1)))
    base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    frames = [base]
    for _ in range(3):
        nxt = np.roll(frames[-1], (1, 2), axis=(0, 1)).copy()
        y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
        nxt[y:y + 8, x:x + 8] = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)     # a patch the flow cannot explain
        frames.append(nxt)
    wob = lambda s: (rng.standard_normal((H, W, 2)) * s).astype(np.float32)
    shift = np.zeros((H, W, 2), dtype=np.float32); shift[..., 0], shift[..., 1] = -2, -1
    flows = [None, shift, (shift + wob(0.05)).astype(np.float32), (shift + wob(0.2)).astype(np.float32)]
    backs = [None, -shift, (-shift + wob(0.05)).astype(np.float32), (-shift + wob(0.6)).astype(np.float32)]
    thr = 16.0
    ev = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3, occlusion=True, photometric=thr)
    keys = ev.video_keys(maps)
    total, pairs = combined_tables(maps, frames, flows, backs, thr, keys)
    plain_total, _ = O.masked_video_tables(maps, flows, backs, SEG6, C6, 2, keys)
    assert total['masked'][0] > plain_total['masked'][0] > 0 and total['misc'][0] > 0    # the flag masks pixels the occlusion check lets through
    st = ev.add_video(maps, flows, 'clip', back_flows=backs, frames=[frames[0], torch.from_numpy(frames[1]).to(dev), frames[2], frames[3]])
    equal_tables({k: st[k] for k in T.NAMES[:4]} | {'misc': np.array([st['in_view'], st['outside']])}, total)
    assert st['occluded'] == int(total['masked'][0]) and st['in_view'] + st['outside'] + st['occluded'] == 3 * H * W
    for got, want in zip(st['pairs'], pairs):
        assert got['occluded'] == int(want['masked'][0]) and got['in_view'] == int(want['misc'][0]) and close(got['tc'], T.terms(want)['tc'])
    # ---- without the option: the tables of the occlusion option as they were
    occ = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3, occlusion=True)
    st2 = occ.add_video(maps, flows, 'clip', back_flows=backs)
    equal_tables({k: st2[k] for k in T.NAMES[:4]} | {'misc': np.array([st2['in_view'], st2['outside']])}, plain_total)
    assert st2['occluded'] == int(plain_total['masked'][0])
    with pytest.raises(ValueError):
        occ.add_pair(maps[0], maps[1], flows[1], back_flow=backs[1], frames=(frames[0], frames[1]))
    with pytest.raises(ValueError):
        ev.add_pair(maps[0], maps[1], flows[1], back_flow=backs[1])
    with pytest.raises(ValueError):
        ev.add_pair(maps[0], maps[1], flows[1], back_flow=backs[1], frames=(frames[0][:-1], frames[1]))
    assert ev._open is None and occ._open is None


def test_run_vps_synthetic_with_the_new_flags_equals_the_restatement_and_leaves_the_other_outputs_alone(dev, tmp_path, monkeypatch):
    """tools/run_vps_synthetic.py --tc-occlusion --flow-photo --tc-photometric 16 on the clip of the --tc-occlusion tool test (one video of
    21 frames at 128 x 256, 20 pairs): flow-photo.json holds the tables of the restatement run on the frames, flows and masks as the tool
    hands them to the evaluator, tc-tracks.json those of the masked restatement fed the restated combined mask; pred.json and the PNGs are
    those of a run with --tc-occlusion alone"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_vps_synthetic as S
    seen, tseen = [], []
    inner, tinner = fp.PhotoEvaluator.add_pair, tc.TcEvaluator.add_pair
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def recording(self, prev_frame, cur_frame, flow, mask=None, residual=None):
        seen.append((host(prev_frame).copy(), host(cur_frame).copy(), host(flow).copy(), None if mask is None else host(mask).copy()))
        return inner(self, prev_frame, cur_frame, flow, mask=mask, residual=residual)

    def trecording(self, prev, cur, flow, keys=None, flicker=None, **kw):
        fr = kw.get('frames')
        tseen.append((host(prev).copy(), host(cur).copy(), host(flow).copy(), np.asarray(keys).copy(), self.seg_class.copy(), self.num_classes,
                      host(kw['back_flow']).copy(), None if fr is None else (host(fr[0]).copy(), host(fr[1]).copy())))
        return tinner(self, prev, cur, flow, keys=keys, flicker=flicker, **kw)
    monkeypatch.setattr(fp.PhotoEvaluator, 'add_pair', recording)
    monkeypatch.setattr(tc.TcEvaluator, 'add_pair', trecording)
    common = ['--videos', '1', '--frames', '21', '--height', '128', '--width', '256']
    a, b = str(tmp_path / 'occ'), str(tmp_path / 'photo')
    ra = S.main(common + ['--out', a, '--tc-occlusion'])
    assert not seen and len(tseen) == 20 and all(s[7] is None for s in tseen) and 'flow_photo' not in ra and 'tc_photometric' not in ra
    plain, tseen[:] = list(tseen), []
    rb = S.main(common + ['--out', b, '--tc-occlusion', '--flow-photo', '--tc-photometric', '16', '--flow-photo-map', os.path.join(b, 'photomap')])
    assert len(seen) == 20 == len(tseen) == rb['flow_photo']['pairs'] and rb['flow_photo']['map_files'] == 20 and rb['tc_photometric'] == {'thr': 16.0}
    assert len(os.listdir(os.path.join(b, 'photomap'))) == 20
    drop = ('tc', 'seconds', 'frames_per_s_upload_prep_model_sequential', 'flow_photo', 'tc_photometric')
    assert {k: v for k, v in rb.items() if k not in drop} == {k: v for k, v in ra.items() if k not in drop}
    for sub in ('pan_pred', 'pan_2ch'):
        fa = sorted(os.listdir(os.path.join(a, 'pred', sub)))
        assert len(fa) == 4 and fa == sorted(os.listdir(os.path.join(b, 'pred', sub)))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(a, 'pred', sub), os.path.join(b, 'pred', sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    assert not os.path.exists(os.path.join(a, 'pred', 'flow-photo.json'))
    # ---- what the two evaluators were handed: the same flows, the frames of the pair, the occlusion mask
    for (pf, cf, fl, mask), t, q in zip(seen, tseen, plain):
        assert np.array_equal(fl, t[2]) and np.array_equal(mask, O.occlusion(fl, t[6])[0]) and pf.shape == (128, 256, 3)
        assert np.array_equal(pf, t[7][0]) and np.array_equal(cf, t[7][1]) and all(np.array_equal(t[i], q[i]) for i in (0, 1, 3))
    # ---- flow-photo.json
    wants = [R.flow_photo(cf, pf, fl, mask, 16.0) for pf, cf, fl, mask in seen]
    total_c, total_s = sum(w['counts'] for w in wants), sum(w['sums'] for w in wants)
    doc = json.load(open(os.path.join(b, 'pred', 'flow-photo.json')))
    assert doc['counts'] == total_c.tolist() and doc['pairs'] == 20 and doc['thr'] == 16.0 and total_c[10] > 0
    npix = 128 * 256
    assert all(abs(x - y) <= (npix + 40) * 2.0 ** -53 * abs(y) for x, y in zip(doc['sums'], total_s.tolist()))
    fig = R.figures(total_c, total_s)
    assert all(same(doc[g][k], fig[g][k]) for g in ('all',) + fp.GROUPS for k in fp.FIGURES)
    assert len(doc['per_pair']) == 20 and all(r['all']['n'] == int(w['counts'][0] + w['counts'][10]) for r, w in zip(doc['per_pair'], wants))
    assert rb['flow_photo']['mae_warp'] == round(doc['all']['mae_warp'], 6)
    assert open(os.path.join(b, 'pred', 'flow-photo.txt')).read() == fp.photo_text(doc)
    # ---- tc-tracks.json: the masked restatement fed the combined mask
    keys, seg, C = tseen[0][3], tseen[0][4], tseen[0][5]
    pairs = [O.masked_pair_tables(p, c, f, w['mask_out'], seg, C, 2, keys) for (p, c, f, *_), w in zip(tseen, wants)]
    total = {k: sum(p[k] for p in pairs) for k in O.NAMES}
    w = T.terms(total)
    tdoc = json.load(open(os.path.join(b, 'pred', 'tc-tracks.json')))
    assert np.array_equal(np.array(tdoc['conf']), total['conf']) and tdoc['in_view'] == w['in_view'] and tdoc['outside'] == w['outside']
    assert tdoc['occluded'] == int(total['masked'][0]) and tdoc['in_view'] + tdoc['outside'] + tdoc['occluded'] == 20 * npix
    assert all(close(tdoc[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track'))
    flagged = sum(int((x['mask_out'] == 3).sum()) for x in wants)               # mask_out == 2 is exactly "not in view": both kernels use one rule
    assert tdoc['occluded'] == flagged + sum(int((x['mask_out'] == 1).sum()) for x in wants) and tdoc['outside'] == int(total_c[20])
