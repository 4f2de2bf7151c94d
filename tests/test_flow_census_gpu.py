"""GPU: `vps_flow_census` (csrc/flow_census_ops.hip), the census names of `vps_amd.flowphoto`, the `census=` option of
`vps_amd.tc.TcEvaluator` and the tool flags against the restatement (tests/flow_census_restate.py). The table, `mask_out` and `residual`
with `array_equal`: the grey is an exact integer, the sample and the code differences are fp32 operations without contraction on both
sides, and everything after the codes is integer arithmetic, so no decision can differ and there is no tolerance anywhere."""
import ctypes
import filecmp
import json
import os
import sys

import numpy as np
import pytest
import torch

import flow_census_restate as R
import flow_occ_restate as O
import flow_photo_restate as P
import tc_restate as T
from test_flow_eval_gpu import canary_bytes, payload
from test_flow_occ_gpu import canaried, put, strided
from test_tc import close
from test_tc_gpu import C6, SEG6, equal_tables, flows_for, rand_map
from vps_amd import flowphoto as fp
from vps_amd import hip, tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DENSE = (2, 0, 0)
ZERO_OFFS = dict(cur=0, prev=0, mask=0, mout=0, res=0)


def tile():
    t = (ctypes.c_int32 * 2)()
    assert hip.load().vps_flow_census_tile(t) == 0
    return int(t[0]), int(t[1])


TR, TC = tile()
SIZES = [(1, 1), (1, 7), (7, 1), (6, 6), (7, 7), (37, 53), (TR + 1, TC + 1), (2 * TR + 5, 2 * TC + 3), (3, 16 * TC + 1)]
BIG = (513, 513)


def edge_frame(H, W, xs, ys):
    """60 / 160: the level changes between column e - 1 and e for every e of xs, and between rows likewise for ys"""
    cx = np.zeros(W, dtype=np.int64)
    for e in xs:
        if 0 < e < W:
            cx[e:] ^= 1
    cy = np.zeros(H, dtype=np.int64)
    for e in ys:
        if 0 < e < H:
            cy[e:] ^= 1
    g = (60 + 100 * (cx[None, :] ^ cy[:, None])).astype(np.uint8)
    return np.stack([g, g // 2 + 30, 255 - g], axis=-1).astype(np.uint8)


def frames_for(rng, H, W):
    """name -> (cur, prev), uint8 [H,W,3]: flat, a ramp, noise, checkerboards of period 1 and 7, and edges on and beside every tile seam
    and 2, 3, 4 pixels from every image border"""
    ys, xs = np.mgrid[0:H, 0:W]
    noise = lambda: rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    small = lambda a: np.clip(a.astype(np.int64) + rng.integers(-3, 4, size=a.shape), 0, 255).astype(np.uint8)
    ramp = np.stack([(3 * xs + 2 * ys) % 256, (5 * ys + xs) % 256, (xs * 2) % 256], axis=-1).astype(np.uint8)
    rep3 = lambda g: np.repeat(g.astype(np.uint8)[..., None], 3, axis=2)
    check1 = rep3(((xs + ys) % 2) * 255)
    check7 = rep3(40 + 150 * ((xs // 7 + ys // 7) % 2))
    sx, sy = list(range(TC, W, TC)), list(range(TR, H, TR))
    on = edge_frame(H, W, sx + [2, 4, W - 2, W - 4], sy + [2, 4, H - 2, H - 4])
    beside = edge_frame(H, W, [s + d for s in sx for d in (-1, 1)] + [3, W - 3], [s + d for s in sy for d in (-1, 1)] + [3, H - 3])
    return {'flat': (np.full((H, W, 3), 120, dtype=np.uint8), np.full((H, W, 3), 123, dtype=np.uint8)), 'ramp': (np.roll(ramp, 1, axis=1), ramp),
            'noise': (noise(), noise()), 'check1': (check1, 255 - check1), 'check7': (check7, np.roll(check7, 2, axis=1)),
            'edges_on': (on, small(np.roll(on, (1, 1), axis=(0, 1)))), 'edges_beside': (small(beside), np.roll(beside, -1, axis=1))}


def all_flows(rng, H, W):
    """the flow kinds of tests/test_tc_gpu.py - zero, +-1, beyond the image, the exact halves of row 3e, NaN / +-inf / +-1e30, smooth, white
    noise - and a sub-pixel field whose weights are neither 0 nor 1"""
    f = flows_for(rng, H, W)
    sub = np.zeros((H, W, 2), dtype=np.float32); sub[..., 0], sub[..., 1] = 0.3125, -0.625
    f['subpixel_wobble'] = (sub + rng.standard_normal((H, W, 2)) * 0.3).astype(np.float32)
    return f


def rand_mask(rng, H, W):
    m = np.where(rng.random((H, W)) < 0.3, rng.choice(np.array([1, 2, 3, 255], dtype=np.uint8), size=(H, W)), 0).astype(np.uint8)
    m[H // 3:H // 3 + 1 + H // 4, W // 4:W // 4 + 1 + W // 2] = 1
    return m


def run_census(dev, cur, prev, flow, mask=None, thr=25, eps=2000.0, lay=DENSE, offs=ZERO_OFFS, want_mout=True, want_res=True, in_place=False,
               repeat=1, zero_between=False, stream=None):
    """`repeat` calls of `vps_flow_census` with the flow at (ld, coff, base offset in floats), the frames and the byte maps 0..3 bytes off a
    dword boundary, the table and a workspace of exactly ws_bytes, everything between canaries (NaN words) -> (table int64 [2,13],
    mask_out or None, residual or None, the bytes of the table and the maps per call). in_place: mask_out is the mask's own buffer.
    Asserts that nothing around any buffer, and no input, changed."""
    lib = hip.load()
    H, W = flow.shape[:2]
    Pt = ctypes.c_void_p
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
    tbuf, taddr = canaried(dev, 208, 64)
    nws = int(lib.vps_flow_census_ws_bytes(H, W))
    assert nws == 12 * ((H * W + 3) // 4 * 4)
    wbuf, waddr = canaried(dev, nws, 64)
    put(tbuf, 64, np.zeros(26, dtype=np.int64))
    mout_addr = (addr['mask'] if in_place else addr['mout']) if want_mout else None
    obytes = lambda: (payload(mbuf, 64 + offs['mask'], 64 + offs['mask'] + H * W) if in_place else payload(obuf, 64 + offs['mout'], 64 + offs['mout'] + H * W))
    per_call = []
    ctx = torch.cuda.stream(stream) if stream is not None else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        ctx.__enter__()
    try:
        for k in range(repeat):
            if k and zero_between:
                put(tbuf, 64, np.zeros(26, dtype=np.int64))
            if k and in_place:
                put(mbuf, 64 + offs['mask'], mask)
            code = lib.vps_flow_census(Pt(addr['cur']), Pt(addr['prev']), H, W, Pt(faddr), ld, coff, Pt(addr['mask']) if mask is not None else None, thr, eps,
                                       Pt(taddr), Pt(mout_addr) if mout_addr else None, Pt(addr['res']) if want_res else None, Pt(waddr), nws,
                                       hip.stream_ptr())
            assert code == 0, code
            if zero_between:
                torch.cuda.current_stream().synchronize()
                per_call.append(payload(tbuf, 64, 64 + 208).tobytes() + (obytes().tobytes() if want_mout else b''))
    finally:
        if stream is not None:
            ctx.__exit__(None, None, None)
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for buf, snap in inputs:
        assert torch.equal(buf, snap)                                            # the inputs and what lies round them
    table = payload(tbuf, 64, 64 + 208).view(np.int64).reshape(2, 13)
    payload(wbuf, 64, 64 + nws)                                                  # the canary right behind a workspace of exactly ws_bytes
    mout = res = None
    if want_mout:
        mout = obytes().reshape(H, W)
    if not want_mout or in_place:
        assert np.array_equal(obuf.view(torch.uint8).cpu().numpy(), canary_bytes(obuf.numel() * 4))
    if want_res:
        res = payload(rbuf, 64 + offs['res'], 64 + offs['res'] + H * W).reshape(H, W)
    else:
        assert np.array_equal(rbuf.view(torch.uint8).cpu().numpy(), canary_bytes(rbuf.numel() * 4))
    return table, mout, res, per_call


def check(got, want, scale=1, what=''):
    table, mout, res = got[:3]
    assert np.array_equal(table, scale * want['table']), (what, table.tolist(), want['table'].tolist())
    if mout is not None:
        assert np.array_equal(mout, want['mask_out']), (what, int((mout != want['mask_out']).sum()))
    if res is not None:
        assert np.array_equal(res, want['residual']), (what, int((res != want['residual']).sum()))
    assert int(table[:, 0].sum() + table[:, 11].sum() + table[:, 12].sum()) == scale * want['n']


@pytest.mark.parametrize('H,W', SIZES)
def test_table_and_maps_equal_the_restatement_for_every_flow_and_frame_kind(dev, H, W):
    rng = np.random.default_rng(900 * H + W)
    frames = sorted(frames_for(rng, H, W).items())
    for i, (name, flow) in enumerate(sorted(all_flows(rng, H, W).items())):
        fname, (cur, prev) = frames[i % len(frames)]
        mask = rand_mask(rng, H, W) if i % 3 else None
        thr, eps = (25, 10, 0, 50)[i % 4], (2000.0, 0.0, 999.5)[i % 3]
        want = R.flow_census(cur, prev, flow, mask, thr, eps)
        check(run_census(dev, cur, prev, flow, mask, thr, eps), want, what=(name, fname))
    for fname, (cur, prev) in frames:                                            # every frame kind under a zero flow and under one pixel
        for u in (0.0, 1.0):
            flow = np.zeros((H, W, 2), dtype=np.float32); flow[..., 0] = u
            check(run_census(dev, cur, prev, flow), R.flow_census(cur, prev, flow), what=(fname, u))


def test_several_hundred_tiles(dev):
    H, W = BIG
    assert ((H + TR - 1) // TR) * ((W + TC - 1) // TC) > 100
    rng = np.random.default_rng(11)
    fl, fr = all_flows(rng, H, W), frames_for(rng, H, W)
    mask = rand_mask(rng, H, W)
    for name, fname in (('subpixel_wobble', 'edges_on'), ('special', 'noise')):
        cur, prev = fr[fname]
        want = R.flow_census(cur, prev, fl[name], mask)
        assert want['table'][0, 0] > 0 and want['table'][1, 0] > 0 and want['table'][:, 10].sum() > 0
        check(run_census(dev, cur, prev, fl[name], mask), want, what=name)


def test_the_three_flow_layouts_and_every_byte_offset_of_the_five_maps(dev):
    H, W = 37, 53
    rng = np.random.default_rng(13)
    flow = (all_flows(rng, H, W)['subpixel_wobble'] - 0.8 * flows_for(rng, H, W)['smooth']).astype(np.float32)
    flow[5, 7] = np.nan; flow[9, :3, 1] = 1e30
    cur, prev = frames_for(rng, H, W)['edges_beside']
    mask = rand_mask(rng, H, W)
    want = R.flow_census(cur, prev, flow, mask)                                  # one reference for every layout
    assert want['table'][:, 11].sum() > 0 and want['table'][0, 10] > 0 and want['table'][1, 0] > 0 and (want['mask_out'] == 3).any()
    modes = set()
    for lay, o in ((DENSE, (0, 0, 0, 0, 0)), ((4, 0, 0), (1, 1, 1, 1, 1)), ((5, 3, 0), (2, 3, 1, 0, 2)), ((2, 0, 1), (3, 2, 0, 3, 1)), ((2, 0, 2), (0, 1, 2, 2, 3)),
                   ((4, 2, 1), (1, 0, 3, 1, 0)), ((3, 1, 0), (2, 2, 2, 2, 2)), (DENSE, (3, 3, 3, 3, 3))):
        modes.add(2 if lay == DENSE else 1 if (lay[0] % 2 == 0 and (lay[1] + lay[2]) % 2 == 0) else 0)
        offs = dict(zip(('cur', 'prev', 'mask', 'mout', 'res'), o))
        check(run_census(dev, cur, prev, flow, mask, lay=lay, offs=offs), want, what=(lay, o))
        check(run_census(dev, cur, prev, flow, mask, lay=lay, offs=offs, in_place=True), want, what=('in place', lay, o))   # the two-buffer result
    assert modes == {0, 1, 2}


def test_special_values_at_small_and_ragged_sizes_read_and_write_nothing_outside(dev):
    for H, W in ((1, 1), (1, 6), (5, 13), (3, TC + 1), (2, 4 * TC + 3)):
        rng = np.random.default_rng(17 * H + W)
        fl = all_flows(rng, H, W)
        cur, prev = frames_for(rng, H, W)['noise']
        mask = rand_mask(rng, H, W)
        for name in ('special', 'halves', 'noise'):
            want = R.flow_census(cur, prev, fl[name], mask)
            for lay, o in ((DENSE, (0, 0, 0, 0, 0)), ((5, 3, 1), (1, 3, 2, 1, 3)), ((2, 0, 2), (3, 2, 1, 3, 2))):
                offs = dict(zip(('cur', 'prev', 'mask', 'mout', 'res'), o))
                check(run_census(dev, cur, prev, fl[name], mask, lay=lay, offs=offs, in_place=(lay != DENSE)), want, what=(H, W, name, lay))


def test_without_the_optional_buffers(dev):
    H, W = 37, 53
    rng = np.random.default_rng(19)
    flow = all_flows(rng, H, W)['subpixel_wobble']
    cur, prev = frames_for(rng, H, W)['ramp']
    mask = rand_mask(rng, H, W)
    for m, want_mout, want_res in ((None, True, True), (mask, False, True), (mask, True, False), (None, False, False)):
        want = R.flow_census(cur, prev, flow, m)
        got = run_census(dev, cur, prev, flow, m, want_mout=want_mout, want_res=want_res)
        assert (got[1] is None) == (not want_mout) and (got[2] is None) == (not want_res)
        check(got, want)
        if m is None:
            assert not got[0][1].any()                                           # every pixel is in group 0


def test_twice_gives_identical_bytes_and_without_zeroing_exactly_double(dev):
    for H, W in ((37, 53), (2 * TR + 2, 2 * TC + 1)):
        rng = np.random.default_rng(23 + H)
        flow = all_flows(rng, H, W)['subpixel_wobble']
        cur, prev = frames_for(rng, H, W)['noise']
        mask = rand_mask(rng, H, W)
        want = R.flow_census(cur, prev, flow, mask)
        table, mout, res, per_call = run_census(dev, cur, prev, flow, mask, repeat=2, zero_between=True)
        check((table, mout, res), want)
        assert per_call[0] == per_call[1] and table.any()
        table2, mout2, res2, _ = run_census(dev, cur, prev, flow, mask, repeat=2)
        assert np.array_equal(table2, 2 * table) and np.array_equal(mout2, mout) and np.array_equal(res2, res)


def test_a_side_stream(dev):
    H, W = 64, 96
    rng = np.random.default_rng(29)
    flow = all_flows(rng, H, W)['smooth']
    cur, prev = frames_for(rng, H, W)['check7']
    mask = rand_mask(rng, H, W)
    check(run_census(dev, cur, prev, flow, mask, stream=torch.cuda.Stream(dev)), R.flow_census(cur, prev, flow, mask))


def test_the_python_entry_validates_and_adds_to_a_caller_owned_table(dev):
    H, W = 37, 53
    rng = np.random.default_rng(31)
    flow = all_flows(rng, H, W)['subpixel_wobble']
    cur, prev = frames_for(rng, H, W)['noise']
    mask = rand_mask(rng, H, W)
    want = R.flow_census(cur, prev, flow, mask, 10, 1000.0)
    wide = torch.full((H, W, 4), float('nan'), dtype=torch.float32, device=dev)  # FlowNet2's padded layout, read in place
    wide[..., :2] = torch.from_numpy(flow).to(dev)
    dflow = torch.from_numpy(flow).to(dev)
    for f, c, m in ((wide[..., :2], cur, mask), (dflow, torch.from_numpy(cur).to(dev), torch.from_numpy(mask).to(dev))):
        mout, res = torch.empty(H, W, dtype=torch.uint8, device=dev), torch.empty(H, W, dtype=torch.uint8, device=dev)
        table = fp.flow_census(c, prev, f, mask=m, thr=10, eps=1000.0, mask_out=mout, residual=res)
        assert table.is_cuda and table.dtype == torch.int64 and tuple(table.shape) == (2, 13)
        check((table.cpu().numpy(), mout.cpu().numpy(), res.cpu().numpy()), want)
    dm = torch.from_numpy(mask).to(dev)
    t2 = fp.flow_census(cur, prev, dflow, mask=dm, thr=10, eps=1000.0, table=table, mask_out=dm)      # in place, into the same table
    assert t2 is table
    check((table.cpu().numpy(), dm.cpu().numpy(), None), want, scale=2)
    for bad in (dict(cur=cur[:-1]), dict(prev=prev[:, :-1]), dict(mask=mask[:-1]), dict(thr=-1), dict(thr=101), dict(thr=12.5), dict(eps=-1.0),
                dict(eps=float('nan')), dict(mask_out=torch.empty(H, W + 1, dtype=torch.uint8, device=dev)),
                dict(residual=torch.empty(H, W, dtype=torch.int32, device=dev)), dict(table=torch.zeros(21, dtype=torch.int64, device=dev))):
        kw = dict(dict(cur=cur, prev=prev, mask=mask, thr=10), **bad)
        with pytest.raises(ValueError):
            fp.flow_census(kw.pop('cur'), kw.pop('prev'), dflow, **kw)
    assert np.array_equal(fp.residual_colour(res).cpu().numpy(), fp.RESIDUAL_PALETTE[want['residual']])


def same(a, b):
    return a == b or close(a, b)


def test_the_evaluator_with_and_without_per_pair_rows(dev):
    H, W = 37, 53
    rng = np.random.default_rng(37)
    fl, fr = all_flows(rng, H, W), frames_for(rng, H, W)
    pairs = [('smooth', 'noise', True), ('subpixel_wobble', 'ramp', False), ('special', 'check7', True), ('zero', 'flat', False)]
    masks = [rand_mask(rng, H, W) if m else None for _, _, m in pairs]
    wants = [R.flow_census(fr[b][0], fr[b][1], fl[a], m, 30, 1500.0) for (a, b, _), m in zip(pairs, masks)]
    total = sum(w['table'] for w in wants)
    want_fig = R.figures(total)
    for per_pair in (True, False):
        ev = fp.CensusEvaluator(dev, thr=30, eps=1500.0, per_pair=per_pair)
        for i, ((a, b, _), m) in enumerate(zip(pairs, masks)):
            flow = torch.from_numpy(fl[a]).to(dev) if i % 2 else fl[a]           # device flows are used as they are, host ones uploaded
            res = torch.empty(H, W, dtype=torch.uint8, device=dev) if i == 1 else None
            ev.add_pair(fr[b][1], fr[b][0], flow, mask=m, residual=res)
            assert res is None or np.array_equal(res.cpu().numpy(), wants[1]['residual'])
        st = ev.end_video('clip')
        assert np.array_equal(st['table'], total) and st['pairs'] == 4
        res = ev.result()
        assert res['table'] == total.tolist() and res['pairs'] == 4 and res['thr'] == 30 and res['eps'] == 1500.0 and json.loads(json.dumps(res)) == res
        for grp in ('all',) + fp.GROUPS:
            assert all(same(res[grp][k], want_fig[grp][k]) for k in fp.CENSUS_FIGURES), grp
        if per_pair:
            assert [r['pair'] for r in res['per_pair']] == [1, 2, 3, 4]
            for r, w in zip(res['per_pair'], wants):
                f = R.figures(w['table'])
                assert all(same(r[g][k], f[g][k]) for g in ('all',) + fp.GROUPS for k in fp.CENSUS_FIGURES) and r['all']['n'] == f['all']['n']
        else:
            assert res['per_pair'] == []
    ev = fp.CensusEvaluator(dev, per_pair=True)                                  # more pairs than one block of rows, through add_video
    n = 18
    st = ev.add_video(([fr['noise'][1], fr['noise'][0]] * (n // 2 + 1))[:n + 1], [None] + [fl['smooth']] * n, 'long')
    one = R.flow_census(fr['noise'][0], fr['noise'][1], fl['smooth'])['table'] + R.flow_census(fr['noise'][1], fr['noise'][0], fl['smooth'])['table']
    assert len(st['per_pair']) == n and np.array_equal(st['table'], (n // 2) * one)
    with pytest.raises(ValueError):
        ev.add_pair(fr['noise'][1][:-1], fr['noise'][0], fl['smooth'])           # frames of another size than the flow's
    with pytest.raises(ValueError):
        ev.add_video([fr['noise'][1]] * 3, [None, fl['smooth']])
    assert ev._n == 0


def test_the_census_option_of_the_tc_evaluator_equals_the_restated_combined_mask(dev):
    H, W = 37, 53
    rng = np.random.default_rng(61)
    maps = [rand_map(rng, H, W)]
    for _ in range(3):
        maps.append(np.roll(maps[-1], (1, 2), axis=(0, 1)))
    base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    frames = [base]
    for k in range(3):
        nxt = np.roll(frames[-1], (1, 2), axis=(0, 1)).copy()
        y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
        nxt[y:y + 8, x:x + 8] = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)     # a patch the flow cannot explain
        frames.append(nxt)
    frames[2] = np.clip(frames[2].astype(np.int64) * 3 // 4 + 40, 0, 255).astype(np.uint8)   # a brightness change: the absolute error sees it everywhere
    wob = lambda s: (rng.standard_normal((H, W, 2)) * s).astype(np.float32)
    shift = np.zeros((H, W, 2), dtype=np.float32); shift[..., 0], shift[..., 1] = -2, -1
    flows = [None, shift, (shift + wob(0.05)).astype(np.float32), (shift + wob(0.2)).astype(np.float32)]
    backs = [None, -shift, (-shift + wob(0.05)).astype(np.float32), (-shift + wob(0.6)).astype(np.float32)]
    for photometric in (None, 16.0):
        ev = tc.TcEvaluator(SEG6, C6, id_channel=2, device=dev, per_pair=True, id_last_stuff=3, occlusion=True, census=25, census_eps=1500.0,
                            photometric=photometric)
        keys = ev.video_keys(maps)
        pairs = []
        for t in range(1, 4):
            occ = O.occlusion(flows[t], backs[t])[0]
            mask = occ if photometric is None else P.flow_photo(frames[t], frames[t - 1], flows[t], occ, photometric)['mask_out']
            mask = R.flow_census(frames[t], frames[t - 1], flows[t], mask, 25, 1500.0)['mask_out']
            assert ((mask == 3) & (occ == 0)).any()
            pairs.append(O.masked_pair_tables(maps[t - 1], maps[t], flows[t], mask, SEG6, C6, 2, keys))
        total = {k: sum(p[k] for p in pairs) for k in O.NAMES}
        st = ev.add_video(maps, flows, 'clip', back_flows=backs, frames=[frames[0], torch.from_numpy(frames[1]).to(dev), frames[2], frames[3]])
        equal_tables({k: st[k] for k in T.NAMES[:4]} | {'misc': np.array([st['in_view'], st['outside']])}, total)
        assert st['occluded'] == int(total['masked'][0]) and st['in_view'] + st['outside'] + st['occluded'] == 3 * H * W
        for got, want in zip(st['pairs'], pairs):
            assert got['occluded'] == int(want['masked'][0]) and close(got['tc'], T.terms(want)['tc'])
        with pytest.raises(ValueError):
            ev.add_pair(maps[0], maps[1], flows[1], back_flow=backs[1])
        assert ev._open is None


def test_run_vps_synthetic_with_the_new_flags_equals_the_restatement_and_leaves_the_other_outputs_alone(dev, tmp_path, monkeypatch):
    """tools/run_vps_synthetic.py --tc-occlusion --flow-census --tc-census 25 on one video of 21 frames at 128 x 256: flow-census.json holds
    the table of the restatement run on the frames, flows and masks as the tool hands them to the evaluator, tc-tracks.json the masked
    restatement fed the restated combined mask; pred.json and the PNGs are those of a run with --tc-occlusion alone"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_vps_synthetic as S
    seen, tseen = [], []
    inner, tinner = fp.CensusEvaluator.add_pair, tc.TcEvaluator.add_pair
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def recording(self, prev_frame, cur_frame, flow, mask=None, residual=None):
        seen.append((host(prev_frame).copy(), host(cur_frame).copy(), host(flow).copy(), None if mask is None else host(mask).copy()))
        return inner(self, prev_frame, cur_frame, flow, mask=mask, residual=residual)

    def trecording(self, prev, cur, flow, keys=None, flicker=None, **kw):
        tseen.append((host(prev).copy(), host(cur).copy(), host(flow).copy(), np.asarray(keys).copy(), self.seg_class.copy(), self.num_classes))
        return tinner(self, prev, cur, flow, keys=keys, flicker=flicker, **kw)
    monkeypatch.setattr(fp.CensusEvaluator, 'add_pair', recording)
    monkeypatch.setattr(tc.TcEvaluator, 'add_pair', trecording)
    common = ['--videos', '1', '--frames', '21', '--height', '128', '--width', '256']
    a, b = str(tmp_path / 'occ'), str(tmp_path / 'census')
    ra = S.main(common + ['--out', a, '--tc-occlusion'])
    assert not seen and len(tseen) == 20 and 'flow_census' not in ra and 'tc_census' not in ra
    tseen[:] = []
    rb = S.main(common + ['--out', b, '--tc-occlusion', '--flow-census', '--tc-census', '25', '--flow-census-map', os.path.join(b, 'censusmap')])
    assert len(seen) == 20 == len(tseen) == rb['flow_census']['pairs'] and rb['flow_census']['map_files'] == 20
    assert rb['tc_census'] == {'thr': 25, 'eps': 2000.0} and len(os.listdir(os.path.join(b, 'censusmap'))) == 20
    drop = ('tc', 'seconds', 'frames_per_s_upload_prep_model_sequential', 'flow_census', 'tc_census')
    assert {k: v for k, v in rb.items() if k not in drop} == {k: v for k, v in ra.items() if k not in drop}
    for sub in ('pan_pred', 'pan_2ch'):
        fa = sorted(os.listdir(os.path.join(a, 'pred', sub)))
        assert len(fa) == 4 and fa == sorted(os.listdir(os.path.join(b, 'pred', sub)))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(a, 'pred', sub), os.path.join(b, 'pred', sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    assert not os.path.exists(os.path.join(a, 'pred', 'flow-census.json'))
    wants = [R.flow_census(cf, pf, fl, mask, 25, 2000.0) for pf, cf, fl, mask in seen]
    total = sum(w['table'] for w in wants)
    doc = json.load(open(os.path.join(b, 'pred', 'flow-census.json')))
    assert doc['table'] == total.tolist() and doc['pairs'] == 20 and doc['thr'] == 25 and total[1, 0] > 0
    fig = R.figures(total)
    assert all(same(doc[g][k], fig[g][k]) for g in ('all',) + fp.GROUPS for k in fp.CENSUS_FIGURES)
    assert len(doc['per_pair']) == 20 and rb['flow_census']['ce_warp'] == round(doc['all']['ce_warp'], 6)
    assert open(os.path.join(b, 'pred', 'flow-census.txt')).read() == fp.census_text(doc)
    keys, seg, C = tseen[0][3], tseen[0][4], tseen[0][5]
    pairs = [O.masked_pair_tables(p, c, f, w['mask_out'], seg, C, 2, keys) for (p, c, f, *_), w in zip(tseen, wants)]
    tot = {k: sum(p[k] for p in pairs) for k in O.NAMES}
    tdoc = json.load(open(os.path.join(b, 'pred', 'tc-tracks.json')))
    w = T.terms(tot)
    assert np.array_equal(np.array(tdoc['conf']), tot['conf']) and tdoc['occluded'] == int(tot['masked'][0]) and tdoc['outside'] == w['outside']
    assert all(close(tdoc[k], w[k]) for k in ('tc', 'tc_sem', 'tc_track'))
