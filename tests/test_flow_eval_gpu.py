"""GPU: `vps_flow_error` (csrc/flow_err_ops.hip), `vps_amd.floweval` and tools/eval_flow_device.py against the per-pixel restatement
(tests/flow_err_restate.py). `counts` and every byte of the error image with `array_equal`: the per-pixel arithmetic is correctly rounded
fp64 on both sides, so no decision can differ. Each `sums` cell within n * 2^-53 * sum|terms| of the `math.fsum` value, n the number of
pixels: the worst-case bound of ANY summation order of at most n terms (Higham, Accuracy and Stability, 4.2: |E| <= (n-1) u sum|x_i| +
O(u^2), u = 2^-53), not a measured tolerance."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import flow_err_restate as R
import flow_occ_restate as O
from test_flow_occ_gpu import NAN_BITS, canaried, put, strided
from test_tc_gpu import SIZES, TILE, flows_for
from vps_amd import floweval as fe
from vps_amd import hip, nhwc, tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FINISH_THREADS = 256                                         # threads of the finishing launch
BIG = (513, 513)                                             # 258 workgroups of 1024 pixels: more slots than the finishing launch has threads
DENSE = (2, 0, 0)


def pairs_for(rng, H, W):
    """name -> (pred, gt): the flow kinds of tests/test_tc_gpu.py (zero, shifts, smooth, noise, NaN / +-inf / +-1e30 / -0.0) in either place"""
    f = flows_for(rng, H, W)
    near = lambda a, s: (a + rng.standard_normal((H, W, 2)) * s).astype(np.float32)
    big = (f['smooth'] * 14).astype(np.float32)                                  # speeds in all three bins
    threes = np.zeros((H, W, 2), dtype=np.float32)
    threes[..., 0] = 3                                                           # epe exactly 3 everywhere: on the boundary of the outlier rule
    return {'zero': (f['zero'], f['zero']), 'right1_zero': (f['right1'], f['zero']), 'zero_left1': (f['zero'], f['left1']), 'down1_up1': (f['down1'], f['up1']),
            'far': (f['far_right'], f['far_up']), 'far_same': (f['far_left'], f['far_left']), 'smooth': (near(f['smooth'], 0.7), f['smooth']),
            'smooth_far': (near(big, 4.0), big), 'halves': (f['halves'], f['smooth']), 'noise': (f['noise'], near(f['noise'], 2.0)),
            'special_pred': (f['special'], f['smooth']), 'special_gt': (near(f['smooth'], 1.0), f['special']),
            'special_both': (f['special'], f['special'][::-1, ::-1].copy()), 'threes': (threes, f['zero'])}


def byte_maps(rng, H, W):
    """(mask with the values 0..3 and 255 in runs and alone, occ_pred with the codes 0..2 and a few 3)"""
    mask = rng.choice(np.array([0, 1, 1, 1, 2, 2, 3, 255], dtype=np.uint8), size=(H, W))
    mask[H // 3:H // 3 + 1 + H // 4, W // 4:W // 4 + 1 + W // 2] = 2
    occ = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3], dtype=np.uint8), size=(H, W))
    return mask, occ


def canary_bytes(n):
    return np.frombuffer(np.full((n + 3) // 4, NAN_BITS, dtype=np.int32).tobytes(), dtype=np.uint8)[:n]


def payload(buf, lo, hi):
    """the bytes lo..hi of a canaried buffer; asserts that every byte in front of and behind them is still the canary"""
    o = buf.view(torch.uint8).cpu().numpy()
    can = canary_bytes(len(o))
    assert np.array_equal(o[:lo], can[:lo]) and np.array_equal(o[hi:], can[hi:]), 'a byte outside the buffer has changed'
    return o[lo:hi].copy()


def run_err(dev, pred, gt, mask=None, occ=None, want_rgb=True, play=DENSE, glay=DENSE, moff=0, ooff=0, roff=0, repeat=1, zero_between=False, stream=None):
    """`repeat` calls of `vps_flow_error` with the flows at (ld, coff, base offset in floats), the byte maps and the image 0..3 bytes off a
    dword boundary, the tables and a workspace of exactly ws_bytes, everything between canaries (NaN words round the flows) -> (counts
    int64 [25], sums float64 [8] and their bytes per call, rgb or None). Asserts that nothing around any buffer, and no input, changed."""
    lib = hip.load()
    H, W = pred.shape[:2]
    inputs = []
    for flow, (ld, coff, off) in ((pred, play), (gt, glay)):
        body = strided(flow, ld, coff)
        buf, addr = canaried(dev, body.nbytes, 64 + 4 * off)
        put(buf, 64 + 4 * off, body)
        inputs.append((buf, addr, buf.clone()))
    for m, off in ((mask, moff), (occ, ooff)):
        if m is None:
            inputs.append((None, None, None))
            continue
        buf, addr = canaried(dev, H * W, 64 + off)
        put(buf, 64 + off, m)
        assert addr % 4 == off
        inputs.append((buf, addr, buf.clone()))
    rbuf, raddr = canaried(dev, 3 * H * W, 64 + roff)
    cbuf, caddr = canaried(dev, 200, 64)
    sbuf, saddr = canaried(dev, 64, 64)
    nws = int(lib.vps_flow_error_ws_bytes(H, W))
    assert nws == 64 * min((H * W + TILE - 1) // TILE, 1024)
    wbuf, waddr = canaried(dev, nws, 64)
    put(cbuf, 64, np.zeros(25, dtype=np.int64))
    put(sbuf, 64, np.zeros(8))
    P = ctypes.c_void_p
    per_call = []
    ctx = torch.cuda.stream(stream) if stream is not None else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        ctx.__enter__()
    try:
        for k in range(repeat):
            if k and zero_between:
                put(cbuf, 64, np.zeros(25, dtype=np.int64))
                put(sbuf, 64, np.zeros(8))
            code = lib.vps_flow_error(P(inputs[0][1]), play[0], play[1], P(inputs[1][1]), glay[0], glay[1], P(inputs[2][1]) if mask is not None else None,
                                      P(inputs[3][1]) if occ is not None else None, H, W, P(caddr), P(saddr), P(raddr) if want_rgb else None, P(waddr), nws,
                                      hip.stream_ptr())
            assert code == 0, code
            if zero_between:
                per_call.append(payload(sbuf, 64, 128).tobytes())
    finally:
        if stream is not None:
            ctx.__exit__(None, None, None)
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for buf, _, snap in inputs:
        assert buf is None or torch.equal(buf, snap)                             # the inputs and what lies round them
    counts = payload(cbuf, 64, 264).view(np.int64)
    sums = payload(sbuf, 64, 128).view(np.float64)
    payload(wbuf, 64, 64 + nws)                                                  # the canary right behind a workspace of exactly ws_bytes
    rgb = payload(rbuf, 64 + roff, 64 + roff + 3 * H * W)
    if not want_rgb:
        assert np.array_equal(rbuf.view(torch.uint8).cpu().numpy(), canary_bytes(rbuf.numel() * 4))
    return counts, sums, (rgb.reshape(H, W, 3) if want_rgb else None), per_call


def check(got, want, scale=1, what=''):
    counts, sums, rgb = got[:3]
    assert np.array_equal(counts, scale * want['counts']), (what, counts.tolist(), want['counts'].tolist())
    if rgb is not None:
        assert np.array_equal(rgb, want['rgb']), (what, int((rgb != want['rgb']).any(axis=2).sum()))
    bound = want['n'] * 2.0 ** -53 * want['abs']
    err = np.abs(sums - scale * want['sums'])
    assert (err <= scale * bound).all(), (what, err.tolist(), bound.tolist())
    c = counts
    assert int(c[0] + c[1] + c[12] + c[13] + c[24]) == scale * want['n']


@pytest.mark.parametrize('H,W', SIZES)
def test_counts_image_and_sums_equal_the_restatement_for_every_flow_kind(dev, H, W):
    rng = np.random.default_rng(700 * H + W)
    for i, (name, (pred, gt)) in enumerate(sorted(pairs_for(rng, H, W).items())):
        mask, occ = byte_maps(rng, H, W)
        mask, occ = (None, mask, mask)[i % 3], (occ, None, occ)[i % 3]
        want = R.flow_error(pred, gt, mask, occ)
        check(run_err(dev, pred, gt, mask, occ), want, what=name)


def test_more_workgroups_than_the_finishing_launch_has_threads(dev):
    H, W = BIG
    assert (H * W + TILE - 1) // TILE > FINISH_THREADS
    rng = np.random.default_rng(11)
    p = pairs_for(rng, H, W)
    mask, occ = byte_maps(rng, H, W)
    for name in ('smooth_far', 'special_both'):
        pred, gt = p[name]
        want = R.flow_error(pred, gt, mask, occ)
        assert (want['counts'][[6, 7, 8]] > 0).all() or name != 'smooth_far'
        check(run_err(dev, pred, gt, mask, occ), want, what=name)


def test_layouts_of_either_flow_and_odd_addresses_of_the_byte_maps_and_the_image(dev):
    H, W = 37, 53
    rng = np.random.default_rng(13)
    pred, gt = pairs_for(rng, H, W)['special_pred']
    gt = gt.copy(); gt[5, 7] = np.nan; gt[9, :3, 1] = 1e10
    mask, occ = byte_maps(rng, H, W)
    want = R.flow_error(pred, gt, mask, occ)                                     # one reference for every layout
    assert want['counts'][24] > 0 and want['counts'][1] > 0 and want['counts'][13] > 0 and want['counts'][2] > 0
    pad4, pad5 = (4, 0, 0), (5, 3, 0)                                            # FlowNet2's padded NHWC layout; an odd ld
    for play, glay, moff, ooff, roff in ((DENSE, DENSE, 0, 0, 0), (pad4, pad4, 0, 0, 0), (pad5, pad5, 1, 2, 3), (pad4, pad5, 3, 1, 2), (pad5, DENSE, 2, 3, 1),
                                         (DENSE, (2, 0, 1), 1, 1, 1), ((2, 0, 1), DENSE, 0, 3, 0), ((2, 0, 2), (4, 2, 1), 3, 0, 2), ((4, 2, 0), (3, 1, 0), 2, 2, 0),
                                         ((4, 0, 1), (4, 1, 1), 0, 0, 3), ((2, 0, 3), (2, 0, 2), 1, 0, 0)):
        check(run_err(dev, pred, gt, mask, occ, play=play, glay=glay, moff=moff, ooff=ooff, roff=roff), want, what=(play, glay, moff, ooff, roff))


def test_special_values_at_sizes_with_partial_chunks_read_and_write_nothing_outside(dev):
    """NaN, inf and 1e30 in either flow between NaN canaries (a read outside a flow would turn a counted pixel into an invalid or bad one),
    the byte maps and the image off a dword boundary at sizes whose last chunk is partial and whose maps end inside a dword"""
    for H, W in ((1, 1), (1, 6), (5, 13), (3, TILE + 1), (2, TILE + 3)):
        rng = np.random.default_rng(17 * H + W)
        p = pairs_for(rng, H, W)
        mask, occ = byte_maps(rng, H, W)
        for name in ('special_pred', 'special_gt', 'special_both'):
            pred, gt = p[name]
            want = R.flow_error(pred, gt, mask, occ)
            for play, glay, moff, ooff, roff in ((DENSE, DENSE, 0, 0, 0), ((4, 0, 0), (5, 3, 1), 1, 3, 2), ((2, 0, 1), (2, 0, 2), 3, 2, 1), (DENSE, DENSE, 2, 1, 3)):
                check(run_err(dev, pred, gt, mask, occ, play=play, glay=glay, moff=moff, ooff=ooff, roff=roff), want, what=(H, W, name, play))


def test_without_the_optional_buffers(dev):
    H, W = 37, 53
    rng = np.random.default_rng(19)
    pred, gt = pairs_for(rng, H, W)['smooth']
    mask, occ = byte_maps(rng, H, W)
    for m, o in ((None, None), (mask, None), (None, occ)):
        want = R.flow_error(pred, gt, m, o)
        got = run_err(dev, pred, gt, m, o, want_rgb=False)
        assert got[2] is None
        check(got, want)
        if o is None:
            assert not got[0][9:12].any() and not got[0][21:24].any()           # untouched without occ_pred
        if m is None:
            assert not got[0][12:25].any()                                       # every pixel is noc


def test_twice_gives_identical_bytes_and_without_zeroing_exactly_double(dev):
    for H, W in ((37, 53), (130, 257)):
        rng = np.random.default_rng(23 + H)
        pred, gt = pairs_for(rng, H, W)['smooth_far']
        mask, occ = byte_maps(rng, H, W)
        want = R.flow_error(pred, gt, mask, occ)
        counts, sums, rgb, per_call = run_err(dev, pred, gt, mask, occ, repeat=2, zero_between=True)
        check((counts, sums, rgb), want)
        assert per_call[0] == per_call[1] == sums.tobytes() and sums.any()      # the same bytes on every call
        counts2, sums2, rgb2, _ = run_err(dev, pred, gt, mask, occ, repeat=2)
        assert np.array_equal(counts2, 2 * counts) and sums2.tobytes() == (2 * sums).tobytes() and np.array_equal(rgb2, rgb)


def test_a_side_stream(dev):
    H, W = 64, 96
    rng = np.random.default_rng(29)
    pred, gt = pairs_for(rng, H, W)['smooth']
    mask, occ = byte_maps(rng, H, W)
    want = R.flow_error(pred, gt, mask, occ)
    side = torch.cuda.Stream(dev)
    got = run_err(dev, pred, gt, mask, occ, stream=side)
    check(got, want)
    assert got[1].tobytes() == run_err(dev, pred, gt, mask, occ)[1].tobytes()   # and the bytes of the default stream


def test_the_python_entry_takes_every_form_of_a_flow(dev):
    H, W = 37, 53
    rng = np.random.default_rng(31)
    pred, gt = pairs_for(rng, H, W)['smooth']
    mask, occ = byte_maps(rng, H, W)
    want = R.flow_error(pred, gt, mask, occ)
    wide = torch.full((1, H, W, 4), float('nan'), dtype=torch.float32, device=dev)               # FlowNet2's padded layout, read in place
    wide[0, :, :, :2] = torch.from_numpy(pred).to(dev)
    nchw = torch.from_numpy(gt).to(dev).permute(2, 0, 1)[None].contiguous()
    for p, g in ((nhwc.FMap(wide, 2, 0), gt), (torch.from_numpy(pred).to(dev), nchw), (pred, torch.from_numpy(gt).to(dev))):
        counts, sums, rgb = fe.flow_error(p, g, mask, torch.from_numpy(occ).to(dev), err_rgb=True)
        assert counts.is_cuda and sums.is_cuda and counts.dtype == torch.int64 and sums.dtype == torch.float64
        check((counts.cpu().numpy(), sums.cpu().numpy(), rgb.cpu().numpy()), want)
    assert fe.flow_error(pred, gt, device=dev)[2] is None
    own = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    assert fe.flow_error(pred, gt, err_rgb=own, device=dev)[2] is own and own.any()
    with pytest.raises(ValueError):
        fe.flow_error(pred, gt[:-1], device=dev)
    with pytest.raises(ValueError):
        fe.flow_error(pred, gt, mask[:, :-1], device=dev)
    with pytest.raises(ValueError):
        fe.flow_error(pred, gt, err_rgb=torch.zeros(H, W, dtype=torch.uint8, device=dev), device=dev)


def close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))                            # a handful of float64 operations on tables that agree to ~1e-16


def test_the_evaluator_with_and_without_per_pair_rows(dev):
    H, W = 37, 53
    rng = np.random.default_rng(37)
    p = pairs_for(rng, H, W)
    names = ('smooth', 'smooth_far', 'special_pred', 'noise')
    maps = [byte_maps(rng, H, W) for _ in names]
    wants = [R.flow_error(p[n][0], p[n][1], m, o) for n, (m, o) in zip(names, maps)]
    total_c, total_s = sum(w['counts'] for w in wants), sum(w['sums'] for w in wants)
    want_fig = R.figures(total_c, total_s, with_occ=True)
    for per_pair in (True, False):
        ev = fe.FlowEvaluator(dev, per_pair=per_pair)
        for i, (n, (m, o)) in enumerate(zip(names, maps)):
            pred = torch.from_numpy(p[n][0]).to(dev) if i % 2 else p[n][0]        # device flows are used as they are, host ones uploaded
            img = ev.add_pair(pred, p[n][1], mask=m, occ_pred=o, err_rgb=True if i == 1 else None, name=n)
            assert (img is None) == (i != 1) and (img is None or np.array_equal(img.cpu().numpy(), wants[1]['rgb']))
        res = ev.result()
        assert res['counts'] == total_c.tolist() and res['pairs'] == 4
        # each pair's cell is within H W u of its fsum (above); the three adds of four non-negative rows cost at most 3 u more, on either side
        assert all(abs(a - b) <= (H * W + 6) * 2.0 ** -53 * abs(b) for a, b in zip(res['sums'], total_s.tolist()))
        for k in fe.FIGURES + fe.OCC_FIGURES:
            assert close(res[k], want_fig[k]), k
        assert json.loads(json.dumps(res)) == res
        if per_pair:
            assert [r['pair'] for r in res['per_pair']] == list(names)
            assert sum(r['n'] for r in res['per_pair']) == res['n'] and sum(r['outliers'] for r in res['per_pair']) == res['outliers']
            for r, w in zip(res['per_pair'], wants):
                f = R.figures(w['counts'], w['sums'], with_occ=True)
                assert all(close(r[k], f[k]) for k in fe.FIGURES + fe.OCC_FIGURES)
        else:
            assert res['per_pair'] == []
    ev = fe.FlowEvaluator(dev, per_pair=True)                                    # more pairs than one block of rows
    for i in range(18):
        ev.add_pair(p['smooth'][0], p['smooth'][1])
    res = ev.result()
    assert len(res['per_pair']) == 18 and res['counts'] == (18 * R.flow_error(*p['smooth'])['counts']).tolist()
    with pytest.raises(ValueError):
        ev.add_pair(p['smooth'][0], p['smooth'][1][:-1])
    ev.add_pair(p['smooth'][0], p['smooth'][1])
    with pytest.raises(ValueError):
        ev.add_pair(p['smooth'][0], p['smooth'][1], occ_pred=maps[0][1])        # with a predicted mask for every pair or for none


def moving_square(H, W, y0, x0, size, d):
    """a still background and a square that sits at columns x0.. in prev and d columns further right in cur -> (fwd on the grid of cur
    pointing into prev, back on the grid of prev pointing into cur, the strip of cur that the square has uncovered: background that was
    hidden in prev)"""
    fwd, back = np.zeros((H, W, 2), dtype=np.float32), np.zeros((H, W, 2), dtype=np.float32)
    fwd[y0:y0 + size, x0 + d:x0 + d + size, 0] = -d
    back[y0:y0 + size, x0:x0 + size, 0] = d
    strip = np.zeros((H, W), dtype=bool)
    strip[y0:y0 + size, x0:x0 + d] = True
    return fwd, back, strip


def test_the_occlusion_figure_on_a_moving_square(dev):
    """the forward-backward check of tc.flow_occlusion flags exactly the uncovered strip (tests/test_flow_occ.py derives it by hand), so with
    the strip as mask value 2 precision and recall are 1; with a backward flow that is wrong on a patch of background they are what the
    restatement says"""
    H, W = 24, 40
    fwd, back, strip = moving_square(H, W, 6, 8, 7, 3)
    mask = np.where(strip, 2, 1).astype(np.uint8)
    mask[0, :5] = 0                                                              # some invalid pixels
    wrong = back.copy()
    wrong[15:19, 20:30, 1] = 2.5                                                 # false alarms on still background
    wrong[6:9, 8:10, 0] = 0                                                      # ... and part of the strip missed
    seen = []
    for b in (back, wrong):
        occ = tc.flow_occlusion(torch.from_numpy(fwd).to(dev), torch.from_numpy(b).to(dev))
        assert np.array_equal(occ.cpu().numpy(), O.occlusion(fwd, b)[0])
        counts, sums, _ = fe.flow_error(fwd, fwd, mask, occ, device=dev)
        want = R.flow_error(fwd, fwd, mask, O.occlusion(fwd, b)[0])
        assert np.array_equal(counts.cpu().numpy(), want['counts']) and not sums.cpu().numpy().any()
        got, fig = fe.flow_from_tables(counts.cpu().numpy(), sums.cpu().numpy(), with_occ=True), R.figures(want['counts'], want['sums'], with_occ=True)
        assert all(got[k] == fig[k] for k in fe.OCC_FIGURES)
        seen.append(got)
    assert seen[0]['occ_precision'] == 1.0 == seen[0]['occ_recall'] and seen[0]['occ_true_share'] == 21 / (H * W - 5.0) == seen[0]['occ_pred_share']
    assert 0 < seen[1]['occ_precision'] < 1 and 0 < seen[1]['occ_recall'] < 1


def test_the_tool_on_a_directory_of_flo_files_and_masks(dev, tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import eval_flow_device as T
    from vps_amd.flowvis import read_flo, write_flo
    H, W = 40, 72
    rng = np.random.default_rng(41)
    p = pairs_for(rng, H, W)
    names = {'frame_0001': 'smooth', 'frame_0002': 'smooth_far', 'frame_0003': 'special_pred'}
    wants = {}
    for d in ('pred', 'gt', 'invalid', 'occlusions'):
        os.makedirs(tmp_path / d)
    for stem, kind in names.items():
        pred, gt = p[kind]
        write_flo(pred, str(tmp_path / 'pred' / (stem + '.flo')))
        write_flo(gt, str(tmp_path / 'gt' / (stem + '.flo')))
        invalid, occluded = rng.random((H, W)) < 0.1, rng.random((H, W)) < 0.3
        Image.fromarray((invalid * 255).astype(np.uint8)).save(str(tmp_path / 'invalid' / (stem + '.png')))
        Image.fromarray(np.where(occluded, rng.integers(1, 256, size=(H, W)), 0).astype(np.uint8)).save(str(tmp_path / 'occlusions' / (stem + '.png')))
        mask = np.where(invalid, 0, np.where(occluded, 2, 1)).astype(np.uint8)
        assert np.array_equal(read_flo(str(tmp_path / 'pred' / (stem + '.flo'))), pred, equal_nan=True)
        wants[stem] = R.flow_error(pred, gt, mask)
    out, maps = str(tmp_path / 'out'), str(tmp_path / 'maps')
    res = T.main(['--pred', str(tmp_path / 'pred'), '--gt', str(tmp_path / 'gt'), '--mask', str(tmp_path / 'invalid'), '--occ-mask', str(tmp_path / 'occlusions'),
                  '--error-map', maps, '--format', 'png', '--out', out])
    total_c, total_s = sum(w['counts'] for w in wants.values()), sum(w['sums'] for w in wants.values())
    assert res['counts'] == total_c.tolist() and res['n_occ'] > 0 and res['invalid'] > 0 and res['bad'] > 0
    fig = R.figures(total_c, total_s)
    assert all(close(res[k], fig[k]) for k in fe.FIGURES)
    doc = json.load(open(os.path.join(out, 'flow-eval.json')))
    assert doc == res and [r['pair'] for r in doc['per_pair']] == sorted(names)
    for r in doc['per_pair']:
        f = R.figures(wants[r['pair']]['counts'], wants[r['pair']]['sums'])
        assert all(close(r[k], f[k]) for k in fe.FIGURES)
    lines = open(os.path.join(out, 'flow-eval.txt')).read().splitlines()
    assert len(lines) == 8 and lines[3].split()[0] == 'frame_0001' and lines[7].split()[:2] == ['All', '(3)'] and lines[7].split()[3] == '%.3f' % res['epe_all']
    for stem in names:                                                           # PNG is lossless: the error image, byte for byte
        assert np.array_equal(np.array(Image.open(os.path.join(maps, stem + '.png'))), wants[stem]['rgb']), stem
    # ---- a directory against itself: no error at all (the NaN of a prediction is unknown ground truth there)
    same = T.main(['--pred', str(tmp_path / 'gt'), '--gt', str(tmp_path / 'gt'), '--out', str(tmp_path / 'same'), '--error-map', str(tmp_path / 'same'),
                   '--format', 'jpg'])
    assert same['epe_all'] == 0.0 and same['fl_all'] == 0.0 and same['acc_1px'] == 1.0 and same['n'] == 3 * H * W and same['per_pair'][0]['epe_all'] == 0.0
    assert sorted(f for f in os.listdir(str(tmp_path / 'same')) if f.endswith('.jpg')) == [s + '.jpg' for s in sorted(names)]
    with pytest.raises(SystemExit):
        T.main(['--pred', str(tmp_path / 'pred'), '--gt', str(tmp_path / 'invalid')])
