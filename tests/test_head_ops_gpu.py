"""Kernel-level tests of the detection head's order-defining kernels (vps_amd/csrc/head_ops.hip) and of vps_row_softmax as the
tracker calls it, through the C ABI, against tests/head_restate.py (numpy restatements of the reference's host code, pinned to the
oracle by tests/test_head_restate.py). Almost every comparison is exact; the two that are not derive their bound in the test from
the float32 restatement's own distance to float64 (figures in tests/tolerances.py).

Every output buffer is pre-filled with a sentinel (-7, or 0x5a bytes) and compared WHOLE: what the contract leaves alone must
still hold the sentinel."""
import ctypes

import numpy as np
import pytest
import torch

import head_restate as R
from oracle import fusetrack as OF
from vps_amd import hip

pytestmark = pytest.mark.gpu

S = -7            # the sentinel


def _sp():
    return hip.stream_ptr()


def _full(dev, shape, dtype=torch.float32):
    return torch.full(shape, S, dtype=dtype, device=dev)


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ vps_track_assign
def _track_case(name):
    """-> comp [K][M+1], M, E, ldb. Finite and -inf scores only."""
    rg = np.random.default_rng(sum(map(ord, name)))
    if name.startswith('one'):
        return np.array([[0.25, 0.5]] if name == 'one_matched' else [[0.5, 0.25]], dtype=np.float32), 1, 3, 4
    if name == 'k40':
        K, M = 40, 30
        comp = (rg.standard_normal((K, M + 1)) - 5).astype(np.float32)
        for r, v in ((0, 1.), (1, 2.), (2, 3.)):              # rising scores on memory entry 4: two undos
            comp[r, 5] = v
        for r, v in ((3, 3.), (4, 2.), (5, 1.)):              # falling scores on entry 8: the first one keeps it
            comp[r, 9] = v
        comp[6:11, 0] = 5.                                    # rows won by column 0: new objects
        comp[20] = -np.inf; comp[20, 3] = -2.                 # -inf everywhere but one column
        comp[21] = -np.inf; comp[21, 0] = -3.
        comp[22, 12] = 4.; comp[30, 12] = 4.                  # a later detection EQUAL to the holder's score: strict >, not reassigned
        return comp, M, 7, 5
    if name == 'ties':
        K, M = 8, 1600
        comp = (rg.standard_normal((K, M + 1)) - 5).astype(np.float32)
        comp[0, 0] = comp[0, 7] = 2.                          # equal maxima at columns 0 and 7: column 0 (a new object)
        comp[1, 300] = comp[1, 1500] = 2.                     # ... at columns 300 and 1500 (another wave, another chunk): 300
        comp[2, 300] = 2.                                     # equal to the holder of entry 299: strict >, it becomes a new object
        comp[3, 10] = comp[3, 1034] = 1.                      # the same thread in two chunks
        comp[4, 255] = comp[4, 256] = comp[4, 1279] = 1.5     # neighbours across the 256-column step, and one chunk on
        comp[5, 1600] = comp[5, 1599] = 3.                    # the last two columns
        comp[6, 64] = comp[6, 63] = 0.5                       # neighbouring waves
        return comp, M, 5, 4
    M = int(name[1:])
    comp = (rg.standard_normal((6, M + 1)) - 5).astype(np.float32)
    for r, c in enumerate([0, 255, 256, min(1023, M), min(1024, M), M]):
        comp[r, c] = 1. + r
    return comp, M, 300, 4


@pytest.mark.parametrize('name', ['one_matched', 'one_new', 'k40', 'ties', 'M1023', 'M1024', 'M1025', 'M2500'])
def test_track_assign(dev, name):
    """ids, the new memory count and the WHOLE memory (embeddings, boxes, labels, the spare rows included) equal the restatement of
    panoptic_fusetrack.py:424-469; the row arg-max is the FIRST maximum across lanes, waves and 1024-column chunks"""
    comp, M, E, ldb = _track_case(name)
    K = comp.shape[0]
    rg = np.random.default_rng(K + M)
    emb = rg.standard_normal((K, E)).astype(np.float32)
    box = rg.uniform(0, 500, (K, ldb)).astype(np.float32)
    label = rg.integers(1, 9, K).astype(np.int64)
    pe = np.full((M + K, E), S, np.float32); pb = np.full((M + K, 4), S, np.float32); pl = np.full(M + K, S, np.int64)
    pe[:M] = rg.standard_normal((M, E)); pb[:M] = rg.uniform(0, 500, (M, 4)); pl[:M] = rg.integers(1, 9, M)
    want_ids, want_m, we, wb, wl = R.track_assign(comp, M, emb, box, label, pe, pb, pl)
    assert np.array_equal(wl[:M], pl[:M])
    d = [_up(dev, a) for a in (comp, emb, box, label, pe, pb, pl)]
    scratch = torch.full((M + 3 * K + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    ids = _full(dev, (K + 3,), torch.int32); m_out = _full(dev, (4,), torch.int32)
    hip.check(hip.load().vps_track_assign(hip.ptr(d[0]), K, M, hip.ptr(d[1]), E, hip.ptr(d[2]), ldb, hip.ptr(d[3]), hip.ptr(d[4]), hip.ptr(d[5]),
                                          hip.ptr(d[6]), hip.ptr(scratch), hip.ptr(ids), hip.ptr(m_out), _sp()), 'vps_track_assign')
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == want_ids.tolist() + [S] * 3
    assert m_out.cpu().tolist() == [want_m, S, S, S]
    assert np.array_equal(d[4].cpu().numpy(), we) and np.array_equal(d[5].cpu().numpy(), wb) and np.array_equal(d[6].cpu().numpy(), wl)
    assert np.array_equal(d[0].cpu().numpy(), comp), 'the scores are read only'
    if name == 'ties':
        assert want_ids[0] >= M and want_ids[1] == 299 and want_ids[2] >= M and want_ids[3] == 9 and want_ids[4] == 254 and want_ids[5] == 1598 and want_ids[6] == 62
    if name == 'k40':
        assert want_ids[2] == 4 and want_ids[0] >= M and want_ids[1] >= M and want_ids[3] == 8 and want_ids[4] >= M and want_ids[22] == 11 and want_ids[30] >= M


# ------------------------------------------------------------------------------------------------ vps_row_softmax
def _softmax_inputs(rows, cols):
    x = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 131 + cols)) * 3.0)
    if cols > 1:
        x[0, cols // 2] = x[0].max() + 90.0                                   # a maximum 90 above the rest of its row
    if rows > 1:
        x[rows - 1, ::3] = float('-inf')                                      # some, not all
        if cols > 1:
            x[rows - 1, 1] = 0.5
    return x


def _softmax_f32_sequential(x, mode):
    """the kernel's formula, one float32 operation after the other in column order (numpy's exp / log)"""
    x = x.numpy()
    out = np.empty_like(x)
    for r in range(x.shape[0]):
        mx = np.float32(-np.inf)
        for v in x[r]:
            mx = max(mx, v)
        e = np.exp(x[r] - mx)
        s = np.float32(0)
        for v in e:
            s = np.float32(s + v)
        out[r] = e / s if mode == 0 else x[r] - mx - np.log(s)
    return out


def softmax_bound(x, mode, verbose=None):
    """per-element tolerance of vps_row_softmax on x: the project's 1e-6 + 1e-5 |ref|; for rows wider than one 64-column step also
    4 x the largest deviation of the sequential float32 restatement from float64 on x (the factor covers expf / logf against
    numpy's), never below the former"""
    ref = (torch.softmax if mode == 0 else torch.log_softmax)(x.double(), dim=1)
    tol = 1e-6 + 1e-5 * ref.abs()
    tol[torch.isinf(ref)] = 0.0
    if x.shape[1] > 64:
        seq = torch.from_numpy(_softmax_f32_sequential(x, mode)).double()
        fin = torch.isfinite(ref)
        assert torch.equal(seq[~fin], ref[~fin])
        dev64 = float((seq[fin] - ref[fin]).abs().max())
        if verbose is not None:
            print('%s: sequential float32 restatement vs float64: %.3e' % (verbose, dev64))
        tol = torch.maximum(tol, torch.full_like(tol, 4 * dev64) * fin)
    return ref, tol


@pytest.mark.parametrize('mode', [0, 1], ids=['softmax', 'log_softmax'])
@pytest.mark.parametrize('rows,cols', [(1, 1), (3, 64), (5, 65), (7, 129), (2, 2101)])
def test_row_softmax_wide_rows_and_ragged_blocks(dev, rows, cols, mode):
    """cols = M + 1 as the tracker calls it (64-column steps, a ragged last step), row counts that are no multiple of the 4 rows of
    a block, against float64 torch; -inf entries give exactly 0 / -inf"""
    x = _softmax_inputs(rows, cols)
    ref, tol = softmax_bound(x, mode, 'row_softmax %dx%d mode %d' % (rows, cols, mode))
    xd = x.to(dev)
    o = _full(dev, (rows + 1, cols))
    hip.check(hip.load().vps_row_softmax(hip.ptr(xd), hip.ptr(o), rows, cols, mode, _sp()), 'vps_row_softmax')
    torch.cuda.synchronize()
    got = o.cpu().double()
    assert (got[rows] == S).all()
    got = got[:rows]
    assert not torch.isnan(got).any()
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf])
    if mode == 0:
        assert (got[x == float('-inf')] == 0).all()
    err = (got - ref).abs()
    err[inf] = 0.0
    print('max err %.3e, smallest tolerance %.3e' % (float(err.max()), float(tol[~inf].min())))
    assert bool((err <= tol).all()), 'max err %.3e at %s' % (float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


# ------------------------------------------------------------------------------------------------ vps_maskroi_select / finish
NC, THR, WTS, IM_HW = 9, 0.6, (10., 10., 5., 5.), (512., 1024.)


def _select_inputs(kind):
    """-> rois [n][5], delta [n][4 nc], prob [n][nc]"""
    n = {'n37': 37, 'none': 37, 'full': 1024, 'over': 1100}[kind]
    rg = np.random.default_rng(n)
    x1 = rg.uniform(0, 900, n); y1 = rg.uniform(0, 440, n)
    rois = np.stack([np.zeros(n), x1, y1, np.minimum(x1 + rg.uniform(3, 200, n), 1023), np.minimum(y1 + rg.uniform(3, 120, n), 511)], 1).astype(np.float32)
    delta = (rg.standard_normal((n, 4 * NC)) * 1.5).astype(np.float32)
    prob = (rg.integers(0, 17, (n, NC)) / 16.0).astype(np.float32)             # steps of 1/16: ties
    if kind in ('n37', 'none'):
        rois[0:4, 1:] = [[5, 100, 60, 200], [950, 100, 1020, 200], [300, 5, 400, 50], [300, 450, 400, 505]]
        d = delta.reshape(n, NC, 4)
        d[0, :, 0] = -30.; d[1, :, 0] = 30.; d[2, :, 1] = -30.; d[3, :, 1] = 30.     # boxes that leave the image on each of its sides
        d[4, :, 2] = 21.5; d[5, :, 3] = 22.; d[6, :, 2:] = 40.                      # beyond the log(1000 / 16) clip (x 5)
        prob[0:7, 1:] = np.maximum(prob[0:7, 1:], np.float32(0.625))               # ... and they are candidates
        prob[7:12, 2] = np.float32(0.6); prob[20, 1:] = np.float32(0.6)            # exactly the threshold: excluded
    if kind == 'none':
        prob = (prob * 0.5).astype(np.float32)
        prob[3, 4] = np.float32(0.6)
    if kind in ('full', 'over'):
        prob = (0.625 + rg.integers(0, 32, (n, NC)) / 128.0).astype(np.float32)    # 32 distinct values, all above the threshold
    return rois, delta, prob


def _run_select(dev, rois, delta, prob, n_valid):
    n = rois.shape[0]
    cap = min(n * (NC - 1), R.SORT_CAP)
    d = [_up(dev, a) for a in (rois, delta, prob)]
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=dev)
    dets = _full(dev, (cap + 2, 5)); cand = _full(dev, (cap + 2,), torch.int32); m_out = _full(dev, (4,), torch.int32)
    wts = (ctypes.c_float * 4)(*WTS)
    hip.check(hip.load().vps_maskroi_select(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), n, hip.ptr(nv), NC, THR, wts, IM_HW[0], IM_HW[1],
                                            hip.ptr(dets), hip.ptr(cand), hip.ptr(m_out), _sp()), 'vps_maskroi_select')
    torch.cuda.synchronize()
    return dets, cand, m_out


def box_bound(rois, delta, prob, n_valid, what=None):
    """tolerance of the decoded boxes: 2 x the largest deviation of the float32 restatement from the same formula in float64 on
    these inputs, at least one float32 ulp of the image width"""
    w32 = R.maskroi_select(rois, delta, prob, n_valid, NC, THR, WTS, IM_HW)
    w64 = R.maskroi_select(rois, delta, prob, n_valid, NC, THR, WTS, IM_HW, dtype=np.float64)
    assert np.array_equal(w32[1], w64[1])
    dev64 = float(np.abs(w32[0][:, :4].astype(np.float64) - w64[0][:, :4]).max()) if w32[2][0] else 0.0
    ulp = float(np.spacing(np.float32(IM_HW[1])))
    if what:
        print('%s: float32 restatement vs float64 boxes %.3e, ulp of the image width %.3e' % (what, dev64, ulp))
    return w32, max(2 * dev64, ulp)


@pytest.mark.parametrize('kind,n_valid', [('n37', None), ('n37', 30), ('n37', 50), ('none', None), ('full', None)])
def test_maskroi_select(dev, kind, n_valid):
    """scores, candidate indices and the count record exact (strict `> thr`, ties: the larger candidate index first, rows past
    n_valid ignored, the full 8192-key sort), boxes within box_bound; rows past m untouched"""
    rois, delta, prob = _select_inputs(kind)
    if n_valid == 30:
        prob[30:, 1:] = np.float32(0.99)                                           # rows that do not exist: must be ignored
    (wd, wc, wm), tol = box_bound(rois, delta, prob, n_valid, 'maskroi_select %s' % kind)
    m = wm[0]
    assert wm == {'n37': [m, 0, min(n_valid or 37, 37)], 'none': [0, 0, 37], 'full': [8192, 0, 1024]}[kind]
    if kind == 'n37':
        assert 60 < m < 296 and np.unique(wd[:, 4]).size <= 7 and (wd[:, :4] == 0).any() and (wd[:, 2] == 1023).any() and (wd[:, 3] == 511).any()
    dets, cand, m_out = _run_select(dev, rois, delta, prob, n_valid)
    assert m_out.cpu().tolist() == wm + [S]
    got, gc = dets.cpu().numpy(), cand.cpu().numpy()
    assert (got[m:] == S).all() and (gc[m:] == S).all()
    assert np.array_equal(gc[:m], wc), 'candidate order: first difference at %s' % np.nonzero(gc[:m] != wc)[0][:3]
    assert np.array_equal(got[:m, 4], wd[:, 4])
    err = float(np.abs(got[:m, :4].astype(np.float64) - wd[:, :4]).max()) if m else 0.0
    print('boxes: max deviation %.3e, bound %.3e' % (err, tol))
    assert err <= tol


def test_maskroi_select_overflow_status(dev):
    """more than 8192 candidates: 8192 are listed and the overflow word is set (which ones fill the slots is not defined)"""
    rois, delta, prob = _select_inputs('over')
    _, _, m_out = _run_select(dev, rois, delta, prob, None)
    assert m_out.cpu().tolist() == [8192, 1, 1100, S]


FINISH_CASES = {
    # name: (nk, max_det, kcap, overflow word, tie runs (first, last kept position))
    'dummy_row': (0, 100, 256, 0, None),
    'five': (5, 100, 256, 0, None),
    'at_cap': (100, 100, 256, 0, None),
    'cut': (120, 100, 256, 0, None),
    'ties_straddle_cap': (120, 100, 256, 0, (97, 104)),
    'ties_end_at_cap': (120, 100, 256, 0, (90, 99)),
    'ties_start_at_cap': (120, 100, 256, 0, (100, 103)),
    'ties_to_the_end': (120, 100, 256, 0, (95, 119)),
    'more_than_kcap': (60, 100, 50, 0, None),
    'cut_then_kcap': (130, 100, 90, 1, (97, 104)),
    'no_max_det': (150, 0, 256, 0, None),
    'overflow_word': (5, 100, 256, 1, None),
}


def _finish_inputs(name):
    nk, max_det, kcap, ovf, ties = FINISH_CASES[name]
    rg = np.random.default_rng(nk + kcap)
    m = 400
    dets = rg.uniform(0, 500, (m, 5)).astype(np.float32)
    dets[:, 4] = np.sort(0.6 + 0.4 * (rg.permutation(4000)[:m].astype(np.float32) + 1) / 4001)[::-1]        # distinct, descending
    keep = np.full(m, m - 1, dtype=np.int32)                 # entries past nkeep point at a valid row, they must not be read
    keep[:nk] = np.sort(rg.permutation(m - 1)[:nk]) if nk else []
    if ties:
        a, b = int(keep[ties[0]]), int(keep[ties[1]])
        dets[a:b + 1, 4] = dets[a, 4]
    cand = rg.integers(0, 300 * (NC - 1), m).astype(np.int32)
    return dets, cand, [m, ovf, 300], keep, nk, max_det, kcap


@pytest.mark.parametrize('name', list(FINISH_CASES))
def test_maskroi_finish(dev, name):
    """header, rows (box, score, class and candidate columns) and everything behind them, exact: the max_det cut keeps every score
    equal to the max_det-th (`>=`), K > kcap raises status bit 1, the overflow word bit 0, an empty list gives the dummy row"""
    dets, cand, m_in, keep, nk, max_det, kcap = _finish_inputs(name)
    head, rows = R.maskroi_finish(dets, cand, m_in, keep, nk, NC, max_det, kcap)
    K = rows.shape[0]
    assert K == {'dummy_row': 1, 'five': 5, 'at_cap': 100, 'cut': 100, 'ties_straddle_cap': 105, 'ties_end_at_cap': 100, 'ties_start_at_cap': 100,
                 'ties_to_the_end': 120, 'more_than_kcap': 50, 'cut_then_kcap': 90, 'no_max_det': 150, 'overflow_word': 5}[name]
    assert int(head[3]) == {'more_than_kcap': 2, 'cut_then_kcap': 3, 'overflow_word': 1}.get(name, 0)
    d = [_up(dev, a) for a in (dets, cand, np.array(m_in + [S], np.int32), keep, np.array([nk, S], np.int32))]
    res = _full(dev, (8 + 8 * kcap + 16,))
    hip.check(hip.load().vps_maskroi_finish(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), hip.ptr(d[3]), hip.ptr(d[4]), NC, max_det, kcap, hip.ptr(res),
                                            _sp()), 'vps_maskroi_finish')
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert got[:8].tolist() == head.tolist() + [S] * 3
    assert np.array_equal(got[8:8 + 8 * K].reshape(K, 8), rows)
    assert (got[8 + 8 * K:] == S).all()
    if nk:
        assert np.array_equal(rows[:, 7], cand[keep[:K]]) and np.array_equal(rows[:, 6], cand[keep[:K]] % (NC - 1) + 1)


def _tied_pairs_do_not_suppress(dets, thr):
    """no two candidates of EQUAL score overlap beyond the NMS threshold: the kept set then does not depend on the order among equal
    scores, which numpy's default argsort (the reference's `scores.argsort()[::-1]`) leaves open"""
    b = torch.from_numpy(dets[:, :4].astype(np.float32))
    iou = OF.bbox_overlaps(b, b).numpy()
    same = (dets[:, 4][:, None] == dets[:, 4][None, :]) & ~np.eye(dets.shape[0], dtype=bool)
    return not (same & (iou > thr - 1e-3)).any()


def _canonical(scores, boxes, cls):
    order = np.lexsort((boxes[:, 3], boxes[:, 2], boxes[:, 1], boxes[:, 0], cls, -scores.astype(np.float64)))
    return scores[order], boxes[order], cls[order]


@pytest.mark.parametrize('kind', ['n37', 'none'])
def test_maskroi_chain_equals_oracle_mask_roi(dev, kind):
    """vps_maskroi_select -> vps_nms_batched (count read from m_out on the device) -> vps_maskroi_finish, wired as
    panoptic_ops.MaskROI.forward wires them, against oracle.fusetrack.mask_roi: scores and classes exact, boxes within box_bound.
    Detections of equal score are compared in a canonical order (the oracle's order among them is numpy's unstable argsort)."""
    lib = hip.load()
    rois, delta, prob = _select_inputs(kind)
    if kind == 'n37':
        # classes of one roi get distinct scores (their boxes overlap): equal scores only between rois
        rg = np.random.default_rng(5)
        for r in range(37):
            prob[r, 1:] = (rg.permutation(17)[:8] / 16.0).astype(np.float32)
        prob[7:12, 2] = np.float32(0.6)
    (wd, _, wm), tol = box_bound(rois, delta, prob, None, 'maskroi chain %s' % kind)
    nms_thr, max_det, kcap = 0.5, 100, 256
    if kind == 'n37':
        assert wm[0] > 60 and np.unique(wd[:, 4]).size < wm[0] and _tied_pairs_do_not_suppress(wd, nms_thr)
    cfg = dict(OF.CFG, bbox_reg_weights=WTS, max_det=max_det, mask_roi=dict(score_thresh=THR, nms_thresh=nms_thr))
    sc, boxes, cls = OF.mask_roi(torch.from_numpy(rois), torch.from_numpy(delta), torch.from_numpy(prob), np.array([[IM_HW[0], IM_HW[1], 1.]], np.float32),
                                 cfg, NC)
    n = rois.shape[0]
    cap = n * (NC - 1)
    d = [_up(dev, a) for a in (rois, delta, prob)]
    dets = _full(dev, (cap, 5)); cand = _full(dev, (cap,), torch.int32); mcnt = _full(dev, (4,), torch.int32)
    cb = (cap + 63) // 64
    mask = torch.empty(cap * cb, dtype=torch.int64, device=dev)
    keep = _full(dev, (cap,), torch.int32); nkeep = _full(dev, (1,), torch.int32)
    res = _full(dev, (8 + 8 * kcap,))
    wts = (ctypes.c_float * 4)(*WTS)
    hip.check(lib.vps_maskroi_select(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), n, None, NC, THR, wts, IM_HW[0], IM_HW[1], hip.ptr(dets), hip.ptr(cand),
                                     hip.ptr(mcnt), _sp()), 'vps_maskroi_select')
    hip.check(lib.vps_nms_batched(hip.ptr(dets), 1, cap, hip.ptr(mcnt), nms_thr, hip.ptr(mask), hip.ptr(keep), hip.ptr(nkeep), _sp()), 'vps_nms_batched')
    hip.check(lib.vps_maskroi_finish(hip.ptr(dets), hip.ptr(cand), hip.ptr(mcnt), hip.ptr(keep), hip.ptr(nkeep), NC, max_det, kcap, hip.ptr(res), _sp()),
              'vps_maskroi_finish')
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    K = int(got[0])
    assert K == sc.shape[0] and got[:8].tolist() == [K, wm[0], int(nkeep.item()), 0, n, S, S, S]
    if kind == 'n37':
        assert 1 < K < wm[0], 'the NMS suppresses something'
    rows = got[8:8 + 8 * K].reshape(K, 8)
    assert (got[8 + 8 * K:] == S).all() and (rows[:, 0] == 0).all()
    gs, gb, gcl = _canonical(rows[:, 5], rows[:, 1:5], rows[:, 6].astype(np.int64))
    ws, wb, wcl = _canonical(sc.numpy(), boxes.numpy()[:, 1:], cls.numpy())
    assert np.array_equal(gs, ws) and np.array_equal(gcl, wcl)
    assert float(np.abs(gb.astype(np.float64) - wb).max()) <= tol
    assert np.array_equal(rows[:, 5], np.sort(rows[:, 5])[::-1]), 'descending scores'
    if K > 1:
        assert np.array_equal(rows[:, 6], rows[:, 7].astype(np.int64) % (NC - 1) + 1)


# ------------------------------------------------------------------------------------------------ vps_rpn_collect
COLLECT_CASES = {
    # name: (nmax, nkeep per level, nms_post, max_num)
    'one_level_fewer_than_max_num': (50, [20], 100, 30),
    'three_levels_nms_post_bites': (100, [60, 0, 45], 50, 70),
    'five_levels': (64, [30, 10, 0, 63, 5], 40, 200),
    'five_levels_cut': (64, [30, 10, 0, 63, 5], 40, 64),
    'all_empty': (16, [0, 0, 0], 16, 40),
    'full_sort': (1024, [1024] * 8, 1024, 2000),
}


@pytest.mark.parametrize('name', list(COLLECT_CASES))
def test_rpn_collect(dev, name):
    """rows and count exact against rpn_head.py:94-104 restated. Scores are POSITIVE, as the sigmoid outputs they are in the pipeline:
    the kernel sorts the float32 bit patterns as unsigned integers, which orders positive floats only. Scores in steps of 1/64, so
    equal scores cross levels: the earlier position of the concatenation comes first."""
    nmax, nkeep, nms_post, max_num = COLLECT_CASES[name]
    nlv = len(nkeep)
    rg = np.random.default_rng(nmax + nlv)
    boxes = rg.uniform(0, 1000, (nlv, nmax, 5)).astype(np.float32)
    boxes[:, :, 4] = -np.sort(-rg.integers(1, 64, (nlv, nmax)) / 64.0, axis=1)          # descending per level, positive
    keep = np.full((nlv, nmax), nmax - 1, dtype=np.int32)        # entries past nkeep point at a valid row, they must not be used
    for l, k in enumerate(nkeep):
        keep[l, :k] = np.arange(nmax) if k == nmax else np.sort(rg.permutation(nmax)[:k])
        assert k in (0, nmax) or not np.array_equal(keep[l, :k], np.arange(k))
    want, n = R.rpn_collect(boxes, keep, nkeep, nms_post, max_num)
    total = sum(min(k, nms_post) for k in nkeep)
    assert n == min(total, max_num) and (name != 'full_sort' or total == 8192)
    if n > 1:
        assert np.unique(want[:n, 4]).size < n, 'ties'
    d = [_up(dev, a) for a in (boxes, keep, np.array(nkeep, np.int32))]
    out = _full(dev, (max_num + 2, 5)); n_out = _full(dev, (2,), torch.int32)
    hip.check(hip.load().vps_rpn_collect(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), nlv, nmax, nms_post, max_num, hip.ptr(out), hip.ptr(n_out), _sp()),
              'vps_rpn_collect')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert n_out.cpu().tolist() == [n, S]
    assert np.array_equal(got[:max_num, 4], want[:, 4])
    assert np.array_equal(got[:max_num], want), 'first differing row %s' % np.nonzero((got[:max_num] != want).any(1))[0][:3]
    assert (got[max_num:] == S).all()


def test_rpn_collect_refuses_more_than_the_sort_buffer(dev):
    """nlv * min(nms_post, nmax) > 8192: a non-zero return and no launch"""
    nlv, nmax = 8, 1025
    boxes = torch.ones(nlv, nmax, 5, device=dev); keep = torch.zeros(nlv, nmax, dtype=torch.int32, device=dev)
    nkeep = torch.ones(nlv, dtype=torch.int32, device=dev)
    out = _full(dev, (10, 5)); n_out = _full(dev, (1,), torch.int32)
    lib = hip.load()
    assert lib.vps_rpn_collect(hip.ptr(boxes), hip.ptr(keep), hip.ptr(nkeep), nlv, nmax, 1025, 10, hip.ptr(out), hip.ptr(n_out), _sp()) != 0
    assert lib.vps_rpn_collect(hip.ptr(boxes), hip.ptr(keep), hip.ptr(nkeep), 9, 16, 16, 10, hip.ptr(out), hip.ptr(n_out), _sp()) != 0
    torch.cuda.synchronize()
    assert (out.cpu() == S).all() and n_out.item() == S
    hip.check(lib.vps_rpn_collect(hip.ptr(boxes), hip.ptr(keep), hip.ptr(nkeep), nlv, nmax, 1024, 10, hip.ptr(out), hip.ptr(n_out), _sp()), 'at the limit')
    torch.cuda.synchronize()
    assert n_out.item() == 8 and (out.cpu()[:8] == 1).all() and (out.cpu()[8:] == 0).all()


# ------------------------------------------------------------------------------------------------ vps_pan_instances
FIELDS = [f for f, _ in hip.PanInst._fields_]


def _pan_rows():
    rg = np.random.default_rng(11)
    n = 12
    rows = np.zeros((n, 8), dtype=np.float32)
    rows[:, 1] = rg.uniform(0, 8, n); rows[:, 2] = rg.uniform(0, 8, n)
    rows[:, 3] = np.resize([10.5, 11.5, 12.49, 12.51], n); rows[:, 4] = np.resize([11.5, 12.51, 10.5, 12.49, 13.5], n)
    rows[:, 5] = np.sort(rg.uniform(0.6, 1, n))[::-1]
    rows[:, 6] = rg.integers(1, 9, n); rows[5, 6] = 0
    rows[:, 7] = rg.integers(0, 1000, n)
    return rows


@pytest.mark.parametrize('case', ['mixed', 'all_kept', 'nothing_kept', 'dummy_row'])
def test_pan_instances(dev, case):
    """the instance table (read back through hip.PanInst), the kept list and the count record, exact: kept detections in walk order,
    the SegTerm crop with half-integer x2 / y2 (rintf and numpy's round: both half to even), a class mapping that is not the
    identity, the nothing-kept record (keep = [0], empty paste box) and the dummy-row call"""
    cm = {c: 19 - c for c in range(1, 9)}
    nclass = 9
    cm_c = (ctypes.c_int32 * nclass)(*[cm.get(c, 0) for c in range(nclass)])
    if case == 'dummy_row':
        rows = np.array([[0, 0, 0, 0, 0, 1, 0, 0]], dtype=np.float32)
        order = flags = tbox = None
    else:
        rows = _pan_rows()
        rg = np.random.default_rng(3)
        order = rg.permutation(12).astype(np.int32)
        flags = {'mixed': (rg.random(12) < 0.5).astype(np.int32), 'all_kept': np.ones(12, np.int32), 'nothing_kept': np.zeros(12, np.int32)}[case]
        if case == 'mixed':
            flags[list(order).index(5)] = 1                                             # the class-0 row is among the kept
            assert 0 < flags.sum() < 12
        tbox = rg.integers(-20, 2000, (12, 4)).astype(np.int32)
    n = rows.shape[0]
    winst, wkeep, wk = R.pan_instances(order, flags, rows, tbox, cm)
    k = wk[0]
    sz = ctypes.sizeof(hip.PanInst)
    assert sz == 40
    rows_d = _up(dev, rows)
    d = [None if a is None else _up(dev, a) for a in (order, flags, tbox)]
    inst = torch.full(((n + 2) * sz,), 0x5a, dtype=torch.uint8, device=dev)
    keep_d = _full(dev, (n + 2,), torch.int32); kinfo = _full(dev, (4,), torch.int32)
    hip.check(hip.load().vps_pan_instances(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(rows_d), hip.ptr(d[2]), n, cm_c, nclass, hip.ptr(inst), hip.ptr(keep_d),
                                           hip.ptr(kinfo), _sp()), 'vps_pan_instances')
    torch.cuda.synchronize()
    raw = inst.cpu().numpy().tobytes()
    table = (hip.PanInst * k).from_buffer_copy(raw[:k * sz])
    assert [[getattr(t, f) for f in FIELDS] for t in table] == winst.tolist()
    assert raw[k * sz:] == b'\x5a' * ((n + 2 - k) * sz)
    assert keep_d.cpu().tolist() == wkeep.tolist() + [S] * (n + 2 - k)
    assert kinfo.cpu().tolist() == wk + [S, S]
    if case == 'nothing_kept':
        assert wkeep.tolist() == [0] and wk == [1, 0] and winst[0, 5:9].tolist() == [0, 0, -1, -1]
    if case == 'all_kept':
        assert sorted(set(winst[:, 2].tolist())) == [0, 11, 13, 14] and wkeep.tolist() == order.tolist()   # round(10.5) = 10, round(11.5) = 12, 12.49 -> 12, 12.51 -> 13; 0: class 0


# ------------------------------------------------------------------------------------------------ vps_frame_tail
@pytest.mark.parametrize('nslots,with_ids,with_mem,K', [(300, True, True, 5), (0, False, False, 16), (300, False, True, 16), (0, True, False, 0)])
def test_frame_tail(dev, nslots, with_ids, with_mem, K):
    """the end-of-frame record, whole: the status maximum over 300 slots (largest value in the last one, larger ones behind it
    unread), ids / mem_count NULL, K = kcap; words 6, 7 and the rows past K untouched"""
    kcap = 16
    rg = np.random.default_rng(nslots + K)
    kinfo = np.array([K, 1, 4, 9], np.int32)
    keep = rg.integers(0, 100, kcap + 4).astype(np.int32); ids = rg.integers(0, 5000, kcap + 4).astype(np.int32)
    st = rg.integers(0, 3, 310).astype(np.int32); st[299] = 6; st[300:] = 50
    tail0 = np.full(8 + 2 * kcap + 4, S, np.int32)
    want = R.frame_tail(tail0, kinfo, keep, ids if with_ids else None, 1234 if with_mem else None, st, nslots, K, kcap)
    assert want[5] == (6 if nslots else 0)
    d = [_up(dev, a) for a in (kinfo, keep, ids, np.array([1234], np.int32), st, tail0)]
    hip.check(hip.load().vps_frame_tail(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]) if with_ids else None, hip.ptr(d[3]) if with_mem else None,
                                        hip.ptr(d[4]) if nslots else None, nslots, K, kcap, hip.ptr(d[5]), _sp()), 'vps_frame_tail')
    torch.cuda.synchronize()
    assert d[5].cpu().tolist() == want.tolist()
