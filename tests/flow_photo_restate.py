"""Plain per-pixel restatement of the photometric warp error (the contract in the docstring of vps_amd/flowphoto.py and in
include/vps_hip.h), sharing no code with vps_amd/flowphoto.py or the kernel, twice: `flow_photo_loop` is one Python loop over the pixels,
`flow_photo` the same on whole arrays (what the larger tests can afford). In both, steps 1 - 3 are np.float32 operations of their own in
the stated order, step 4 is float64, and the sums are `math.fsum` of the per-pixel terms; tests/test_flow_photo.py holds the two against
each other. The definition itself is the warp / interpolation error Middlebury reports beside EPE, restated from memory; what pins it
are the hand-derived answers of tests/test_flow_photo.py.

    flow_photo(cur, prev, flow, mask, thr)        -> {'counts' int64 [21], 'sums' float64 [4] (fsum), 'abs' float64 [4] (the fsum of the
                                                      terms' magnitudes: the terms are non-negative, so the sums themselves), 'n' (pixels),
                                                      'mask_out' uint8 [H,W], 'residual' uint8 [H,W]}
    flow_photo_loop(.., in_place=False)           -> the same, pixel by pixel; in_place: mask_out is written into the mask's own array
    figures(counts, sums)                         -> the figures of the docstring, restated
"""
import math

import numpy as np

F = np.float32
D = np.float64
LEVELS = (4.0, 8.0, 16.0, 32.0)


def _clamp(i, n):
    return min(max(int(i), 0), n - 1)


def _check(cur, prev, flow, mask):
    cur, prev, flow = np.asarray(cur), np.asarray(prev), np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    H, W = flow.shape[:2]
    assert cur.dtype == prev.dtype == np.uint8 and cur.shape == prev.shape == (H, W, 3)
    assert mask is None or (mask.dtype == np.uint8 and mask.shape == (H, W))
    return cur, prev, flow, H, W


def flow_photo_loop(cur, prev, flow, mask=None, thr=16.0, in_place=False):
    cur, prev, flow, H, W = _check(cur, prev, flow, mask)
    thr = D(F(thr))                                                              # the threshold travels as a float
    counts = np.zeros(21, dtype=np.int64)
    terms = [[], [], [], []]
    mask_out = mask if in_place else np.zeros((H, W), dtype=np.uint8)
    residual = np.zeros((H, W), dtype=np.uint8)
    half, one = F(0.5), F(1)
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                u, v = flow[y, x, 0], flow[y, x, 1]
                sx, sy = F(x) + u, F(y) + v
                qx, qy = np.floor(sx + half), np.floor(sy + half)
                if not (qx >= F(0) and qx <= F(W - 1) and qy >= F(0) and qy <= F(H - 1)):
                    counts[20] += 1
                    mask_out[y, x] = 2
                    continue
                m = 0 if mask is None else int(mask[y, x])                       # read before mask_out[y, x] is written
                g = 1 if m else 0
                x0, y0 = np.floor(sx), np.floor(sy)
                wx, wy = sx - x0, sy - y0
                x1, y1 = x0 + one, y0 + one
                ix0, ix1, iy0, iy1 = _clamp(x0, W), _clamp(x1, W), _clamp(y0, H), _clamp(y1, H)
                dw = []
                a_s = q_s = 0
                for c in range(3):
                    b00, b01, b10, b11 = F(prev[iy0, ix0, c]), F(prev[iy0, ix1, c]), F(prev[iy1, ix0, c]), F(prev[iy1, ix1, c])
                    top = b00 + wx * (b01 - b00)
                    bot = b10 + wx * (b11 - b10)
                    s = top + wy * (bot - top)
                    assert all(type(t) is np.float32 for t in (sx, qx, wx, x1, top, bot, s))
                    dw.append(D(s) - D(cur[y, x, c]))
                    d = int(prev[y, x, c]) - int(cur[y, x, c])
                    a_s += abs(d)
                    q_s += d * d
                aw = (abs(dw[0]) + abs(dw[1])) + abs(dw[2])
                qw = (dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]
                e = aw / D(3.0)
                assert type(aw) is np.float64 and type(qw) is np.float64 and type(e) is np.float64
                flagged = bool(e > thr)
                k = 10 * g
                counts[k] += 1
                counts[k + 1] += flagged
                counts[k + 2] += a_s
                counts[k + 3] += q_s
                for i, lv in enumerate(LEVELS):
                    counts[k + 4 + i] += bool(e > D(lv))
                counts[k + 8] += bool(aw < D(a_s))
                counts[k + 9] += bool(aw > D(a_s))
                terms[2 * g].append(float(aw))
                terms[2 * g + 1].append(float(qw))
                mask_out[y, x] = m if m else (3 if flagged else 0)
                residual[y, x] = min(255, int(math.floor(e + D(0.5))))
    sums = np.array([math.fsum(t) for t in terms], dtype=np.float64)
    return {'counts': counts, 'sums': sums, 'abs': sums.copy(), 'n': H * W, 'mask_out': mask_out, 'residual': residual}


def flow_photo(cur, prev, flow, mask=None, thr=16.0):
    cur, prev, flow, H, W = _check(cur, prev, flow, mask)
    thr = D(F(thr))
    xs = np.arange(W, dtype=np.int64).astype(F)[None, :]
    ys = np.arange(H, dtype=np.int64).astype(F)[:, None]
    with np.errstate(all='ignore'):
        u, v = flow[..., 0], flow[..., 1]
        sx, sy = xs + u, ys + v
        qx, qy = np.floor(sx + F(0.5)), np.floor(sy + F(0.5))
        inview = (qx >= F(0)) & (qx <= F(W - 1)) & (qy >= F(0)) & (qy <= F(H - 1))
        x0, y0 = np.floor(sx), np.floor(sy)
        wx, wy = sx - x0, sy - y0
        x1, y1 = x0 + F(1), y0 + F(1)
        idx = lambda f, n: np.clip(np.where(inview, f, F(0)).astype(np.int64), 0, n - 1)     # no index from a float that is not in view
        ix0, ix1, iy0, iy1 = idx(x0, W), idx(x1, W), idx(y0, H), idx(y1, H)
        dw = []
        for c in range(3):
            b = prev[..., c].astype(F)
            b00, b01, b10, b11 = b[iy0, ix0], b[iy0, ix1], b[iy1, ix0], b[iy1, ix1]
            top = b00 + wx * (b01 - b00)
            bot = b10 + wx * (b11 - b10)
            s = top + wy * (bot - top)
            assert all(a.dtype == np.float32 for a in (sx, qx, wx, x1, top, bot, s))
            dw.append(s.astype(D) - cur[..., c].astype(D))
        aw = (np.abs(dw[0]) + np.abs(dw[1])) + np.abs(dw[2])
        qw = (dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]
        e = aw / D(3.0)
        assert aw.dtype == qw.dtype == e.dtype == np.float64
    d = prev.astype(np.int64) - cur.astype(np.int64)
    a_s, q_s = np.abs(d).sum(axis=2), (d * d).sum(axis=2)
    m = np.zeros((H, W), dtype=np.uint8) if mask is None else mask
    flagged = inview & (e > thr)
    counts = np.zeros(21, dtype=np.int64)
    sums = np.zeros(4, dtype=np.float64)
    for g in (0, 1):
        sel = inview & ((m != 0) == (g == 1))
        k = 10 * g
        counts[k], counts[k + 1], counts[k + 2], counts[k + 3] = sel.sum(), (sel & flagged).sum(), a_s[sel].sum(), q_s[sel].sum()
        for i, lv in enumerate(LEVELS):
            counts[k + 4 + i] = (sel & (e > D(lv))).sum()
        counts[k + 8], counts[k + 9] = (sel & (aw < a_s.astype(D))).sum(), (sel & (aw > a_s.astype(D))).sum()
        sums[2 * g], sums[2 * g + 1] = math.fsum(aw[sel].tolist()), math.fsum(qw[sel].tolist())
    counts[20] = (~inview).sum()
    mask_out = np.where(inview, np.where(m != 0, m, np.where(flagged, 3, 0)), 2).astype(np.uint8)
    residual = np.where(inview, np.minimum(255, np.floor(np.where(inview, e, 0.0) + D(0.5))), 0).astype(np.uint8)
    return {'counts': counts, 'sums': sums, 'abs': sums.copy(), 'n': H * W, 'mask_out': mask_out, 'residual': residual}


def _group(c, s):
    n = int(c[0])
    q = lambda a, b: float(a) / float(b) if b else 0.0
    psnr = lambda mse: 10.0 * math.log10(65025.0 / mse) if mse > 0 else float('inf')
    mse_w, mse_s = q(s[1], 3 * n), q(c[3], 3 * n)
    f = {'n': n, 'flagged': int(c[1]), 'mae_warp': q(s[0], 3 * n), 'rms_warp': math.sqrt(mse_w), 'psnr_warp': psnr(mse_w), 'mae_static': q(c[2], 3 * n),
         'rms_static': math.sqrt(mse_s), 'psnr_static': psnr(mse_s), 'above_4': q(c[4], n), 'above_8': q(c[5], n), 'above_16': q(c[6], n),
         'above_32': q(c[7], n), 'helped': q(c[8], n), 'hurt': q(c[9], n), 'flagged_share': q(c[1], n)}
    f['ratio'] = q(f['mae_warp'], f['mae_static'])
    f['gain_db'] = f['psnr_warp'] - f['psnr_static'] if math.isfinite(f['psnr_warp']) and math.isfinite(f['psnr_static']) else 0.0
    return f


def figures(counts, sums):
    c, s = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
    out = {'visible': _group(c[0:10], s[0:2]), 'masked': _group(c[10:20], s[2:4]), 'all': _group(c[0:10] + c[10:20], s[0:2] + s[2:4]),
           'outside': int(c[20])}
    n = out['all']['n'] + out['outside']
    out['outside_share'] = out['outside'] / n if n else 0.0
    return out
