"""Plain restatement of the ternary census warp error (the contract in the docstring of vps_amd/flowphoto.py and in include/vps_hip.h,
DESIGN.md 6 row 3i), sharing no code with vps_amd or the kernel, twice: `flow_census_loop` is one Python loop over the pixels and their
48 neighbours, `flow_census` the same on whole arrays (what the larger tests can afford). The grey, the in-view rule, the bilinear sample
and the code differences are np.float32 operations of their own in the stated order; every count and decision after the codes is a
Python / int64 integer. The definition is the hard ternary census (Stein 2004) as UnFlow (Meister et al. 2018) uses it, restated from
memory; what pins it are the hand-derived answers of tests/test_flow_census.py.

    flow_census(cur, prev, flow, mask, thr, eps)  -> {'table' int64 [2,13], 'mask_out' uint8 [H,W], 'residual' uint8 [H,W], 'n' (pixels),
                                                      'd_w', 'n_w', 'd_s', 'n_s' int64 [H,W] (n_w, d_w: 0 where the pixel is not in view),
                                                      'in_view' bool [H,W]}
    flow_census_loop(.., in_place=False)          -> the same, pixel by pixel; in_place: mask_out is written into the mask's own array
    figures(table)                                -> the figures of the docstring, restated
"""
import numpy as np

F = np.float32
R = 3
CELLS = 13
LEVELS = (10, 25, 50)


def _clamp(i, n):
    return min(max(int(i), 0), n - 1)


def _check(cur, prev, flow, mask, thr, eps):
    cur, prev, flow = np.asarray(cur), np.asarray(prev), np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    H, W = flow.shape[:2]
    assert cur.dtype == prev.dtype == np.uint8 and cur.shape == prev.shape == (H, W, 3)
    assert mask is None or (mask.dtype == np.uint8 and mask.shape == (H, W))
    assert int(thr) == thr and 0 <= thr <= 100 and np.isfinite(F(eps)) and F(eps) >= 0
    return cur, prev, flow, H, W, int(thr), F(eps)


def grey(img):
    """299 R + 587 G + 114 B of a BGR uint8 image as float32 (exact: at most 255 000)"""
    i = img.astype(np.int64)
    return (299 * i[..., 2] + 587 * i[..., 1] + 114 * i[..., 0]).astype(F)


def _code(d, eps):
    return 1 if d > eps else (-1 if d < -eps else 0)


def _tally(table, g, in_view, d_w, n_w, d_s, n_s, thr):
    """one pixel into row g; -> (scored, flagged, residual)"""
    if not in_view:
        table[g, 11] += 1
        return False, False, 0
    if n_w == 0:
        table[g, 12] += 1
        return False, False, 0
    row = table[g]
    row[0] += 1
    row[1] += d_w; row[2] += n_w; row[3] += d_s; row[4] += n_s
    for i, lv in enumerate(LEVELS):
        row[5 + i] += 100 * d_w > lv * n_w
    row[8] += d_w * n_s < d_s * n_w
    row[9] += d_w * n_s > d_s * n_w
    flagged = 100 * d_w > thr * n_w
    row[10] += flagged
    return True, flagged, (255 * d_w + n_w // 2) // n_w


def warp_loop(prev_grey, flow):
    """Wg as float32 [H,W] and the in-view map, pixel by pixel"""
    H, W = prev_grey.shape
    wg, inv = np.full((H, W), -1, dtype=F), np.zeros((H, W), dtype=bool)
    half, one = F(0.5), F(1)
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                u, v = flow[y, x, 0], flow[y, x, 1]
                sx, sy = F(x) + u, F(y) + v
                qx, qy = np.floor(sx + half), np.floor(sy + half)
                if not (qx >= F(0) and qx <= F(W - 1) and qy >= F(0) and qy <= F(H - 1)):
                    continue
                x0, y0 = np.floor(sx), np.floor(sy)
                wx, wy = sx - x0, sy - y0
                x1, y1 = x0 + one, y0 + one
                ix0, ix1, iy0, iy1 = _clamp(x0, W), _clamp(x1, W), _clamp(y0, H), _clamp(y1, H)
                g00, g01, g10, g11 = prev_grey[iy0, ix0], prev_grey[iy0, ix1], prev_grey[iy1, ix0], prev_grey[iy1, ix1]
                top = g00 + wx * (g01 - g00)
                bot = g10 + wx * (g11 - g10)
                s = top + wy * (bot - top)
                assert all(type(t) is np.float32 for t in (sx, qx, wx, x1, top, bot, s))
                wg[y, x], inv[y, x] = s, True
    return wg, inv


def flow_census_loop(cur, prev, flow, mask=None, thr=25, eps=2000.0, in_place=False):
    cur, prev, flow, H, W, thr, eps = _check(cur, prev, flow, mask, thr, eps)
    gc, gp = grey(cur), grey(prev)
    wg, inv = warp_loop(gp, flow)
    table = np.zeros((2, CELLS), dtype=np.int64)
    mask_out = mask if in_place else np.zeros((H, W), dtype=np.uint8)
    residual = np.zeros((H, W), dtype=np.uint8)
    maps = {k: np.zeros((H, W), dtype=np.int64) for k in ('d_w', 'n_w', 'd_s', 'n_s')}
    for y in range(H):
        for x in range(W):
            d_w = n_w = d_s = n_s = 0
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    qy, qx = y + dy, x + dx
                    if (dx == 0 and dy == 0) or not (0 <= qy < H and 0 <= qx < W):
                        continue
                    cc = _code(gc[qy, qx] - gc[y, x], eps)
                    assert type(gc[qy, qx] - gc[y, x]) is np.float32
                    n_s += 1
                    d_s += cc != _code(gp[qy, qx] - gp[y, x], eps)
                    if inv[y, x] and inv[qy, qx]:
                        n_w += 1
                        d_w += cc != _code(wg[qy, qx] - wg[y, x], eps)
            m = 0 if mask is None else int(mask[y, x])                           # read before mask_out[y, x] is written
            scored, flagged, res = _tally(table, 1 if m else 0, bool(inv[y, x]), d_w, n_w, d_s, n_s, thr)
            mask_out[y, x] = 2 if not inv[y, x] else (m if m else (3 if flagged else 0))
            residual[y, x] = res
            maps['d_w'][y, x], maps['n_w'][y, x], maps['d_s'][y, x], maps['n_s'][y, x] = d_w, n_w, d_s, n_s
    return dict(maps, table=table, mask_out=mask_out, residual=residual, n=H * W, in_view=inv)


def warp(prev_grey, flow):
    H, W = prev_grey.shape
    xs = np.arange(W, dtype=np.int64).astype(F)[None, :]
    ys = np.arange(H, dtype=np.int64).astype(F)[:, None]
    with np.errstate(all='ignore'):
        u, v = flow[..., 0], flow[..., 1]
        sx, sy = xs + u, ys + v
        qx, qy = np.floor(sx + F(0.5)), np.floor(sy + F(0.5))
        inv = (qx >= F(0)) & (qx <= F(W - 1)) & (qy >= F(0)) & (qy <= F(H - 1))
        x0, y0 = np.floor(sx), np.floor(sy)
        wx, wy = sx - x0, sy - y0
        x1, y1 = x0 + F(1), y0 + F(1)
        idx = lambda f, n: np.clip(np.where(inv, f, F(0)).astype(np.int64), 0, n - 1)        # no index from a float that is not in view
        ix0, ix1, iy0, iy1 = idx(x0, W), idx(x1, W), idx(y0, H), idx(y1, H)
        g00, g01, g10, g11 = prev_grey[iy0, ix0], prev_grey[iy0, ix1], prev_grey[iy1, ix0], prev_grey[iy1, ix1]
        top = g00 + wx * (g01 - g00)
        bot = g10 + wx * (g11 - g10)
        s = top + wy * (bot - top)
        assert all(a.dtype == np.float32 for a in (sx, qx, wx, x1, top, bot, s))
    return np.where(inv, s, F(-1)).astype(F), inv


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies in the image, else fill"""
    H, W = a.shape
    b = np.full((H, W), fill, dtype=a.dtype)
    ys0, ys1, xs0, xs1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        b[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return b


def _codes(a, q, eps):
    with np.errstate(all='ignore'):
        d = q - a
        assert d.dtype == np.float32
        return (d > eps).astype(np.int8) - (d < -eps).astype(np.int8)


def flow_census(cur, prev, flow, mask=None, thr=25, eps=2000.0):
    cur, prev, flow, H, W, thr, eps = _check(cur, prev, flow, mask, thr, eps)
    gc, gp = grey(cur), grey(prev)
    wg, inv = warp(gp, flow)
    d_w, n_w, d_s, n_s = (np.zeros((H, W), dtype=np.int64) for _ in range(4))
    inside = np.ones((H, W), dtype=bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx == 0 and dy == 0:
                continue
            there = _shifted(inside, dy, dx, False)
            cc = _codes(gc, _shifted(gc, dy, dx, F(0)), eps)
            n_s += there
            d_s += there & (cc != _codes(gp, _shifted(gp, dy, dx, F(0)), eps))
            both = there & inv & _shifted(inv, dy, dx, False)
            n_w += both
            d_w += both & (cc != _codes(wg, _shifted(wg, dy, dx, F(0)), eps))
    m = np.zeros((H, W), dtype=np.uint8) if mask is None else mask
    scored = inv & (n_w >= 1)
    flagged = scored & (100 * d_w > thr * n_w)
    table = np.zeros((2, CELLS), dtype=np.int64)
    for g in (0, 1):
        grp = (m != 0) == (g == 1)
        sel = grp & scored
        row = table[g]
        row[0], row[1], row[2], row[3], row[4] = sel.sum(), d_w[sel].sum(), n_w[sel].sum(), d_s[sel].sum(), n_s[sel].sum()
        for i, lv in enumerate(LEVELS):
            row[5 + i] = (sel & (100 * d_w > lv * n_w)).sum()
        row[8], row[9] = (sel & (d_w * n_s < d_s * n_w)).sum(), (sel & (d_w * n_s > d_s * n_w)).sum()
        row[10], row[11], row[12] = (grp & flagged).sum(), (grp & ~inv).sum(), (grp & inv & (n_w == 0)).sum()
    mask_out = np.where(inv, np.where(m != 0, m, np.where(flagged, 3, 0)), 2).astype(np.uint8)
    residual = np.where(scored, (255 * d_w + n_w // 2) // np.maximum(n_w, 1), 0).astype(np.uint8)
    return {'table': table, 'mask_out': mask_out, 'residual': residual, 'n': H * W, 'd_w': d_w, 'n_w': n_w, 'd_s': d_s, 'n_s': n_s, 'in_view': inv}


def _group(c):
    q = lambda a, b: float(a) / float(b) if b else 0.0
    n = int(c[0])
    f = {'n': n, 'ce_warp': q(c[1], c[2]), 'ce_static': q(c[3], c[4]), 'above_10': q(c[5], n), 'above_25': q(c[6], n), 'above_50': q(c[7], n),
         'helped': q(c[8], n), 'hurt': q(c[9], n), 'flagged': int(c[10]), 'flagged_share': q(c[10], n), 'outside': int(c[11]), 'alone': int(c[12])}
    f['ratio'] = q(f['ce_warp'], f['ce_static'])
    f['gain'] = f['ce_static'] - f['ce_warp']
    tot = n + f['outside'] + f['alone']
    f['outside_share'] = q(f['outside'], tot)
    return f


def figures(table):
    t = np.asarray(table, dtype=np.int64).reshape(2, CELLS)
    return {'visible': _group(t[0]), 'masked': _group(t[1]), 'all': _group(t[0] + t[1])}
