"""Plain per-pixel restatement of the forward-backward occlusion check (the contract in the docstring of vps_amd/tc.py and in
include/vps_hip.h), sharing no code with vps_amd/tc.py or the kernel, twice: `occlusion_loop` is one Python loop over the pixels, `occlusion` the same on
whole np.float32 arrays (what the larger tests can afford); in both every operation is an np.float32 operation of its own in the stated
order, and tests/test_flow_occ.py holds them against each other. The definition itself is restated from memory of Sundaram et al. (ECCV 2010) as used by
UnFlow (Meister et al., AAAI 2018); what pins it are the hand-derived answers of tests/test_flow_occ.py.

    occlusion(fwd, back, alpha, beta)               -> (codes uint8 [H,W]: 0 visible, 1 occluded, 2 not in view; counts int64 [3])
    occlusion_loop(fwd, back, alpha, beta)          -> the same, pixel by pixel
    masked_pair_tables(prev, cur, flow, mask, ...)  -> the TC tables of one pair with the masked pixels skipped, the masked count and
                                                       the inconsistency map with code 4 (on top of tc_restate.pair_tables)
    masked_video_tables(maps, flows, backs, ...)    -> (the video's tables, the per-pair list), masks from `occlusion`
"""
import numpy as np

import tc_restate as R

F = np.float32
NAMES = R.NAMES + ('masked',)


def _clamp(i, n):
    return min(max(int(i), 0), n - 1)


def occlusion(fwd, back, alpha=0.01, beta=0.5):
    fwd, back = np.asarray(fwd), np.asarray(back)
    assert fwd.dtype == back.dtype == np.float32 and fwd.shape == back.shape and fwd.ndim == 3 and fwd.shape[2] == 2
    H, W = fwd.shape[:2]
    alpha, beta = F(alpha), F(beta)
    xs = np.arange(W, dtype=np.int64).astype(F)[None, :]
    ys = np.arange(H, dtype=np.int64).astype(F)[:, None]
    with np.errstate(all='ignore'):
        u, v = fwd[..., 0], fwd[..., 1]
        sx, sy = xs + u, ys + v
        qx, qy = np.floor(sx + F(0.5)), np.floor(sy + F(0.5))
        inview = (qx >= F(0)) & (qx <= F(W - 1)) & (qy >= F(0)) & (qy <= F(H - 1))
        x0, y0 = np.floor(sx), np.floor(sy)
        wx, wy = sx - x0, sy - y0
        x1, y1 = x0 + F(1), y0 + F(1)
        idx = lambda f, n: np.clip(np.where(inview, f, F(0)).astype(np.int64), 0, n - 1)     # no index from a float that is not in view
        ix0, ix1, iy0, iy1 = idx(x0, W), idx(x1, W), idx(y0, H), idx(y1, H)
        bt = []
        for c in range(2):
            b = back[..., c]
            b00, b01, b10, b11 = b[iy0, ix0], b[iy0, ix1], b[iy1, ix0], b[iy1, ix1]
            top = b00 + wx * (b01 - b00)
            bot = b10 + wx * (b11 - b10)
            bt.append(top + wy * (bot - top))
        dx, dy = u + bt[0], v + bt[1]
        d2 = dx * dx + dy * dy
        m = (u * u + v * v) + (bt[0] * bt[0] + bt[1] * bt[1])
        thr = alpha * m + beta
        assert all(a.dtype == np.float32 for a in (sx, qx, wx, x1, bt[0], d2, m, thr))
        codes = np.where(inview, np.where(d2 <= thr, 0, 1), 2).astype(np.uint8)
    return codes, np.bincount(codes.reshape(-1), minlength=3).astype(np.int64)


def occlusion_loop(fwd, back, alpha=0.01, beta=0.5):
    fwd, back = np.asarray(fwd), np.asarray(back)
    assert fwd.dtype == back.dtype == np.float32 and fwd.shape == back.shape and fwd.ndim == 3 and fwd.shape[2] == 2
    H, W = fwd.shape[:2]
    alpha, beta = F(alpha), F(beta)
    codes = np.zeros((H, W), dtype=np.uint8)
    counts = np.zeros(3, dtype=np.int64)
    half, one = F(0.5), F(1)
    with np.errstate(all='ignore'):
        for y in range(H):
            for x in range(W):
                u, v = fwd[y, x, 0], fwd[y, x, 1]
                sx, sy = F(x) + u, F(y) + v
                qx, qy = np.floor(sx + half), np.floor(sy + half)
                if not (qx >= F(0) and qx <= F(W - 1) and qy >= F(0) and qy <= F(H - 1)):
                    codes[y, x] = 2
                    counts[2] += 1
                    continue
                x0, y0 = np.floor(sx), np.floor(sy)
                wx, wy = sx - x0, sy - y0
                x1, y1 = x0 + one, y0 + one
                ix0, ix1, iy0, iy1 = _clamp(x0, W), _clamp(x1, W), _clamp(y0, H), _clamp(y1, H)
                bt = []
                for c in range(2):
                    b00, b01, b10, b11 = back[iy0, ix0, c], back[iy0, ix1, c], back[iy1, ix0, c], back[iy1, ix1, c]
                    top = b00 + wx * (b01 - b00)
                    bot = b10 + wx * (b11 - b10)
                    bt.append(top + wy * (bot - top))
                dx, dy = u + bt[0], v + bt[1]
                d2 = dx * dx + dy * dy
                m = (u * u + v * v) + (bt[0] * bt[0] + bt[1] * bt[1])
                thr = alpha * m + beta
                assert all(type(t) is np.float32 for t in (sx, qx, wx, x1, bt[0], d2, m, thr))
                code = 0 if bool(d2 <= thr) else 1
                codes[y, x] = code
                counts[code] += 1
    return codes, counts


def masked_pair_tables(prev, cur, flow, mask, seg_class, C, id_channel, keys):
    """The TC tables of the pixels that are not masked, by tc_restate.pair_tables itself: the in-view pixels with mask != 0 are left
    out, the others are laid out as one row - cur's pixel beside the pixel of prev the flow leads to, under a zero flow, or under a flow
    that leaves the row where the pixel is not in view - and counted as tc_restate counts. 'masked' [1] is the number left out,
    'map' has code 4 there."""
    prev, cur, mask = np.asarray(prev), np.asarray(cur), np.asarray(mask)
    H, W = cur.shape[:2]
    assert mask.shape == (H, W) and mask.dtype == np.uint8 and prev.shape == cur.shape
    inview, ix, iy = R.warp(flow)
    drop = inview & (mask != 0)
    ys, xs = np.nonzero(~drop)
    N = len(ys)
    out = {'map': np.full((H, W), 4, dtype=np.uint8), 'masked': np.array([int(drop.sum())], dtype=np.int64)}
    if N == 0:
        n = len(keys)
        out.update(conf=np.zeros((C + 1, C + 1), dtype=np.int64), prev_size=np.zeros(n, dtype=np.int64), cur_size=np.zeros(n, dtype=np.int64),
                   same=np.zeros(n, dtype=np.int64), misc=np.zeros(2, dtype=np.int64))
        return out
    row_flow = np.zeros((1, N, 2), dtype=np.float32)
    row_flow[0, ~inview[ys, xs], 0] = N + 5
    tab = R.pair_tables(prev[iy[ys, xs], ix[ys, xs]][None], cur[ys, xs][None], row_flow, seg_class, C, id_channel, keys)
    out.update({k: tab[k] for k in R.NAMES})
    out['map'][ys, xs] = tab['map'][0]
    return out


def masked_video_tables(maps, flows, backs, seg_class, C, id_channel, keys, alpha=0.01, beta=0.5):
    """(the video's tables = the sum over its pairs, [the tables of pair 1, 2, ..]); flows[t] and backs[t] belong to (maps[t-1], maps[t])"""
    pairs = []
    for t in range(1, len(maps)):
        codes, _ = occlusion(flows[t], backs[t], alpha, beta)
        pairs.append(masked_pair_tables(maps[t - 1], maps[t], flows[t], codes, seg_class, C, id_channel, keys))
    total = {k: sum(p[k] for p in pairs) for k in NAMES}
    return total, pairs


def flat(tab):
    """the six tables in the order they lie in one block"""
    return np.concatenate([np.asarray(tab[k]).reshape(-1) for k in NAMES])
