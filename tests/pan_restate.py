"""Plain numpy restatements of the reference's panoptic head HOST code, with the arithmetic type as a parameter: what the kernels of
vps_amd/csrc/pan_ops.hip are compared with (tests/test_pan_ops_gpu.py). Nothing here knows of tiles, instance lists or staging: the
logits are built densely, [nstuff + k, H, W], the way detectors/panoptic_fusetrack.py:588-597 builds them. tests/test_pan_restate.py
pins the float32 evaluation to the oracle (oracle/fusetrack.py, oracle/ops.py); the float64 evaluation is the yardstick of the margins.

An instance table is an int32 array [k, 10] in the field order of vps_pan_inst (hip.PanInst):
    sx0 sy0 sx1 sy1 seg_ch   the SegTerm crop [sy0:sy1, sx0:sx1] of channel seg_ch (utils/unary_logits.py:96-106)
    bx1 by1 bx2 by2 mask_idx the int32-truncated box the resized mask logits are pasted into (utils/mask_removal.py:59-85)"""
import numpy as np

SX0, SY0, SX1, SY1, SEG_CH, BX1, BY1, BX2, BY2, MASK_IDX = range(10)


def _lin_axis(n_out, n_in, up, dtype):
    """F.interpolate(bilinear, align_corners=False) along one axis: source coordinate scale * (dst + 0.5) - 0.5 clamped at 0, with
    scale = the float32 value of 1 / up -> (i0, i1, lambda1)"""
    scale = dtype(np.float32(1.0) / np.float32(up))
    s = scale * (np.arange(n_out).astype(dtype) + dtype(0.5)) - dtype(0.5)
    s = np.maximum(s, dtype(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (s - i0.astype(dtype)).astype(dtype)


def upsample(score_hwc, up, dtype):
    """upsnetFPN.py:81, F.interpolate(fcn_score, None, up, 'bilinear', align_corners=False): score [Hs, Ws, C] -> [C, up Hs, up Ws]"""
    s = np.ascontiguousarray(np.transpose(np.asarray(score_hwc), (2, 0, 1))).astype(dtype)
    Hs, Ws = s.shape[1:]
    y0, y1, ly = _lin_axis(Hs * up, Hs, up, dtype)
    x0, x1, lx = _lin_axis(Ws * up, Ws, up, dtype)
    one = dtype(1)
    hx, hy = (one - lx)[None, None, :], (one - ly)[None, :, None]
    lx, ly = lx[None, None, :], ly[None, :, None]
    top = hx * s[:, y0][:, :, x0] + lx * s[:, y0][:, :, x1]
    bot = hx * s[:, y1][:, :, x0] + lx * s[:, y1][:, :, x1]
    return (hy * top + ly * bot).astype(dtype)


def _cv_axis(dst, src):
    """cv2.resize(INTER_LINEAR) along one axis: the coordinate in double, cast to float32; edge taps clamped with zero weight"""
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    f[s < 0] = 0; s[s < 0] = 0
    f[s >= src - 1] = 0; s[s >= src - 1] = src - 1
    return s, np.minimum(s + 1, src - 1), f


def resize_linear(m, w, h, dtype):
    """cv2.resize(m, (w, h)) with the default INTER_LINEAR (utils/mask_removal.py:67): float32 coordinates used in `dtype`,
    the horizontal pass first, then the vertical one"""
    m = np.asarray(m).astype(dtype)
    x0, x1, fx = _cv_axis(int(w), m.shape[1])
    y0, y1, fy = _cv_axis(int(h), m.shape[0])
    fx, fy, one = fx.astype(dtype), fy.astype(dtype), dtype(1)
    rows = m[:, x0] * (one - fx)[None, :] + m[:, x1] * fx[None, :]
    return (rows[y0, :] * (one - fy)[:, None] + rows[y1, :] * fy[:, None]).astype(dtype)


def box_region(b, H, W):
    """utils/mask_removal.py:62-74 on an int32 box -> (w, h) of the resize target, the clipped region x0, x1, y0, y1 (may be empty)"""
    bx1, by1, bx2, by2 = (int(v) for v in b)
    return (max(bx2 - bx1 + 1, 1), max(by2 - by1 + 1, 1),
            max(bx1, 0), min(bx2 + 1, W), max(by1, 0), min(by2 + 1, H))


def pasted_logit(m, b, H, W, dtype):
    """the resized mask of box b inside its clipped region -> (array [y1 - y0, x1 - x0], x0, x1, y0, y1), or None when it is empty"""
    w, h, x0, x1, y0, y1 = box_region(b, H, W)
    if x1 <= x0 or y1 <= y0:
        return None
    bx1, by1 = int(b[0]), int(b[1])
    # (only the clipped rows and columns of the w x h image are evaluated: the passes are separable)
    mm = np.asarray(m).astype(dtype)
    cx0, cx1, fx = (a[x0 - bx1:x1 - bx1] for a in _cv_axis(w, mm.shape[1]))
    cy0, cy1, fy = (a[y0 - by1:y1 - by1] for a in _cv_axis(h, mm.shape[0]))
    fx, fy, one = fx.astype(dtype), fy.astype(dtype), dtype(1)
    rows = mm[:, cx0] * (one - fx)[None, :] + mm[:, cx1] * fx[None, :]
    return (rows[cy0, :] * (one - fy)[:, None] + rows[cy1, :] * fy[:, None]).astype(dtype), x0, x1, y0, y1


def pan_logits(score, up, nstuff, insts, masks, dtype):
    """panoptic_fusetrack.py:585-589: cat(stuff channels, SegTerm crop + pasted mask logits per instance) -> [nstuff + k, H, W].
    score [Hs, Ws, C] (the C channels that exist), insts [k, 10], masks [n, S, S]"""
    fcn = upsample(score, up, dtype)
    H, W = fcn.shape[1:]
    insts = np.asarray(insts).reshape(-1, 10)
    out = np.zeros((nstuff + insts.shape[0], H, W), dtype=dtype)
    out[:nstuff] = fcn[:nstuff]
    for j, it in enumerate(insts):
        sx0, sy0, sx1, sy1 = (int(v) for v in it[SX0:SY1 + 1])
        assert sx0 >= 0 and sy0 >= 0, 'a SegTerm crop starts inside the image (clipped boxes)'
        out[nstuff + j, sy0:max(sy1, 0), sx0:max(sx1, 0)] = fcn[it[SEG_CH], sy0:max(sy1, 0), sx0:max(sx1, 0)]
        p = pasted_logit(masks[it[MASK_IDX]], it[BX1:BY2 + 1], H, W, dtype)
        if p is not None:
            v, x0, x1, y0, y1 = p
            out[nstuff + j, y0:y1, x0:x1] += v
    return out


def sem_logits(score, up, dtype):
    return upsample(score, up, dtype)


def combine(score, up, nstuff, insts, masks, dtype):
    """panoptic_fusetrack.py:590-593 without the (monotone) softmax: the FIRST maximum of the panoptic and of the semantic logits
    -> (pan [H, W], sem [H, W]) uint8"""
    pan = np.argmax(pan_logits(score, up, nstuff, insts, masks, dtype), axis=0)
    sem = np.argmax(sem_logits(score, up, dtype), axis=0)
    assert pan.max() <= 255
    return pan.astype(np.uint8), sem.astype(np.uint8)


def margins(logits):
    """[C, H, W] -> distance between the largest and the second largest value per pixel (inf for one channel)"""
    if logits.shape[0] < 2:
        return np.full(logits.shape[1:], np.inf)
    top = np.partition(logits, logits.shape[0] - 2, axis=0)[-2:]
    return top[1] - top[0]


def _decision(ms, ov, thr):
    return bool(ms != 0 and not (ov / ms > thr))


def mask_removal_walk(boxes_i32, cls0, masks, order, H, W, thr, dtype, unsure_bound):
    """utils/mask_removal.py:58-86 for the detections boxes_i32 [n, 4] / cls0 [n] (0-based class) / masks [n, S, S], visited in
    `order` (the descending-score walk). Per walk position: ms (mask_sum), ov (the overlap with the kept earlier boxes of the class),
    keep = ms != 0 and not (ov / ms > thr), u = pixels of the clipped box whose resized logit is within unsure_bound of zero, and
    decisive = the decision stays when up to u pixels move into or out of ms and of ov and the pixels of the box where the occupancy
    left by earlier boxes is itself unsure (uo) move into or out of ov. Also keep_inds (order[keep]), the occupancy planes
    occ [ncls, H, W] (bool) and the planes `unsure` of the pixels where a kept box's logit is within the bound."""
    n = len(order)
    ncls = int(np.max(cls0)) + 1
    occ = np.zeros((ncls, H, W), dtype=bool)
    unsure = np.zeros((ncls, H, W), dtype=bool)
    res = dict(ms=[], ov=[], keep=[], u=[], uo=[], decisive=[])
    for i in order:
        c = int(cls0[i])
        p = pasted_logit(masks[i], boxes_i32[i], H, W, dtype)
        ms = ov = u = uo = 0
        if p is not None:
            v, x0, x1, y0, y1 = p
            pos = v > 0
            near = np.abs(v) <= unsure_bound
            ms, ov = int(pos.sum()), int((pos & occ[c, y0:y1, x0:x1]).sum())
            u, uo = int(near.sum()), int(unsure[c, y0:y1, x0:x1].sum())
        keep = _decision(ms, ov, thr)
        lo_ms, hi_ms, lo_ov, hi_ov = max(ms - u, 0), ms + u, max(ov - u - uo, 0), ov + u + uo
        res['decisive'].append(all(_decision(a, b, thr) == keep for a in (lo_ms, hi_ms) for b in (lo_ov, hi_ov)))
        if keep:
            occ[c, y0:y1, x0:x1] |= pos
            unsure[c, y0:y1, x0:x1] |= near
        for key, val in (('ms', ms), ('ov', ov), ('keep', keep), ('u', u), ('uo', uo)):
            res[key].append(val)
    res = {key: np.array(val) for key, val in res.items()}
    res['keep_inds'] = np.asarray(order)[res['keep']].astype(np.int64)
    res['occ'], res['unsure'] = occ, unsure
    return res


# ------------------------------------------------------------------------------------------------ the inputs of the tests
# (shared by tests/test_pan_restate.py, which asserts on the CPU what the GPU comparison relies on, and tests/test_pan_ops_gpu.py)
NO_BOX = (0, 0, -1, -1)           # an empty paste region, as vps_pan_instances writes it for "nothing kept"


def _inst(crop, seg_ch, box=NO_BOX, mask_idx=0):
    return [crop[0], crop[1], crop[2], crop[3], seg_ch, box[0], box[1], box[2], box[3], mask_idx]


def _exact_score(rg, Hs, Ws, nclass, ld=None, negative=()):
    """multiples of 1/8 in [-4, 4], six distinct values; channels listed in `negative` draw from the negative ones only"""
    vals = np.array([-4., -1.5, -0.125, 0.25, 1., 3.875], dtype=np.float32)
    s = vals[rg.integers(0, 6, (Hs, Ws, ld or nclass))]
    for c in negative:
        s[:, :, c] = vals[rg.integers(0, 3, (Hs, Ws))]
    return s


EXACT_CASES = ('k0', 'k1_nothing', 'k5_borders', 'chunk_second', 'chunk_first', 'up2', 'up8', 'up1', 'c33', 'ld24', 'nstuff0', 'allstuff')


def exact_case(name):
    """family A: every product and sum of the bilinear upsampling is exact in float32 (scores are multiples of 1/8, the weights of
    up = 1, 2, 4, 8 multiples of 1/16) and the mask logits are zero, so float64, float32 and the kernel agree bit for bit and
    equal logits are EQUAL: duplicated channels and instances that add nothing tie at thousands of pixels.
    -> dict(score [Hs, Ws, ld], nclass, nstuff, up, insts [k, 10], masks [n, S, S])"""
    rg = np.random.default_rng(EXACT_CASES.index(name) + 100)
    Hs, Ws, up, nclass, nstuff, ld, S = 13, 22, 4, 19, 11, None, 28
    neg = ()
    if name in ('k1_nothing', 'chunk_second', 'chunk_first'):
        neg = tuple(range(12))                                  # every stuff channel and thing channel 11 are negative everywhere
    elif name == 'up2':
        Hs, Ws, up = 20, 50, 2
    elif name == 'up8':
        Hs, Ws, up = 5, 9, 8
    elif name == 'up1':
        Hs, Ws, up = 24, 40, 1
    elif name == 'c33':
        nclass, nstuff = 33, 20
    elif name == 'ld24':
        ld = 24
    elif name == 'nstuff0':
        nstuff = 0
    elif name == 'allstuff':
        nstuff = 19
    score = _exact_score(rg, Hs, Ws, nclass, ld, neg)
    if not neg:
        score[:, :, 5] = score[:, :, 2]                         # two stuff channels tie everywhere (nstuff >= 6), sem ties too
        score[:, :, nclass - 1] = score[:, :, 3]                # the last thing channel ties with stuff channel 3
    if ld:
        score[:, :, nclass:] = 1e30                             # a read past nclass wins every arg-max
    H, W = Hs * up, Ws * up
    th0 = min(nstuff, nclass - 1)                               # first thing channel (any channel when all are stuff)
    if name == 'k0':
        insts = []
    elif name == 'k1_nothing':
        insts = [_inst((0, 0, 0, 0), 0)]
    elif name == 'chunk_second':
        # 0..63 cover the image with a negative channel; 64..69 miss most tiles: the winner of a pixel is the lowest of them that is
        # 0 there, which only the "first skipped" rule lists - found in the SECOND ballot round, behind 64 listed instances
        insts = [_inst((0, 0, W, H), 11) for _ in range(64)]
        insts += [_inst(c, 11) for c in ((2, 1, 30, 7), (20, 4, 40, 12), (33, 9, 63, 15), (30, 6, 70, 26), (64, 40, 88, 52), (5, 30, 6, 31))]
    elif name == 'chunk_first':
        # the mirror: the first skipped instance is in chunk 0 (5, or 6.. where 5 hits), every instance of chunk 1 hits every tile
        insts = [_inst((0, 0, W, H), 11) for _ in range(5)]
        insts += [_inst(c, 11) for c in ((2, 1, 30, 7), (20, 4, 40, 12), (33, 9, 63, 15), (30, 6, 70, 26), (64, 40, 88, 52))]
        for j in range(10, 64):
            x, y = int(rg.integers(0, W - 3)), int(rg.integers(0, H - 3))
            insts.append(_inst((x, y, x + int(rg.integers(1, 40)), y + int(rg.integers(1, 12))), 11))
        insts += [_inst((0, 0, W, H), 11) for _ in range(6)]
    else:
        # crops that ARE a 32 x 8 tile, straddle four tiles, sit inside one, reach the ragged last tile / the image corner, a 1-pixel
        # crop, an empty one; paste boxes (zero logits: they add 0 but list the instance on their tiles); two instances on ONE channel
        # with overlapping crops (the lower one wins the tie), one on the channel that ties with stuff channel 3 (the stuff wins)
        fx, fy = W / 88.0, H / 52.0
        crops = [(0, 0, 32, 8), (30, 6, 34, 10), (32, 8, 64, 16), (33, 9, 63, 15), (64, 40, 88, 52), (5, 30, 6, 31), (40, 20, 40, 30)]
        crops = [(int(a * fx), int(b * fy), max(int(c * fx), 0), max(int(d * fy), 0)) for a, b, c, d in crops]
        k = {'k5_borders': 5, 'up2': 7, 'up8': 4, 'up1': 4, 'c33': 6, 'ld24': 5, 'nstuff0': 6, 'allstuff': 3}[name]
        chans = [th0, th0, nclass - 1, min(th0 + 2, nclass - 1), th0, nclass - 1, th0]
        boxes = [NO_BOX, (int(10 * fx), int(20 * fy), int(50 * fx), int(30 * fy)), NO_BOX, (-3, -2, 4, 3), (W - 5, H - 3, W + 6, H + 2), NO_BOX, NO_BOX]
        insts = [_inst(crops[j], chans[j], boxes[j], j % 3) for j in range(k)]
        insts[1][SX0:SY1 + 1] = [crops[0][0] + 3, crops[0][1] + 2, crops[0][2] + 9, crops[0][3] + 5]         # overlaps instance 0, same channel
    return dict(score=score, nclass=nclass, nstuff=nstuff, up=up, insts=np.array(insts, dtype=np.int32).reshape(-1, 10),
                masks=np.zeros((3, S, S), dtype=np.float32))


#                name         Hs  Ws  up  k   nclass nstuff S  permuted mask_idx
RANDOM_CASES = {'k5':        (13, 22, 4, 5,   19, 11, 28, False),
                'up2_k70':   (20, 50, 2, 70,  19, 11, 28, False),
                'up1_k3':    (24, 40, 1, 3,   19, 11, 28, False),
                'up8_k12':   (5,  9,  8, 12,  19, 11, 28, False),
                'k244':      (13, 22, 4, 244, 19, 11, 28, False),
                'c33_k12':   (13, 22, 4, 12,  33, 20, 28, False),
                's7_k12':    (13, 22, 4, 12,  19, 11, 7,  True)}
RANDOM_SEEDS = {name: 200 + i for i, name in enumerate(RANDOM_CASES)}


def random_boxes(rg, n, H, W):
    """float32 boxes x1, y1, x2, y2: sizes log-uniform from 1 pixel to the whole image, about a third moved over one of the four edges
    by up to 6 pixels; then by hand (the first rows, as many as n allows): a 1-pixel box, a box outside the image, an inverted box
    (x2 < x1: the resize target is 1 wide), the whole image"""
    bw = np.exp(rg.uniform(0, np.log(W), n)); bh = np.exp(rg.uniform(0, np.log(H), n))
    x1 = rg.uniform(0, W - bw); y1 = rg.uniform(0, H - bh)
    b = np.stack([x1, y1, x1 + bw - 1, y1 + bh - 1], 1)
    edge = rg.integers(0, 12, n)                                   # 0..3: over the left, top, right, bottom edge
    over = rg.uniform(0.5, 6, n)
    for i in range(n):
        if edge[i] == 0: b[i, [0, 2]] -= b[i, 0] + over[i]
        elif edge[i] == 1: b[i, [1, 3]] -= b[i, 1] + over[i]
        elif edge[i] == 2: b[i, [0, 2]] += W - 1 - b[i, 2] + over[i]
        elif edge[i] == 3: b[i, [1, 3]] += H - 1 - b[i, 3] + over[i]
    hand = [(W // 3 + 0.4, H // 2 + 0.7, W // 3 + 0.9, H // 2 + 0.8), (W + 2.5, 3.2, W + 9.0, H / 2.0), (W // 2 + 5.3, 2.6, W // 2 + 1.2, H - 4.5),
            (0.0, 0.0, W - 1.0, H - 1.0)]
    b[:min(n, 4)] = hand[:min(n, 4)]
    return b.astype(np.float32)


def table_of(boxes, cls, H, W, nstuff, mask_idx=None):
    """the instance table vps_pan_instances writes for detections boxes [k, 4] (float32) / cls [k] (1-based): the SegTerm crop
    int(b), int(round(b) + 1) of the CLIPPED float box (MaskROI clips its boxes; unary_logits.py:102-105), the int32-truncated box"""
    lim = np.array([W - 1, H - 1, W - 1, H - 1], dtype=np.float32)
    cb = np.clip(boxes, np.float32(0), lim)
    tb = boxes.astype(np.int32)
    idx = np.arange(len(boxes)) if mask_idx is None else mask_idx
    rows = [[int(cb[j, 0]), int(cb[j, 1]), int(np.round(cb[j, 2]) + 1), int(np.round(cb[j, 3]) + 1), nstuff + int(cls[j]) - 1,
             tb[j, 0], tb[j, 1], tb[j, 2], tb[j, 3], idx[j]] for j in range(len(boxes))]
    return np.array(rows, dtype=np.int32).reshape(-1, 10), cb


def random_case(name):
    """family B: scores 3 N(0,1), mask logits 2 N(0,1) + 0.6, boxes of random_boxes()"""
    Hs, Ws, up, k, nclass, nstuff, S, permuted = RANDOM_CASES[name]
    rg = np.random.default_rng(RANDOM_SEEDS[name])
    H, W = Hs * up, Ws * up
    score = (rg.standard_normal((Hs, Ws, nclass)) * 3).astype(np.float32)
    masks = (rg.standard_normal((k, S, S)) * 2 + 0.6).astype(np.float32)
    boxes = random_boxes(rg, k, H, W)
    cls = rg.integers(1, nclass - nstuff + 1, k)
    mask_idx = rg.permutation(k) if permuted else None
    insts, cb = table_of(boxes, cls, H, W, nstuff, mask_idx)
    return dict(score=score, nclass=nclass, nstuff=nstuff, up=up, insts=insts, masks=masks, boxes=boxes, clipped=cb, cls=cls)


def margin_bound(case):
    """the bound of family B for one case: 4 x the largest distance of the float32 restatement from the float64 one over ALL logits of
    the case (the factor of tests/tolerances.py for a kernel against a float32 restatement: contraction, another association of the
    same four-tap sums), never below one float32 ulp of the largest |logit| -> (bound, f32-f64 distance, pan64, sem64)"""
    a = (case['score'][:, :, :case['nclass']], case['up'], case['nstuff'], case['insts'], case['masks'])
    p32, p64 = pan_logits(*a, np.float32), pan_logits(*a, np.float64)
    s32, s64 = sem_logits(a[0], a[1], np.float32), sem_logits(a[0], a[1], np.float64)
    dist = max(float(np.abs(p32 - p64).max()) if p64.size else 0.0, float(np.abs(s32 - s64).max()))
    ulp = float(np.spacing(np.float32(max(np.abs(p64).max() if p64.size else 0.0, np.abs(s64).max()))))
    return max(4 * dist, ulp), dist, p64, s64


def margin_compare(got, logits64, bound):
    """the rule of family B for one map: where the float64 margin between the largest and the second largest logit is above `bound`
    or exactly 0 (a structural tie: the lowest index wins) the map equals the float64 first-maximum arg-max; elsewhere (excluded from
    the exact comparison) it names a channel within `bound` of the maximum -> (wrong exact pixels, wrong excluded pixels, excluded)"""
    m = margins(logits64)
    want = np.argmax(logits64, axis=0)
    excluded = (m > 0) & (m <= bound)
    got = got.astype(np.int64)
    in_range = got < logits64.shape[0]
    val = np.take_along_axis(logits64, np.minimum(got, logits64.shape[0] - 1)[None], 0)[0]
    near = in_range & (val >= logits64.max(0) - bound)
    return int(((got != want) & ~excluded).sum()), int((excluded & ~near).sum()), int(excluded.sum())


REMOVAL_HW, REMOVAL_S, REMOVAL_THR = (64, 96), 28, 0.3
#                 name       n   classes seed
REMOVAL_LISTS = {'n1':      (1,  1, 301),
                 'n12_c3':  (12, 3, 302),
                 'n40_c2':  (40, 2, 303),
                 'n40_c1':  (40, 1, 304)}


def removal_list(name):
    """a detection list for MaskRemoval on 64 x 96: rows [n, 8] (0, x1, y1, x2, y2, score, class, index) with distinct scores in a
    shuffled order, mask logits [n, S, S]"""
    H, W = REMOVAL_HW
    if name.startswith('thr'):
        return threshold_list(int(name[3:]))
    n, ncls, seed = REMOVAL_LISTS[name]
    rg = np.random.default_rng(seed)
    rows = np.zeros((n, 8), dtype=np.float32)
    rows[:, 1:5] = random_boxes(rg, n, H, W)
    rows[:, 5] = rg.permutation(n) / np.float32(4 * n) + np.float32(0.6)
    rows[:, 6] = rg.integers(1, ncls + 1, n)
    rows[:, 7] = np.arange(n)
    masks = (rg.standard_normal((n, REMOVAL_S, REMOVAL_S)) * 2 + 0.6).astype(np.float32)
    return rows, masks


def threshold_list(overlap):
    """mask logits all +1 (every pixel of a box is positive: the counts are areas). Class 1: a 10 x 10 box, a 1-pixel box beside it,
    then (lowest score) a 10 x 10 box with 3 of its 10 columns = 30 of its 100 pixels on the first - and, for overlap = 31, one more
    pixel on the 1-pixel box (two 10 x 10 rectangles alone cannot share 31 pixels). 30 / 100 > 0.3 is false: kept; 31 / 100: dropped.
    A fourth box (class 2, the best score) lies outside the image: mask_sum == 0, dropped."""
    assert overlap in (30, 31)
    rows = np.zeros((4, 8), dtype=np.float32)
    rows[0, 1:5] = (20, 30, 29, 39)
    rows[1, 1:5] = (36, 35, 36, 35) if overlap == 31 else (50, 35, 50, 35)
    rows[2, 1:5] = (27, 30, 36, 39)
    rows[3, 1:5] = (100, 10, 110, 20)
    rows[:, 5] = (0.9, 0.8, 0.7, 0.95)
    rows[:, 6] = (1, 1, 1, 2)
    rows[:, 7] = np.arange(4)
    return rows, np.ones((4, REMOVAL_S, REMOVAL_S), dtype=np.float32)


def removal_walk(rows, masks, dtype=np.float32):
    """mask_removal_walk on a list of removal_list() with the list's own unsure_bound = 4 x the largest distance between the float32
    and the float64 resized logits of its boxes -> (walk, unsure_bound, f32-f64 distance)"""
    H, W = REMOVAL_HW
    boxes = rows[:, 1:5].astype(np.int32)
    order = np.argsort(rows[:, 5])[::-1]
    dist = 0.0
    for i in range(len(rows)):
        p32, p64 = pasted_logit(masks[i], boxes[i], H, W, np.float32), pasted_logit(masks[i], boxes[i], H, W, np.float64)
        if p32 is not None:
            dist = max(dist, float(np.abs(p32[0] - p64[0]).max()))
    walk = mask_removal_walk(boxes, rows[:, 6].astype(np.int64) - 1, masks, order, H, W, REMOVAL_THR, dtype, 4 * dist)
    return walk, 4 * dist, dist


def oracle_mask_removal(boxes, prob, masks, cls, hw, thr):
    """oracle.fusetrack.mask_removal -> (keep_inds, mask_energy). A box that lies beyond the right or the bottom edge by more than
    a pixel (x_0 > x_1) is not given to it: the host code's slices (mask_removal.py:76-80) turn negative there and do not fit one
    another (MaskROI clips its boxes, the reference never sees one). Such a box has mask_sum == 0: it is dropped, and no other
    decision depends on it."""
    import torch
    from oracle import fusetrack as OF
    H, W = hw
    tb = boxes.astype(np.int32)
    sel = np.array([j for j in range(len(tb)) if max(tb[j, 0], 0) <= min(tb[j, 2] + 1, W) and max(tb[j, 1], 0) <= min(tb[j, 3] + 1, H)])
    keep, energy = OF.mask_removal(torch.from_numpy(boxes[sel]), torch.from_numpy(np.asarray(prob)[sel]), torch.from_numpy(masks[sel]),
                                   torch.from_numpy(np.asarray(cls)[sel].astype(np.int64)), (H, W), thr)
    assert energy.shape[1] == len(keep) and np.abs(energy.numpy()).max() > 0, 'something is kept'
    return sel[keep], energy
