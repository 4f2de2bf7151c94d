"""Plain numpy restatements of the glue kernels of vps_amd/csrc/nn_ops.hip and of the non-correlation half of vps_amd/csrc/flow_ops.hip:
the yardstick of tests/test_nn_ops_gpu.py, pinned to torch / the oracle by tests/test_nn_restate.py.

Every function takes a `dtype`. The float64 evaluation is the yardstick; the float32 evaluation is only there to derive bounds (its distance
from the float64 one says how much a different but equally valid float32 evaluation order may move a result). INDEX arithmetic is part of
the operator and stays in float32 in both evaluations, exactly as ATen / the reference CUDA computes it (a float64 index picks another
source pixel at exact ratios); only the values and weights derived after the index is fixed follow `dtype`.

Layouts: the C ABI of most of these kernels is NHWC-only, so those take [N, H, W, C] (or [npix, C]) arrays - the channel window already
cut out; resample2d / channelnorm / the transposes take NCHW. `wrong=` selects a deliberately WRONG variant (tests/test_nn_restate.py
proves on the GPU tests' own inputs that each would be noticed).

Reference lines (relative to mmdet/models of the reference, as the kernels cite them):
  resize            ATen upsample_bilinear2d / upsample_nearest2d CPU kernels (F.interpolate, align_corners=False)
  pool              F.max_pool2d(3, 2, 1) / F.avg_pool2d(3, 2, 1) (count_include_pad)
  bfp gather        extra_necks/bfp_tcea.py:96-109 (refine_level 0)
  bfp scatter       extra_necks/bfp_tcea.py:139-147
  groupnorm         panoptic/upsnetFPN.py:39-52
  tcea              utils/tcea_modules.py:50-65 (temporal), :74-77 (modulate)
  resample2d        flow_modules/resample2d_package/resample2d_kernel.cu:15-72
  channelnorm       flow_modules/channelnorm_package/channelnorm_kernel.cu:18-60
  flow_warp         flow_modules/flow_modules.py:126-148 (WarpingLayer)
  flow_prep         utils/flow_utils.py:5-10, flow_modules/flownet2.py:135-139
  flow_stage        flow_modules/flownet2.py:142-187"""
import numpy as np

F32 = np.float32


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return 1 / (1 + np.exp(-x))


# ------------------------------------------------------------------------------------------------ resize
def bilinear_index(n_in, n_out, align_corners=False):
    """float32 source index of every destination index -> (i0, i1, lambda float32): max(scale (dst + 0.5) - 0.5, 0), scale = in / out.
    The multiply-subtract is ONE fused operation (a single rounding), as nvcc, hipcc and the ATen CPU build all contract it: float64
    holds the product of two float32 exactly, so it is taken there and rounded once (tests/test_nn_restate.py pins this to torch)."""
    dst = np.arange(n_out, dtype=F32)
    if align_corners:                                                          # the WRONG variant
        scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        src = scale * dst
    else:
        scale = F32(n_in) / F32(n_out)
        src = np.maximum((np.float64(scale) * (dst + F32(0.5)).astype(np.float64) - 0.5).astype(F32), F32(0))
    assert src.dtype == F32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0.astype(F32)


def nearest_index(n_in, n_out):
    """min(floor(dst * scale), in - 1) in float32"""
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def resize(x, Ho, Wo, mode, alpha, dtype, wrong=None):
    """x [N, Hi, Wi, C] -> [N, Ho, Wo, C] * alpha; mode 'bilinear' (align_corners=False) or 'nearest'"""
    x = x.astype(dtype)
    if wrong == 'batch':
        x = np.broadcast_to(x[:1], x.shape)
    Hi, Wi = x.shape[1:3]
    if mode == 'nearest':
        v = x[:, nearest_index(Hi, Ho)][:, :, nearest_index(Wi, Wo)]
    else:
        ac = wrong == 'align_corners'
        y0, y1, ly = bilinear_index(Hi, Ho, ac)
        x0, x1, lx = bilinear_index(Wi, Wo, ac)
        ly = ly.astype(dtype)[None, :, None, None]; lx = lx.astype(dtype)[None, None, :, None]
        hy, hx = dtype(1) - ly, dtype(1) - lx
        top, bot = x[:, y0], x[:, y1]
        v = hy * (hx * top[:, :, x0] + lx * top[:, :, x1]) + ly * (hx * bot[:, :, x0] + lx * bot[:, :, x1])
    return v * dtype(F32(alpha))


# ------------------------------------------------------------------------------------------------ pool 3x3 stride 2 pad 1
def pool3x3s2(x, mode, dtype, wrong=None):
    """x [N, Hi, Wi, C]; 'max': -inf padding; 'avg': zero padding, divisor 9 always (count_include_pad)"""
    x = x.astype(dtype)
    if wrong == 'batch':
        x = np.broadcast_to(x[:1], x.shape)
    N, Hi, Wi, C = x.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    pad = dtype(-np.inf) if mode == 'max' and wrong != 'zero_pad' else dtype(0)
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), pad, dtype=dtype)
    xp[:, 1:Hi + 1, 1:Wi + 1] = x
    ins = np.zeros((1, 2 * Ho + 1, 2 * Wo + 1, 1), dtype=dtype)
    ins[:, 1:Hi + 1, 1:Wi + 1] = 1
    acc = cnt = None
    for dy in range(3):                                                        # the reference's visiting order: dy outer, dx inner
        for dx in range(3):
            t = xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
            c = ins[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
            if acc is None:
                acc, cnt = t.copy(), c.copy()
            elif mode == 'max':
                acc = np.maximum(acc, t)
            else:
                acc, cnt = acc + t, cnt + c
    if mode == 'max':
        return acc
    return acc / (cnt if wrong == 'exclude_pad' else dtype(9))


# ------------------------------------------------------------------------------------------------ BFP gather / scatter
def bfp_gather(levels, ratios, dtype, wrong=None):
    """levels[l] [N, H0 / r_l, W0 / r_l, C]: every level nearest-resized to level 0 (an integer ratio: y // r), summed IN LEVEL ORDER,
    divided by the level count"""
    s = None
    for lv, r in zip(levels, ratios):
        lv = lv.astype(dtype)
        if wrong == 'batch':
            lv = np.broadcast_to(lv[:1], lv.shape)
        up = np.repeat(np.repeat(lv, r, axis=1), r, axis=2)
        s = dtype(0) + up if s is None else s + up
    return s / dtype(5 if wrong == 'div5' else len(levels))


def bfp_scatter(bsf, level, r, dtype, wrong=None):
    """adaptive_max_pool2d(bsf, size of the level) with exact r x r windows, + level. bsf [N, H0, W0, C], level [N, H0 / r, W0 / r, C]"""
    bsf, level = bsf.astype(dtype), level.astype(dtype)
    if wrong == 'batch':
        bsf = np.broadcast_to(bsf[:1], bsf.shape)
    N, H0, W0, C = bsf.shape
    if wrong == 'window':                                                      # windows one pixel to the right (clamped)
        bsf = bsf[:, :, np.minimum(np.arange(W0) + 1, W0 - 1)]
    m = bsf.reshape(N, H0 // r, r, W0 // r, r, C).max(axis=(2, 4))
    return m + level


# ------------------------------------------------------------------------------------------------ axpb
def axpb(x, a, b, dtype, fma=False):
    """x * a + b: one multiply, one add. fma=True: the single rounding of a contracted multiply-add, np.float32(np.float64(x) a + b)"""
    if fma:
        return (x.astype(np.float64) * np.float64(F32(a)) + np.float64(F32(b))).astype(F32)
    return x.astype(dtype) * dtype(F32(a)) + dtype(F32(b))


# ------------------------------------------------------------------------------------------------ GroupNorm (+ ReLU), one image
def groupnorm(x, G, gamma, beta, eps, relu, dtype, sums=None, wrong=None):
    """x [npix, C]: per group of C / G channels the BIASED variance over npix * cpg values (sum of squares / count - mean^2, clamped
    at 0), 1 / sqrt(var + eps), affine, ReLU. sums [nrep, 2 G] float64 (sum, sum of squares per group, as partial copies to be added
    up) replaces the statistics of x where given (vps_groupnorm_apply)."""
    x = x.astype(dtype)
    npix, C = x.shape
    cpg = C // G
    if wrong == 'per_channel':
        G, cpg = C, 1
    xg = x.reshape(npix, G, cpg)
    cnt = dtype(npix * cpg)
    if wrong == 'float32_stats':                                               # what the far-mean case is there to notice
        x32 = xg.astype(F32)
        s, q = x32.sum(axis=(0, 2)).astype(dtype), (x32 * x32).sum(axis=(0, 2)).astype(dtype)
    elif sums is None:
        s, q = xg.sum(axis=(0, 2)), (xg * xg).sum(axis=(0, 2))
    else:
        tot = np.asarray(sums, dtype=np.float64).sum(axis=0).astype(dtype)
        s, q = tot[0::2], tot[1::2]
    mean = s / cnt
    var = q / cnt - mean * mean
    if wrong == 'unbiased':
        var = var * cnt / (cnt - dtype(1))
    var = np.maximum(var, dtype(0))
    rstd = dtype(1) / np.sqrt(var + dtype(F32(eps)))
    y = ((xg - mean[None, :, None]) * rstd[None, :, None]).reshape(npix, C) * gamma.astype(dtype) + beta.astype(dtype)
    if (relu != 0) != (wrong == 'relu_flip'):
        y = np.maximum(y, dtype(0))
    return y


def group_sums(x, G):
    """float64 (sum, sum of squares) per group, interleaved [2 G]: what vps_groupnorm_apply is handed"""
    npix, C = x.shape
    xg = x.astype(np.float64).reshape(npix, G, C // G)
    return np.stack([xg.sum(axis=(0, 2)), (xg * xg).sum(axis=(0, 2))], axis=1).reshape(-1)


# ------------------------------------------------------------------------------------------------ TCEA
def tcea_temporal(emb, emb_ref, fea0, fea1, dtype, wrong=None):
    """emb [npix, 2 C] (frame 0 | frame 1), emb_ref, fea0, fea1 [npix, C] -> [npix, 2 C]: fea_i * sigmoid(sum_c emb_i emb_ref)"""
    emb, emb_ref, fea0, fea1 = (a.astype(dtype) for a in (emb, emb_ref, fea0, fea1))
    C = emb_ref.shape[1]
    e0, e1 = emb[:, :C], emb[:, C:]
    if wrong == 'swap_frames':
        e0, e1 = e1, e0
    p0 = _sigmoid((e0 * emb_ref).sum(axis=1, keepdims=True))
    p1 = _sigmoid((e1 * emb_ref).sum(axis=1, keepdims=True))
    return np.concatenate([fea0 * p0, fea1 * p1], axis=1)


def tcea_modulate(fea, att, att_add, dtype, wrong=None):
    """fea * sigmoid(att) * 2 + att_add"""
    fea, att, att_add = (a.astype(dtype) for a in (fea, att, att_add))
    return fea * _sigmoid(att) * dtype(1 if wrong == 'no_factor_2' else 2) + att_add


# ------------------------------------------------------------------------------------------------ layout transposes
def nchw_to_nhwc(x, Cpad):
    """x [N, C, H, W] -> [N, H, W, Cpad], the pad channels +0.0; bit patterns kept (works on any 4-byte dtype)"""
    N, C, H, W = x.shape
    out = np.zeros((N, H, W, Cpad), dtype=x.dtype)
    out[..., :C] = np.transpose(x, (0, 2, 3, 1))
    return out


def nhwc_to_nchw(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


# ------------------------------------------------------------------------------------------------ resample2d / channelnorm (NCHW)
def _resample_taps(img, xf, yf, dtype, zero_pad=False):
    """img [C, H, W] in dtype, xf / yf [H, W] float32 sample positions: the reference's tap formula, literally - weights
    (1 - a)(1 - b), a (1 - b), (1 - a) b, a b on the border-CLAMPED corners, four separate additions"""
    C, H, W = img.shape
    fx, fy = np.floor(xf), np.floor(yf)
    a, b = (xf - fx).astype(dtype), (yf - fy).astype(dtype)                    # exact in float32: the fraction of a float32
    one = dtype(1)

    def tap(yy, xx):
        yc, xc = np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, W - 1).astype(np.int64)
        v = img[:, yc, xc]
        if zero_pad:                                                           # the WRONG variant
            v = np.where(((yy == yc) & (xx == xc))[None], v, dtype(0))
        return v
    val = np.zeros((C, H, W), dtype=dtype)
    val = val + (one - a) * (one - b) * tap(fy, fx)
    val = val + a * (one - b) * tap(fy, fx + 1)
    val = val + (one - a) * b * tap(fy + 1, fx)
    val = val + a * b * tap(fy + 1, fx + 1)
    return val


def resample2d(img, flow, dtype, wrong=None):
    """img [B, C, H, W], flow [B, 2, H, W] (x, y): out(y, x) = bilinear tap of img at (x + dx, y + dy); x + dx is a float32 sum"""
    B, C, H, W = img.shape
    xs, ys = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    out = np.empty((B, C, H, W), dtype=dtype)
    for b in range(B):
        src = 0 if wrong == 'batch' else b
        dx, dy = flow[src, 0].astype(F32), flow[src, 1].astype(F32)
        if wrong == 'swap_xy':
            dx, dy = dy, dx
        out[b] = _resample_taps(img[src].astype(dtype), xs + dx, ys + dy, dtype, zero_pad=wrong == 'zero_pad')
    return out


def channelnorm(x, dtype, wrong=None):
    """x [B, C, H, W] -> [B, 1, H, W]: sqrt of the sum of squares over the channels, added in channel order"""
    x = x.astype(dtype)
    if wrong == 'batch':
        x = np.broadcast_to(x[:1], x.shape)
    acc = np.zeros_like(x[:, 0])
    for c in range(x.shape[1]):
        acc = acc + (np.abs(x[:, c]) if wrong == 'l1' else x[:, c] * x[:, c])
    return (acc if wrong == 'l1' else np.sqrt(acc))[:, None]


# ------------------------------------------------------------------------------------------------ flow_warp (WarpingLayer)
def linspace_m1_p1(n, dtype):
    """torch.linspace(-1, 1, n): the CPU kernel's symmetric evaluation around the midpoint"""
    i = np.arange(n)
    step = dtype(2) / dtype(n - 1)
    return np.where(i < n // 2, dtype(-1) + step * i.astype(dtype), dtype(1) - step * (n - 1 - i).astype(dtype)).astype(dtype)


def flow_warp(x, flow, dtype, wrong=None):
    """x [N, H, W, C], flow [N, H, W, 2] (x, y): grid = linspace(-1, 1) + flow / ((size - 1) / 2), then grid_sample (bilinear, zeros,
    align_corners=False) - the reference's align_corners mismatch is reproduced: zero flow does NOT give the input back. Coordinates
    in dtype throughout (grid_sample is continuous in them)."""
    x, flow = x.astype(dtype), flow.astype(dtype)
    N, H, W, C = x.shape
    out = np.zeros_like(x)
    for n in range(N):
        src = 0 if wrong == 'batch' else n
        fx, fy = flow[src, ..., 0], flow[src, ..., 1]
        if wrong == 'swap_xy':
            fx, fy = fy, fx
        gx = linspace_m1_p1(W, dtype)[None, :] + fx / ((dtype(W) - dtype(1)) / dtype(2))
        gy = linspace_m1_p1(H, dtype)[:, None] + fy / ((dtype(H) - dtype(1)) / dtype(2))
        if wrong == 'align_corners':                                           # the unnormalisation that would undo the linspace
            ix, iy = (gx + dtype(1)) / dtype(2) * dtype(W - 1), (gy + dtype(1)) / dtype(2) * dtype(H - 1)
        else:
            ix, iy = ((gx + dtype(1)) * dtype(W) - dtype(1)) / dtype(2), ((gy + dtype(1)) * dtype(H) - dtype(1)) / dtype(2)
        if wrong == 'border':
            ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
        x0, y0 = np.floor(ix), np.floor(iy)
        acc = np.zeros((H, W, C), dtype=dtype)
        for yy, xx, w in ((y0, x0, (x0 + 1 - ix) * (y0 + 1 - iy)), (y0, x0 + 1, (ix - x0) * (y0 + 1 - iy)),
                          (y0 + 1, x0, (x0 + 1 - ix) * (iy - y0)), (y0 + 1, x0 + 1, (ix - x0) * (iy - y0))):
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            yc, xc = np.clip(yy, 0, H - 1).astype(np.int64), np.clip(xx, 0, W - 1).astype(np.int64)
            acc = np.where(ok[..., None], acc + x[src][yc, xc] * w[..., None], acc)
        out[n] = acc
    return out


# ------------------------------------------------------------------------------------------------ FlowNet2 input prep
def flow_prep(img, ref, mean3, std3, Hp, Wp, dtype, wrong=None):
    """img, ref [3, H, W] (the detector's normalised frames) -> ([Hp, Wp, 6], rgb_mean [3]): x * std + mean (two roundings), zero pad to
    [Hp, Wp] in 0..255 space, the mean per colour over BOTH padded frames, (x - mean) / 255, channels img | ref"""
    if wrong == 'swap_frames':
        img, ref = ref, img
    H, W = img.shape[1:]
    pair = np.zeros((2, 3, Hp, Wp), dtype=dtype)
    for i, f in enumerate((img, ref)):
        den = f.astype(dtype) * std3.astype(dtype)[:, None, None]
        pair[i, :, :H, :W] = den + mean3.astype(dtype)[:, None, None]
    if wrong == 'mean_unpadded':
        rgb_mean = pair[:, :, :H, :W].sum(axis=(0, 2, 3)) / dtype(2 * H * W)
    else:
        rgb_mean = pair.sum(axis=(0, 2, 3)) / dtype(2 * Hp * Wp)
    out = (pair - rgb_mean[None, :, None, None]) / dtype(255)
    return np.concatenate([out[0], out[1]], axis=0).transpose(1, 2, 0), rgb_mean


# ------------------------------------------------------------------------------------------------ FlowNet2 inter-stage builder
def flow_stage(x6, flo, up_mode, mul, div_mode, flow_out_div, dtype, wrong=None):
    """x6 [H, W, 6] (img1 | img2), flo [H / 4, W / 4, 2] -> dict of
      flow [H, W, 2]   the x4 upsample (up_mode 0: bilinear align_corners=False, 1: nearest) of flo * mul (div_mode 0) or flo / mul (1),
                       divided by flow_out_div where that is > 0
      flownorm [H, W]  |flow| (before flow_out_div)
      warp [H, W, 3]   Resample2d of img2 with the flow
      diffnorm [H, W]  ChannelNorm of img1 - warp
      img [H, W, 3]    img1
    The (int) source index of the upsample and floor(x + flow) are float32 index arithmetic."""
    x6, flo = x6.astype(dtype), flo.astype(dtype)
    H, W = x6.shape[:2]
    Hl, Wl = H // 4, W // 4
    m = dtype(F32(mul))
    lo = flo / m if (div_mode != 0) != (wrong == 'mul_div') else flo * m
    if up_mode == 1:
        f = lo[np.arange(H) // 4][:, np.arange(W) // 4]
    else:
        y0, y1, ly = bilinear_index(Hl, H)                                     # scale = Hl / H = 0.25 exactly
        x0, x1, lx = bilinear_index(Wl, W)
        ly = ly.astype(dtype)[:, None, None]; lx = lx.astype(dtype)[None, :, None]
        hy, hx = dtype(1) - ly, dtype(1) - lx
        top, bot = lo[y0], lo[y1]
        f = hy * (hx * top[:, x0] + lx * top[:, x1]) + ly * (hx * bot[:, x0] + lx * bot[:, x1])
    fx, fy = f[..., 0], f[..., 1]
    if wrong == 'swap_xy':
        fx, fy = fy, fx
    xs, ys = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    warp = _resample_taps(np.ascontiguousarray(x6[..., 3:6].transpose(2, 0, 1)), xs + fx.astype(F32), ys + fy.astype(F32), dtype,
                          zero_pad=wrong == 'zero_pad').transpose(1, 2, 0)
    nrm = np.zeros((H, W), dtype=dtype)
    for c in range(3):
        d = x6[..., c] - warp[..., c]
        nrm = nrm + d * d
    fo = np.stack([fx, fy], axis=-1)
    return dict(flow=fo / dtype(F32(flow_out_div)) if flow_out_div > 0 else fo, flownorm=np.sqrt(fx * fx + fy * fy), warp=warp,
                diffnorm=np.sqrt(nrm), img=x6[..., :3])


def flow_stage_full(x6, flow_a, flow_b, mode, mul, dtype, wrong=None):
    """[H, W, 12]. mode 0 (FlowNetS input, flownet2.py:142-163): img1 img2 | warped img2 | flow / mul | |img1 - warped|, flow = bilinear
    x4 of flow_a * mul. mode 1 (FlowNetFusion input, :166-187): img1 | flow_sd | flow_s2 | |flow_sd| | |flow_s2| | diff_sd | diff_s2 | 0,
    flow_s2 = nearest x4 of flow_a * mul, flow_sd = nearest x4 of flow_b / mul"""
    x6 = x6.astype(dtype)
    if mode == 0:
        s = flow_stage(x6, flow_a, 0, mul, 0, mul, dtype, wrong)
        return np.concatenate([x6, s['warp'], s['flow'], s['diffnorm'][..., None]], axis=-1)
    s2 = flow_stage(x6, flow_a, 1, mul, 0, 0.0, dtype, wrong)
    sd = flow_stage(x6, flow_b, 1, mul, 1, 0.0, dtype, wrong)
    return np.concatenate([x6[..., :3], sd['flow'], s2['flow'], sd['flownorm'][..., None], s2['flownorm'][..., None], sd['diffnorm'][..., None],
                           s2['diffnorm'][..., None], np.zeros(x6.shape[:2] + (1,), dtype=dtype)], axis=-1)


# ------------------------------------------------------------------------------------------------ bounds
FACTOR = 4          # a different but equally valid summation / contraction order (the factor of the head and pan suites)


def derive_bound(r32, r64):
    """-> (bound, distance, floor): bound = max(floor, FACTOR x max|float32 restatement - float64 restatement|), floor = one float32 ulp
    of the largest |reference| value of the case"""
    r64 = np.asarray(r64, dtype=np.float64)
    fin = np.isfinite(r64)
    dist = float(np.abs(np.asarray(r32, dtype=np.float64) - r64)[fin].max()) if fin.any() else 0.0
    floor = float(np.spacing(F32(np.abs(r64[fin]).max()))) if fin.any() else 0.0
    return max(floor, FACTOR * dist), dist, floor
