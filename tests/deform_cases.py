"""Operands of the deformable-conv tests (tests/test_deform_restate.py, tests/test_deform_conv_gpu.py). No project code.

EDGE OFFSET FIELD. Every (image, tap, output pixel) draws ONE class of sampling position - per tap, not per pixel, so the nine taps of
a pixel land in different classes:
  a  fractional, inside the map                      f  exactly -1, exactly H-1 (W-1) or exactly H (W) in one coordinate
  b  exact integers (bilinear weights 1, 0, 0, 0)    g  wholly outside, by 1 to 3 map sizes
  c  integer row, fractional column, or the converse h  an offset of +-1e9, +-3e38 or +-inf
  d  h or w in (-1, 0)                               i  NaN in dh, dw or both
  e  h in (H-1, H) or w in (W-1, W)
Positions are drawn as targets; the offset is target - tap position. Half of the fractional parts are multiples of 2^-12 (offset and
position are then exact in fp32), the others are arbitrary floats. `check_field` re-derives every class's property from the fp32
positions the kernels will form, and the shares the tests rely on.

INTEGER OPERANDS. Activations and weights are integers in [-4, 4]; one output channel's weights are scaled by 2^-9 and another's by
2^6 (the per-channel power-of-two scaling of f16x3 undoes both exactly; 4 * 2^-9 and 4 * 2^6 are bf16 and fp16 numbers); offsets
come from the classes b, f, g, h, i with integer positions only, so every bilinear weight is 0 or 1. With K = 9 * cin <= 2304 every
partial sum is an integer multiple of its channel's unit below 2^24 units: every operand plane is exact and no fp32 addition rounds
in any mode or order - a kernel must equal the float64 result bitwise."""
import functools
import math
import zlib

import torch

CLASSES = 'abcdefghi'
EDGE_SHARES = dict(a=0.20, b=0.12, c=0.12, d=0.10, e=0.10, f=0.10, g=0.09, h=0.09, i=0.08)
INT_SHARES = dict(b=0.52, f=0.18, g=0.10, h=0.10, i=0.10)
HUGE = (1e9, -1e9, 3e38, -3e38, math.inf, -math.inf)

# name, cin, cout, N, H, W, stride, requested arithmetic, switches -> the route: kernel, tile_n, ksplit, tile_counter set.
# Settled with the stand-alone planner and conv_geometry (tests/test_deform_restate.py asserts the geometry half without a GPU).
# Channel counts decide the route, not the map: 32 input channels are ONE chunk (never split), 64 / 96 / 256 are 2 / 3 / 8 chunks and
# split into as many ranges on any map below 256 tiles - so the maps are the smallest with two images, more than one 128-pixel tile, a
# tile that straddles the two images and a ragged last tile: 9 x 13 (117 pixels per image) and 11 x 15 (165). The 256-column kernel
# needs 256 pixel tiles: 2 x 127 x 131 = 33274 pixels = 259 tiles + 122 rows, tile 129 straddles the images.
ROUTES = [
    ('f32_tapmajor_forced', 12, 40, 2, 9, 13, 1, 'f16x3', (), ('f32', 64, 1, False)),
    ('f32_split_reduce', 64, 48, 2, 11, 15, 1, 'f32', (), ('f32', 64, 2, False)),
    ('f32_unsplit', 32, 128, 2, 11, 15, 1, 'f32', (), ('f32', 128, 1, False)),
    ('p_split8_bf16x3', 256, 128, 2, 9, 13, 1, 'bf16x3', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 128, 8, True)),
    ('p_split8_bf16x6', 256, 128, 2, 9, 13, 1, 'bf16x6', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 128, 8, True)),
    ('p_split8_f16x3', 256, 128, 2, 9, 13, 1, 'f16x3', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 128, 8, True)),
    ('p_split3_bf16x3', 96, 48, 2, 9, 13, 1, 'bf16x3', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 64, 3, True)),
    ('p_split3_bf16x6', 96, 48, 2, 9, 13, 1, 'bf16x6', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 64, 3, True)),
    ('p_split3_f16x3', 96, 48, 2, 9, 13, 1, 'f16x3', (('SPLITK_LAST_BLOCK', True),), ('bf16p', 64, 3, True)),
    ('p_split3_reduce_f16x3', 96, 48, 2, 9, 13, 1, 'f16x3', (), ('bf16p', 64, 3, False)),
    ('p_unsplit_f16x3', 32, 256, 2, 11, 15, 1, 'f16x3', (('DCN256', False),), ('bf16p', 128, 1, False)),
    ('p_unsplit_bf16x6', 32, 256, 2, 11, 15, 1, 'bf16x6', (), ('bf16p', 128, 1, False)),
    ('dcn256', 32, 256, 2, 127, 131, 1, 'f16x3', (), ('dcn256', 256, 1, False)),
    ('s2_f32', 64, 64, 1, 17, 23, 2, 'f32', (), ('f32', 64, 2, False)),
    ('s2_f16x3', 64, 64, 1, 17, 23, 2, 'f16x3', (), ('bf16p', 64, 2, False)),
]
# the GroupNorm-sum epilogue exists on the unsplit split-operand routes, for ONE image: the same layers on one map
GN_ROUTES = [
    ('p_unsplit_f16x3', 32, 256, 1, 11, 15, 1, 'f16x3', (('DCN256', False),), ('bf16p', 128, 1, False)),
    ('p_unsplit_bf16x6', 32, 256, 1, 11, 15, 1, 'bf16x6', (), ('bf16p', 128, 1, False)),
    ('dcn256', 32, 256, 1, 181, 182, 1, 'f16x3', (), ('dcn256', 256, 1, False)),        # 32942 pixels = 257 tiles + 46 rows
]


def out_hw(H, W, stride, padding=1, k=3):
    return (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1


def _frac(n, g, integer):
    """fractional parts in (0, 1): half multiples of 2^-12, half arbitrary; zeros for integer fields"""
    if integer:
        return torch.zeros(n, dtype=torch.float64)
    q = torch.randint(1, 4096, (n,), generator=g).double() / 4096.0
    r = torch.rand(n, generator=g, dtype=torch.float64).clamp(1e-3, 1 - 1e-3)
    return torch.where(torch.rand(n, generator=g) < 0.5, q, r)


def _inside(n, L, g, integer):
    """a coordinate inside the map: fractional in (0, L-1), or an integer in [0, L-1]"""
    if integer:
        return torch.randint(0, L, (n,), generator=g).double()
    return torch.randint(0, L - 1, (n,), generator=g).double() + _frac(n, g, False)


def offset_field(N, H, W, stride, padding, g, shares=EDGE_SHARES, k=3):
    """-> offset fp32 [N, 2 k k, Ho, Wo], cls int64 [N, k k, Ho, Wo] (index into CLASSES)"""
    integer = shares is INT_SHARES
    Ho, Wo = out_hw(H, W, stride, padding, k)
    T = k * k
    n = N * T * Ho * Wo
    p = torch.tensor([shares.get(c, 0.0) for c in CLASSES], dtype=torch.float64)
    cls = torch.multinomial(p, n, replacement=True, generator=g)
    ky = torch.arange(k).repeat_interleave(k).view(1, T, 1, 1)
    kx = torch.arange(k).repeat(k).view(1, T, 1, 1)
    by = (torch.arange(Ho).view(1, 1, Ho, 1) * stride - padding + ky).expand(N, T, Ho, Wo).reshape(-1).double()
    bx = (torch.arange(Wo).view(1, 1, 1, Wo) * stride - padding + kx).expand(N, T, Ho, Wo).reshape(-1).double()
    sub = torch.randint(0, 3, (n,), generator=g)             # which coordinate carries the class: 0 = h, 1 = w, 2 = both
    coin = torch.rand(n, generator=g) < 0.5
    th, tw = _inside(n, H, g, integer), _inside(n, W, g, integer)          # class a (and the other coordinate of every class)
    C = {c: cls == i for i, c in enumerate(CLASSES)}
    ih, iw = torch.randint(0, H, (n,), generator=g).double(), torch.randint(0, W, (n,), generator=g).double()
    on_h, on_w = sub != 1, sub != 0
    # b, c: integers
    th = torch.where(C['b'] | (C['c'] & coin), ih, th)
    tw = torch.where(C['b'] | (C['c'] & ~coin), iw, tw)
    # d: (-1, 0); e: (L-1, L)
    th = torch.where(C['d'] & on_h, -_frac(n, g, integer), th)
    tw = torch.where(C['d'] & on_w, -_frac(n, g, integer), tw)
    th = torch.where(C['e'] & on_h, (H - 1) + _frac(n, g, integer), th)
    tw = torch.where(C['e'] & on_w, (W - 1) + _frac(n, g, integer), tw)
    # f: exactly -1, L-1 or L in ONE coordinate
    pick = torch.randint(0, 3, (n,), generator=g)
    fh = torch.tensor([-1.0, H - 1.0, H], dtype=torch.float64)[pick]
    fw = torch.tensor([-1.0, W - 1.0, W], dtype=torch.float64)[pick]
    th = torch.where(C['f'] & coin, fh, th)
    tw = torch.where(C['f'] & ~coin, fw, tw)
    # g: beyond the far edge, or before -1, by 1 to 3 map sizes
    for L, on, is_h in ((H, on_h, True), (W, on_w, False)):
        d = torch.randint(L, 3 * L + 1, (n,), generator=g).double() + _frac(n, g, integer)
        far = torch.where(torch.rand(n, generator=g) < 0.5, L + d, -1.0 - d)
        if is_h:
            th = torch.where(C['g'] & on, far, th)
        else:
            tw = torch.where(C['g'] & on, far, tw)
    dh, dw = (th - by).float(), (tw - bx).float()
    # h, i: the OFFSET is huge / infinite / NaN
    huge = torch.tensor(HUGE, dtype=torch.float32)[torch.randint(0, len(HUGE), (n,), generator=g)]
    nan = torch.full((n,), math.nan)
    dh = torch.where(C['h'] & on_h, huge, dh)
    dw = torch.where(C['h'] & on_w, huge, dw)
    dh = torch.where(C['i'] & on_h, nan, dh)
    dw = torch.where(C['i'] & on_w, nan, dw)
    off = torch.stack([dh.view(N, T, Ho, Wo), dw.view(N, T, Ho, Wo)], dim=2).reshape(N, 2 * T, Ho, Wo).contiguous()
    return off, cls.view(N, T, Ho, Wo)


def check_field(off, cls, h, w, valid, H, W, shares=EDGE_SHARES):
    """asserts, from the fp32 positions h, w [N, T, Ho, Wo] that the kernels form (deform_restate.positions): every sample has the
    property of its class, every class of `shares` holds >= 2 % of the samples, and at least half of the samples are valid"""
    dh, dw = off[:, 0::2], off[:, 1::2]
    fr_h, fr_w = h != torch.floor(h), w != torch.floor(w)
    in_h, in_w = (h >= 0) & (h <= H - 1), (w >= 0) & (w <= W - 1)
    prop = dict(
        a=in_h & in_w & fr_h & fr_w,
        b=in_h & in_w & ~fr_h & ~fr_w,
        c=in_h & in_w & (fr_h ^ fr_w),
        d=valid & (((h > -1) & (h < 0)) | ((w > -1) & (w < 0))),
        e=valid & (((h > H - 1) & (h < H)) | ((w > W - 1) & (w < W))),
        f=(h == -1) | (h == H - 1) | (h == H) | (w == -1) | (w == W - 1) | (w == W),
        g=~valid & ((h >= 2 * H) | (h <= -1 - H) | (w >= 2 * W) | (w <= -1 - W)),
        h=~valid & ((dh.abs() >= 1e9) | (dw.abs() >= 1e9)),
        i=~valid & (torch.isnan(dh) | torch.isnan(dw)))
    n = cls.numel()
    for i, c in enumerate(CLASSES):
        m = cls == i
        assert bool(prop[c][m].all()), 'class %s: %d samples without its property' % (c, int((~prop[c][m]).sum()))
        if c in shares:
            assert int(m.sum()) >= 0.02 * n, 'class %s holds %d of %d samples' % (c, int(m.sum()), n)
        else:
            assert int(m.sum()) == 0
    assert int(valid.sum()) * 2 >= n, 'only %d of %d samples are valid' % (int(valid.sum()), n)
    if shares is INT_SHARES:
        ok = torch.isfinite(h) & torch.isfinite(w)
        assert bool(((h == torch.floor(h)) & (w == torch.floor(w)))[ok].all())


@functools.lru_cache(maxsize=None)
def operands(route, kind):
    """route: a row of ROUTES / GN_ROUTES; kind 'edge' (edge field, float operands) or 'int' -> x [N, C, H, W], w [O, C, 3, 3],
    off [N, 18, Ho, Wo], cls. Cached: the tests share them and leave them unchanged."""
    name, cin, cout, N, H, W, stride = route[:7]
    g = torch.Generator().manual_seed(zlib.crc32(('%s/%s/%d' % (name, kind, N)).encode()))
    x, w = (integer_operands if kind == 'int' else float_operands)(cin, cout, N, H, W, g)
    off, cls = offset_field(N, H, W, stride, 1, g, INT_SHARES if kind == 'int' else EDGE_SHARES)
    return x, w, off, cls


def float_operands(cin, cout, N, H, W, g):
    """random operands; the activations span three decades over the channels"""
    x = torch.randn(N, cin, H, W, generator=g) * torch.logspace(-1.5, 1.5, cin).view(1, cin, 1, 1)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    return x, w


def integer_operands(cin, cout, N, H, W, g):
    assert 9 * cin <= 2304 and cout >= 4
    x = torch.randint(-4, 5, (N, cin, H, W), generator=g).float()
    w = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float()
    w[1] *= 2.0 ** -9
    w[cout - 2] *= 2.0 ** 6
    return x, w
