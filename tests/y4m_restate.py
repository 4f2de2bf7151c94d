"""NumPy restatement of the two Y4M conversions (`vps_yuv_to_bgr`, `vps_bgr_to_yuv`; include/vps_hip.h states the arithmetic). The integer
coefficients are derived HERE, in float64, from (Kr, Kb) and the range - the library's table (csrc/yuv_tables.h) is not imported. The
real-valued conversions the integers approximate are here too (`decode_real`, `encode_real`), for tests/test_y4m.py."""
import numpy as np

KRKB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
SAMPLINGS = ('420jpeg', '420mpeg2', '422', '444', 'mono')


def scales(rng):
    """(luma offset, luma levels, chroma levels) of a range"""
    return (16, 219.0, 224.0) if rng == 'limited' else (0, 255.0, 255.0)


def q16(c):
    return int(np.floor(np.float64(c) * 65536.0 + 0.5))


def real_coefficients(matrix, rng):
    """decode: ky, cr_r, cb_g, cr_g, cb_b; encode rows y, cb, cr in (R, G, B) order - real numbers"""
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    _, yl, cl = scales(rng)
    ys, cs = yl / 255.0, cl / 255.0
    dec = dict(ky=1.0 / ys, cr_r=2.0 * (1.0 - kr) / cs, cb_g=-2.0 * kb * (1.0 - kb) / kg / cs, cr_g=-2.0 * kr * (1.0 - kr) / kg / cs,
               cb_b=2.0 * (1.0 - kb) / cs)
    enc = dict(y=(kr * ys, kg * ys, kb * ys),
               cb=(-kr / (2.0 * (1.0 - kb)) * cs, -kg / (2.0 * (1.0 - kb)) * cs, 0.5 * cs),
               cr=(0.5 * cs, -kg / (2.0 * (1.0 - kr)) * cs, -kb / (2.0 * (1.0 - kr)) * cs))
    return dec, enc


def int_coefficients(matrix, rng):
    dec, enc = real_coefficients(matrix, rng)
    return {k: q16(v) for k, v in dec.items()}, {k: tuple(q16(c) for c in v) for k, v in enc.items()}


def plane_size(H, W, sampling):
    hw, hh = (W + 1) // 2, (H + 1) // 2
    return {'420jpeg': (hh, hw), '420mpeg2': (hh, hw), '422': (H, hw), '444': (H, W), 'mono': (0, 0)}[sampling]


def frame_bytes(H, W, sampling):
    ch, cw = plane_size(H, W, sampling)
    return H * W + 2 * ch * cw


def split(planar, H, W, sampling):
    planar = np.asarray(planar, dtype=np.uint8).reshape(-1)
    ch, cw = plane_size(H, W, sampling)
    y = planar[:H * W].reshape(H, W)
    cb = planar[H * W:H * W + ch * cw].reshape(ch, cw)
    cr = planar[H * W + ch * cw:H * W + 2 * ch * cw].reshape(ch, cw)
    return y, cb, cr


def _axis(n, cn, mode):
    """per output position: (index of the first sample, index of the second, weight, weight), weights summing to 4, indices clamped"""
    x = np.arange(n)
    if mode == 'none':
        return x, x, np.full(n, 4), np.zeros(n, dtype=np.int64)
    j = x // 2
    odd = (x & 1) == 1
    if mode == 'centre':                                   # the sample the position lies in: 3, its neighbour on the nearer side: 1
        other = np.clip(np.where(odd, j + 1, j - 1), 0, cn - 1)
        return j, other, np.full(n, 3), np.ones(n, dtype=np.int64)
    assert mode == 'cosited'                                # even positions sit on a sample, odd ones half-way to the next
    return j, np.clip(j + 1, 0, cn - 1), np.where(odd, 2, 4), np.where(odd, 2, 0)


SITING = {'420jpeg': ('centre', 'centre'), '420mpeg2': ('centre', 'cosited'), '422': ('none', 'cosited'), '444': ('none', 'none')}   # (vertical, horizontal)


def upsample(c, H, W, sampling):
    """chroma plane -> [H, W] int64, (sum wy wx s + 8) >> 4"""
    vm, hm = SITING[sampling]
    c = c.astype(np.int64)
    r0, r1, wr0, wr1 = _axis(H, c.shape[0], vm)
    c0, c1, wc0, wc1 = _axis(W, c.shape[1], hm)
    s = (wr0[:, None] * wc0[None, :]) * c[r0][:, c0] + (wr0[:, None] * wc1[None, :]) * c[r0][:, c1] \
        + (wr1[:, None] * wc0[None, :]) * c[r1][:, c0] + (wr1[:, None] * wc1[None, :]) * c[r1][:, c1]
    return (s + 8) >> 4


def decode_pixels(y, cb, cr, matrix='bt601', rng='limited'):
    """integer arrays of equal shape -> (B, G, R) uint8"""
    d, _ = int_coefficients(matrix, rng)
    yoff = scales(rng)[0]
    yy = d['ky'] * (y.astype(np.int64) - yoff) + 32768
    u, v = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    b = (yy + d['cb_b'] * u) >> 16
    g = (yy + d['cb_g'] * u + d['cr_g'] * v) >> 16
    r = (yy + d['cr_r'] * v) >> 16
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (b, g, r))


def yuv_to_bgr(planar, H, W, sampling='420jpeg', rng='limited', matrix='bt601'):
    """uint8 planar frame -> BGR uint8 [H, W, 3]"""
    y, cb, cr = split(planar, H, W, sampling)
    if sampling == 'mono':
        u = v = np.full((H, W), 128, dtype=np.int64)
    else:
        u, v = upsample(cb, H, W, sampling), upsample(cr, H, W, sampling)
    return np.stack(decode_pixels(y, u, v, matrix, rng), axis=2)


def encode_pixels(b, g, r, matrix='bt601', rng='limited'):
    """integer arrays -> (Y, Cb, Cr) int64, rounded and clamped per pixel"""
    _, e = int_coefficients(matrix, rng)
    yoff = scales(rng)[0]
    lo, yhi, chi = (16, 235, 240) if rng == 'limited' else (0, 255, 255)
    b, g, r = (a.astype(np.int64) for a in (b, g, r))
    y = (e['y'][0] * r + e['y'][1] * g + e['y'][2] * b + (yoff << 16) + 32768) >> 16
    cb = (e['cb'][0] * r + e['cb'][1] * g + e['cb'][2] * b + (128 << 16) + 32768) >> 16
    cr = (e['cr'][0] * r + e['cr'][1] * g + e['cr'][2] * b + (128 << 16) + 32768) >> 16
    return np.clip(y, lo, yhi), np.clip(cb, lo, chi), np.clip(cr, lo, chi)


def reduce_chroma(c, sampling):
    """full-resolution chroma [H, W] int64 -> the plane of `sampling`; source indices clamped to the image"""
    if sampling == '444':
        return c
    H, W = c.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    r0, r1 = 2 * np.arange(ch), np.minimum(2 * np.arange(ch) + 1, H - 1)
    rows = c[r0] + c[r1]
    x = 2 * np.arange(cw)
    if sampling == '420jpeg':
        return (rows[:, x] + rows[:, np.minimum(x + 1, W - 1)] + 2) >> 2
    assert sampling == '420mpeg2'
    return (rows[:, np.maximum(x - 1, 0)] + 2 * rows[:, x] + rows[:, np.minimum(x + 1, W - 1)] + 4) >> 3


def bgr_to_yuv(bgr, sampling='420jpeg', rng='limited', matrix='bt601'):
    """BGR uint8 [H, W, 3] -> uint8 planar frame (Y, Cb, Cr)"""
    bgr = np.asarray(bgr)
    y, cb, cr = encode_pixels(bgr[:, :, 0], bgr[:, :, 1], bgr[:, :, 2], matrix, rng)
    return np.concatenate([p.astype(np.uint8).reshape(-1) for p in (y, reduce_chroma(cb, sampling), reduce_chroma(cr, sampling))])


def half_up(x):
    return np.floor(x + 0.5)


def decode_real(y, cb, cr, matrix, rng):
    """the real-valued conversion in float64, rounded half up and clamped -> (B, G, R) int64"""
    d, _ = real_coefficients(matrix, rng)
    yoff = scales(rng)[0]
    yy = d['ky'] * (y.astype(np.float64) - yoff)
    u, v = cb.astype(np.float64) - 128.0, cr.astype(np.float64) - 128.0
    out = (yy + d['cb_b'] * u, yy + d['cb_g'] * u + d['cr_g'] * v, yy + d['cr_r'] * v)
    return tuple(np.clip(half_up(a), 0, 255).astype(np.int64) for a in out)


def encode_real(b, g, r, matrix, rng):
    _, e = real_coefficients(matrix, rng)
    yoff = scales(rng)[0]
    lo, yhi, chi = (16, 235, 240) if rng == 'limited' else (0, 255, 255)
    b, g, r = (a.astype(np.float64) for a in (b, g, r))
    y = yoff + e['y'][0] * r + e['y'][1] * g + e['y'][2] * b
    cb = 128.0 + e['cb'][0] * r + e['cb'][1] * g + e['cb'][2] * b
    cr = 128.0 + e['cr'][0] * r + e['cr'][1] * g + e['cr'][2] * b
    return (np.clip(half_up(y), lo, yhi).astype(np.int64), np.clip(half_up(cb), lo, chi).astype(np.int64),
            np.clip(half_up(cr), lo, chi).astype(np.int64))


def cube_slabs():
    """the 2^24 colour cube in 256 slabs: (first coordinate scalar array, second [256,1], third [1,256]) broadcastable int64"""
    b = np.arange(256, dtype=np.int64)
    for a in range(256):
        yield np.full((1, 1), a, dtype=np.int64), b[:, None], b[None, :]


def round_trip_error(matrix, rng):
    """max |decode444(encode444(BGR)) - BGR| of the restatement over the whole BGR cube"""
    worst = 0
    for b, g, r in cube_slabs():
        b, g, r = np.broadcast_arrays(b, g, r)
        back = decode_pixels(*encode_pixels(b, g, r, matrix, rng), matrix, rng)
        worst = max(worst, max(int(np.abs(x.astype(np.int64) - s).max()) for x, s in zip(back, (b, g, r))))
    return worst
