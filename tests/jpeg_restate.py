"""NumPy restatement of the device half of the JPEG path (`vps_amd/csrc/jpeg_ops.hip`): quantised coefficients -> BGR uint8, in the
integer arithmetic libjpeg's default decode defines. Written from the published algorithms of jidctint.c (jpeg_idct_islow: 13-bit
constants, PASS1_BITS 2, two DESCALE roundings, the `& 1023` range-limit table), jdsample.c (h2v1 / h2v2 fancy upsampling, chosen
only for a down-sampled width above 2, edges at the true down-sampled size) and jdcolor.c (16-bit fixed-point YCbCr -> RGB).
The tests compare it with PIL's decode (libjpeg-turbo) - it is the CPU twin the device stage itself does not have."""
import ctypes

import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(v, shift):
    """v: eight int64 arrays (the 8 inputs of one 1-D transform) -> eight outputs, descaled by `shift`"""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * F['f0_541']
    tmp2 = z1 + z3 * (-F['f1_847'])
    tmp3 = z1 + z2 * F['f0_765']
    z2, z3 = v[0], v[4]
    tmp0 = (z2 + z3) << CONST_BITS
    tmp1 = (z2 - z3) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F['f1_175']
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F['f0_298'], tmp1 * F['f2_053'], tmp2 * F['f3_072'], tmp3 * F['f1_501']
    z1, z2, z3, z4 = z1 * -F['f0_899'], z2 * -F['f2_562'], z3 * -F['f1_961'], z4 * -F['f0_390']
    z3, z4 = z3 + z5, z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [_descale(tmp10 + tmp3, shift), _descale(tmp11 + tmp2, shift), _descale(tmp12 + tmp1, shift), _descale(tmp13 + tmp0, shift),
            _descale(tmp13 - tmp0, shift), _descale(tmp12 - tmp1, shift), _descale(tmp11 - tmp2, shift), _descale(tmp10 - tmp3, shift)]


def idct_plane(coef, q, brows, bcols):
    """coef int16 [brows*bcols*64] (natural order), q [64] -> uint8 sample plane [brows*8, bcols*8]"""
    x = coef.reshape(brows * bcols, 8, 8).astype(np.int64) * q.reshape(1, 8, 8).astype(np.int64)
    ws = np.stack(_idct_pass([x[:, r, :] for r in range(8)], CONST_BITS - PASS1_BITS), 1)           # pass 1: columns
    out = np.stack(_idct_pass([ws[:, :, c] for c in range(8)], CONST_BITS + PASS1_BITS + 3), 2)      # pass 2: rows
    s = ((out + 512) & 1023) - 512 + 128                       # range_limit[x & RANGE_MASK]: 10-bit wrap, then the clamp
    px = np.clip(s, 0, 255).astype(np.uint8)
    return px.reshape(brows, bcols, 8, 8).transpose(0, 2, 1, 3).reshape(brows * 8, bcols * 8)


def _h2_fancy(t, bias_even, bias_odd, shift):
    """columns of t (int64 [rows, cw]) doubled with the 3:1 triangle filter, edge columns replicated"""
    p = np.pad(t, ((0, 0), (1, 1)), mode='edge')
    out = np.empty((t.shape[0], t.shape[1] * 2), dtype=np.int64)
    out[:, 0::2] = (3 * t + p[:, :-2] + bias_even) >> shift
    out[:, 1::2] = (3 * t + p[:, 2:] + bias_odd) >> shift
    return out


def upsample(plane, H, W, hs, vs):
    """chroma plane (padded) -> [H, W] at full resolution, as jdsample.c does for luma sampling (hs, vs) and 1x1 chroma"""
    if hs == 1 and vs == 1:
        return plane[:H, :W].astype(np.int64)
    assert hs == 2 and vs in (1, 2)
    cw = (W + 1) // 2
    ch = (H + 1) // 2 if vs == 2 else H
    t = plane[:ch, :cw].astype(np.int64)                         # the TRUE down-sampled size: the MCU padding takes no part
    if cw <= 2:                                                  # no fancy upsampling for such a narrow plane: box replication
        return np.repeat(np.repeat(t, vs, 0), 2, 1)[:H, :W]
    if vs == 1:
        return _h2_fancy(t, 1, 2, 2)[:H, :W]
    p = np.pad(t, ((1, 1), (0, 0)), mode='edge')
    rows = np.empty((ch * 2, cw), dtype=np.int64)
    rows[0::2] = 3 * t + p[:-2]                                  # upper output row: 3 * this row + the row above
    rows[1::2] = 3 * t + p[2:]                                   # lower output row: 3 * this row + the row below
    return _h2_fancy(rows, 8, 7, 4)[:H, :W]


def ycc_to_bgr(y, cb, cr):
    y, u, v = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * v + 32768) >> 16)
    g = y + ((-22554 * u - 46802 * v + 32768) >> 16)
    b = y + ((116130 * u + 32768) >> 16)
    return np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8)


class Info:
    pass


def jpeg_info(lib, data):
    """vps_jpeg_info on the file's bytes -> (status, Info)"""
    buf = (ctypes.c_char * len(data)).from_buffer_copy(bytes(data))
    H, W, nc, nb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    samp, grid = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    qt = np.zeros((3, 64), dtype=np.uint16)
    st = lib.vps_jpeg_info(buf, len(data), ctypes.byref(H), ctypes.byref(W), ctypes.byref(nc), samp, grid, qt.ctypes.data_as(ctypes.c_void_p),
                           ctypes.byref(nb))
    i = Info()
    i.H, i.W, i.ncomp, i.coef_bytes, i.qt = H.value, W.value, nc.value, nb.value, qt
    i.samp = [(samp[2 * c], samp[2 * c + 1]) for c in range(3)]
    i.grid = [(grid[2 * c], grid[2 * c + 1]) for c in range(3)]
    return st, i


def decode_coef(lib, data, info):
    buf = (ctypes.c_char * len(data)).from_buffer_copy(bytes(data))
    coef = np.full(info.coef_bytes // 2, 0x5A5A, dtype=np.int16)             # poisoned: the decoder must write every coefficient
    st = lib.vps_jpeg_decode_coef(buf, len(data), coef.ctypes.data_as(ctypes.c_void_p), coef.nbytes)
    return st, coef


def restate(coef, info):
    """what vps_jpeg_reconstruct computes: coefficients + geometry -> BGR uint8 [H, W, 3]"""
    planes, off = [], 0
    for c in range(info.ncomp):
        br, bc = info.grid[c]
        n = br * bc * 64
        planes.append(idct_plane(coef[off:off + n], info.qt[c], br, bc))
        off += n
    H, W = info.H, info.W
    if info.ncomp == 1:
        return np.ascontiguousarray(np.repeat(planes[0][:H, :W, None], 3, 2))
    hs, vs = info.samp[0]
    return ycc_to_bgr(planes[0][:H, :W], upsample(planes[1], H, W, hs, vs), upsample(planes[2], H, W, hs, vs))
