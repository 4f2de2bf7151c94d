"""NumPy restatement of the device half of the JPEG OUTPUT path (`vps_amd/csrc/jpeg_enc_ops.hip`): RGB uint8 -> quantised coefficients
in the layout of `vps_jpeg_decode_coef`, and the overlay renderer in front of it. Written from the published algorithms of libjpeg's
default compressor: jccolor.c (16-bit fixed-point RGB -> YCbCr), jcsample.c (h2v2 box filter, bias alternating 1, 2; the right edge
replicated in the SOURCE), jcprepct.c (the bottom edge: source rows replicated to a whole row group, then the last row of every
component repeated to a whole iMCU row), jfdctint.c (jpeg_fdct_islow: rows first), jcdctmgr.c (rounded division by 8 * table entry)
and jccoefct.c (dummy blocks: AC zero, DC of the preceding block of the MCU). tests/test_jpeg_enc.py pins it to Pillow
(libjpeg-turbo) coefficient by coefficient; the GPU tests compare the kernels with it. The ctypes helpers call the host functions
of the library the way tests/jpeg_restate.py does for the input path."""
import ctypes

import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)

SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """d: eight int64 arrays (the 8 inputs of one 1-D transform) -> eight outputs; `first` = the row pass"""
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << PASS1_BITS, (tmp10 - tmp11) << PASS1_BITS
    else:
        o[0], o[4] = _descale(tmp10 + tmp11, PASS1_BITS), _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * F['f0_541']
    o[2] = _descale(z1 + tmp13 * F['f0_765'], sh)
    o[6] = _descale(z1 + tmp12 * -F['f1_847'], sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F['f1_175']
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F['f0_298'], tmp5 * F['f2_053'], tmp6 * F['f3_072'], tmp7 * F['f1_501']
    z1, z2, z3, z4 = z1 * -F['f0_899'], z2 * -F['f2_562'], z3 * -F['f1_961'] + z5, z4 * -F['f0_390'] + z5
    o[7] = _descale(tmp4 + z1 + z3, sh)
    o[5] = _descale(tmp5 + z2 + z4, sh)
    o[3] = _descale(tmp6 + z2 + z3, sh)
    o[1] = _descale(tmp7 + z1 + z4, sh)
    return o


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode='edge')


def h2v2(p):
    """p: int64 [even rows, even columns] -> the box-filtered plane, the bias 1 on even and 2 on odd output columns"""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2, 2, 1)[None, :]
    return (s + bias) >> 2


def grid_of(H, W, sub):
    """[(block rows, block columns)] of the three components, padded to whole MCUs (what vps_jpeg_info reports for such a file)"""
    m = 16 if sub == 2 else 8
    mr, mc = -(-H // m), -(-W // m)
    f = m // 8
    return [(mr * f, mc * f), (mr, mc), (mr, mc)]


def fdct_quant(plane, q):
    """int64 sample plane [8 * rows, 8 * cols] -> int64 [rows, cols, 64] quantised coefficients in natural order"""
    rows, cols = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3) - 128                           # [rows, cols, y, x]
    ws = np.stack(_fdct_pass([x[..., k] for k in range(8)], True), -1)                         # pass 1: along every row
    out = np.stack(_fdct_pass([ws[..., k, :] for k in range(8)], False), -2)                   # pass 2: along every column
    qv = q.reshape(8, 8).astype(np.int64) * 8
    a = (np.abs(out) + (qv >> 1)) // qv
    return (np.where(out < 0, -a, a)).reshape(rows, cols, 64)


def restate(rgb, qt, sub):
    """what vps_jpeg_encode_coef computes: RGB uint8 [H, W, 3], qt [2][64], sub 0 / 2 -> int16 coefficients, flat"""
    H, W = rgb.shape[:2]
    grid = grid_of(H, W, sub)
    y, cb, cr = rgb_to_ycc(rgb)
    wb, hb = -(-W // 8), -(-H // 8)                                               # luma blocks that hold pixels
    out = []
    for c, p in enumerate((y, cb, cr)):
        br, bc = grid[c]
        if c == 0 or sub == 0:
            real = fdct_quant(_pad_edge(p, hb * 8, wb * 8), qt[min(c, 1)])
        else:
            ch = -(-H // 2)
            src = _pad_edge(p, 2 * ch, bc * 16)                                   # source rows to a whole row group, columns to whole blocks
            real = fdct_quant(_pad_edge(h2v2(src), br * 8, bc * 8), qt[1])        # then the last down-sampled row is repeated
        full = np.zeros((br, bc, 64), dtype=np.int64)
        full[:real.shape[0], :real.shape[1]] = real
        # dummy blocks, in MCU order: right of the last real column the DC of the block to the left; in a dummy row the DC of the
        # right block of the row above (by then filled)
        for bx in range(real.shape[1], bc):
            full[:real.shape[0], bx, 0] = full[:real.shape[0], bx - 1, 0]
        for by in range(real.shape[0], br):
            full[by, :, 0] = np.repeat(full[by - 1, 1::2, 0], 2)
        out.append(full.reshape(-1))
    return np.concatenate(out).astype(np.int16)


def render_overlay(frame_bgr, colour_rgb, alpha):
    """what vps_overlay_render computes -> RGB uint8 [H, W, 3]"""
    f = frame_bgr[..., ::-1].astype(np.int64)
    c = colour_rgb.astype(np.int64)
    out = (f * (256 - alpha) + c * alpha + 128) >> 8
    void = (colour_rgb == 0).all(-1)
    out[void] = f[void]
    edge = np.zeros(void.shape, dtype=bool)
    edge[:, :-1] |= (colour_rgb[:, :-1] != colour_rgb[:, 1:]).any(-1)
    edge[:-1, :] |= (colour_rgb[:-1, :] != colour_rgb[1:, :]).any(-1)
    out[edge] = 255
    return out.astype(np.uint8)


# ---- inputs of the tests (seeded; the sizes reach every edge rule) ----
SIZES = [(8, 8), (16, 16), (17, 33), (24, 40), (40, 24), (64, 96)]
QUALITIES = [1, 50, 75, 90, 100]


def smooth_noise(H, W, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0), 128 + 90 * np.cos(xx / 11.0 - yy / 9.0), 40 + 3.0 * xx + 1.5 * yy], -1)
    return np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def primaries(H, W):
    pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(pal[(xx // 3 + yy // 5) % 8])


def constant(H, W):
    return np.full((H, W, 3), (200, 30, 90), np.uint8)


def images():
    """[(name, RGB uint8)]: a smooth-plus-noise image per size, saturated primaries and a constant image"""
    out = [('noise_%dx%d' % s, smooth_noise(s[0], s[1], 7 + i)) for i, s in enumerate(SIZES)]
    return out + [('primaries_24x40', primaries(24, 40)), ('constant_17x33', constant(17, 33))]


# ---- the library's host functions ----
def quant_tables(host, quality):
    qt = np.zeros((2, 64), dtype=np.uint16)
    st = host.vps_jpeg_quant_tables(quality, qt.ctypes.data_as(ctypes.c_void_p))
    return st, qt


def write_file(host, coef, H, W, sub, qt, capacity=None):
    """vps_jpeg_write -> (status, bytes)"""
    if capacity is None:
        cap = ctypes.c_int64(0)
        assert host.vps_jpeg_write_bound(H, W, sub, ctypes.byref(cap)) == 0
        capacity = cap.value
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    qt = np.ascontiguousarray(qt, dtype=np.uint16)
    out = np.full(capacity + 64, 0xA5, dtype=np.uint8)                           # the tail must stay as it is
    n = ctypes.c_int64(-1)
    st = host.vps_jpeg_write(coef.ctypes.data_as(ctypes.c_void_p), H, W, sub, qt.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                             capacity, ctypes.byref(n))
    assert (out[capacity:] == 0xA5).all(), 'vps_jpeg_write stored beyond its capacity'
    return st, out[:max(n.value, 0)].tobytes()


def pil_file(rgb, quality, sub):
    import io

    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format='JPEG', quality=quality, subsampling=sub, optimize=False)
    return b.getvalue()


def scan_of(data):
    """the bytes from the SOS marker to the end of the file"""
    pos = 2
    while data[pos + 1] != 0xDA:                                                 # walk the segments: a table may hold the bytes FF DA
        assert data[pos] == 0xFF
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return data[pos:]
