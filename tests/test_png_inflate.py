"""CPU: `vps_png_inflate` (csrc/png_host.cpp), the host half of the opt-in PNG path whose un-filter runs on the device. It must deliver
exactly what zlib makes of the concatenated IDAT data, refuse what `vps_png_decode_bgr8` refuses with the same codes, and leave the
decoder (which now shares the chunk walk and the inflate with it) as it was."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest
import torch

import png_filter_cases as P
from vps_amd import hip
from vps_amd.pipeline import ClipFeeder, png_decode, png_inflate

EARG = lambda x: -1000 - x


def _call(fn, data, cap):
    """-> (return code, output bytes) of one of the two host functions on `data` with an output buffer of `cap` bytes"""
    buf = (ctypes.c_char * len(data)).from_buffer_copy(data)
    out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    return fn(buf, len(data), out.ctypes.data_as(ctypes.c_void_p), cap), out[:cap]


def _idat(data):
    """the concatenated IDAT payloads of a PNG file"""
    pos, got = 8, b''
    while pos + 12 <= len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b'IDAT':
            got += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return got


@pytest.mark.parametrize('C', [1, 3, 4])
def test_inflate_returns_what_zlib_makes_of_the_idat_chunks(C):
    lib = hip.load_host()
    H, W = 33, 67
    img = P.noise(H, W, C, seed=C)
    data, raw = P.encode(img, P.types_all_pairs(H), idat_parts=5)
    assert data.count(b'IDAT') >= 5
    want = zlib.decompress(_idat(data))
    assert want == raw and len(want) == H * (1 + W * C)
    rc, got = _call(lib.vps_png_inflate, data, len(want))
    assert rc == 0 and got.tobytes() == want
    scan, pi = png_inflate(data)
    assert (pi.H, pi.W, pi.C, pi.scan_bytes) == (H, W, C, len(want)) and scan.tobytes() == want
    # a larger buffer: the bytes behind the scanlines are not touched
    rc, got = _call(lib.vps_png_inflate, data, len(want) + 7)
    assert rc == 0 and got[:len(want)].tobytes() == want and (got[len(want):] == 0xA5).all()


def _refusals():
    img = P.noise(9, 11, 3, seed=7)
    good, raw = P.encode(img, P.types_all_pairs(9))
    stream = zlib.compress(raw, 6)
    cases = {
        'palette': P.container(9, 11, 1, zlib.compress(P.filtered(img[:, :, 0], [0] * 9)), ctype=3),
        '16-bit': P.container(9, 11, 3, zlib.compress(bytes(9 * (1 + 11 * 6))), depth=16),
        'interlaced': P.container(9, 11, 3, stream, interlace=1),
        'truncated stream': P.container(9, 11, 3, stream[:len(stream) // 2]),
        'truncated file': good[:len(good) - 40],
        'short stream': P.container(9, 11, 3, zlib.compress(raw[:-1], 6)),
        'not a png': b'\x89PNX' + good[4:],
        'damaged header': good[:17] + bytes([good[17] ^ 1]) + good[18:],
    }
    bad = bytearray(raw)
    bad[4 * (1 + 11 * 3)] = 5                                    # row 4 claims filter type 5
    cases['filter byte 5'] = P.container(9, 11, 3, zlib.compress(bytes(bad), 6))
    return good, cases


def test_refusals_are_the_decoders():
    lib = hip.load_host()
    good, cases = _refusals()
    scan_bytes, bgr_bytes = 9 * (1 + 11 * 3), 9 * 11 * 3
    want = {'palette': EARG(3), '16-bit': EARG(3), 'interlaced': EARG(3), 'truncated stream': EARG(7), 'truncated file': EARG(7),
            'short stream': EARG(7), 'not a png': EARG(1), 'damaged header': EARG(1), 'filter byte 5': EARG(8)}
    for name, data in cases.items():
        rc_i, _ = _call(lib.vps_png_inflate, data, scan_bytes)
        rc_d, _ = _call(lib.vps_png_decode_bgr8, data, bgr_bytes)
        assert rc_i == rc_d == want[name], (name, rc_i, rc_d)
    # capacity one byte short (and a null buffer): refused before anything is written
    rc_i, out = _call(lib.vps_png_inflate, good, scan_bytes - 1)
    rc_d, _ = _call(lib.vps_png_decode_bgr8, good, bgr_bytes - 1)
    assert rc_i == rc_d == EARG(4) and (out == 0xA5).all()
    buf = (ctypes.c_char * len(good)).from_buffer_copy(good)
    assert lib.vps_png_inflate(buf, len(good), None, scan_bytes) == EARG(4)
    assert _call(lib.vps_png_inflate, good, scan_bytes)[0] == 0
    # the Python helper: None for a flavour the native path does not take, like png_decode
    assert png_inflate(cases['palette']) is None and png_decode(cases['palette']) is None
    with pytest.raises(hip.VpsHipError):
        png_inflate(cases['filter byte 5'])


@pytest.mark.parametrize('C', [1, 3, 4])
def test_decoder_still_equals_pil_and_the_original(C):
    from PIL import Image
    for (H, W), seed, high in (((33, 67), 10, 256), ((7, 5), 11, 256), ((26, 9), 12, 4)):
        img = P.noise(H, W, C, seed=seed + C, high=high)
        data, _ = P.encode(img, P.types_all_pairs(H))
        got = png_decode(data)
        assert got is not None and np.array_equal(got, P.bgr(img)), (C, H, W)
        with Image.open(io.BytesIO(data)) as im:
            pil = np.asarray(im.convert('RGB'))
        assert np.array_equal(got, pil[:, :, ::-1]), (C, H, W)


def test_feeder_png_device_on_a_host_prep_delivers_what_png_host_delivers(tmp_path):
    """without a device `png='device'` decodes on the host, as a JPEG does (the reconstruction has no CPU twin)"""
    files = []
    for t in range(4):
        img = P.noise(16, 24, (3, 4, 1, 3)[t], seed=40 + t)
        fn = tmp_path / ('f%d.png' % t)
        fn.write_bytes(P.encode(img, P.types_all_pairs(16))[0])
        files.append(str(fn))

    class HostPrep:                                              # stand-in for DeviceImagePrep on a host without a GPU
        device = torch.device('cpu')

        def prep(self, img):
            a = np.asarray(img)
            return torch.from_numpy(a.astype(np.float32).transpose(2, 0, 1).copy()), a.shape, a.shape, 1.0

    got = {}
    for mode in ('host', 'device'):
        fd = ClipFeeder(files, HostPrep(), workers=2, png=mode)
        got[mode] = [(fd(t).clone(), fd.meta(t)) for t in range(4)]
        fd.close()
        assert fd.fallback_decodes == 0 and fd.native_png_device == 0 and fd.decodes == 4
    for (a, ma), (b, mb) in zip(got['host'], got['device']):
        assert torch.equal(a, b) and ma == mb
    with pytest.raises(AssertionError):
        ClipFeeder(files, HostPrep(), png='gpu')
