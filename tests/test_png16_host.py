"""CPU: `vps_png16_info` / `vps_png16_inflate` (csrc/png_host.cpp), the host half of the KITTI flow reader, and the host arithmetic of
`vps_png_encode_bound_bpp`. The inflate must deliver exactly what zlib makes of the concatenated IDAT data of a 16-bit RGB file, refuse
every other file with the family's codes without writing behind `scan_capacity`, and leave the 8-bit entry points refusing 16-bit files.
The files are written by tests/png16_cases.py."""
import ctypes
import zlib

import numpy as np
import pytest

import png16_cases as P
from vps_amd import hip

EARG = lambda x: -1000 - x
GUARD = 64


def _inflate(data, cap, fn=None):
    """-> (return code, the `cap` bytes of the buffer, the guard bytes behind them)"""
    lib = hip.load_host()
    fn = lib.vps_png16_inflate if fn is None else fn
    buf = (ctypes.c_char * max(len(data), 1)).from_buffer_copy(data or b'\0')
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    rc = fn(buf, len(data), out.ctypes.data_as(ctypes.c_void_p), cap)
    return rc, out[:cap], out[cap:]


def _info(data, fn=None):
    lib = hip.load_host()
    fn = lib.vps_png16_info if fn is None else fn
    buf = (ctypes.c_char * max(len(data), 1)).from_buffer_copy(data or b'\0')
    H, W, C = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    return fn(buf, len(data), ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)), (H.value, W.value, C.value)


CASES = [(33, 67, P.types_all_pairs(33)), (7, 5, P.types_all_pairs(7, 3)), (1, 1, [4]), (9, 1, [3, 4, 2, 1, 0, 4, 4, 3, 2]), (1, 67, [1]),
         (5, 4, [0, 0, 0, 0, 0])]


@pytest.mark.parametrize('idat_parts', [1, 5])
@pytest.mark.parametrize('H,W,types', CASES)
def test_inflate_returns_what_zlib_makes_of_the_idat_chunks(H, W, types, idat_parts):
    raw = P.noise(H, W, seed=H * 100 + W)
    data, scan = P.encode(raw, types, idat_parts=idat_parts)
    if idat_parts > 1 and H * W > 4:
        assert data.count(b'IDAT') >= 2                                            # the stream is split across chunks
    want = zlib.decompress(P.idat_of(data))
    assert want == scan and len(want) == H * (1 + 6 * W)
    assert _info(data) == (0, (H, W, 3))
    rc, got, guard = _inflate(data, len(want))
    assert rc == 0 and got.tobytes() == want and (guard == 0xA5).all()
    rc, got, guard = _inflate(data, len(want) + 7)                                 # a larger buffer: the bytes behind the scanlines stay
    assert rc == 0 and got[:len(want)].tobytes() == want and (got[len(want):] == 0xA5).all() and (guard == 0xA5).all()
    assert np.array_equal(P.unfilter(got[:len(want)], H, W), raw)                  # (and the reference's un-filter gives the image back)


def _good():
    raw = P.noise(9, 11, seed=7)
    data, scan = P.encode(raw, P.types_all_pairs(9), idat_parts=3)
    return raw, data, scan


def test_other_flavours_are_refused_with_the_flavour_code():
    raw, good, scan = _good()
    n8 = 9 * (1 + 11 * 3)
    cases = {
        '8-bit rgb': P.container(9, 11, zlib.compress(bytes(n8)), depth=8, ctype=2),
        'grey-16': P.container(9, 11, zlib.compress(bytes(9 * (1 + 11 * 2))), depth=16, ctype=0),
        'rgba-16': P.container(9, 11, zlib.compress(bytes(9 * (1 + 11 * 8))), depth=16, ctype=6),
        'palette': P.container(9, 11, zlib.compress(bytes(9 * (1 + 11))), depth=8, ctype=3),
        'interlaced': P.container(9, 11, zlib.compress(scan), interlace=1),
    }
    for name, data in cases.items():
        assert _info(data)[0] == EARG(3), name
        rc, got, guard = _inflate(data, len(scan))
        assert rc == EARG(3) and (got == 0xA5).all() and (guard == 0xA5).all(), name


def test_a_file_cut_at_every_chunk_boundary_is_refused():
    raw, good, scan = _good()
    ends = [8] + [e for _, _, e in P.chunks(good)]
    assert len(ends) == 6 and ends[-1] == len(good)                               # signature, IHDR, three IDATs, IEND
    want = [EARG(1), EARG(7), EARG(7), EARG(7), EARG(7)]                          # no IHDR; no data; part of the data; all data but no IEND
    for cut, code in zip(ends[:-1], want):
        rc, got, guard = _inflate(good[:cut], len(scan))
        assert rc == code and (guard == 0xA5).all(), (cut, rc)
    assert _inflate(good, len(scan))[0] == 0
    assert _inflate(b'', len(scan))[0] == EARG(1) and _inflate(good[:20], len(scan))[0] == EARG(1)
    # cut inside a chunk, and every shorter file down to the signature, in steps: never a crash, never a success
    for cut in range(8, len(good), 7):
        rc, _, guard = _inflate(good[:cut], len(scan))
        assert rc in (EARG(1), EARG(7)) and (guard == 0xA5).all(), (cut, rc)


def test_wrong_crc_filter_byte_5_short_stream_and_short_capacity():
    raw, good, scan = _good()
    damaged = good[:29] + bytes([good[29] ^ 1]) + good[30:]                       # the IHDR chunk's CRC
    assert _info(damaged)[0] == EARG(1) and _inflate(damaged, len(scan))[0] == EARG(1)
    field = good[:17] + bytes([good[17] ^ 1]) + good[18:]                         # a header field under a CRC that no longer fits
    assert _info(field)[0] == EARG(1)
    assert _inflate(b'\x89PNX' + good[4:], len(scan))[0] == EARG(1)
    bad = bytearray(scan)
    bad[4 * (1 + 11 * 6)] = 5                                                     # row 4 claims filter type 5
    rc, _, guard = _inflate(P.container(9, 11, zlib.compress(bytes(bad))), len(scan))
    assert rc == EARG(8) and (guard == 0xA5).all()
    stream = zlib.compress(scan)
    assert _inflate(P.container(9, 11, stream[:len(stream) // 2]), len(scan))[0] == EARG(7)
    assert _inflate(P.container(9, 11, zlib.compress(scan[:-1])), len(scan))[0] == EARG(7)
    # a stream one byte longer than the image: taken like the 8-bit path takes it, and nothing lands behind the capacity
    rc, got, guard = _inflate(P.container(9, 11, zlib.compress(scan + b'\0')), len(scan))
    assert rc == 0 and got.tobytes() == scan and (guard == 0xA5).all()
    zero_w = P.container(9, 0, zlib.compress(b''))
    assert _info(zero_w)[0] == EARG(2)
    # a capacity one byte short (and a null buffer): refused before anything is written
    rc, got, guard = _inflate(good, len(scan) - 1)
    assert rc == EARG(4) and (got == 0xA5).all() and (guard == 0xA5).all()
    buf = (ctypes.c_char * len(good)).from_buffer_copy(good)
    assert hip.load_host().vps_png16_inflate(buf, len(good), None, len(scan)) == EARG(4)
    assert hip.load_host().vps_png16_inflate(None, len(good), None, len(scan)) == EARG(1)


def test_the_8_bit_entry_points_still_refuse_the_16_bit_file_and_the_16_bit_ones_the_8_bit_file():
    lib = hip.load_host()
    raw, good, scan = _good()
    assert _info(good, lib.vps_png_info)[0] == EARG(3)
    rc, got, guard = _inflate(good, len(scan), lib.vps_png_inflate)
    assert rc == EARG(3) and (got == 0xA5).all()
    rc, got, guard = _inflate(good, 9 * 11 * 3, lib.vps_png_decode_bgr8)
    assert rc == EARG(3) and (got == 0xA5).all()
    rgb8 = P.container(9, 11, zlib.compress(bytes(9 * (1 + 11 * 3))), depth=8, ctype=2)
    assert _info(rgb8, lib.vps_png_info) == (0, (9, 11, 3)) and _info(rgb8)[0] == EARG(3)
    # an 8-bit file without its IEND chunk is still taken by the 8-bit path (the 16-bit path asks for the chunk)
    assert _inflate(rgb8[:-12], 9 * (1 + 11 * 3), lib.vps_png_inflate)[0] == 0


def test_python_bindings():
    from vps_amd import kittiflow
    raw, good, scan = _good()
    assert kittiflow.png16_info(good) == (9, 11) and kittiflow.png16_info(good[:33]) == (9, 11)
    assert kittiflow.png16_info(P.container(9, 11, b'', depth=8)) is None
    got, H, W = kittiflow.png16_inflate(good)
    assert (H, W) == (9, 11) and got.tobytes() == scan
    with pytest.raises(ValueError):
        kittiflow.png16_inflate(P.container(9, 11, b'', depth=8))
    with pytest.raises(hip.VpsHipError):
        kittiflow.png16_inflate(good[:-12])


def test_encode_bound_bpp_covers_the_worst_case_and_refuses_other_pixel_sizes():
    lib = hip.load()
    SEG = 8192

    def bound(H, rowbytes, bpp):
        cap, ws = ctypes.c_int64(-1), ctypes.c_int64(-1)
        return lib.vps_png_encode_bound_bpp(H, rowbytes, bpp, ctypes.byref(cap), ctypes.byref(ws)), cap.value, ws.value
    for H, W in ((1, 1), (7, 5), (33, 67), (375, 1242), (1024, 2048)):
        rc, cap, ws = bound(H, 6 * W, 6)
        assert rc == 0
        N = H * (1 + 6 * W)
        nseg = -(-N // SEG)
        # the worst case of the documented stream: every byte a 9-bit literal; per segment 3 header bits, 7 bits end of block, 3 bits and
        # the padding of the stored block with its 4 bytes; 2 bytes in front, 03 00 and the Adler-32 behind
        worst = 2 + sum((3 + 9 * min(SEG, N - k * SEG) + 7 + 3 + 7) // 8 + 4 for k in range(nseg)) + 6
        assert cap >= worst and ws >= H + nseg * ((9 * SEG + 7) // 8 + 7), (H, W, cap, worst)
        # the same figures as the 8-bit entry point gives for a row of as many bytes
        cap3, ws3 = ctypes.c_int64(), ctypes.c_int64()
        assert lib.vps_png_encode_bound(H, 2 * W, 3, ctypes.byref(cap3), ctypes.byref(ws3)) == 0 and (cap3.value, ws3.value) == (cap, ws)
        assert bound(H, 6 * W, 3)[:2] == (0, cap) and bound(H, 6 * W, 1)[:2] == (0, cap)
    for bpp in (2, 4, 0, 5, 8, -1):
        assert bound(7, 6 * 5 * 4, bpp)[0] == EARG(2), bpp
    assert bound(0, 30, 6)[0] == EARG(1) and bound(7, 0, 6)[0] == EARG(1) and bound(7, 31, 6)[0] == EARG(1) and bound(65536, 30, 6)[0] == EARG(1)
    assert bound(7, 6 * 65536, 6)[0] == EARG(1) and bound(7, 6 * 65535, 6)[0] == 0
    assert lib.vps_png_encode_bound_bpp(7, 30, 6, None, None) == EARG(3)
    # the old entry point keeps its refusals
    cap, ws = ctypes.c_int64(), ctypes.c_int64()
    assert lib.vps_png_encode_bound(7, 5, 6, ctypes.byref(cap), ctypes.byref(ws)) == EARG(2)
