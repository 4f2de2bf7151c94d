"""CPU: the host half of the JPEG output path (`vps_jpeg_quant_tables`, `vps_jpeg_write`: csrc/jpeg_enc_host.cpp) and the NumPy
restatement of the device half (tests/jpeg_enc_restate.py) against Pillow (libjpeg-turbo): `Image.save(format='JPEG', quality=q,
subsampling=s, optimize=False)` writes the reference file, the project's own `vps_jpeg_info` / `vps_jpeg_decode_coef` read its tables
and coefficients back, and every comparison is exact equality. The kernels themselves are compared with the restatement in
tests/test_jpeg_enc_gpu.py."""
import io

import numpy as np
import pytest

import jpeg_enc_restate as E
import jpeg_restate as R
from vps_amd import hip

SUBS = [2, 0]


def _pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == 'RGB'
        return np.asarray(im).copy()


def _read_back(host, data):
    st, info = R.jpeg_info(host, data)
    assert st == 0, st
    st, coef = R.decode_coef(host, data, info)
    assert st == 0, st
    return info, coef


def test_quant_tables_equal_pillows_for_every_quality():
    host = hip.load_host()
    img = E.smooth_noise(8, 8, 1)
    for q in range(1, 101):
        st, qt = E.quant_tables(host, q)
        assert st == 0, q
        st, info = R.jpeg_info(host, E.pil_file(img, q, 2))
        assert st == 0, q
        assert np.array_equal(qt[0], info.qt[0]) and np.array_equal(qt[1], info.qt[1]) and np.array_equal(qt[1], info.qt[2]), q
    assert E.quant_tables(host, 0)[0] <= -1000 and E.quant_tables(host, 101)[0] <= -1000


@pytest.mark.parametrize('sub', SUBS)
def test_writer_reproduces_pillows_scan_from_pillows_coefficients(sub):
    """Pillow's file -> vps_jpeg_decode_coef -> vps_jpeg_write: the same scan bytes, the same pixels, the same geometry"""
    host = hip.load_host()
    for name, img in E.images():
        H, W = img.shape[:2]
        for q in E.QUALITIES:
            ref = E.pil_file(img, q, sub)
            info, coef = _read_back(host, ref)
            st, ours = E.write_file(host, coef, H, W, sub, info.qt[:2])
            assert st == 0, (name, q, st)
            assert E.scan_of(ours) == E.scan_of(ref), (name, q)
            assert ours[-2:] == b'\xff\xd9'
            assert np.array_equal(_pil_rgb(ours), _pil_rgb(ref)), (name, q)
            st, mine = R.jpeg_info(host, ours)
            assert st == 0, (name, q, st)
            assert (mine.H, mine.W, mine.ncomp, mine.samp, mine.grid, mine.coef_bytes) == (info.H, info.W, 3, info.samp, info.grid, info.coef_bytes)
            assert mine.grid == E.grid_of(H, W, sub) and np.array_equal(mine.qt, info.qt)
            # the project's own decoder reads the same coefficients back from the project's file
            st, again = R.decode_coef(host, ours, mine)
            assert st == 0 and np.array_equal(again, coef), (name, q)


def test_writer_refuses_a_short_buffer_and_bad_arguments():
    host = hip.load_host()
    img = E.smooth_noise(24, 40, 3)
    ref = E.pil_file(img, 90, 2)
    info, coef = _read_back(host, ref)
    st, ours = E.write_file(host, coef, 24, 40, 2, info.qt[:2])
    assert st == 0
    st, exact = E.write_file(host, coef, 24, 40, 2, info.qt[:2], capacity=len(ours))       # smaller than the bound, but it fits
    assert st == 0 and exact == ours
    for cap in (len(ours) - 1, len(ours) - 2, 700, 100, 0):                                  # write_file checks the bytes behind the capacity
        st, part = E.write_file(host, coef, 24, 40, 2, info.qt[:2], capacity=cap)
        assert st <= -1000 and part == b'', cap
    assert E.write_file(host, coef, 24, 40, 1, info.qt[:2], capacity=1 << 16)[0] <= -1000    # 4:2:2 is not written
    bad = coef.copy()
    bad[5] = 3000                                                                            # no AC coefficient of 8-bit data is that large
    assert E.write_file(host, bad, 24, 40, 2, info.qt[:2])[0] <= -1000


@pytest.mark.parametrize('sub', SUBS)
def test_restated_front_end_gives_pillows_coefficients(sub):
    host = hip.load_host()
    wrong = []
    for name, img in E.images():
        H, W = img.shape[:2]
        for q in E.QUALITIES:
            info, coef = _read_back(host, E.pil_file(img, q, sub))
            st, qt = E.quant_tables(host, q)
            assert st == 0 and info.grid == E.grid_of(H, W, sub)
            got = E.restate(img, qt, sub)
            assert got.shape == coef.shape, (name, q)
            mm = int((got != coef).sum())
            print('%-18s sub %d q %3d: %d of %d coefficients differ' % (name, sub, q, mm, coef.size))
            if mm:
                wrong.append((name, q, mm))
    assert not wrong, wrong


def test_the_cases_reach_dummy_blocks_and_both_edge_stages():
    """24x40 in 4:2:0: three real luma block rows in two MCU rows, five real block columns in three MCU columns"""
    assert E.grid_of(24, 40, 2) == [(4, 6), (2, 3), (2, 3)] and E.grid_of(40, 24, 2) == [(6, 4), (3, 2), (3, 2)]
    assert E.grid_of(17, 33, 2) == [(4, 6), (2, 3), (2, 3)] and E.grid_of(17, 33, 0) == [(3, 5)] * 3
    host = hip.load_host()
    img = E.smooth_noise(24, 40, 3)
    st, qt = E.quant_tables(host, 90)
    coef = E.restate(img, qt, 2)[:24 * 64].reshape(4, 6, 64)
    assert not coef[3, :, 1:].any() and not coef[:, 5, 1:].any() and coef[:3, :5, 1:].any()
    assert np.array_equal(coef[:3, 5, 0], coef[:3, 4, 0]) and np.array_equal(coef[3, :, 0], np.repeat(coef[2, 1::2, 0], 2))


def test_render_overlay_restatement_on_a_hand_made_case():
    frame = (np.arange(4 * 5 * 3).reshape(4, 5, 3) * 4 + 3).astype(np.uint8)                 # BGR
    A, B = (200, 100, 50), (10, 250, 30)
    colour = np.zeros((4, 5, 3), np.uint8)                                                   # RGB; row 0 and column 0 stay void
    colour[1:, 1:3] = A
    colour[1:, 3:] = B
    colour[3, 4] = A                                                                         # a one-pixel segment in the last row and column
    edges = np.zeros((4, 5), bool)
    edges[0, 1:] = True                                                                      # void above a segment
    edges[1:, 0] = True                                                                      # void left of a segment
    edges[1:, 2] = True                                                                      # A | B
    edges[2, 4] = True                                                                       # B above the one-pixel segment
    edges[3, 3] = True                                                                       # B left of it
    rgb = frame[..., ::-1].astype(np.int64)
    for alpha in (0, 128, 256):
        got = E.render_overlay(frame, colour, alpha)
        assert got.dtype == np.uint8 and got.shape == (4, 5, 3)
        assert (got[edges] == 255).all()
        assert np.array_equal(got[0, 0], rgb[0, 0])                                          # void, no boundary: the frame
        for (y, x), col in (((1, 1), A), ((3, 1), A), ((1, 3), B), ((1, 4), B), ((3, 4), A)):
            assert not edges[y, x]
            want = (rgb[y, x] * (256 - alpha) + np.array(col) * alpha + 128) >> 8
            assert np.array_equal(got[y, x], want), (alpha, y, x)
        if alpha == 0:
            assert np.array_equal(got[~edges], rgb[~edges])
        if alpha == 256:
            assert np.array_equal(got[3, 4], A) and np.array_equal(got[1, 1], A)
    # the last row has no lower and the last column no right neighbour: a uniform map has no boundary at all
    flat = np.full((4, 5, 3), 77, np.uint8)
    assert not (E.render_overlay(frame, flat, 256) == 255).any()
