"""CPU: the stream format of the device PNG encoder, checked on its NumPy restatement (tests/png_restate.py) for every case of
tests/png_cases.py: PIL and the library's own PNG decoder read the file back, zlib inflates its IDAT to the filtered stream S with the
filter bytes the format defines; `vps_png_encode_bound` covers the worst case and refuses bad arguments."""
import ctypes
import io
import zlib

import numpy as np
import pytest

import png_cases
import png_restate as R
from vps_amd import hip

NAMES = sorted(png_cases.cases())


def _bound(H, W, C):
    cap, wsb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = hip.load().vps_png_encode_bound(H, W, C, ctypes.byref(cap), ctypes.byref(wsb))
    return rc, cap.value, wsb.value


def test_the_case_list_is_the_one_the_format_needs():
    c = png_cases.cases()
    assert {'1x1x1', '1x1x3', '1x7x3', '5x1x3', 'runs', 'lit144', 'const', 'twos', 'up2', 'noise', 'ff_rgb', 'ff_grey', 'labels', 'full'} <= set(c)
    assert sum(k.startswith('align') for k in c) == 8
    assert c['const'].size == 3 * (R.SEG + 5) and c['full'].shape == (1088, 1920, 3) and c['noise'].shape == (64, 96, 3)
    assert [c[k].shape for k in ('1x1x1', '1x1x3', '1x7x3', '5x1x3')] == [(1, 1), (1, 1, 3), (1, 7, 3), (5, 1, 3)]   # rows of 2, 4, 22, 4 bytes
    assert sorted(np.unique(R.filter_rows(c['noise'])[1])) == [0, 1, 2]        # every filter type is chosen somewhere
    S, ft = R.filter_rows(c['up2'])
    assert ft.tolist()[1] == 2 and S[41:].tolist() == [2] * 41               # the Up filter byte merges into the run of 2s
    assert len(R.filter_rows(c['full'])[0]) // R.SEG + 1 > 2 * 256             # more segments than the scan kernel's block of 256 takes in two steps
    # the run case: every rest length 0..6 and the 258 cap once and twice, each followed by rests 0..4
    S = R.filter_rows(c['runs'])[0]
    starts = np.flatnonzero(np.concatenate(([True], S[1:] != S[:-1])))
    lens = set(np.diff(np.concatenate((starts, [len(S)]))).tolist())
    assert {1 + r for r in list(range(7)) + list(range(258, 263)) + list(range(516, 521))} <= lens


@pytest.mark.parametrize('name', NAMES)
def test_restated_file_reads_back(name):
    from PIL import Image
    img = png_cases.cases()[name]
    data = png_cases.restated(name)
    with Image.open(io.BytesIO(data)) as im:
        assert np.array_equal(np.asarray(im), img)
    # the library's own decoder (BGR, grey replicated)
    H, W = img.shape[:2]
    host = hip.load_host()
    buf = np.frombuffer(data, np.uint8)
    h, w, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert host.vps_png_info(buf.ctypes.data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == 0
    assert (h.value, w.value, c.value) == (H, W, 1 if img.ndim == 2 else 3)
    out = np.empty((H, W, 3), np.uint8)
    assert host.vps_png_decode_bgr8(buf.ctypes.data, len(data), out.ctypes.data, out.size) == 0
    want = np.repeat(img[:, :, None], 3, 2) if img.ndim == 2 else img[:, :, ::-1]
    assert np.array_equal(out, want)
    # zlib: the IDAT is the filtered stream, and its filter bytes are the minimum-sum choice
    S, ftype = R.filter_rows(img)
    assert zlib.decompress(R.idat_of(data)) == S.tobytes()
    rows = S.reshape(H, -1)
    assert np.array_equal(rows[:, 0], ftype) and ftype[0] != 2 and ftype.max() <= 2
    raw = img.reshape(H, -1).astype(np.int64)
    C = 1 if img.ndim == 2 else 3
    for y in (0, H // 2, H - 1):                                    # the chosen filter is no worse than the others, lower number on a tie
        left = np.concatenate((np.zeros(C, np.int64), raw[y, :-C]))
        up = raw[y - 1] if y else np.zeros_like(raw[y])
        sc = [int(np.abs(((r & 255) ^ 128) - 128).sum()) for r in (raw[y], raw[y] - left, raw[y] - up)]
        assert sc[ftype[y]] == min(sc) and ftype[y] == sc.index(min(sc)), (y, sc)


def test_full_size_label_map_is_at_most_a_sixteenth():
    img = png_cases.cases()['full']
    n = len(png_cases.restated('full'))
    print('full-size label map: %d bytes, 1/%.1f of the raw size' % (n, img.size / n))
    assert 16 * n <= img.size


def test_segments_end_on_every_bit_alignment():
    got = set()
    for k, img in png_cases.cases().items():
        if k.startswith('align'):
            S = R.filter_rows(img)[0]
            got.add((3 + R.segment_token_bits(S) + 7) % 8)
    assert got == set(range(8))


def test_encode_bound_covers_noise_and_refuses_bad_arguments():
    img = png_cases.cases()['noise']
    rc, cap, wsb = _bound(64, 96, 3)
    stream = R.idat_of(png_cases.restated('noise'))
    assert rc == 0 and cap >= len(stream) and wsb > 0
    assert len(stream) > img.size                                   # pure noise: all literals, the stream is larger than the image
    for name in ('1x1x1', 'const', 'ff_grey', 'full'):
        im = png_cases.cases()[name]
        rc, cap, _ = _bound(im.shape[0], im.shape[1], 1 if im.ndim == 2 else 3)
        assert rc == 0 and cap >= len(R.idat_of(png_cases.restated(name)))
    # worst case per byte: 9 bits (every byte a literal >= 144)
    worst = np.random.default_rng(1).integers(144, 256, (40, 300, 3)).astype(np.uint8)
    S = R.filter_rows(worst)[0]
    rc, cap, _ = _bound(40, 300, 3)
    assert rc == 0 and cap >= len(R.deflate_stream(np.where(S < 144, 200, S).astype(np.uint8)))
    for bad in ((64, 96, 2), (64, 96, 4), (64, 96, 0), (0, 96, 3), (64, 0, 3), (-1, 5, 1), (5, -1, 1)):
        rc, cap, wsb = _bound(*bad)
        assert rc <= -1000 and cap == -7 and wsb == -7, bad
    assert hip.load().vps_png_encode_bound(4, 4, 3, None, None) <= -1000
