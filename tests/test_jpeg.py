"""CPU: the host half of the JPEG input path (`vps_jpeg_info`, `vps_jpeg_decode_coef`: csrc/jpeg_host.cpp) against PIL.

The device half (csrc/jpeg_ops.hip) has no CPU twin in the package; `tests/jpeg_restate.py` restates it in NumPy from libjpeg's
published algorithms, so that `restate(decode_coef(file))` can be compared, bit for bit, with what libjpeg-turbo decodes: the arrays
committed in tests/golden/jpeg_cases.npz (written by tests/golden/make_jpeg_golden.py with PIL) and PIL on the running machine.
The same fixtures go through the real device stage in tests/test_jpeg_gpu.py."""
import ctypes
import io
import os
import warnings

import numpy as np
import pytest
import torch

import jpeg_restate as R
from vps_amd import hip, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')


@pytest.fixture(scope='module')
def cases():
    z = np.load(CASES)
    return {k: z[k] for k in z.files}


def _accepted(cases):
    return sorted(k[5:] for k in cases if k.startswith('file/'))


def _pil(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return im.size, im.mode, np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def _turbo():
    from PIL import features
    return bool(features.check_feature('libjpeg_turbo'))


def test_fixture_matrix_is_complete(cases):
    names = _accepted(cases)
    for sub in ('444', '422', '420', 'grey'):
        for size in ('64x96', '40x56', '37x53', '31x47', '1x1', '8x17'):
            assert '%s_%s_q90' % (sub, size) in names
        for tail in ('37x53_q50', '37x53_q100', '40x56_edges_q50', '40x56_edges_q100', '40x56_optimize', '37x53_rst_blocks4', '64x96_rst_rows1'):
            assert '%s_%s' % (sub, tail) in names
    assert {k for k in cases if k.startswith('refuse/')} == {'refuse/progressive', 'refuse/cmyk', 'refuse/exif_orientation6', 'refuse/truncated'}
    assert os.path.getsize(CASES) < (1 << 20)
    # what the fixtures are meant to contain: restart intervals, non-default Huffman tables, SOF2
    assert b'\xff\xdd' in cases['file/420_37x53_rst_blocks4'].tobytes() and b'\xff\xdd' in cases['file/420_64x96_rst_rows1'].tobytes()
    assert b'\xff\xd0' in cases['file/420_64x96_rst_rows1'].tobytes()
    assert b'\xff\xc2' in cases['refuse/progressive'].tobytes()[:700]


def test_info_geometry_equals_pil(cases):
    lib = hip.load_host()
    for n in _accepted(cases):
        data = cases['file/' + n].tobytes()
        st, i = R.jpeg_info(lib, data)
        assert st == 0, (n, st)
        (w, h), mode, _ = _pil(data)
        assert (i.H, i.W) == (h, w), n
        assert i.ncomp == {'L': 1, 'RGB': 3}[mode], n
        sub = n.split('_')[0]
        assert i.samp[0] == {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': (1, 1)}[sub], n
        mh, mw = 8 * i.samp[0][1], 8 * i.samp[0][0]
        rows, cols = -(-h // mh), -(-w // mw)
        assert i.grid[0] == (rows * i.samp[0][1], cols * i.samp[0][0]), n
        if i.ncomp == 3:
            assert i.samp[1] == i.samp[2] == (1, 1) and i.grid[1] == i.grid[2] == (rows, cols), n
        assert i.coef_bytes == sum(i.grid[c][0] * i.grid[c][1] for c in range(i.ncomp)) * 128, n
        assert i.qt.min() >= 1


def _mismatches(cases, reference):
    lib = hip.load_host()
    wrong = []
    for n in _accepted(cases):
        data = cases['file/' + n].tobytes()
        st, i = R.jpeg_info(lib, data)
        assert st == 0, n
        st, coef = R.decode_coef(lib, data, i)
        assert st == 0, (n, st)
        got = R.restate(coef, i)
        want = reference(n, data)
        assert got.shape == want.shape, n
        mm = int((got != want).sum())
        print('%-28s mismatches: %d' % (n, mm))
        if mm:
            wrong.append((n, mm))
    return wrong


def test_decoded_coefficients_restate_to_the_committed_pixels(cases):
    """mismatch count 0 on every accepted fixture against the arrays libjpeg-turbo decoded when the archive was written"""
    wrong = _mismatches(cases, lambda n, data: cases['bgr/' + n])
    assert not wrong, wrong


def test_decoded_coefficients_restate_to_pil_on_this_machine(cases):
    if not _turbo():
        pytest.skip('PIL on this machine is not built on libjpeg-turbo: its IDCT / upsampling may differ from the pinned one')
    wrong = _mismatches(cases, lambda n, data: _pil(data)[2])
    assert not wrong, wrong


def test_hard_edged_fixture_reaches_the_range_limiter(cases):
    """the edge pattern's ringing leaves 0..255 after the inverse DCT: without the range limit the restatement cannot be right there"""
    lib = hip.load_host()
    data = cases['file/444_40x56_edges_q100'].tobytes()
    st, i = R.jpeg_info(lib, data)
    st, coef = R.decode_coef(lib, data, i)
    x = coef[:i.grid[0][0] * i.grid[0][1] * 64].reshape(-1, 8, 8).astype(np.int64) * i.qt[0].reshape(1, 8, 8).astype(np.int64)
    ws = np.stack(R._idct_pass([x[:, r, :] for r in range(8)], 11), 1)
    out = np.stack(R._idct_pass([ws[:, :, c] for c in range(8)], 18), 2) + 128
    assert out.min() < 0 and out.max() > 255


def test_refused_files_return_the_argument_error_and_imread_still_reads_them(cases, tmp_path):
    from vps_amd.pipeline import ClipFeeder, imread, jpeg_info
    lib = hip.load_host()

    class HostPrep:
        device = torch.device('cpu')

        def prep(self, img):
            return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float(), tuple(img.shape), tuple(img.shape), 1.0

    readable = []
    for k in sorted(k for k in cases if k.startswith('refuse/')):
        data = cases[k].tobytes()
        st, _ = R.jpeg_info(lib, data)
        assert st <= -1000, (k, st)
        assert jpeg_info(data) is None
        if k != 'refuse/truncated':                                          # PIL raises on the truncated file
            fn = str(tmp_path / (k.split('/')[1] + '.jpg'))
            with open(fn, 'wb') as f:
                f.write(data)
            with pytest.warns(UserWarning, match='decoded with PIL'):
                img = imread(fn)
            assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (40, 56, 3)
            assert np.array_equal(img, _pil(data)[2])
            readable.append(fn)
    # an accepted file beside them: on the host stand-in (no device stage) every JPEG takes the imread route
    fn = str(tmp_path / 'accepted.jpg')
    with open(fn, 'wb') as f:
        f.write(cases['file/420_40x56_optimize'].tobytes())
    files = readable + [fn]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fd = ClipFeeder(files, HostPrep(), workers=2)
        for t in range(len(files)):
            assert tuple(fd(t).shape) == (1, 3, 40, 56)
        fd.close()
    assert fd.decodes == len(files) and fd.fallback_decodes == len(files) and fd.native_jpeg == 0
    assert np.array_equal(fd(len(files) - 1)[0].permute(1, 2, 0).numpy().astype(np.uint8), cases['bgr/420_40x56_optimize'])


def test_damaged_streams_are_refused_not_decoded(cases):
    """a flipped byte inside the scan either still decodes (a different picture) or returns the argument error - never a crash, and
    a stream cut anywhere is refused by vps_jpeg_info (no EOI), one cut inside the scan by vps_jpeg_decode_coef too"""
    lib = hip.load_host()
    data = bytearray(cases['file/420_64x96_rst_rows1'].tobytes())
    st, i = R.jpeg_info(lib, bytes(data))
    assert st == 0
    for cut in (len(data) - 2, len(data) * 3 // 4, len(data) // 2):
        assert R.jpeg_info(lib, bytes(data[:cut]))[0] <= -1000
        if cut == len(data) - 2:                                             # only the EOI marker is missing: every coefficient is there
            continue
        part = bytes(data[:cut])
        coef = np.zeros(i.coef_bytes // 2, dtype=np.int16)
        buf = (ctypes.c_char * len(part)).from_buffer_copy(part)
        assert lib.vps_jpeg_decode_coef(buf, len(part), coef.ctypes.data_as(ctypes.c_void_p), coef.nbytes) <= -1000
    rng = np.random.RandomState(0)
    sos = bytes(data).index(b'\xff\xda')
    for _ in range(200):
        d = bytearray(data)
        d[rng.randint(sos + 14, len(d) - 2)] = rng.randint(0, 256)
        st, coef = R.decode_coef(lib, bytes(d), i)
        assert st == 0 or st <= -1000
    # too small an output buffer is an argument error, not a write
    buf = (ctypes.c_char * len(data)).from_buffer(data)
    small = np.zeros(64, dtype=np.int16)
    assert lib.vps_jpeg_decode_coef(buf, len(data), small.ctypes.data_as(ctypes.c_void_p), small.nbytes) <= -1000


@pytest.mark.parametrize('sub', [2, 1, 0])
def test_1080x1920_decodes_equal_to_pil(sub):
    """the VIPER frame size, encoded here: 1080 rows end in half an MCU row for 4:2:0"""
    from PIL import Image
    if not _turbo():
        pytest.skip('PIL on this machine is not built on libjpeg-turbo')
    lib = hip.load_host()
    fr = synth.synth_frame(1080, 1920, seed=5).astype(np.uint8)
    fr[500:560, 800:900] = np.where(np.indices((60, 100)).sum(0)[..., None] % 2, 255, 0)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(fr[..., ::-1])).save(b, 'JPEG', quality=92, subsampling=sub)
    data = b.getvalue()
    st, i = R.jpeg_info(lib, data)
    assert st == 0 and (i.H, i.W) == (1080, 1920)
    if sub == 2:
        assert i.coef_bytes == (1088 * 1920 + 2 * 544 * 960) * 2
    st, coef = R.decode_coef(lib, data, i)
    assert st == 0
    got = R.restate(coef, i)
    mm = int((got != _pil(data)[2]).sum())
    print('1080x1920 subsampling %d: mismatches vs PIL %d' % (sub, mm))
    assert mm == 0
