"""GPU: `vps_png_reconstruct` (csrc/png_in_ops.hip) must undo the five scanline filters and swap to BGR byte for byte like the host
decoder. The files are written here with a chosen filter type per scanline (tests/png_filter_cases.py); the expected image is the
ORIGINAL array, and `png_decode` of the same file must equal it too. The shapes are the smallest at which the wavefront can go wrong:
every pair of adjacent filter types, every type as row 0, rows shorter than the lag between lanes, one row, a group longer than a
band, many one-row groups, every misalignment of a row start and of the output rows (dword stores where W*3 is a multiple of 4)."""
import ctypes
import io

import numpy as np
import pytest
import torch

import png_filter_cases as P
from vps_amd import hip
from vps_amd.pipeline import ClipFeeder, DeviceImagePrep, png_decode, png_inflate, png_reconstruct

pytestmark = pytest.mark.gpu


def _check(dev, img, types, offset=0):
    """file -> host inflate -> upload (at `offset` bytes into its buffer) -> device reconstruct == the original == png_decode"""
    data, raw = P.encode(img, types)
    want = P.bgr(img)
    host = png_decode(data)
    assert host is not None and np.array_equal(host, want)
    scan, pi = png_inflate(data)
    assert scan.tobytes() == raw
    buf = torch.zeros(offset + scan.size + 8, dtype=torch.uint8)
    buf[offset:offset + scan.size] = torch.from_numpy(scan)
    d = buf.to(dev)[offset:offset + scan.size]
    assert d.data_ptr() % 4 == offset % 4
    got = png_reconstruct(d, pi.H, pi.W, pi.C).cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, ('first differing (row, column, channel)', bad[0].tolist(), 'of', len(bad), 'filter types', list(types)[:40])


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('H,W', [(7, 5), (33, 67), (9, 8), (27, 12)])
def test_every_pair_of_adjacent_filter_types_and_every_type_as_row_0(dev, C, H, W):
    """(7,5) takes five files to walk all 25 ordered pairs; (9,8) and (27,12): W*3 a multiple of 4, the dword-store path"""
    pairs = len(P.ALL_PAIRS) - 1
    for k, start in enumerate(range(0, pairs, max(H - 1, 1)) if H < 26 else [0]):
        types = [P.ALL_PAIRS[(start + y) % pairs] for y in range(H)]
        _check(dev, P.noise(H, W, C, seed=100 * C + k), types)
    for t0 in range(5):                                          # Up, Average and Paeth without a row above
        _check(dev, P.noise(H, W, C, seed=200 * C + t0), [t0] + P.types_all_pairs(H)[1:])


@pytest.mark.parametrize('C', [1, 3, 4])
def test_low_amplitude_image_hits_the_paeth_ties(dev, C):
    img = P.noise(33, 67, C, seed=300 + C, high=4)               # values 0..3: pa == pb and pb == pc occur on most pixels
    _check(dev, img, [1] + [4] * 32)
    _check(dev, img, P.types_all_pairs(33))


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('H,W', [(9, 1), (9, 2), (1, 1), (1, 67), (1, 4)])
def test_rows_shorter_than_the_wavefront_lag_and_a_single_row(dev, C, H, W):
    for t0 in range(5):
        _check(dev, P.noise(H, W, C, seed=400 + 10 * C + t0), [t0] + [4, 3, 2, 4, 3, 2, 4, 3][:H - 1])


@pytest.mark.parametrize('ft', [4, 3, 2])
def test_one_group_longer_than_a_block(dev, ft):
    """H = block_rows + 3 rows behind a Sub row 0: the second band starts from the first band's last rebuilt row"""
    R = hip.png_block_rows()
    assert R >= 1
    H = R + 3
    _check(dev, P.noise(H, 5, 3, seed=500 + ft), [1] + [ft] * (H - 1))


@pytest.mark.parametrize('C,W', [(1, 9), (4, 8)])
def test_a_group_of_two_bands_and_a_bit_for_grey_and_rgba(dev, C, W):
    """the row above a later band is read back from the BGR output: grey from its replicated bytes, RGBA without its alpha"""
    H = 2 * hip.png_block_rows() + 2
    _check(dev, P.noise(H, W, C, seed=550 + C), [0] + [4, 3, 4, 2] * ((H - 1) // 4) + [4] * ((H - 1) % 4))


def test_many_one_row_groups(dev):
    rg = np.random.default_rng(600)
    _check(dev, P.noise(64, 9, 3, seed=601), rg.integers(0, 2, 64).tolist())


def test_alternating_group_lengths(dev):
    types = []
    for n in range(1, 12):                                       # groups of 1, 2, 3 .. 11 rows
        types += [n % 2] + [2 + (n + k) % 3 for k in range(n - 1)]
    _check(dev, P.noise(len(types), 21, 3, seed=700), types)


@pytest.mark.parametrize('C,W', [(1, 4), (1, 5), (1, 6), (3, 8), (3, 7), (3, 6), (4, 5)])
@pytest.mark.parametrize('offset', [0, 1])
def test_row_length_1_2_3_mod_4_and_a_scan_pointer_off_by_one(dev, C, W, offset):
    assert (1 + W * C) % 4 in (1, 2, 3) or C == 4
    _check(dev, P.noise(13, W, C, seed=800 + W), P.types_all_pairs(13), offset=offset)


def test_argument_errors_return_a_negative_code_and_launch_nothing(dev):
    lib = hip.load()
    H, W, C = 6, 5, 3
    scan = torch.zeros(H * (1 + W * C), dtype=torch.uint8, device=dev)
    need = ctypes.c_int64()
    assert lib.vps_png_reconstruct_ws(H, W, C, ctypes.byref(need)) == 0 and need.value >= 4
    assert lib.vps_png_reconstruct_ws(0, W, C, ctypes.byref(need)) < 0
    assert lib.vps_png_reconstruct_ws(H, W, 2, ctypes.byref(need)) < 0
    assert lib.vps_png_reconstruct_ws(H, W, C, None) < 0
    out = torch.full((H * W * 3 + 16,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device=dev)

    def call(h, cap, wsb, s=scan, o=out, w=ws):
        return lib.vps_png_reconstruct(hip.ptr(s) if s is not None else None, h, W, C, hip.ptr(o) if o is not None else None, cap,
                                       hip.ptr(w) if w is not None else None, wsb, hip.stream_ptr())
    assert call(0, out.numel(), ws.numel()) < 0                   # H = 0
    assert call(H, out.numel(), need.value - 1) < 0               # workspace too small
    assert call(H, H * W * 3 - 1, ws.numel()) < 0                 # output capacity too small
    assert call(H, out.numel(), ws.numel(), s=None) < 0 and call(H, out.numel(), ws.numel(), o=None) < 0 and call(H, out.numel(), ws.numel(), w=None) < 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((ws == 0xA5).all())
    assert call(H, H * W * 3, need.value) == 0                    # exactly enough of both
    torch.cuda.synchronize()
    assert bool((out[:H * W * 3] == 0).all()) and bool((out[H * W * 3:] == 0xA5).all())      # zeros, type None: zeros; nothing behind them


def test_pil_written_png_with_adaptive_filters(dev):
    """a 128x256 low-passed random frame (the synthetic camera frame of the input benchmark, scaled down) as PIL writes it: a file no code of
    this repository encoded. PIL picks Sub for row 0 and Paeth for nearly every other row of such a frame, so the filter pattern is close to the
    all-Paeth group cases above; what this case adds is a real encoder's stream (its own IDAT split, filter heuristic and pixel statistics)."""
    from PIL import Image
    from vps_amd import synth
    fr = synth.synth_frame(128, 256, seed=1, shift=(2, 1), noise=2.0).astype(np.uint8)
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(f, format='PNG', compress_level=6)
    data = f.getvalue()
    scan, pi = png_inflate(data)
    assert (pi.H, pi.W, pi.C) == (128, 256, 3)
    types = scan.reshape(128, 1 + 256 * 3)[:, 0]
    assert len(set(types.tolist())) >= 2, 'the encoder chose one filter type only: %s' % set(types.tolist())
    got = png_reconstruct(torch.from_numpy(scan).to(dev), 128, 256, 3).cpu().numpy()
    assert np.array_equal(got, fr) and np.array_equal(png_decode(data), fr)


def test_feeder_png_device_equals_png_host(dev, tmp_path):
    from PIL import Image
    from vps_amd import synth
    files = []
    for t in range(4):
        fr = synth.synth_frame(64, 128, seed=t, shift=(t, 1), noise=2.0).astype(np.uint8)
        fn = str(tmp_path / ('f%d_leftImg8bit.png' % t))
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, compress_level=6)
        files.append(fn)
    prep = DeviceImagePrep(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32, img_scale=(128, 64),
                           device=dev)
    got = {}
    for mode in ('host', 'device'):
        fd = ClipFeeder(files, prep, workers=2, png=mode)
        got[mode] = [(fd(t).clone(), fd.meta(t)) for t in range(4)]
        torch.cuda.synchronize()
        fd.close()
        assert fd.fallback_decodes == 0 and fd.decodes == 4
        assert fd.native_png_device == (4 if mode == 'device' else 0)
    for (a, ma), (b, mb) in zip(got['host'], got['device']):
        assert torch.equal(a, b) and ma == mb
