"""GPU: the device PNG encoder (`vps_png_deflate`, csrc/png_ops.hip) must produce, byte for byte, the file of its NumPy restatement
(tests/png_restate.py) on every case of tests/png_cases.py, and `DevicePngWriter` must write files that read back equal without ever
waiting for the caller's stream."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

import png_cases
import png_restate as R
from vps_amd import hip
from vps_amd import postprocess as pp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(png_cases.cases())


def _pil(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im)


def _device_file(t):
    buf, size = pp.png_deflate(t)
    n = int(size.item())
    assert n > 0
    C = 1 if t.dim() == 2 else int(t.shape[2])
    return pp.png_container(buf[:n].cpu().numpy().tobytes(), int(t.shape[0]), int(t.shape[1]), C)


@pytest.mark.parametrize('name', NAMES)
def test_device_bytes_equal_the_restatement(dev, name):
    img = png_cases.cases()[name]
    want = png_cases.restated(name)
    got = _device_file(torch.from_numpy(img).to(dev))
    if got != want:                                                  # say where: which segment, which byte
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(len(a), len(b))
        d = np.flatnonzero(a[:k] != b[:k])
        pytest.fail('%s: %d / %d bytes, first difference at file byte %s' % (name, len(a), len(b), d[:1].tolist()))
    assert np.array_equal(_pil(got), img)


def test_container_is_the_restatements():
    s = b'\x78\x01\x03\x00\x00\x00\x00\x01'
    assert pp.png_container(s, 5, 7, 3) == R.container(s, 5, 7, 3) and pp.png_container(s, 2, 9, 1) == R.container(s, 2, 9, 1)


def test_capacity_one_byte_short_returns_minus_one_and_stores_nothing(dev):
    img = png_cases.cases()['labels']
    t = torch.from_numpy(img).to(dev)
    need = len(R.idat_of(png_cases.restated('labels')))
    _, wsb = pp.png_encode_bound(*img.shape)
    guard = 4096
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    for cap, ok in ((need - 1, False), (need, True)):
        out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        hip.check(hip.load().vps_png_deflate(hip.ptr(t), img.shape[0], img.shape[1], 3, img.shape[1] * 3, hip.ptr(out), cap, hip.ptr(size),
                                             hip.ptr(ws), wsb, hip.stream_ptr()), 'vps_png_deflate')
        host = out.cpu().numpy()
        assert int(size.item()) == (need if ok else -1)
        assert (host[cap:] == 0xA5).all()                            # the guard band after `out`
        if ok:
            assert host[:cap].tobytes() == R.idat_of(png_cases.restated('labels'))
        else:
            assert (host == 0xA5).all()                              # nothing at all was stored
    # a workspace that is too small is an argument error, not a launch
    assert hip.load().vps_png_deflate(hip.ptr(t), img.shape[0], img.shape[1], 3, img.shape[1] * 3, hip.ptr(out), cap, hip.ptr(size), hip.ptr(ws),
                                      wsb - 1, hip.stream_ptr()) <= -1000


@pytest.mark.parametrize('name,pad,x0', [('labels', 5, 1), ('labels', 64, 4), ('noise', 3, 1), ('ff_grey', 7, 1), ('ff_grey', 8, 4), ('1x7x3', 2, 1)])
def test_row_stride_larger_than_the_row(dev, name, pad, x0):
    """a view into a wider buffer = its contiguous copy; strides and offsets that are multiples of 4 bytes (the filter pass reads words)
    and ones that are not (it reads bytes)"""
    img = png_cases.cases()[name]
    H, W = img.shape[:2]
    wide = torch.full((H, W + pad) + img.shape[2:], 0x5A, dtype=torch.uint8, device=dev)
    view = wide[:, x0:W + x0]
    view.copy_(torch.from_numpy(img))
    assert not view.is_contiguous() or H == 1
    t, _, _, _, stride = pp._png_view(view)
    assert t.data_ptr() == view.data_ptr() and (H == 1 or stride == (W + pad) * (img.size // (H * W)))    # encoded in place, no copy
    assert _device_file(view) == png_cases.restated(name)


def _slow_conv(dev):
    """'fpn/tcea 256->256 3x3 @256x512' of tools/bench_conv.py in fp32 arithmetic: ~1.2 ms a launch"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bench_conv
    from vps_amd import nhwc
    name, cin, cout, k, s, p, H, W, tr, df = next(r for r in bench_conv.SHAPES if r[0].startswith('fpn/tcea 256->256 3x3'))
    g = torch.Generator().manual_seed(0)
    pc = nhwc.PackedConv(torch.randn(cout, cin, k, k, generator=g) * 0.05, torch.zeros(cout), None, stride=s, padding=p, act=hip.ACT_LEAKY,
                         device=dev, prec=hip.PREC_F32)
    x = nhwc.FMap(torch.randn(1, H, W, cin, device=dev), cin, 0)
    ws = nhwc.Workspace(dev)
    out = pc(x, ws=ws, name='png_test_out')
    return lambda: pc(x, out=out, ws=ws)


def test_submit_does_not_wait_for_the_callers_stream(dev, tmp_path):
    img = png_cases.cases()['labels']
    t = torch.from_numpy(img).to(dev)
    conv = _slow_conv(dev)
    w = pp.DevicePngWriter(dev, workers=2, slots=8)
    w.submit(t, str(tmp_path / 'warm.png'))                          # sizes the ring slots (allocations happen here)
    torch.cuda.synchronize()
    for _ in range(12):                                              # ~15 ms of work ahead of the encode on the same stream
        conv()
    w.submit(t, str(tmp_path / 'after_conv.png'))
    ev = torch.cuda.Event()
    ev.record()
    done = ev.query()                                                # True only if the stream had already run dry: submit waited
    w.close()
    assert not done, 'submit returned only after the stream had completed'
    assert w.device_encoded == 2 and w.fallback_encoded == 0
    for n in ('warm.png', 'after_conv.png'):
        assert open(tmp_path / n, 'rb').read() == png_cases.restated('labels')


def test_writer_on_mixed_host_and_device_inputs(dev, tmp_path):
    c = png_cases.cases()
    names = ['labels', 'noise', 'ff_grey', 'const', '1x7x3', 'runs']
    w = pp.DevicePngWriter(dev, workers=2, slots=3)                  # fewer slots than device images: the ring wraps
    want = {}
    for i in range(12):
        img = c[names[i % 6]]
        fn = str(tmp_path / 'sub' / ('%02d.png' % i))
        want[fn] = img
        w.submit(torch.from_numpy(img).to(dev) if i % 3 else img, fn)         # 4 host arrays, 8 device tensors
    assert sorted(w.close()) == sorted(want)
    assert (w.device_encoded, w.fallback_encoded) == (8, 4)
    for fn, img in want.items():
        assert np.array_equal(_pil(open(fn, 'rb').read()), img), fn


def test_writer_close_reraises_a_workers_exception(dev, tmp_path):
    blocker = tmp_path / 'file'
    blocker.write_text('x')
    w = pp.DevicePngWriter(dev)
    w.submit(torch.from_numpy(png_cases.cases()['1x7x3']).to(dev), str(blocker / 'under_a_file.png'))
    with pytest.raises(OSError):
        w.close()


def test_inference_panoptic_video_with_the_device_writer(dev, tmp_path):
    """the frames of tests/test_postprocess.py::test_inference_panoptic_video_writes_the_reference_files: same file names, same pred.json,
    every PNG decodes to what the default writer's PNG decodes to"""
    from test_postprocess import _Colors, _pan2ch_clip
    H, W, nvid, nfr = 64, 96, 2, 30
    rng = np.random.default_rng(5)
    frames = []
    for v in range(nvid):
        frames += _pan2ch_clip(rng, H, W, nfr)
    names = ['%04d_%04d_city_%06d_newImg8bit.png' % (v, f, f) for v in range(nvid) for f in range(nfr)]
    snames = names[4::5]
    a, b = tmp_path / 'default', tmp_path / 'device'
    dev_frames = [torch.from_numpy(f).to(dev) for f in frames]
    pans_a, pj_a = pp.inference_panoptic_video(dev_frames, str(a), None, snames, n_video=nvid, color_generator=_Colors(), device=dev)
    w = pp.DevicePngWriter(dev)
    mixed = [f if i % 2 else frames[i] for i, f in enumerate(dev_frames)]          # host arrays and device tensors alike
    pans_b, pj_b = pp.inference_panoptic_video(mixed, str(b), None, snames, n_video=nvid, color_generator=_Colors(), device=dev, writer=w)
    w.close()
    assert (w.device_encoded, w.fallback_encoded) == (24, 0)
    assert pj_a == pj_b and json.load(open(a / 'pred.json')) == json.load(open(b / 'pred.json'))
    assert all(np.array_equal(x, y) for x, y in zip(pans_a, pans_b)) and len(pans_b) == 12
    for sub in ('pan_2ch', 'pan_pred'):
        assert sorted(os.listdir(a / sub)) == sorted(os.listdir(b / sub)) and len(os.listdir(b / sub)) == 12
        for fn in os.listdir(a / sub):
            assert np.array_equal(_pil(open(a / sub / fn, 'rb').read()), _pil(open(b / sub / fn, 'rb').read())), (sub, fn)
