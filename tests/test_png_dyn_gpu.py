"""GPU: `vps_png_deflate_h` / `vps_png_deflate_bpp_h` (csrc/png_ops.hip). With huffman = 1 the stream is, byte for byte, the one of the
NumPy restatement tests/png_dyn_restate.py on every case of tests/png_dyn_cases.py; with huffman = 0 it is the existing entry points'."""
import io
import zlib

import numpy as np
import pytest
import torch

import png16_cases as P
import png_dyn_cases as C
import png_dyn_restate as D
import png_restate as R
from vps_amd import hip, kittiflow
from vps_amd import postprocess as pp

pytestmark = pytest.mark.gpu
NAMES = sorted(C.cases())


def _stream(t, huffman):
    buf, size = pp.png_deflate(t, huffman=huffman)
    n = int(size.item())
    assert n > 0
    return buf[:n].cpu().numpy().tobytes()


def _where(got, want):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    k = min(len(a), len(b))
    d = np.flatnonzero(a[:k] != b[:k])
    return '%d / %d bytes, first difference at stream byte %s' % (len(a), len(b), d[:1].tolist())


@pytest.mark.parametrize('name', NAMES)
def test_dynamic_bytes_equal_the_restatement(dev, name):
    img = C.cases()[name]
    want = R.idat_of(C.restated(name))
    t = torch.from_numpy(img).to(dev)
    got = _stream(t, 'dynamic')
    assert got == want, '%s: %s' % (name, _where(got, want))
    fixed = _stream(t, 'fixed')
    assert fixed == R.png_stream(img)                                 # huffman 0: the fixed stream, as it was
    assert len(got) <= len(fixed)
    from PIL import Image
    C_ = 1 if img.ndim == 2 else img.shape[2]
    with Image.open(io.BytesIO(pp.png_container(got, img.shape[0], img.shape[1], C_))) as im:
        assert np.array_equal(np.asarray(im), img)


def _raw_call(fn, t, H, W, Cn, stride, cap, wsb, *tail):
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=t.device)
    size = torch.zeros(1, dtype=torch.int64, device=t.device)
    ws = torch.empty(wsb, dtype=torch.uint8, device=t.device)
    rc = fn(hip.ptr(t), H, W, Cn, stride, hip.ptr(out), cap, hip.ptr(size), hip.ptr(ws), wsb, hip.stream_ptr(), *tail)
    return rc, out.cpu().numpy(), int(size.item())


@pytest.mark.parametrize('name', ['rgb', 'three_and_tail', 'zeros'])
def test_huffman_0_equals_the_existing_entry_point(dev, name):
    img = C.cases()[name]
    H, W = img.shape[:2]
    Cn = 1 if img.ndim == 2 else 3
    t = torch.from_numpy(img).to(dev)
    cap, wsb = pp.png_encode_bound(H, W, Cn)
    lib = hip.load()
    rc0, a, na = _raw_call(lib.vps_png_deflate, t, H, W, Cn, W * Cn, cap, wsb)
    rc1, b, nb = _raw_call(lib.vps_png_deflate_h, t, H, W, Cn, W * Cn, cap, wsb, 0)
    assert rc0 == 0 and rc1 == 0 and na == nb > 0 and np.array_equal(a, b)
    rc2, c, nc = _raw_call(lib.vps_png_deflate_h, t, H, W, Cn, W * Cn, cap, wsb, 1)
    assert rc2 == 0 and 0 < nc <= na and (c[cap:] == 0xA5).all()     # the bound is the fixed code's: it holds for both
    # any other value is refused before a launch: nothing is written, not even the size
    for bad in (2, -1):
        rc, d, nd = _raw_call(lib.vps_png_deflate_h, t, H, W, Cn, W * Cn, cap, wsb, bad)
        assert rc == -1007 and nd == 0 and (d == 0xA5).all()
    rc, d, nd = _raw_call(lib.vps_png_deflate_bpp_h, t, H, W * Cn, Cn, W * Cn, cap, wsb, 2)
    assert rc == -1007 and nd == 0 and (d == 0xA5).all()


@pytest.mark.parametrize('name,pad,x0', [('grey', 5, 1), ('rgb', 3, 1), ('grey', 8, 4)])
def test_odd_row_stride_and_unaligned_base(dev, name, pad, x0):
    img = C.cases()[name]
    H, W = img.shape[:2]
    wide = torch.full((H, W + pad) + img.shape[2:], 0x5A, dtype=torch.uint8, device=dev)
    view = wide[:, x0:W + x0]
    view.copy_(torch.from_numpy(img))
    t, _, _, _, stride = pp._png_view(view)
    assert t.data_ptr() == view.data_ptr() and stride == (W + pad) * (img.size // (H * W))
    assert _stream(view, 'dynamic') == R.idat_of(C.restated(name))


def test_bpp_6_smooth_flow_through_the_kitti_encoder(dev):
    H, W = 24, 96
    flow = C.smooth_flow(H, W)
    raw = kittiflow.kitti_flow_encode(torch.from_numpy(flow).to(dev))            # device uint8 [H][6 W]
    S, _ = P.device_filter_rows(raw.cpu().numpy())
    want = D.deflate_stream(S)
    buf, size = kittiflow.png_deflate_bpp(raw, 6, huffman='dynamic')
    got = buf[:int(size.item())].cpu().numpy().tobytes()
    assert got == want, _where(got, want)
    assert zlib.decompress(got) == S.tobytes()
    fbuf, fsize = kittiflow.png_deflate_bpp(raw, 6)
    lib = hip.load()
    cap, wsb = kittiflow.png_encode_bound_bpp(H, 6 * W, 6)
    rc, old, nold = _raw_call(lib.vps_png_deflate_bpp, raw, H, 6 * W, 6, 6 * W, cap, wsb)
    fixed = fbuf[:int(fsize.item())].cpu().numpy().tobytes()
    assert rc == 0 and old[:nold].tobytes() == fixed == R.deflate_stream(S)
    assert len(got) < len(fixed)
    # the file of the Python surface opens in PIL and holds the same stream
    data = kittiflow.kitti_flow_bytes(torch.from_numpy(flow).to(dev), huffman='dynamic')
    assert P.idat_of(data) == want
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.size == (W, H)
        im.load()


def test_capacity_one_byte_short_returns_minus_one_and_stores_nothing(dev):
    img = C.cases()['three_and_tail']
    H, W = img.shape
    t = torch.from_numpy(img).to(dev)
    want = R.idat_of(C.restated('three_and_tail'))
    _, wsb = pp.png_encode_bound(H, W, 1)
    lib = hip.load()
    rc, host, n = _raw_call(lib.vps_png_deflate_h, t, H, W, 1, W, len(want) - 1, wsb, 1)
    assert rc == 0 and n == -1 and (host == 0xA5).all()
    rc, host, n = _raw_call(lib.vps_png_deflate_h, t, H, W, 1, W, len(want), wsb, 1)
    assert rc == 0 and n == len(want) and host[:n].tobytes() == want and (host[n:] == 0xA5).all()


def test_writers_take_the_coder(dev, tmp_path):
    from vps_amd.flowvis import FlowWriter
    img = C.cases()['rgb']
    w = pp.DevicePngWriter(dev, workers=1, slots=2, huffman='dynamic')
    w.submit(torch.from_numpy(img).to(dev), str(tmp_path / 'a.png'))
    w.close()
    assert open(tmp_path / 'a.png', 'rb').read() == C.restated('rgb')
    flow = torch.from_numpy(C.smooth_flow(24, 96)).to(dev)
    fw = FlowWriter(dev, workers=1, slots=2, fmt='kitti', huffman='dynamic')
    fw.submit(flow, str(tmp_path / 'f.png'))
    fw.close()
    assert open(tmp_path / 'f.png', 'rb').read() == kittiflow.kitti_flow_bytes(flow, huffman='dynamic')
    with pytest.raises(ValueError):
        pp.png_deflate(torch.from_numpy(img).to(dev), huffman='best')
