"""GPU: the entropy coder on the device (`vps_jpeg_encode_scan`: csrc/jpeg_scan_ops.hip), `jpeg_encode(entropy='device')`,
`DeviceJpegWriter(entropy='device')` and `FlowWriter(entropy='device')`. The oracle is `vps_jpeg_write` on the same coefficients (pinned
to libjpeg-turbo in tests/test_jpeg_enc.py), and Pillow's own file where Pillow is installed; the acceptance rule is the same bytes.
What the crafted arrays of tests/jpeg_scan_cases.py contain is asserted on the CPU in tests/test_jpeg_scan.py."""
import os

import numpy as np
import pytest
import torch

import jpeg_enc_restate as E
import jpeg_scan_cases as C
from vps_amd import hip
from vps_amd.postprocess import (JPEG_SCAN_OK, JPEG_SCAN_RANGE, JPEG_SCAN_SHORT, DeviceJpegWriter, jpeg_encode, jpeg_encode_bound,
                                 jpeg_encode_coef, jpeg_encode_scan, jpeg_scan_bound)

pytestmark = pytest.mark.gpu
SUBS = [2, 0]
NAME = {2: '4:2:0', 0: '4:4:4'}
CANARY = 0x5A
IMAGES = dict(E.images())                                                        # 8x8, 17x33, 64x96 among them
IMAGES['noise_1x1'] = E.smooth_noise(1, 1, 5)                                    # one MCU: 6 blocks at 4:2:0, 3 at 4:4:4


def _have_pillow():
    try:
        from PIL import Image  # noqa: F401
        return True
    except ImportError:
        return False


def _device_scan(dev, coef, H, W, sub, capacity=None):
    """upload, `jpeg_encode_scan` into buffers with canary bytes behind `out` and behind `ws` -> (bytes, status, out[:min(bytes, capacity)])"""
    wsb, cap = jpeg_scan_bound(H, W, sub)
    capacity = cap if capacity is None else capacity
    d_coef = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.int16)).to(dev)
    out = torch.full((capacity + 256,), CANARY, dtype=torch.uint8, device=dev)
    ws = torch.full((wsb + 256,), CANARY, dtype=torch.uint8, device=dev)
    result = torch.full((2,), -7, dtype=torch.int64, device=dev)
    jpeg_encode_scan(d_coef, H, W, sub, out[:capacity], ws[:wsb], result)
    n, status = (int(v) for v in result.cpu())
    assert (out[capacity:].cpu().numpy() == CANARY).all(), 'a store at or beyond out + capacity'
    assert (ws[wsb:].cpu().numpy() == CANARY).all(), 'a store beyond the workspace'
    return n, status, out[:min(max(n, 0), capacity)].cpu().numpy().tobytes()


@pytest.mark.parametrize('sub', SUBS)
def test_images_device_entropy_equals_host_entropy_and_pillow(dev, sub):
    for name, img in IMAGES.items():
        d_img = torch.from_numpy(img).to(dev)
        for q in E.QUALITIES:
            ours = jpeg_encode(d_img, q, NAME[sub], entropy='device')
            assert ours == jpeg_encode(d_img, q, NAME[sub], entropy='host'), (name, q)
            assert ours == jpeg_encode(d_img, q, NAME[sub]), (name, q)
            if _have_pillow():
                assert E.scan_of(ours) == E.scan_of(E.pil_file(img, q, sub)), (name, q)


@pytest.mark.parametrize('sub', SUBS)
def test_crafted_coefficients_give_the_host_coders_scan(dev, sub):
    host = hip.load_host()
    H, W = C.SIZE[sub]
    for name, coef in C.cases(sub):
        st, ref = C.reference_scan(host, coef, H, W, sub)
        assert st == 0, name
        n, status, got = _device_scan(dev, coef, H, W, sub)
        assert (n, status) == (len(ref), JPEG_SCAN_OK), (name, n, status, len(ref))
        assert got == ref, (name, next(i for i in range(len(ref)) if got[i] != ref[i]))


@pytest.mark.parametrize('sub', SUBS)
def test_short_capacities_report_the_true_size_and_keep_the_canaries(dev, sub):
    host = hip.load_host()
    H, W = C.SIZE[sub]
    chunk = C.stuff_chunk()
    for name in ('all_1023', 'sparse_random'):
        coef = dict(C.cases(sub))[name]
        st, ref = C.reference_scan(host, coef, H, W, sub)
        for cap in sorted({0, 1, len(ref) // 2, chunk - 1, chunk, chunk + 1, len(ref) - 1} & set(range(len(ref)))):
            n, status, got = _device_scan(dev, coef, H, W, sub, capacity=cap)   # the canaries are checked in there
            assert (n, status) == (len(ref), JPEG_SCAN_SHORT), (name, cap, n, status)
            assert got == ref[:cap], (name, cap)                                 # what fits is the beginning of the scan
        n, status, got = _device_scan(dev, coef, H, W, sub, capacity=len(ref))   # the repeated call with the true size
        assert (n, status) == (len(ref), JPEG_SCAN_OK) and got == ref, name


def test_jpeg_encode_repeats_the_call_when_its_first_buffer_is_short(dev):
    """`jpeg_encode(entropy='device')` starts with an eighth of the coefficients' bytes: noise at quality 100 needs more"""
    img = np.random.RandomState(3).randint(0, 256, (64, 96, 3)).astype(np.uint8)
    d_img = torch.from_numpy(img).to(dev)
    ours = jpeg_encode(d_img, 100, '4:4:4', entropy='device')
    assert len(ours) - C.HEADER_BYTES - 2 > max(4096, jpeg_encode_bound(64, 96, 0)[1] // 8)
    assert ours == jpeg_encode(d_img, 100, '4:4:4', entropy='host')


@pytest.mark.parametrize('sub', SUBS)
def test_out_of_range_coefficients_give_the_range_status_and_no_fault(dev, sub):
    host = hip.load_host()
    H, W = C.SIZE[sub]
    good = dict(C.cases(sub))['sparse_random']
    order = C.scan_order(H, W, sub)
    ac = good.copy()
    ac[order[len(order) // 2][1] * 64 + 9] = 1024                                # an AC coefficient of category 11
    dc = good.copy()
    luma = [b for c, b in order if c == 0]
    dc[luma[3] * 64], dc[luma[4] * 64] = 1024, -1024                             # a DC difference of -2048: category 12
    wild = np.random.RandomState(5).randint(-32768, 32768, good.size).astype(np.int16)
    for name, bad in (('ac', ac), ('dc', dc), ('wild', wild)):
        assert C.reference_scan(host, bad, H, W, sub)[0] <= -1000, name          # the host coder refuses it too
        for cap in (None, 100, 0):
            n, status, got = _device_scan(dev, bad, H, W, sub, capacity=cap)     # the canaries are checked in there
            assert (n, status) == (0, JPEG_SCAN_RANGE), (name, cap, n, status)
    st, ref = C.reference_scan(host, good, H, W, sub)
    n, status, got = _device_scan(dev, good, H, W, sub)                          # a valid call afterwards is not affected
    assert (n, status) == (len(ref), JPEG_SCAN_OK) and got == ref


def test_the_same_call_twice_gives_the_same_bytes_and_follows_stream_order(dev):
    host = hip.load_host()
    sub = 2
    H, W = C.SIZE[sub]
    coef = dict(C.cases(sub))['dense_random']
    first, second = _device_scan(dev, coef, H, W, sub), _device_scan(dev, coef, H, W, sub)
    assert first == second and first[1] == JPEG_SCAN_OK
    # on a side stream, behind jpeg_encode_coef on that stream: it reads the finished coefficients of THIS image, not what the
    # buffer held before
    img = IMAGES['noise_64x96']
    d_img = torch.from_numpy(img).to(dev)
    nelem = jpeg_encode_bound(64, 96, sub)[1] // 2
    d_coef = torch.zeros(nelem, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        jpeg_encode_coef(d_img, 90, NAME[sub], d_coef)
        out, result = jpeg_encode_scan(d_coef, 64, 96, NAME[sub])
    side.synchronize()
    n, status = (int(v) for v in result.cpu())
    st, ref = E.write_file(host, d_coef.cpu().numpy(), 64, 96, sub, E.quant_tables(host, 90)[1])
    assert st == 0 and status == JPEG_SCAN_OK
    assert out[:n].cpu().numpy().tobytes() == ref[C.HEADER_BYTES:-2]
    assert d_coef.cpu().numpy().any()


def _write_all(dev, tmp_path, tag, images, **kw):
    w = DeviceJpegWriter(dev, workers=2, slots=2, quality=90, **kw)
    names = [str(tmp_path / tag / ('f%02d.jpg' % i)) for i in range(len(images))]
    for img, name in zip(images, names):
        w.submit(img, name)
    assert w.close() == names
    return w, [open(n, 'rb').read() for n in names]


def test_writer_files_are_identical_in_both_modes_and_a_slot_grows(dev, tmp_path):
    imgs = [torch.from_numpy(E.smooth_noise(40, 24, i)).to(dev) for i in range(3)] + \
           [torch.from_numpy(E.smooth_noise(64, 96, 10 + i)).to(dev) for i in range(3)]      # the larger size second: 2 slots have to grow
    wh, host_files = _write_all(dev, tmp_path, 'host', imgs)
    wd, dev_files = _write_all(dev, tmp_path, 'device', imgs, entropy='device')
    assert dev_files == host_files
    assert (wd.submitted, wd.device_encoded, wd.scan_encoded, wd.fallback_encoded) == (6, 6, 6, 0)
    assert (wh.scan_encoded, wh.fallback_encoded) == (0, 0)
    assert wd.bytes_written == wh.bytes_written == sum(len(f) for f in host_files)
    # what crossed: the scans and 16 bytes each, against every coefficient
    assert wd.bytes_downloaded == sum(len(f) - C.HEADER_BYTES - 2 + 16 for f in host_files)
    assert wh.bytes_downloaded == 3 * jpeg_encode_bound(40, 24)[1] + 3 * jpeg_encode_bound(64, 96)[1]
    if _have_pillow():
        for img, data in zip(imgs, dev_files):
            assert E.scan_of(data) == E.scan_of(E.pil_file(img.cpu().numpy(), 90, 2))
    with pytest.raises(ValueError):
        DeviceJpegWriter(dev, entropy='gpu')


def test_writer_with_a_tiny_scan_slot_falls_back_to_the_host_coder_and_counts_it(dev, tmp_path):
    imgs = [torch.from_numpy(E.smooth_noise(64, 96, 20 + i)).to(dev) for i in range(3)]
    _, host_files = _write_all(dev, tmp_path, 'host', imgs)
    w, files = _write_all(dev, tmp_path, 'tiny', imgs, entropy='device', scan_capacity=64)
    assert files == host_files
    assert (w.device_encoded, w.scan_encoded, w.fallback_encoded) == (3, 0, 3)


def test_flow_writer_jpg_files_are_identical_in_both_modes(dev, tmp_path):
    from vps_amd.flowvis import FlowWriter
    rng = np.random.RandomState(2)
    flows = [torch.from_numpy((rng.randn(40, 56, 2) * 4).astype(np.float32)).to(dev) for _ in range(3)]
    files = {}
    for mode in ('host', 'device'):
        w = FlowWriter(dev, fmt='jpg', entropy=mode)
        names = [str(tmp_path / mode / ('flow%d.jpg' % i)) for i in range(3)]
        for f, n in zip(flows, names):
            w.submit(f, n)
        assert w.close() == names
        files[mode] = [open(n, 'rb').read() for n in names]
        assert w.images.scan_encoded == (3 if mode == 'device' else 0)
    assert files['device'] == files['host'] and all(len(f) > C.HEADER_BYTES for f in files['host'])
    assert os.path.getsize(names[0]) == len(files['device'][0])
