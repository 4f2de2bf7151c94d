"""GPU: the KITTI flow path - `vps_kitti_flow_reconstruct` (csrc/png_in_ops.hip), `vps_kitti_flow_encode` (csrc/kitti_flow_ops.hip),
`vps_png_deflate_bpp` (csrc/png_ops.hip) and vps_amd/kittiflow.py - against tests/png16_cases.py + tests/kitti_flow_restate.py. Everything is
exact: the un-filter is byte arithmetic, the decode is exact in fp32, the coding is a stated fp32 rule; every comparison is `array_equal`.
The shapes mirror tests/test_png_reconstruct_gpu.py at 6 bytes per pixel: the smallest at which the wavefront can go wrong."""
import ctypes
import io
import zlib

import numpy as np
import pytest
import torch

import flow_err_restate as FE
import kitti_flow_restate as K
import png16_cases as P
from vps_amd import floweval, hip, kittiflow

pytestmark = pytest.mark.gpu
F = np.float32


def _reconstruct(dev, scan, H, W, noc=None, offset=0):
    buf = torch.zeros(offset + len(scan) + 8, dtype=torch.uint8)
    buf[offset:offset + len(scan)] = torch.frombuffer(bytearray(scan), dtype=torch.uint8)
    d = buf.to(dev)[offset:offset + len(scan)]
    assert d.data_ptr() % 4 == offset % 4
    nv = None if noc is None else torch.from_numpy(np.ascontiguousarray(noc)).to(dev)
    flow, mask = kittiflow.kitti_flow_reconstruct(d, H, W, nv)
    return flow.cpu().numpy(), mask.cpu().numpy()


def _check(dev, raw, types, offset=0, noc=None):
    """file -> host inflate -> upload at `offset` -> device un-filter + decode == the restatement's decode of the ORIGINAL bytes"""
    H, W = raw.shape[0], raw.shape[1] // 6
    data, scan = P.encode(raw, types)
    got_scan, h, w = kittiflow.png16_inflate(data)
    assert (h, w) == (H, W) and got_scan.tobytes() == scan
    want_flow, valid = K.decode(P.rgb16(raw))
    flow, mask = _reconstruct(dev, scan, H, W, noc, offset)
    bad = np.argwhere(flow != want_flow)
    assert bad.size == 0, ('first differing (row, column, component)', bad[0].tolist(), 'of', len(bad), 'filter types', list(types)[:40])
    assert np.array_equal(mask, K.mask_codes(valid, noc))


@pytest.mark.parametrize('H,W', [(7, 5), (33, 67)])
def test_every_pair_of_adjacent_filter_types_and_every_type_as_row_0(dev, H, W):
    pairs = len(P.ALL_PAIRS) - 1
    for k, start in enumerate(range(0, pairs, max(H - 1, 1)) if H < 26 else [0]):
        _check(dev, P.noise(H, W, seed=100 + k), P.types_all_pairs(H, start))
    for t0 in range(5):                                          # Up, Average and Paeth without a row above
        _check(dev, P.noise(H, W, seed=200 + t0), [t0] + P.types_all_pairs(H)[1:])


def test_values_0_1_255_hit_the_paeth_ties(dev):
    raw = P.noise(33, 67, seed=300, values=(0, 1, 255))
    _check(dev, raw, [1] + [4] * 32)
    _check(dev, raw, P.types_all_pairs(33))


@pytest.mark.parametrize('H,W', [(9, 1), (9, 2), (9, 3), (9, 4), (9, 5), (1, 1), (1, 67), (1, 4)])
def test_rows_shorter_than_the_wavefront_lag_partial_chunks_and_a_single_row(dev, H, W):
    for t0 in range(5):
        _check(dev, P.noise(H, W, seed=400 + 10 * W + t0), [t0] + [4, 3, 2, 4, 3, 2, 4, 3][:H - 1])


@pytest.mark.parametrize('ft', [2, 3, 4])
def test_one_group_longer_than_a_band_reads_the_carried_raw_row(dev, ft):
    """block_rows + 3 rows behind a Sub row 0: the second band starts from the first band's last RAW row, which the decoded output no
    longer holds - that row has B = 256, B = 0 (with R and G set) and B = 1 pixels, so a row rebuilt from the flow would differ"""
    R = hip.png_block_rows()
    H, W = R + 3, 5
    raw = P.noise(H, W, seed=500 + ft)
    rgb = P.rgb16(raw)
    rgb[R - 1, :, 2] = [256, 0, 1, 0, 256]
    raw = P.raw_of(rgb)
    assert not K.decode(rgb)[1][R - 1, 1] and rgb[R - 1, 1, 0] != 0
    _check(dev, raw, [1] + [ft] * (H - 1))


def test_two_bands_and_a_bit_in_wider_rows_and_many_one_row_groups(dev):
    R = hip.png_block_rows()
    H = 2 * R + 2
    _check(dev, P.noise(H, 9, seed=550), [0] + [4, 3, 4, 2] * ((H - 1) // 4) + [4] * ((H - 1) % 4))
    rg = np.random.default_rng(600)
    _check(dev, P.noise(64, 9, seed=601), rg.integers(0, 2, 64).tolist())
    types = []
    for n in range(1, 12):                                       # groups of 1, 2, 3 .. 11 rows
        types += [n % 2] + [2 + (n + k) % 3 for k in range(n - 1)]
    _check(dev, P.noise(len(types), 21, seed=700), types)


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
@pytest.mark.parametrize('W', [6, 7])
def test_all_four_misalignments_of_the_scan(dev, W, offset):
    _check(dev, P.noise(13, W, seed=800 + W), P.types_all_pairs(13), offset=offset)


@pytest.mark.parametrize('H,W', [(13, 7), (12, 8)])
def test_mask_codes_with_and_without_the_noc_file(dev, H, W):
    rg = np.random.default_rng(900 + W)
    raw = P.noise(H, W, seed=901)
    rgb = P.rgb16(raw)
    rgb[..., 2] = np.array([0, 1, 256, 65535], np.uint16)[rg.integers(0, 4, (H, W))]
    raw = P.raw_of(rgb)
    noc = np.where(rg.random((H, W)) < 0.5, rg.integers(1, 256, (H, W)), 0).astype(np.uint8)
    codes = K.mask_codes(K.decode(rgb)[1], noc)
    assert set(np.unique(codes).tolist()) == {0, 1, 2}
    _check(dev, raw, P.types_all_pairs(H), noc=noc)
    _check(dev, raw, P.types_all_pairs(H))


def test_known_answers_read(dev):
    rgb = np.zeros((1, len(K.KNOWN_READ) + len(K.KNOWN_VALID), 3), np.uint16)
    want_u, want_valid = [], []
    for i, (R, u) in enumerate(K.KNOWN_READ):
        rgb[0, i] = (R, 65535 - R if R else 1, 1)
        want_u.append(u); want_valid.append(True)
    for j, (B, ok) in enumerate(K.KNOWN_VALID):
        rgb[0, len(K.KNOWN_READ) + j] = (32768 + 64, 32768 - 128, B)
        want_u.append(1.0 if ok else 0.0); want_valid.append(ok)
    raw = P.raw_of(rgb)
    flow, mask = _reconstruct(dev, P.encode(raw, [4])[1], 1, rgb.shape[1])
    assert flow[0, :, 0].tolist() == want_u and mask[0].tolist() == [int(v) for v in want_valid]
    assert flow[0, len(K.KNOWN_READ):, 1].tolist() == [-2.0 if ok else 0.0 for _, ok in K.KNOWN_VALID]


def _encode(dev, flow, valid=None):
    return kittiflow.kitti_flow_encode(torch.from_numpy(flow).to(dev), valid).cpu().numpy()


def test_known_answers_write(dev):
    u = np.array([a for a, _ in K.KNOWN_WRITE] + [np.nan, np.inf, -np.inf, 1.0, 1.0, 1.0], F)
    v = np.array([-a for a, _ in K.KNOWN_WRITE] + [1.0, 1.0, 1.0, np.nan, np.inf, -np.inf], F)
    flow = np.stack([u, v], axis=-1)[None]
    got = P.rgb16(_encode(dev, flow))
    n = len(K.KNOWN_WRITE)
    assert got[0, :n, 0].tolist() == [r for _, r in K.KNOWN_WRITE] and (got[0, :n, 2] == 1).all()
    assert (got[0, n:] == 0).all()                                # NaN and +-inf in either component: (0, 0, 0)
    assert np.array_equal(got, K.encode(flow))


def _field(H, W, seed):
    rg = np.random.default_rng(seed)
    flow = (rg.standard_normal((H, W, 2)) * 40).astype(F)
    flow.reshape(-1)[rg.integers(0, flow.size, 12)] = [np.nan, np.inf, -np.inf, 600.0, -600.0, 512.0, -512.0, 1 / 128, -1 / 128, 0.0, 511.99, -513.0]
    valid = (rg.random((H, W)) < 0.8).astype(np.uint8)
    return flow, valid


@pytest.mark.parametrize('H,W', [(5, 1), (9, 67), (3, 66)])
def test_encode_padded_layout_valid_given_or_null(dev, H, W):
    flow, valid = _field(H, W, 1000 + W)
    want = P.raw_of(K.encode(flow, valid))
    assert np.array_equal(_encode(dev, flow, torch.from_numpy(valid).to(dev)), want)
    assert np.array_equal(_encode(dev, flow, valid), want) and np.array_equal(_encode(dev, flow, valid.astype(bool)), want)
    assert np.array_equal(_encode(dev, flow), P.raw_of(K.encode(flow)))
    # a padded NHWC layout (ld 4, coff 1), through the C entry point, against the dense one
    pad = torch.full((H, W, 4), 7.0, dtype=torch.float32, device=dev)
    pad[:, :, 1:3] = torch.from_numpy(flow).to(dev)
    out = torch.full((H * 6 * W + 16,), 0xA5, dtype=torch.uint8, device=dev)
    v = torch.from_numpy(valid).to(dev)
    assert hip.load().vps_kitti_flow_encode(hip.ptr(pad), 4, 1, hip.ptr(v), H, W, hip.ptr(out), hip.stream_ptr()) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:H * 6 * W].reshape(H, 6 * W), want) and (got[H * 6 * W:] == 0xA5).all()


@pytest.mark.parametrize('H,W', [(37, 53), (1, 1), (300, 20)])
def test_round_trip_and_the_file(dev, tmp_path, H, W):
    flow, valid = _field(H, W, 1100 + W) if H * W > 12 else (np.array([[[1.5, -2.25]]], F), np.ones((1, 1), np.uint8))
    qflow, qvalid = K.quantised(flow, valid)
    name = kittiflow.write_kitti_flow(torch.from_numpy(flow).to(dev), str(tmp_path / 'a' / 'f.png'), valid)
    data = open(name, 'rb').read()
    assert data == kittiflow.kitti_flow_bytes(torch.from_numpy(flow).to(dev), valid)
    # the file: IHDR 16 / 2, every CRC (P.chunks checks them), one IDAT that inflates to the documented filter rule's bytes
    ch = P.chunks(data)
    assert [t for t, _, _ in ch] == [b'IHDR', b'IDAT', b'IEND'] and P.ihdr_of(data) == (W, H, 16, 2, 0, 0, 0)
    raw = P.raw_of(K.encode(flow, valid))
    S, ftype = P.device_filter_rows(raw)
    assert zlib.decompress(ch[1][1]) == S.tobytes() and ch[1][1][:2] == b'\x78\x01'
    # the restatement's reader and the device reader both give the quantised field
    rflow, rvalid = K.read_file(data)
    assert np.array_equal(rflow, qflow) and np.array_equal(rvalid, qvalid)
    dflow, dmask = kittiflow.read_kitti_flow(name, device=dev)
    assert np.array_equal(dflow.cpu().numpy(), qflow) and np.array_equal(dmask.cpu().numpy(), qvalid.astype(np.uint8))
    # flow_occ + flow_noc: the noc file is the same field with fewer valid pixels
    noc_valid = valid & (np.arange(H * W).reshape(H, W) % 3 != 0)
    noc = kittiflow.write_kitti_flow(torch.from_numpy(flow).to(dev), str(tmp_path / 'noc.png'), noc_valid)
    dflow, dmask = kittiflow.read_kitti_flow(name, noc, device=dev)
    assert np.array_equal(dflow.cpu().numpy(), qflow) and np.array_equal(dmask.cpu().numpy(), K.mask_codes(qvalid, K.read_file(open(noc, 'rb').read())[1]))


def test_deflate_bpp_equals_deflate_for_one_and_three_bytes(dev):
    from vps_amd import postprocess as pp
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 3, (19, 23, 3), dtype=np.uint8)).to(dev)
    a, na = pp.png_deflate(img)
    b, nb = kittiflow.png_deflate_bpp(img.view(19, 69), 3)
    assert int(na) == int(nb) > 0 and torch.equal(a[:int(na)], b[:int(nb)])
    a, na = pp.png_deflate(img[:, :, 0].contiguous())
    b, nb = kittiflow.png_deflate_bpp(img[:, :, 0].contiguous(), 1)
    assert int(na) == int(nb) > 0 and torch.equal(a[:int(na)], b[:int(nb)])


def test_flow_writer_kitti(dev, tmp_path):
    from vps_amd.flowvis import FlowWriter, flow_name
    w = FlowWriter(dev, fmt='kitti', slots=2)
    fields, names = [], []
    for k, (H, W) in enumerate(((24, 40), (37, 53), (24, 40))):
        flow = _field(H, W, 1200 + k)[0]
        names.append(flow_name(str(tmp_path), 'frame_%d.jpg' % k, 'kitti'))
        w.submit(torch.from_numpy(flow).to(dev), names[-1])
        fields.append(flow)
    assert w.close() == names and w.written == 3 and all(n.endswith('.png') for n in names)
    for flow, name in zip(fields, names):
        data = open(name, 'rb').read()
        assert data == kittiflow.kitti_flow_bytes(torch.from_numpy(flow).to(dev))
        assert np.array_equal(K.read_file(data)[0], K.quantised(flow)[0])


def test_third_party_reader(dev, tmp_path):
    """a library that reads 16-bit RGB PNGs, where one is installed, must read what `write_kitti_flow` wrote and write what
    `read_kitti_flow` reads"""
    flow, valid = _field(37, 53, 1300)
    name = kittiflow.write_kitti_flow(torch.from_numpy(flow).to(dev), str(tmp_path / 'f.png'), valid)
    want = K.encode(flow, valid)
    readers = []
    try:
        import cv2
        if callable(getattr(cv2, 'imread', None)) and getattr(cv2, '__version__', None):
            readers.append(('cv2', lambda fn: cv2.imread(fn, cv2.IMREAD_UNCHANGED)[:, :, ::-1]))
    except ImportError:
        pass
    try:
        import imageio
        readers.append(('imageio', lambda fn: np.asarray(imageio.imread(fn))))
    except ImportError:
        pass
    try:
        import png as pypng
        readers.append(('pypng', lambda fn: np.vstack([np.asarray(r, np.uint16) for r in pypng.Reader(filename=fn).asDirect()[2]]).reshape(37, 53, 3)))
    except ImportError:
        pass
    try:
        from torchvision.io import ImageReadMode, read_image
        readers.append(('torchvision', lambda fn: read_image(fn, ImageReadMode.UNCHANGED).permute(1, 2, 0).numpy().astype(np.uint16)))
    except Exception:
        pass
    if not readers:
        pytest.skip('no library that reads 16-bit RGB PNGs is installed (cv2, imageio, pypng, torchvision)')
    for lib, read in readers:
        got = read(name)
        assert got.dtype == np.uint16 and np.array_equal(got, want), lib


def test_against_the_evaluator(dev, tmp_path):
    """a 37x53 KITTI-coded pair through FlowEvaluator: counts and image equal the restatement of the measures on the restatement's decode"""
    H, W = 37, 53
    rg = np.random.default_rng(1400)
    gt, gt_valid = _field(H, W, 1401)
    gt[~np.isfinite(gt)] = 3.0
    pred = (gt + rg.standard_normal((H, W, 2)) * np.where(rg.random((H, W, 1)) < 0.3, 8.0, 0.5)).astype(F)
    pred_valid = (rg.random((H, W)) < 0.95).astype(np.uint8)
    noc_valid = gt_valid & (rg.random((H, W)) < 0.7)
    files = {k: str(tmp_path / (k + '.png')) for k in ('pred', 'occ', 'noc')}
    open(files['pred'], 'wb').write(K.write_file(pred, pred_valid, P.types_all_pairs(H)))
    open(files['occ'], 'wb').write(K.write_file(gt, gt_valid, P.types_all_pairs(H, 7), idat_parts=3))
    open(files['noc'], 'wb').write(K.write_file(gt, noc_valid, [1] + [4] * (H - 1)))
    # the reference: the restatement's decode, invalid predicted pixels as NaN
    rp, rpv = K.read_file(open(files['pred'], 'rb').read())
    rg_, rgv = K.read_file(open(files['occ'], 'rb').read())
    rmask = K.mask_codes(rgv, K.read_file(open(files['noc'], 'rb').read())[1])
    rp = np.where(rpv[..., None], rp, F(np.nan)).astype(F)
    want = FE.flow_error(rp, rg_, rmask)
    assert want['counts'][0] > 0 and want['counts'][12] > 0 and want['counts'][24] > 0 and want['counts'][1] + want['counts'][13] > 0
    p, pm = kittiflow.read_kitti_flow(files['pred'], device=dev)
    p.masked_fill_((pm == 0).unsqueeze(-1), float('nan'))
    g, gm = kittiflow.read_kitti_flow(files['occ'], files['noc'], device=dev)
    ev = floweval.FlowEvaluator(dev)
    img = ev.add_pair(p, g, mask=gm, err_rgb=True)
    res = ev.result()
    assert res['counts'] == want['counts'].tolist() and np.array_equal(img.cpu().numpy(), want['rgb'])
    fig = FE.figures(want['counts'], want['sums'])
    n = want['n']
    for k in ('epe_all', 'epe_noc', 'epe_occ'):
        # |E| <= n u sum|x_i| for any summation order of at most n terms (the bound of tests/test_flow_eval_gpu.py), over the divisor
        assert abs(res[k] - fig[k]) <= n * 2.0 ** -53 * float(want['abs'].sum()) / max(fig['n'], 1) + 1e-300, k


def test_argument_errors_return_before_any_launch(dev):
    lib = hip.load()
    H, W = 6, 5
    need = ctypes.c_int64()
    assert lib.vps_kitti_flow_reconstruct_ws(H, W, ctypes.byref(need)) == 0 and need.value >= 4 * H
    assert lib.vps_kitti_flow_reconstruct_ws(0, W, ctypes.byref(need)) < 0 and lib.vps_kitti_flow_reconstruct_ws(H, 65536, ctypes.byref(need)) < 0
    assert lib.vps_kitti_flow_reconstruct_ws(H, W, None) < 0
    assert lib.vps_kitti_flow_reconstruct_ws(H, W, ctypes.byref(need)) == 0
    scan = torch.zeros(H * (1 + 6 * W), dtype=torch.uint8, device=dev)
    flow = torch.full((H * W * 2 + 8,), 7.0, dtype=torch.float32, device=dev)
    mask = torch.full((H * W + 8,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((need.value + 16,), 0xA5, dtype=torch.uint8, device=dev)
    P_ = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)

    def call(h=H, cap=H * W * 8, wsb=need.value, s=scan, f=flow, foff=0, m=mask, w=ws, woff=0):
        return lib.vps_kitti_flow_reconstruct(P_(s), h, W, None, P_(f, foff), cap, P_(m), P_(w, woff), wsb, hip.stream_ptr())
    assert call(h=0) == -1001 and call(s=None) == -1001 and call(f=None) == -1001 and call(m=None) == -1001 and call(w=None) == -1001
    assert call(foff=8) == -1003 and call(woff=2) == -1003
    assert call(cap=H * W * 8 - 1) == -1004 and call(wsb=need.value - 1) == -1006
    img = torch.full((H * 6 * W + 8,), 0xA5, dtype=torch.uint8, device=dev)

    def enc(f=flow, ld=2, coff=0, h=H, w=W, o=img, ooff=0, foff=0):
        return lib.vps_kitti_flow_encode(P_(f, foff), ld, coff, None, h, w, P_(o, ooff), hip.stream_ptr())
    assert enc(f=None) == -1001 and enc(o=None) == -1001 and enc(h=0) == -1002 and enc(w=65536) == -1002
    assert enc(ld=1) == -1003 and enc(coff=-1) == -1003 and enc(ld=2, coff=1) == -1003
    assert enc(ooff=2) == -1004 and enc(foff=2) == -1004
    cap, wsb, size = ctypes.c_int64(), ctypes.c_int64(), torch.zeros(1, dtype=torch.int64, device=dev)
    assert lib.vps_png_encode_bound_bpp(H, 6 * W, 6, ctypes.byref(cap), ctypes.byref(wsb)) == 0
    out = torch.full((cap.value,), 0xA5, dtype=torch.uint8, device=dev)
    dws = torch.full((wsb.value,), 0xA5, dtype=torch.uint8, device=dev)
    d = lambda bpp=6, rb=6 * W, stride=6 * W, wsn=wsb.value: lib.vps_png_deflate_bpp(P_(img), H, rb, bpp, stride, P_(out), cap.value, P_(size), P_(dws), wsn,
                                                                                  hip.stream_ptr())
    assert d(bpp=2) == -1002 and d(bpp=4) == -1002 and d(rb=31) == -1001 and d(stride=29) == -1004 and d(wsn=wsb.value - 1) == -1006
    torch.cuda.synchronize()
    assert bool((flow == 7.0).all()) and bool((mask == 0xA5).all()) and bool((ws == 0xA5).all()) and bool((img == 0xA5).all())
    assert bool((out == 0xA5).all()) and bool((dws == 0xA5).all())
    assert call() == 0                                            # exactly enough of everything: zeros, type None
    torch.cuda.synchronize()
    assert bool((flow[:H * W * 2] == 0).all()) and bool((flow[H * W * 2:] == 7.0).all())
    assert bool((mask[:H * W] == 0).all()) and bool((mask[H * W:] == 0xA5).all()) and bool((ws[need.value:] == 0xA5).all())
