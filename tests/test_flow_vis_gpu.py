"""GPU: the flow colour kernels (`vps_flow_max_radius`, `vps_flow_colour`: csrc/flow_vis_ops.hip), `FlowWriter` and the detector's
`keep_flow`. The colour coding is fp64 arithmetic in a fixed order whose result does not depend on the last ulps of atan2
(tests/test_flow_vis.py), so every comparison is exact equality: with the reference's own float64 images
(tests/golden/flow_vis_cases.npz) and with the NumPy restatement (tests/flow_vis_restate.py)."""
import io
import os

import numpy as np
import pytest
import torch

import flow_vis_restate as F
import vps_amd
from vps_amd import flowvis, nhwc, synth
from vps_amd.flowvis import FlowWriter, flow_colour, flow_max_radius
from vps_amd.postprocess import jpeg_encode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, _ = F.load_golden()
VIEWS = [(2, 0), (4, 0), (8, 2)]          # (ld, coff): dense, FlowNet2's own layout, a window of a wider map
FILL = 777.0


def _fmap(flow, ld, coff, dev):
    """the flow as an FMap window of a [1,H,W,ld] map whose other channels hold FILL"""
    wide = torch.from_numpy(F.strided(flow, ld, coff, FILL)).to(dev)[None].contiguous()
    return nhwc.FMap(wide, 2, coff), wide


def _pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert('RGB')).copy()


@pytest.mark.parametrize('case', sorted(CASES))
def test_max_radius_equals_numpy_bit_for_bit(dev, case):
    flow = CASES[case]['flow']
    want = F.max_radius(flow)
    got = flow_max_radius(torch.from_numpy(flow).to(dev))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (1,)
    assert got.cpu().numpy().tobytes() == np.float64(want).tobytes(), (float(got), want)
    nchw = torch.from_numpy(np.ascontiguousarray(flow.transpose(2, 0, 1))[None]).to(dev)
    assert flow_max_radius(nchw).cpu().numpy().tobytes() == np.float64(want).tobytes()
    for ld, coff in VIEWS[1:]:
        fm, _ = _fmap(flow, ld, coff, dev)
        out = torch.full((1,), 5e300, dtype=torch.float64, device=dev)           # the call zeroes its result itself
        assert flow_max_radius(fm, out) is out
        assert out.cpu().numpy().tobytes() == np.float64(want).tobytes(), (ld, coff, float(out), want)


@pytest.mark.parametrize('case', sorted(CASES))
def test_colour_equals_the_float64_golden(dev, case):
    flow, want = CASES[case]['flow'], CASES[case]['rgb64']
    got = flow_colour(torch.from_numpy(flow).to(dev))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
    got = got.cpu().numpy()
    print('%s: %d differing levels of %d' % (case, int((got != want).sum()), want.size))
    assert np.array_equal(got, want)
    nchw = torch.from_numpy(np.ascontiguousarray(flow.transpose(2, 0, 1))[None]).to(dev)
    assert np.array_equal(flow_colour(nchw).cpu().numpy(), want)
    for ld, coff in VIEWS[1:]:
        fm, wide = _fmap(flow, ld, coff, dev)
        before = wide.clone()
        first = flow_colour(fm).cpu().numpy()
        second = flow_colour(fm).cpu().numpy()
        assert np.array_equal(first, want), (ld, coff, int((first != want).sum()))
        assert first.tobytes() == second.tobytes()                              # twice: identical bytes
        assert torch.equal(wide, before)                                         # the padding channels (and the flow) are untouched
        pad = [c for c in range(ld) if not coff <= c < coff + 2]
        assert bool((wide[..., pad] == FILL).all())


def test_fixed_normaliser_equals_the_restatement(dev):
    """max_rad = 4 on an N(0, 4) field: about 60 % of the pixels are beyond it and take the darkened branch"""
    rng = np.random.default_rng(7)
    flow = rng.normal(0, 4, (64, 96, 2)).astype(np.float32)
    u, v = F.known(flow)
    over = float((np.sqrt(u * u + v * v) > 4.0).mean())
    assert 0.5 < over < 0.7, over
    want = F.colour(flow, 4.0)
    d_flow = torch.from_numpy(flow).to(dev)
    assert np.array_equal(flow_colour(d_flow, max_rad=4.0).cpu().numpy(), want)
    rad = torch.tensor([4.0], dtype=torch.float64, device=dev)
    assert np.array_equal(flow_colour(d_flow, max_rad=rad).cpu().numpy(), want)  # a device scalar
    assert not np.array_equal(flow_colour(d_flow).cpu().numpy(), want)           # the frame's own maximum is another image
    for ld, coff in VIEWS[1:]:
        assert np.array_equal(flow_colour(_fmap(flow, ld, coff, dev)[0], 4.0).cpu().numpy(), want)


def test_more_than_one_block_and_a_ragged_tail(dev):
    """33 x 63 = 2079 pixels: three blocks of 1024, the last with 31 pixels = 93 bytes (23 dwords and one byte)"""
    rng = np.random.default_rng(3)
    flow = (rng.normal(0, 2, (33, 63, 2)) * rng.uniform(0, 3, (33, 63, 1))).astype(np.float32)
    guard = torch.full((33 * 63 * 3 + 64,), 201, dtype=torch.uint8, device=dev)
    out = guard[:33 * 63 * 3].view(33, 63, 3)
    assert flow_colour(torch.from_numpy(flow).to(dev), out=out) is out
    assert np.array_equal(out.cpu().numpy(), F.colour(flow))
    assert bool((guard[33 * 63 * 3:] == 201).all())                             # nothing behind the image
    assert flow_max_radius(torch.from_numpy(flow).to(dev)).item() == F.max_radius(flow)


def test_bad_arguments_are_refused(dev):
    lib = vps_amd.hip.load()
    t = torch.zeros(4, 4, 2, device=dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    rgb = torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev)
    P = vps_amd.hip.ptr
    assert lib.vps_flow_max_radius(P(t), 2, 1, 4, 4, P(out), None) == -1002     # coff + 2 > ld
    assert lib.vps_flow_max_radius(P(t), 2, 0, 0, 4, P(out), None) == -1001
    assert lib.vps_flow_colour(P(t), 2, 0, 4, 4, None, P(rgb), None) == -1003
    assert lib.vps_flow_colour(P(t), 2, 0, 4, 4, P(out), None, None) == -1004
    with pytest.raises(vps_amd.hip.VpsHipError):
        flow_colour(torch.zeros(4, 4, 2))                                        # a host tensor: no CPU path


def test_flow_writer_flo_files_equal_the_references(dev, tmp_path):
    w = FlowWriter(dev, workers=2, slots=2, fmt='flo')
    names = {}
    for i, (case, c) in enumerate(sorted(CASES.items())):
        ld, coff = VIEWS[i % 3]
        names[case] = str(tmp_path / 'flo' / (case + '.flo'))
        w.submit(_fmap(c['flow'], ld, coff, dev)[0] if ld > 2 else torch.from_numpy(c['flow']).to(dev), names[case])
    assert sorted(w.close()) == sorted(names.values())
    for case, n in names.items():
        assert open(n, 'rb').read() == CASES[case]['flo'], case
        assert flowvis.read_flo(n).tobytes() == CASES[case]['flow'].tobytes()
    assert (w.submitted, w.written) == (4, 4) and w.free.qsize() == 2
    assert flowvis.flo_bytes(torch.from_numpy(CASES['3x5']['flow']).to(dev)) == CASES['3x5']['flo']       # the device branch of flo_bytes


@pytest.mark.parametrize('fmt', ['jpg', 'png'])
def test_flow_writer_images(dev, tmp_path, fmt):
    from PIL import Image
    w = FlowWriter(dev, workers=2, slots=2, fmt=fmt, quality=85)
    names = {}
    for case, c in sorted(CASES.items()):
        names[case] = str(tmp_path / fmt / (case + '.' + fmt))
        w.submit(_fmap(c['flow'], 4, 0, dev)[0], names[case])
    assert sorted(w.close()) == sorted(names.values())
    for case, n in names.items():
        rgb = flow_colour(torch.from_numpy(CASES[case]['flow']).to(dev))
        assert np.array_equal(rgb.cpu().numpy(), CASES[case]['rgb64'])
        data = open(n, 'rb').read()
        if fmt == 'jpg':
            # the file decodes to the image PIL decodes from jpeg_encode of flow_colour's own pixels (the entropy scan itself is pinned to
            # libjpeg's by tests/test_jpeg_enc_gpu.py)
            assert np.array_equal(_pil_rgb(data), _pil_rgb(jpeg_encode(rgb, quality=85))), case
            assert data == jpeg_encode(rgb, quality=85)
        else:
            with Image.open(n) as im:
                assert im.mode == 'RGB' and np.array_equal(np.asarray(im), CASES[case]['rgb64']), case       # lossless: the golden image
    assert (w.submitted, w.written) == (4, 4) and w.bytes_written == sum(os.path.getsize(n) for n in names.values())
    assert w.images.free.qsize() == 2                                            # every slot of the image writer came back


def test_submit_reads_the_flow_before_it_returns(dev, tmp_path):
    """12 frames through 2 slots from ONE source buffer that is overwritten right after each submit - a ring slot of the detector"""
    rng = np.random.default_rng(11)
    flows = [rng.normal(0, 1 + i, (40, 72, 2)).astype(np.float32) for i in range(12)]
    for fmt in ('flo', 'jpg'):
        src = torch.empty(1, 40, 72, 4, device=dev)
        fm = nhwc.FMap(src, 2, 0)
        w = FlowWriter(dev, workers=2, slots=2, fmt=fmt)
        names = [str(tmp_path / fmt / ('f%02d.%s' % (i, fmt))) for i in range(12)]
        for f, n in zip(flows, names):
            src.copy_(torch.from_numpy(F.strided(f, 4, 0))[None], non_blocking=False)
            w.submit(fm, n)
            src.fill_(-3.0)                                                      # stream-ordered behind submit's reads
        assert w.close() == names
        for f, n in zip(flows, names):
            data = open(n, 'rb').read()
            if fmt == 'flo':
                assert data == flowvis.flo_bytes(f), n
            else:
                rgb = torch.from_numpy(F.colour(f)).to(dev)
                assert data == jpeg_encode(rgb, quality=90), n
        assert (w.free if fmt == 'flo' else w.images.free).qsize() == 2


def test_write_flows(dev, tmp_path):
    flows = [torch.from_numpy(CASES[c]['flow']).to(dev) for c in ('67x131', '96x160_smooth')]
    out = flowvis.write_flows(flows, ['a/x_newImg8bit.png', 'y.jpg'], str(tmp_path / 'fl'), device=dev, fmt='png', max_rad=6.0)
    assert out == [str(tmp_path / 'fl' / 'x_newImg8bit.png'), str(tmp_path / 'fl' / 'y.png')]
    from PIL import Image
    for n, c in zip(out, ('67x131', '96x160_smooth')):
        with Image.open(n) as im:
            assert np.array_equal(np.asarray(im), F.colour(CASES[c]['flow'], 6.0))
    with pytest.raises(ValueError):
        FlowWriter(dev, fmt='gif')


def test_detector_keeps_the_flow(dev):
    """128x256, synthetic weights, the library-default f32 mode: `pano_results['flow']` is compute_flow's field for both frames, and
    nothing else of the result changes"""
    H, W = 128, 256
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synth.load_synth(model, 0)
    model.ensure_packed(dev)
    assert model.keep_flow is False
    frames = [f.to(dev) for f in synth.synth_clip(H, W, 2, 0)]

    def run(keep):
        model.keep_flow = keep
        model.reset_tracker()
        outs = []
        for t in range(2):
            meta = synth.img_meta(H, W, 10000 + t + 1)
            out = model(return_loss=False, rescale=True, img=[frames[t]], img_meta=[[meta]], ref_img=[frames[t - 1 if t else 0]])
            torch.cuda.synchronize()
            outs.append(out[2])
        return outs
    plain, kept = run(False), run(True)
    for t in range(2):
        assert 'flow' not in plain[t] and set(kept[t]) == set(plain[t]) | {'flow'}
        for k in plain[t]:
            assert np.array_equal(kept[t][k].cpu().numpy(), plain[t][k].cpu().numpy()), (t, k)
        flow = kept[t]['flow']
        assert flow.is_cuda and flow.dtype == torch.float32 and tuple(flow.shape) == (H, W, 2) and flow.is_contiguous()
        want, _ = model.compute_flow(frames[t], frames[t - 1 if t else 0])
        assert torch.equal(flow, want[0].permute(1, 2, 0)), (t, float((flow - want[0].permute(1, 2, 0)).abs().max()))
        assert flow.abs().max() > 0
    assert kept[0]['flow'].data_ptr() != kept[1]['flow'].data_ptr()              # fresh tensors: frame 0's survives frame 1
    # a cropped frame: img_shape smaller than the padded tensor
    meta = synth.img_meta(H, W, 10001)
    meta['img_shape'] = (120, 250, 3)
    model.reset_tracker()
    out = model(return_loss=False, rescale=True, img=[frames[0]], img_meta=[[meta]], ref_img=[frames[0]])
    assert tuple(out[2]['flow'].shape) == (120, 250, 2) and torch.equal(out[2]['flow'], kept[0]['flow'][:120, :250])
    model.keep_flow = False


def test_panoptic_track_has_no_flow_to_keep(dev):
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'track.py'))
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    model.keep_flow = True
    img = torch.zeros(1, 3, 128, 256, device=dev)
    with pytest.raises(vps_amd.hip.VpsHipError, match='keep_flow'):
        model(return_loss=False, rescale=True, img=[img], img_meta=[[synth.img_meta(128, 256, 10001)]], ref_img=[img])


@pytest.mark.parametrize('fmt', ['jpg', 'png', 'flo'])
def test_run_vps_synthetic_writes_a_readable_flow_file_per_frame(dev, tmp_path, fmt):
    """tools/run_vps_synthetic.py --flow DIR --flow-format FMT: its model loop on one clip of three 128x256 frames"""
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location('run_vps_synthetic', os.path.join(ROOT, 'tools', 'run_vps_synthetic.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / 'flow')
    res, _ = tool.run_model('f32', 1, 3, 128, 256, dev, flow=(out, fmt, 6.0 if fmt == 'png' else None))
    want = [os.path.join(out, os.path.splitext(n)[0] + '.' + fmt) for n in res['all_names']]
    assert len(want) == 3 and res['flow_files'] == want and sorted(os.listdir(out)) == sorted(os.path.basename(n) for n in want)
    for n in want:
        if fmt == 'flo':
            flow = flowvis.read_flo(n)
            assert flow.shape == (128, 256, 2) and np.isfinite(flow).all() and np.abs(flow).max() > 0
        else:
            with Image.open(n) as im:
                assert im.mode == 'RGB' and np.asarray(im).shape == (128, 256, 3)
