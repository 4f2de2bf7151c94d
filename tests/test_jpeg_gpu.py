"""GPU: the device half of the JPEG input path (`vps_jpeg_reconstruct`, csrc/jpeg_ops.hip) and the clip feeder on JPEG files.
Everything is integer arithmetic that libjpeg defines, so every comparison is bitwise: against the arrays PIL (libjpeg-turbo) decoded
from the committed fixtures (tests/golden/jpeg_cases.npz) and against PIL's decode of files written by the test itself."""
import io
import os
import warnings

import numpy as np
import pytest
import torch

import vps_amd
from vps_amd import synth
from vps_amd.pipeline import ClipFeeder, DeviceImagePrep, jpeg_decode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')


def _pil_bgr(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def _encode(bgr_u8, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr_u8[..., ::-1])).save(b, 'JPEG', **kw)
    return b.getvalue()


def _clip_frames(n, H=128, W=256):
    return [synth.synth_frame(H, W, seed=3, shift=(2 * t, t), noise=2.0 if t else 0.0).astype(np.uint8) for t in range(n)]


def _write_clip(tmp_path, n, progressive_at=None):
    files = []
    for t, fr in enumerate(_clip_frames(n)):
        fn = str(tmp_path / ('frame_%02d.jpg' % t))
        with open(fn, 'wb') as f:
            f.write(_encode(fr, quality=90, subsampling=2, progressive=(t == progressive_at)))
        files.append(fn)
    return files


def _prep(dev):
    return DeviceImagePrep(synth.MEAN, synth.STD, to_rgb=True, size_divisor=32, img_scale=(256, 128), device=dev)


def test_reconstruct_is_bitwise_libjpeg_on_every_fixture(dev):
    z = np.load(CASES)
    names = sorted(k[5:] for k in z.files if k.startswith('file/'))
    assert len(names) >= 60
    wrong = []
    for n in names:
        got = jpeg_decode(z['file/' + n].tobytes(), dev)
        assert got is not None and got.is_cuda and got.dtype == torch.uint8, n
        want = torch.from_numpy(z['bgr/' + n])
        if got.shape != want.shape or not torch.equal(got.cpu(), want):
            wrong.append((n, int((got.cpu() != want).sum()) if got.shape == want.shape else tuple(got.shape)))
    assert not wrong, wrong


@pytest.mark.parametrize('sub', [2, 1, 0])
def test_reconstruct_1080x1920_is_bitwise_pil(dev, sub):
    """the VIPER frame size: 1080 rows end in half an MCU row (4:2:0), where the chroma edge is the true down-sampled height"""
    fr = synth.synth_frame(1080, 1920, seed=5).astype(np.uint8)
    fr[500:560, 800:900] = np.where(np.indices((60, 100)).sum(0)[..., None] % 2, 255, 0)           # a hard-edged patch
    data = _encode(fr, quality=92, subsampling=sub)
    got = jpeg_decode(data, dev)
    want = torch.from_numpy(_pil_bgr(data))
    assert tuple(got.shape) == (1080, 1920, 3)
    assert int((got.cpu() != want).sum()) == 0


def test_refused_files_return_none(dev):
    z = np.load(CASES)
    for k in [k for k in z.files if k.startswith('refuse/')]:
        assert jpeg_decode(z[k].tobytes(), dev) is None, k


def test_clip_feeder_on_a_jpeg_clip(dev, tmp_path):
    files = _write_clip(tmp_path, 8)
    prep = _prep(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)               # the PIL route warns that its pixels are not pinned: it must not be taken
        fd = ClipFeeder(files, prep, workers=3)
        prev, outs = None, []
        for t in range(8):
            img = fd(t)
            assert fd(t) is img
            if prev is not None:
                assert fd(t - 1) is prev                              # the same tensor object is frame t's img and frame t+1's ref_img
            outs.append(img)
            prev = img
        torch.cuda.synchronize()
        fd.close()
    assert fd.decodes == 8 and fd.native_jpeg == 8 and fd.fallback_decodes == 0
    for t in range(8):
        want = prep.prep(torch.from_numpy(_pil_bgr(open(files[t], 'rb').read())).to(dev))[0]
        assert tuple(outs[t].shape) == (1, 3, 128, 256)
        assert torch.equal(outs[t][0], want), t
        assert fd.meta(t)['ori_shape'] == (128, 256, 3)


def test_clip_feeder_falls_back_for_a_progressive_frame(dev, tmp_path):
    files = _write_clip(tmp_path, 8, progressive_at=5)
    prep = _prep(dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fd = ClipFeeder(files, prep, workers=2)
        outs = [fd(t) for t in range(8)]
        torch.cuda.synchronize()
        fd.close()
    assert fd.decodes == 8 and fd.native_jpeg == 7 and fd.fallback_decodes == 1
    for t in range(8):
        want = prep.prep(torch.from_numpy(_pil_bgr(open(files[t], 'rb').read())).to(dev))[0]
        assert torch.equal(outs[t][0], want), t


def test_detector_outputs_of_a_jpeg_fed_clip_equal_those_of_pil_decoded_frames(dev, tmp_path):
    """files -> ClipFeeder (native JPEG) -> ClipShardRunner + DetectorBackend == the same frames decoded by PIL and uploaded"""
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    H, W, n = 128, 256, 4
    files = _write_clip(tmp_path, n)
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    m = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synth.load_synth(m, 0)
    m.to(dev)
    m.ensure_packed(dev)
    prep = _prep(dev)
    frd = [prep.prep(torch.from_numpy(_pil_bgr(open(f, 'rb').read())).to(dev))[0].unsqueeze(0) for f in files]
    m._cache = None; m._pf = None; m.reset_tracker()
    ref = ClipShardRunner(DetectorBackend(m, H, W, prefetch=True), 0, 1, None, dev).run(lambda t: frd[t], n)
    keys = ('panoptic_det_obj_ids', 'panoptic_outputs', 'fcn_outputs', 'panoptic_cls_prob')
    ref = [{k: (o[k].cpu().numpy().copy() if torch.is_tensor(o[k]) else np.asarray(o[k]).copy()) for k in keys} for o in ref]
    m._cache = None; m._pf = None; m.reset_tracker()
    fd = ClipFeeder(files, prep, workers=2)
    outs = ClipShardRunner(DetectorBackend(m, H, W, prefetch=True), 0, 1, None, dev).run(fd, n)
    fd.close()
    assert fd.native_jpeg == n and fd.fallback_decodes == 0
    for t in range(n):
        for k in keys:
            got = outs[t][k]
            got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
            assert np.array_equal(got, ref[t][k]), (t, k)
