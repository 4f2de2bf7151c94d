"""GPU: the device half of the JPEG output path (`vps_overlay_render`, `vps_jpeg_encode_coef`: csrc/jpeg_enc_ops.hip), `jpeg_encode` and
`DeviceJpegWriter`. Everything is integer arithmetic that libjpeg defines, so every comparison is exact equality: with the NumPy
restatement (tests/jpeg_enc_restate.py, pinned to Pillow coefficient by coefficient in tests/test_jpeg_enc.py) and with Pillow's files
directly."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_enc_restate as E
import jpeg_restate as R
from vps_amd import hip
from vps_amd.pipeline import jpeg_decode
from vps_amd.postprocess import DeviceJpegWriter, jpeg_encode, jpeg_encode_bound, jpeg_encode_coef, jpeg_quant_tables, render_overlay

pytestmark = pytest.mark.gpu
SUBS = [2, 0]
NAME = {2: '4:2:0', 0: '4:4:4'}


def _have_pillow():
    try:
        from PIL import Image  # noqa: F401
        return True
    except ImportError:
        return False


def _pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert('RGB')).copy()


def _colour_map(H, W, seed):
    """a random painted map: vertical bands, void regions (0,0,0), one-pixel-wide segments in both directions, a one-pixel segment in
    the last row and column"""
    rng = np.random.RandomState(seed)
    pal = rng.randint(1, 256, (9, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    idx = (xx * 5 // W + (yy * 3 // H) * 2) % 9
    m = pal[idx]
    m[H // 4:H // 2, W // 5:W // 2] = 0                                          # a void block
    m[:, W // 3] = pal[8]                                                        # a segment one pixel wide
    m[H // 2, :] = pal[7]                                                        # and one pixel high
    m[0, 0] = 0
    m[H - 1, W - 1] = (1, 2, 3)
    m[rng.rand(H, W) < 0.03] = 0                                                 # void specks
    return np.ascontiguousarray(m)


@pytest.mark.parametrize('sub', SUBS)
def test_device_coefficients_equal_the_restatement_and_pillow(dev, sub):
    host = hip.load_host()
    wrong = []
    for name, img in E.images():
        H, W = img.shape[:2]
        d_img = torch.from_numpy(img).to(dev)
        wide = torch.full((H, W + 5, 3), 99, dtype=torch.uint8, device=dev)      # a view with a row stride of 3 * (W + 5) bytes
        wide[:, :W] = d_img
        for q in E.QUALITIES:
            qt = jpeg_quant_tables(q)
            want = E.restate(img, qt, sub)
            got = jpeg_encode_coef(d_img, q, NAME[sub]).cpu().numpy()
            assert got.shape == want.shape, (name, q)
            strided = jpeg_encode_coef(wide[:, :W], q, NAME[sub]).cpu().numpy()
            bad = [int((got != want).sum()), int((strided != want).sum())]
            if _have_pillow():
                st, info = R.jpeg_info(host, E.pil_file(img, q, sub))
                assert st == 0
                st, ref = R.decode_coef(host, E.pil_file(img, q, sub), info)
                assert st == 0 and info.grid == jpeg_encode_bound(H, W, NAME[sub])[0]
                bad.append(int((got != ref).sum()))
            print('%-18s sub %d q %3d: differing coefficients (restatement, strided, Pillow) %s' % (name, sub, q, bad))
            if any(bad):
                wrong.append((name, q, bad))
    assert not wrong, wrong


@pytest.mark.parametrize('size', [(17, 33), (64, 96)])
def test_render_overlay_equals_its_restatement(dev, size):
    H, W = size
    rng = np.random.RandomState(H)
    frame = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    colour = _colour_map(H, W, W)
    assert (colour == 0).all(-1).any() and (colour != 0).any(-1).any()
    for alpha in (0, 77, 128, 256):
        got = render_overlay(torch.from_numpy(frame).to(dev), torch.from_numpy(colour).to(dev), alpha)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
        want = E.render_overlay(frame, colour, alpha)
        assert np.array_equal(got.cpu().numpy(), want), (alpha, int((got.cpu().numpy() != want).sum()))
    # host arrays are uploaded
    assert np.array_equal(render_overlay(frame, torch.from_numpy(colour).to(dev), 128).cpu().numpy(), E.render_overlay(frame, colour, 128))


@pytest.mark.parametrize('sub', SUBS)
def test_end_to_end_file_equals_pillows_scan_and_decodes_to_pillows_pixels(dev, sub):
    for (H, W), q in (((64, 96), 90), ((17, 33), 75), ((24, 40), 50)):
        frame = E.smooth_noise(H, W, 11)[..., ::-1].copy()                       # BGR
        colour = _colour_map(H, W, 5)
        rgb = render_overlay(torch.from_numpy(frame).to(dev), torch.from_numpy(colour).to(dev), 128)
        data = jpeg_encode(rgb, quality=q, subsampling=NAME[sub])
        assert isinstance(data, bytes) and data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
        ref = E.pil_file(rgb.cpu().numpy(), q, sub)
        assert E.scan_of(data) == E.scan_of(ref), (H, W, q)
        # and back through the project's own decoder: the library's pixels in both directions
        back = jpeg_decode(data, dev)
        assert back is not None
        assert np.array_equal(back.cpu().numpy()[..., ::-1], _pil_rgb(ref)), (H, W, q)
        assert np.array_equal(_pil_rgb(data), _pil_rgb(ref))


def test_device_jpeg_writer_ring(dev, tmp_path):
    frames = [torch.from_numpy(E.smooth_noise(64, 96, 20 + i)).to(dev) for i in range(12)]
    w = DeviceJpegWriter(dev, workers=2, slots=4, quality=85)
    names = [str(tmp_path / 'overlay' / ('f%02d.jpg' % i)) for i in range(12)]
    for t, n in zip(frames, names):
        w.submit(t, n)
    assert sorted(w.close()) == names
    total = 0
    for t, n in zip(frames, names):
        data = open(n, 'rb').read()
        assert data == jpeg_encode(t, quality=85), n
        total += len(data)
    assert (w.submitted, w.device_encoded, w.bytes_written) == (12, 12, total)
    assert w.free.qsize() == 4                                                   # every slot came back


def test_device_jpeg_writer_surfaces_a_workers_exception(dev, tmp_path):
    blocker = tmp_path / 'not_a_directory'
    blocker.write_text('a file where the output folder should be')
    w = DeviceJpegWriter(dev, workers=2, slots=4)
    t = torch.from_numpy(E.smooth_noise(64, 96, 1)).to(dev)
    w.submit(t, str(tmp_path / 'ok.jpg'))
    w.submit(t, str(blocker / 'x.jpg'))
    with pytest.raises(OSError):
        w.close()
    assert os.path.exists(str(tmp_path / 'ok.jpg')) and w.device_encoded == 1 and w.submitted == 2
    assert w.free.qsize() == 4


def test_full_size_frame_equals_the_restatement(dev):
    """1024x2048 in 4:2:0: 49152 blocks, the grid arithmetic beyond 16-bit block indices"""
    H, W = 1024, 2048
    img = E.smooth_noise(H, W, 2)
    img[300:360, 900:1000] = np.where(np.indices((60, 100)).sum(0)[..., None] % 2, 255, 0)       # a hard-edged patch
    qt = jpeg_quant_tables(90)
    want = E.restate(img, qt, 2)
    assert want.size == 49152 * 64
    got = jpeg_encode_coef(torch.from_numpy(img).to(dev), 90, '4:2:0').cpu().numpy()
    assert got.shape == want.shape and int((got != want).sum()) == 0


class _Colours:
    """a deterministic colour generator with the converter's `get_color(category)` contract"""

    def __init__(self):
        self.n = 0

    def get_color(self, cat):
        self.n += 1
        return [(40 + 37 * self.n) % 256, (90 + 11 * cat) % 256, (7 * self.n + 3) % 255 + 1]


def _pan_2ch(H, W, seed):
    """a unified 3-channel map (pan_seg, pan_ins, pan_obj): two stuff bands, one void band (255) and two objects"""
    yy, xx = np.mgrid[0:H, 0:W]
    seg = np.where(yy < H // 3, 0, np.where(yy < 2 * H // 3, 3, 255)).astype(np.uint8)
    ins, obj = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for k, (cy, cx) in enumerate(((H // 4 + seed, W // 4), (H // 2, 3 * W // 4 - seed))):
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= (H // 6) ** 2
        seg[m], ins[m], obj[m] = 11 + k, k + 1, 20 + k
    return np.ascontiguousarray(np.stack([seg, ins, obj], -1))


def test_write_overlays_writes_every_frame_and_clip_feeder_keeps_the_frames(dev, tmp_path):
    from PIL import Image

    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    from vps_amd.postprocess import TrackConverter, write_overlays
    from vps_amd import synth
    H, W, n = 64, 96, 6
    files = []
    for t in range(n):
        fn = str(tmp_path / ('v_%02d_newImg8bit.png' % t))
        Image.fromarray(E.smooth_noise(H, W, 30 + t)).save(fn)
        files.append(fn)
    prep = DeviceImagePrep(synth.MEAN, synth.STD, to_rgb=True, size_divisor=32, img_scale=(W, H), device=dev)
    fd = ClipFeeder(files, prep, workers=2, keep_frames=True)
    frames = []
    for t in range(n):
        fd(t)
        frames.append(fd.frame(t))
        assert np.array_equal(frames[-1].cpu().numpy(), E.smooth_noise(H, W, 30 + t)[..., ::-1])     # the decoded BGR frame
    fd.close()
    with pytest.raises(KeyError):
        fd.frame(0)                                                              # long out of the window
    twos = [_pan_2ch(H, W, t % 3) for t in range(n)]
    names = [os.path.basename(f) for f in files]
    out = write_overlays(twos, frames, names, str(tmp_path / 'ov'), _Colours(), 3, device=dev, alpha=100, quality=80)
    assert out == [str(tmp_path / 'ov' / n_.replace('.png', '.jpg')) for n_ in names] and sorted(os.listdir(str(tmp_path / 'ov'))) == sorted(os.path.basename(o) for o in out)
    gen, conv = _Colours(), TrackConverter(dev)
    for v0 in (0, 3):                                                            # two videos of three frames, converted as write_overlays does
        _, cols, _ = conv.convert_device(twos[v0:v0 + 3], gen)
        for j, col in enumerate(cols):
            assert (col.cpu().numpy() == 0).all(-1).any()                        # the void band stays unpainted
            want = jpeg_encode(render_overlay(frames[v0 + j], col, 100), quality=80)
            assert open(out[v0 + j], 'rb').read() == want, v0 + j
            assert _pil_rgb(want).shape == (H, W, 3)
