"""GPU: the Y4M kernels (`vps_yuv_to_bgr`, `vps_bgr_to_yuv`: csrc/yuv_ops.hip) against the NumPy restatement (tests/y4m_restate.py) -
integer arithmetic, so every comparison is exact equality -, their argument handling, `ClipFeeder` on a .y4m clip, `Y4mWriter`, the
round trip through a file and `write_overlays(video=...)`."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import y4m_restate as R
from test_y4m import ROUND_TRIP_BOUND
from vps_amd import hip, y4m

pytestmark = pytest.mark.gpu

RANGES, MATRICES = ('limited', 'full'), ('bt601', 'bt709')


def _tiles():
    a, b = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    assert hip.load().vps_yuv_tile(a, b) == 0
    return (a[0], a[1]), (b[0], b[1])


DEC_TILE, ENC_TILE = _tiles()
# (H, W): all-border chroma and odd plane offsets; one and several lane groups; one pixel row / two columns past a workgroup's tile of
# each kernel (4 x 256 decode, 8 x 512 encode - read from the library)
SIZES = [(1, 1), (2, 2), (3, 3), (1, 7), (7, 1), (16, 16), (17, 33), (DEC_TILE[0] + 1, DEC_TILE[1] + 2), (ENC_TILE[0] + 1, ENC_TILE[1] + 2)]


def _info(H, W, sampling, rng):
    return y4m.make_info(W, H, (30, 1), sampling, rng)


def _planes(n, seed):
    rs = np.random.RandomState(seed)
    extremes = rs.choice(np.array([0, 1, 15, 16, 17, 128, 234, 235, 236, 240, 241, 254, 255], dtype=np.uint8), n)
    return [rs.randint(0, 256, n, dtype=np.uint8), np.zeros(n, np.uint8), np.full(n, 255, np.uint8), extremes]


@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('rng', RANGES)
@pytest.mark.parametrize('sampling', R.SAMPLINGS)
def test_yuv_to_bgr_equals_the_restatement(dev, sampling, rng, matrix):
    assert DEC_TILE == (4, 256) and ENC_TILE == (8, 512)
    for H, W in SIZES:
        info = _info(H, W, sampling, rng)
        assert info.frame_bytes == R.frame_bytes(H, W, sampling)
        for k, planar in enumerate(_planes(info.frame_bytes, H * 1000 + W)):
            want = R.yuv_to_bgr(planar, H, W, sampling, rng, matrix)
            out = torch.full((H * W * 3 + 64,), 0xAB, dtype=torch.uint8, device=dev)
            got = y4m.yuv_to_bgr(torch.from_numpy(planar).to(dev), info, matrix, out[:H * W * 3])
            assert np.array_equal(got.cpu().numpy().reshape(H, W, 3), want), (H, W, k, sampling, rng, matrix)
            assert bool((out[H * W * 3:] == 0xAB).all())


@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('rng', RANGES)
@pytest.mark.parametrize('sampling', y4m.ENCODABLE)
def test_bgr_to_yuv_equals_the_restatement(dev, sampling, rng, matrix):
    for H, W in SIZES:
        n = R.frame_bytes(H, W, sampling)
        for k, flat in enumerate(_planes(H * W * 3, H * 1000 + W + 1)):
            bgr = flat.reshape(H, W, 3)
            want = R.bgr_to_yuv(bgr, sampling, rng, matrix)
            out = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
            y4m.bgr_to_yuv(torch.from_numpy(bgr).to(dev), sampling, rng, matrix, out[:n])
            assert np.array_equal(out[:n].cpu().numpy(), want), (H, W, k, sampling, rng, matrix)
            assert bool((out[n:] == 0xAB).all())
            if k == 0:                                             # rows 3 W + 5 bytes apart (odd row phases), and the R, G, B order
                ld = 3 * W + 5
                wide = torch.full((H * ld,), 0x5A, dtype=torch.uint8, device=dev)
                view = torch.as_strided(wide, (H, W, 3), (ld, 3, 1))
                view.copy_(torch.from_numpy(bgr).to(dev))
                assert np.array_equal(y4m.bgr_to_yuv(view, sampling, rng, matrix).cpu().numpy(), want), (H, W, 'strided')
                rgb = torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1])).to(dev)
                assert np.array_equal(y4m.bgr_to_yuv(rgb, sampling, rng, matrix, order='rgb').cpu().numpy(), want), (H, W, 'rgb')


def test_bad_arguments_are_refused_with_nothing_written(dev):
    lib, H, W = hip.load(), 6, 10
    info = _info(H, W, '420jpeg', 'limited')
    frame = torch.zeros(info.frame_bytes + 4, dtype=torch.uint8, device=dev)
    out = torch.full((H * W * 3 + 32,), 0xAB, dtype=torch.uint8, device=dev)
    s, f, o, n, cap = hip.stream_ptr(), hip.ptr(frame), hip.ptr(out), info.frame_bytes, H * W * 3
    calls = [(None, n, H, W, 0, 0, 0, o, cap, s), (f, n, H, W, 0, 0, 0, None, cap, s), (f, n, 0, W, 0, 0, 0, o, cap, s), (f, n, H, -1, 0, 0, 0, o, cap, s),
             (f, n, 65536, 65536, 0, 0, 0, o, cap, s), (f, n, H, W, 5, 0, 0, o, cap, s), (f, n, H, W, -1, 0, 0, o, cap, s), (f, n, H, W, 0, 2, 0, o, cap, s),
             (f, n, H, W, 0, 0, 2, o, cap, s), (f, n - 1, H, W, 0, 0, 0, o, cap, s), (f, n, H, W, 0, 0, 0, o, cap - 1, s),
             (ctypes.c_void_p(frame.data_ptr() + 1), n, H, W, 0, 0, 0, o, cap, s)]
    for c in calls:
        assert lib.vps_yuv_to_bgr(*c) <= -1000, c
    bgr = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    b = hip.ptr(bgr)
    calls = [(None, H, W, 3 * W, 0, 0, 0, 0, o, n, s), (b, H, W, 3 * W, 0, 0, 0, 0, None, n, s), (b, 0, W, 3 * W, 0, 0, 0, 0, o, n, s),
             (b, H, W, 3 * W - 1, 0, 0, 0, 0, o, n, s), (b, H, W, 3 * W, 0, 2, 0, 0, o, n, s), (b, H, W, 3 * W, 0, 4, 0, 0, o, n, s),
             (b, H, W, 3 * W, 0, 0, 2, 0, o, n, s), (b, H, W, 3 * W, 0, 0, 0, 2, o, n, s), (b, H, W, 3 * W, 0, 0, 0, 0, o, n - 1, s),
             (b, H, W, 3 * W, 0, 3, 0, 0, o, H * W * 3 - 1, s)]
    for c in calls:
        assert lib.vps_bgr_to_yuv(*c) <= -1000, c
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    with pytest.raises(ValueError):
        y4m.bgr_to_yuv(bgr, sampling='422')
    with pytest.raises(ValueError):
        y4m.yuv_to_bgr(frame, info, matrix='bt2020')


def test_conversion_is_ordered_behind_the_kernel_that_writes_its_input(dev):
    H, W = 64, 96
    info = _info(H, W, '420mpeg2', 'limited')
    planar = np.random.RandomState(8).randint(0, 256, info.frame_bytes, dtype=np.uint8)
    src = torch.from_numpy(planar).to(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        big = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
        for _ in range(8):
            big.add_(1)                                                # keeps the stream busy in front of the writer of the input
        frame = torch.zeros(info.frame_bytes, dtype=torch.uint8, device=dev)
        frame.copy_(src)
        bgr = y4m.yuv_to_bgr(frame, info)
        back = y4m.bgr_to_yuv(bgr, '420mpeg2')                         # and its own result feeds the next conversion
    stream.synchronize()
    want = R.yuv_to_bgr(planar, H, W, '420mpeg2')
    assert np.array_equal(bgr.cpu().numpy(), want)
    assert np.array_equal(back.cpu().numpy(), R.bgr_to_yuv(want, '420mpeg2'))


def _smooth(H, W, t):
    yy, xx = np.mgrid[0:H, 0:W]
    rs = np.random.RandomState(t)
    img = np.stack([(yy * 3 + xx * 2 + 20 * t) % 256, (xx * 5 + 7 * t) % 256, (yy * xx + t) % 256], -1) + rs.randint(-9, 10, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_clip_feeder_on_a_y4m_clip(dev, tmp_path):
    from vps_amd import synth
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    H, W, n = 64, 96, 6
    info = _info(H, W, '420jpeg', 'limited')
    frames = [R.bgr_to_yuv(_smooth(H, W, t), '420jpeg') for t in range(n)]
    path = str(tmp_path / 'clip.y4m')
    with open(path, 'wb') as f:
        f.write(y4m.y4m_header(info))
        for t, fr in enumerate(frames):
            f.write((b'FRAME Ip\n' if t % 2 else b'FRAME\n') + fr.tobytes())
        f.write(b'FRAME\n' + bytes(100))                                 # a partial frame behind the clip
    prep = DeviceImagePrep(synth.MEAN, synth.STD, to_rgb=True, size_divisor=32, img_scale=(W, H), device=dev)
    want_bgr = [R.yuv_to_bgr(fr, H, W, '420jpeg') for fr in frames]
    want = [prep.prep(torch.from_numpy(b).to(dev))[0].unsqueeze(0).clone() for b in want_bgr]
    fd = ClipFeeder(path, prep, workers=2, keep_frames=True)
    assert len(fd) == n and fd._y4m.dropped == 1
    for t in range(n):
        out = fd(t)
        assert torch.equal(out, want[t]), t
        assert np.array_equal(fd.frame(t).cpu().numpy(), want_bgr[t]), t
        assert fd.meta(t)['filename'] == '%s#%d' % (path, t) and fd.meta(t)['ori_shape'] == (H, W, 3)
    assert fd.native_y4m == fd.decodes == n and fd.fallback_decodes == 0 and fd.out_of_window == 0
    fd.close()
    fd = ClipFeeder(y4m.Y4mReader(path), prep, workers=2, ahead=2)       # a reader of the caller's; a shard that asks for its last frame first
    fd.set_range(1, 5)
    for t in (4, 1, 2, 3, 4):
        assert torch.equal(fd(t), want[t]), t
    assert fd._next <= 5 and 5 not in fd._pending and 5 not in fd._ready    # the read-ahead stopped at the end of the range
    assert fd.native_y4m == fd.decodes
    fd.close()
    assert fd._y4m._fd is not None                                       # the caller's reader stays open
    fd._y4m.close()


class _Sink(io.RawIOBase):
    """a writable binary stream that is not a file: keeps what it gets"""

    def __init__(self):
        super().__init__()
        self.parts = []

    def writable(self):
        return True

    def write(self, b):
        self.parts.append(bytes(b))
        return len(b)


@pytest.mark.parametrize('sampling', ['420jpeg', '420mpeg2', '444'])
def test_writer_writes_the_restatements_planes_in_submission_order(dev, tmp_path, sampling):
    H, W, n = 34, 50, 5
    imgs = [_smooth(H, W, 40 + t) for t in range(n)]
    want = y4m.y4m_header(y4m.make_info(W, H, (25, 1), sampling, 'full')) + b''.join(b'FRAME\n' + R.bgr_to_yuv(im, sampling, 'full', 'bt709').tobytes() for im in imgs)
    sink, path = _Sink(), str(tmp_path / 'sub' / 'out.y4m')
    for dst in (path, sink):
        w = y4m.Y4mWriter(dst, W, H, fps=(25, 1), sampling=sampling, range='full', matrix='bt709', device=dev, slots=2)   # more frames than slots
        for im in imgs:
            w.submit(torch.from_numpy(im).to(dev))
        w.close()
        w.close()
        assert (w.submitted, w.frames, w.bytes) == (n, n, len(want))
        with pytest.raises(ValueError):
            w.submit(torch.from_numpy(imgs[0]).to(dev))
    assert open(path, 'rb').read() == want
    assert b''.join(sink.parts) == want and not sink.closed
    with pytest.raises(ValueError):
        y4m.Y4mWriter(sink, W, H, sampling='422', device=dev)


@pytest.mark.parametrize('matrix, rng', sorted(ROUND_TRIP_BOUND))
def test_round_trip_through_a_file_stays_within_the_restatements_bound(dev, tmp_path, matrix, rng):
    H, W, n = 48, 64, 3
    imgs = [np.random.RandomState(70 + t).randint(0, 256, (H, W, 3), dtype=np.uint8) for t in range(n)]
    path = str(tmp_path / 'rt.y4m')
    w = y4m.Y4mWriter(path, W, H, sampling='444', range=rng, matrix=matrix, device=dev)
    for im in imgs:
        w.submit(torch.from_numpy(im).to(dev))
    w.close()
    r = y4m.Y4mReader(path)
    assert len(r) == n and r.info.sampling == '444' and r.info.range == rng
    slot = torch.empty(r.info.frame_bytes, dtype=torch.uint8).pin_memory()
    for t in range(n):
        r.readinto(t, slot)
        back = y4m.yuv_to_bgr(slot.to(dev), r.info, matrix).cpu().numpy().astype(np.int64)
        worst = int(np.abs(back - imgs[t]).max())
        print('%s %s frame %d: round trip differs by at most %d' % (matrix, rng, t, worst))
        assert worst <= ROUND_TRIP_BOUND[(matrix, rng)]
    r.close()


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


def test_write_overlays_video_beside_unchanged_jpegs(dev, tmp_path):
    from vps_amd.postprocess import TrackConverter, render_overlay, write_overlays
    H, W, n = 34, 50, 4
    frames = [torch.from_numpy(_smooth(H, W, t)).to(dev) for t in range(n)]
    twos = [_pan_2ch(H, W, t % 3) for t in range(n)]
    names = ['%04d_%04d_city_newImg8bit.png' % (7 + t // 2, t) for t in range(n)]      # videos 0007 and 0008
    plain = write_overlays(twos, frames, names, str(tmp_path / 'a'), _Colours(), 2, device=dev, alpha=100, quality=80)
    video = str(tmp_path / 'b' / 'ov.y4m')
    vids = []
    both = write_overlays(twos, frames, names, str(tmp_path / 'b'), _Colours(), 2, device=dev, alpha=100, quality=80, video=video,
                          video_sampling='420mpeg2', video_files=vids)
    assert vids == [str(tmp_path / 'b' / 'ov.0007.y4m'), str(tmp_path / 'b' / 'ov.0008.y4m')]          # the video's name goes into FILE
    assert [os.path.basename(p) for p in plain] == [os.path.basename(p) for p in both]
    for p, q in zip(plain, both):
        assert open(p, 'rb').read() == open(q, 'rb').read()                  # the JPEGs do not notice the option
    only = write_overlays(twos, frames, names, None, _Colours(), 2, device=dev, alpha=100, video=str(tmp_path / 'c.y4m'), video_sampling='420mpeg2')
    assert only == [str(tmp_path / 'c.0007.y4m'), str(tmp_path / 'c.0008.y4m')]
    one = write_overlays(twos[:2], frames[:2], names[:2], None, _Colours(), 2, device=dev, alpha=100, video=str(tmp_path / 'one.y4m'))
    assert one == [str(tmp_path / 'one.y4m')] and os.path.getsize(one[0]) > 2 * 34 * 50                  # a single video: FILE itself
    gen, conv = _Colours(), TrackConverter(dev)
    for v in range(2):                                                       # two videos of two frames, one stream each
        _, cols, _ = conv.convert_device(twos[2 * v:2 * v + 2], gen)
        r = y4m.Y4mReader(vids[v])
        assert len(r) == 2 and (r.info.W, r.info.H, r.info.sampling, r.info.range) == (W, H, '420mpeg2', 'limited')
        assert open(r.path, 'rb').read() == open(only[v], 'rb').read()
        slot = np.empty(r.info.frame_bytes, dtype=np.uint8)
        for j, col in enumerate(cols):
            rgb = render_overlay(frames[2 * v + j], col, 100)
            r.readinto(j, slot)
            assert np.array_equal(slot, y4m.bgr_to_yuv(rgb, '420mpeg2', order='rgb').cpu().numpy())
            assert np.array_equal(slot, R.bgr_to_yuv(rgb.cpu().numpy()[:, :, ::-1], '420mpeg2'))
        r.close()
