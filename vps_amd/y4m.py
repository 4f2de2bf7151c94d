"""Y4M (YUV4MPEG2) video in and out: the uncompressed container every video tool reads and writes
(`ffmpeg -i in.mp4 -f yuv4mpegpipe in.y4m`, and back), 8-bit planar frames, no codec library.

The host only parses the two kinds of header line (`csrc/y4m_host.cpp`: `vps_y4m_info`, `vps_y4m_frame_header`,
`vps_y4m_write_header`) and moves bytes; chroma resampling at the declared siting and the colour matrix run on the device
(`csrc/yuv_ops.hip`: `vps_yuv_to_bgr`, `vps_bgr_to_yuv`; integer arithmetic stated in include/vps_hip.h, restated in NumPy by
tests/y4m_restate.py and compared for equality). Y4M has no tag for the colour matrix, so it is a call parameter (default bt601).

    Y4mReader(path)            seekable file -> frame index; `readinto(t, pinned_slot)` fills a slot with frame t's planes
    yuv_to_bgr(planar, info)   device planar frame -> device BGR uint8 [H,W,3]   (what `ClipFeeder('clip.y4m', prep)` does per frame)
    bgr_to_yuv(bgr, ...)       device BGR (or RGB) uint8 [H,W,3] -> device planar frame
    Y4mWriter(dst, W, H, ...)  `submit(device frame)` -> one stream, frames in submission order, written by one thread

There is no host path for the conversions: without a device they raise, like every kernel of the package."""
import ctypes
import os
import queue
import threading

import torch

from . import hip

SAMPLINGS = ('420jpeg', '420mpeg2', '422', '444', 'mono')           # VPS_Y4M_*
RANGES = ('limited', 'full')                                        # VPS_YUV_LIMITED / _FULL
MATRICES = ('bt601', 'bt709')                                       # VPS_YUV_BT601 / _BT709
ENCODABLE = ('444', '420jpeg', '420mpeg2')
HEADER_MAX, FRAME_LINE_MAX = 256, 80

REFUSALS = {
    1: 'null or negative argument', 2: 'not a YUV4MPEG2 stream (bad magic)', 3: 'no newline within the first 256 bytes (truncated header)',
    4: 'malformed number or ratio in a header tag', 5: 'W or H missing', 6: 'W or H not positive', 7: 'frame size too large (W*H beyond 2^31)',
    8: 'interlaced stream (It / Ib / Im)', 9: '420paldv chroma siting is not supported', 10: 'more than 8 bits per sample',
    11: '444alpha is not supported', 12: 'unknown C (colour space) tag', 13: 'unknown XCOLORRANGE', 14: 'unknown I (interlacing) tag',
    20: 'not a FRAME line', 21: 'no newline within the 80 bytes of a FRAME line (truncated)',
    30: 'header field out of range', 31: 'capacity too small for the header',
}


def _refuse(code, what):
    return ValueError('%s: %s (code %d)' % (what, REFUSALS.get(-1000 - code, 'refused'), code))


def _index(names, v, what):
    if v not in names:
        raise ValueError('%s is one of %s, got %r' % (what, ', '.join(names), v))
    return names.index(v)


class Y4mInfo:
    """a stream header: W, H, chroma plane size CW x CH (rounded up for odd sizes; 0 for mono), sampling (one of SAMPLINGS),
    range ('limited' / 'full'), fps and aspect as (num, den) with (0, 0) = absent, progressive (the Ip tag), header_bytes,
    frame_bytes (payload of one frame, without its FRAME line)"""
    __slots__ = ('W', 'H', 'CW', 'CH', 'sampling', 'range', 'fps', 'aspect', 'progressive', 'header_bytes', 'frame_bytes')

    def __init__(self, d):
        self.W, self.H, self.CW, self.CH = d.W, d.H, d.CW, d.CH
        self.sampling, self.range = SAMPLINGS[d.sampling], RANGES[d.range]
        self.fps, self.aspect = (d.fps_num, d.fps_den), (d.aspect_num, d.aspect_den)
        self.progressive = bool(d.interlace)
        self.header_bytes, self.frame_bytes = d.header_bytes, d.frame_bytes

    def desc(self):
        d = hip.Y4mDesc()
        d.W, d.H, d.CW, d.CH = self.W, self.H, self.CW, self.CH
        d.sampling, d.range = SAMPLINGS.index(self.sampling), RANGES.index(self.range)
        (d.fps_num, d.fps_den), (d.aspect_num, d.aspect_den) = self.fps, self.aspect
        d.interlace, d.header_bytes, d.frame_bytes = int(self.progressive), self.header_bytes, self.frame_bytes
        return d

    def __eq__(self, o):
        return isinstance(o, Y4mInfo) and all(getattr(self, k) == getattr(o, k) for k in self.__slots__)

    def __repr__(self):
        return 'Y4mInfo(%s)' % ', '.join('%s=%r' % (k, getattr(self, k)) for k in self.__slots__)


def _cbuf(data):
    return (ctypes.c_char * len(data)).from_buffer(data) if isinstance(data, (bytearray, memoryview)) and not getattr(data, 'readonly', False) \
        else (ctypes.c_char * len(data)).from_buffer_copy(bytes(data))


def y4m_info(data):
    """the stream header at the start of `data` (bytes-like; the first 256 bytes suffice) -> Y4mInfo; ValueError names the refusal"""
    d = hip.Y4mDesc()
    st = hip.load_host().vps_y4m_info(_cbuf(data), len(data), ctypes.byref(d))
    if st:
        raise _refuse(st, 'y4m_info')
    return Y4mInfo(d)


def frame_header(data):
    """length of the `FRAME[ params]\\n` line at the start of `data`; ValueError names the refusal"""
    n = ctypes.c_int32(0)
    st = hip.load_host().vps_y4m_frame_header(_cbuf(data), len(data), ctypes.byref(n))
    if st:
        raise _refuse(st, 'y4m frame header')
    return n.value


def make_info(W, H, fps=(30, 1), sampling='420jpeg', range='limited', aspect=(0, 0), progressive=True):
    """the Y4mInfo of a stream to be written (plane sizes and byte counts filled in by the library)"""
    d = hip.Y4mDesc()
    d.W, d.H, d.sampling, d.range = int(W), int(H), _index(SAMPLINGS, sampling, 'sampling'), _index(RANGES, range, 'range')
    (d.fps_num, d.fps_den), (d.aspect_num, d.aspect_den), d.interlace = (int(v) for v in fps), (int(v) for v in aspect), int(bool(progressive))
    return y4m_info(_header_of(d))


def _header_of(d):
    out = (ctypes.c_char * HEADER_MAX)()
    n = ctypes.c_int32(0)
    st = hip.load_host().vps_y4m_write_header(ctypes.byref(d), out, HEADER_MAX, ctypes.byref(n))
    if st:
        raise _refuse(st, 'y4m header')
    return out.raw[:n.value]


def y4m_header(info):
    """the header line `vps_y4m_write_header` writes for a Y4mInfo: what `y4m_info` parses back to the same values"""
    return _header_of(info.desc())


def yuv_to_bgr(planar, info, matrix='bt601', out=None):
    """device uint8 planar frame (Y, Cb, Cr as they lie in the file, at least info.frame_bytes, 4-byte aligned storage) -> device BGR
    uint8 [H,W,3] on the current stream, no sync (`vps_yuv_to_bgr`): chroma up-sampled at the siting `info.sampling` declares,
    `matrix` 'bt601' / 'bt709' at `info.range`"""
    assert torch.is_tensor(planar) and planar.dtype == torch.uint8 and planar.is_contiguous(), 'a contiguous uint8 tensor holding the planes'
    m = _index(MATRICES, matrix, 'matrix')
    if out is None:
        out = torch.empty(info.H, info.W, 3, dtype=torch.uint8, device=planar.device)
    hip.check(hip.load().vps_yuv_to_bgr(hip.ptr(planar), planar.numel(), info.H, info.W, SAMPLINGS.index(info.sampling), RANGES.index(info.range), m,
                                        hip.ptr(out), out.numel(), hip.stream_ptr()), 'vps_yuv_to_bgr')
    return out


def planar_bytes(H, W, sampling):
    """bytes of one planar frame of that size and sampling"""
    cw, ch = {'420jpeg': ((W + 1) // 2, (H + 1) // 2), '420mpeg2': ((W + 1) // 2, (H + 1) // 2), '422': ((W + 1) // 2, H), '444': (W, H),
              'mono': (0, 0)}[sampling]
    return H * W + 2 * cw * ch


def bgr_to_yuv(bgr, sampling='420jpeg', range='limited', matrix='bt601', out=None, order='bgr'):
    """device uint8 [H,W,3] (unit-stride pixels, rows may be strided) -> device uint8 planar frame (Y, then Cb, then Cr) of `sampling`
    ('444', '420jpeg', '420mpeg2') on the current stream, no sync (`vps_bgr_to_yuv`, one launch). `order`: 'bgr' (a decoded frame) or
    'rgb' (what `render_overlay` returns). `out`: caller-owned uint8 buffer of at least `planar_bytes(H, W, sampling)`."""
    assert torch.is_tensor(bgr) and bgr.dtype == torch.uint8 and bgr.dim() == 3 and bgr.shape[2] == 3, 'uint8 [H,W,3]'
    if sampling not in ENCODABLE:
        raise ValueError('bgr_to_yuv writes %s, got %r' % (', '.join(ENCODABLE), sampling))
    r, m, o = _index(RANGES, range, 'range'), _index(MATRICES, matrix, 'matrix'), _index(('bgr', 'rgb'), order, 'order')
    H, W = int(bgr.shape[0]), int(bgr.shape[1])
    if not (bgr.stride(2) == 1 and bgr.stride(1) == 3 and (H == 1 or bgr.stride(0) >= 3 * W)):
        bgr = bgr.contiguous()
    stride = int(bgr.stride(0)) if H > 1 else 3 * W
    if out is None:
        out = torch.empty(planar_bytes(H, W, sampling), dtype=torch.uint8, device=bgr.device)
    assert out.dtype == torch.uint8 and out.is_contiguous()
    hip.check(hip.load().vps_bgr_to_yuv(hip.ptr(bgr), H, W, stride, o, SAMPLINGS.index(sampling), r, m, hip.ptr(out), out.numel(),
                                        hip.stream_ptr()), 'vps_bgr_to_yuv')
    return out


class Y4mReader:
    """A seekable .y4m file as a list of frames. The FRAME lines are walked once at open (`len()` = complete frames; a trailing partial
    frame is dropped and counted in `dropped`); `readinto(t, slot)` checks frame t's FRAME line again and reads its planes straight
    into `slot` (a uint8 CPU tensor - a pinned staging slot - or any writable buffer of at least `info.frame_bytes`). Reads are
    positional (`os.pread`), so decode threads share one reader."""

    def __init__(self, path):
        self.path = str(path)
        self._fd = None
        self._fd = os.open(self.path, os.O_RDONLY)
        try:
            size = os.fstat(self._fd).st_size
            self.info = y4m_info(os.pread(self._fd, HEADER_MAX, 0))
            self._lines, self.dropped = [], 0                       # (offset of the FRAME line, its length)
            pos, fb = self.info.header_bytes, self.info.frame_bytes
            while pos < size:
                line = os.pread(self._fd, FRAME_LINE_MAX, pos)
                try:
                    n = frame_header(line)
                except ValueError as e:
                    if pos + len(line) >= size and len(line) < FRAME_LINE_MAX and b'FRAME'.startswith(line[:5]) and b'\n' not in line:
                        self.dropped += 1                            # the file ends inside a FRAME line
                        break
                    raise ValueError('%s: frame %d at byte %d: %s' % (self.path, len(self._lines), pos, e))
                if pos + n + fb > size:
                    self.dropped += 1
                    break
                self._lines.append((pos, n))
                pos += n + fb
        except BaseException:
            os.close(self._fd)
            self._fd = None
            raise

    def __len__(self):
        return len(self._lines)

    def readinto(self, t, slot):
        pos, n = self._lines[t]
        if frame_header(os.pread(self._fd, n, pos)) != n:
            raise ValueError('%s: the FRAME line of frame %d changed since the file was opened' % (self.path, t))
        fb = self.info.frame_bytes
        mv = memoryview(slot.numpy() if torch.is_tensor(slot) else slot).cast('B')
        assert len(mv) >= fb, 'slot of %d bytes, frame of %d' % (len(mv), fb)
        got = 0
        while got < fb:
            k = os.preadv(self._fd, [mv[got:fb]], pos + n + got)
            if k <= 0:
                raise IOError('%s: frame %d is cut short (file truncated since it was opened)' % (self.path, t))
            got += k
        return fb

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        self.close()


class _Y4mSlot:
    def __init__(self, nbytes, device):
        self.planar = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.event = torch.cuda.Event()
        self.image = None


class Y4mWriter:
    """`DeviceJpegWriter`'s shape for ONE video stream: `submit(device BGR uint8 [H,W,3])` enqueues `bgr_to_yuv` on the CURRENT stream into
    one of `slots` ring slots (planar buffer on the device, pinned staging of the same size, an event), records the event and returns -
    it never synchronises the caller's stream and blocks only while every slot is busy. ONE writer thread waits for each slot's event
    in submission order, downloads the planes on its own copy stream and writes `FRAME\\n` + payload, so the stream's frames are in
    submission order. `dst`: a path, or any writable binary stream (a pipe to a player or an encoder; it is flushed, not closed).
    `order='rgb'` takes `render_overlay`'s images. `close()` drains, re-raises the writer thread's exception and may be called twice.
    Counters: `submitted`, `frames` (written), `bytes` (written, headers included)."""

    def __init__(self, dst, W, H, fps=(30, 1), sampling='420jpeg', range='limited', matrix='bt601', device='cuda', slots=4, order='bgr'):
        if sampling not in ENCODABLE:
            raise ValueError('Y4mWriter writes %s, got %r' % (', '.join(ENCODABLE), sampling))
        self.info = make_info(W, H, fps, sampling, range)
        self.matrix, self.order = MATRICES[_index(MATRICES, matrix, 'matrix')], ('bgr', 'rgb')[_index(('bgr', 'rgb'), order, 'order')]
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise hip.VpsHipError('Y4mWriter converts on the device; there is no host path')
        self._own = isinstance(dst, (str, bytes, os.PathLike))
        if self._own:
            os.makedirs(os.path.dirname(os.fspath(dst)) or '.', exist_ok=True)
        self._f = open(dst, 'wb') if self._own else dst
        self.submitted = self.frames = self.bytes = 0
        header = y4m_header(self.info)
        self._f.write(header)
        self.bytes += len(header)
        self._free, self._work = queue.Queue(), queue.Queue()
        for _ in [None] * int(slots):                                # (`range` is the colour range here)
            self._free.put(_Y4mSlot(self.info.frame_bytes, self.device))
        self._error = None
        self._closed = False
        self._thread = threading.Thread(target=self._run, name='Y4mWriter', daemon=True)
        self._thread.start()

    def _run(self):
        stream = torch.cuda.Stream(self.device)
        while True:
            slot = self._work.get()
            if slot is None:
                return
            try:
                if self._error is None:                              # after a failure the ring is still drained: submit() must not block for ever
                    slot.event.synchronize()                         # the writer waits, not the caller
                    with torch.cuda.stream(stream):
                        slot.host.copy_(slot.planar, non_blocking=True)
                    stream.synchronize()
                    self._f.write(b'FRAME\n')
                    self._f.write(memoryview(slot.host.numpy()))
                    self.frames += 1
                    self.bytes += 6 + slot.host.numel()
            except BaseException as e:                               # kept for close() / the next submit()
                self._error = e
            finally:
                slot.image = None
                self._free.put(slot)

    def submit(self, image):
        if self._closed:
            raise ValueError('Y4mWriter.submit after close()')
        if self._error is not None:
            raise self._error
        if not (torch.is_tensor(image) and image.is_cuda):
            image = torch.as_tensor(image).to(self.device)
        assert image.dtype == torch.uint8 and tuple(image.shape) == (self.info.H, self.info.W, 3), \
            'uint8 [%d,%d,3], got %s %s' % (self.info.H, self.info.W, image.dtype, tuple(image.shape))
        slot = self._free.get()                                      # blocks only when every slot is in flight
        try:
            slot.image = image                                       # alive until the conversion has read it
            bgr_to_yuv(image, self.info.sampling, self.info.range, self.matrix, slot.planar, self.order)
            slot.event.record()
        except BaseException:
            slot.image = None
            self._free.put(slot)
            raise
        self.submitted += 1
        self._work.put(slot)

    def close(self):
        if self._closed:
            return
        self._closed = True
        self._work.put(None)
        self._thread.join()
        try:
            if self._own:
                self._f.close()
            else:
                self._f.flush()
        finally:
            if self._error is not None:
                raise self._error
