"""Optical-flow output: the flow of a frame as a colour image (JPEG / PNG) or a Middlebury .flo file.

The reference ships `readFlow`, `writeFlow` and `vis_flow` (mmdet/datasets/pipelines/flow_utils.py). Here the colour coding runs on the
device (`vps_flow_max_radius`, `vps_flow_colour`: csrc/flow_vis_ops.hip) and feeds the encoders of postprocess.py: `jpeg_encode_coef` +
the host Huffman coder, or `png_deflate`. The image is `vis_flow(flow.astype(np.float64))` of the reference, level for level, as RGB.
A .flo file is the raw field, byte for byte what `writeFlow` writes.

A flow is an `nhwc.FMap` (one image, two channels: what `FlowNet2.run` returns and the detector keeps in its ring), or a device fp32
tensor [H,W,2] (`pano_results['flow']` with `keep_flow`) or [1,2,H,W] (`compute_flow`). No CPU path for the colours."""
import os
import struct

import numpy as np
import torch

from . import hip, nhwc
from . import postprocess as pp

FLO_TAG = 202021.25                    # 'PIEH' read as a little-endian float32
FORMATS = ('jpg', 'png', 'flo', 'kitti')


def _flow_view(flow):
    """-> (tensor that owns the memory, ld, coff, H, W) of a device flow"""
    if isinstance(flow, nhwc.FMap):
        assert flow.N == 1 and flow.C == 2, 'a flow map is one image with two channels, got N %d C %d' % (flow.N, flow.C)
        return flow.t, int(flow.ld), int(flow.coff), int(flow.H), int(flow.W)
    if not (torch.is_tensor(flow) and flow.is_cuda):
        raise hip.VpsHipError('the flow colour kernels need a device flow (FMap or device tensor); there is no CPU path')
    assert flow.dtype == torch.float32, 'fp32 flow, got %s' % flow.dtype
    if flow.dim() == 4:
        assert flow.shape[0] == 1 and flow.shape[1] == 2, 'NCHW flow is [1,2,H,W], got %s' % (tuple(flow.shape),)
        flow = flow[0].permute(1, 2, 0)
    assert flow.dim() == 3 and flow.shape[2] == 2, 'flow is [H,W,2] or [1,2,H,W], got %s' % (tuple(flow.shape),)
    flow = flow.contiguous()
    return flow, 2, 0, int(flow.shape[0]), int(flow.shape[1])


def _max_radius(view, out=None):
    t, ld, coff, H, W = view
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=t.device)
    assert out.dtype == torch.float64 and out.is_cuda and out.numel() == 1
    hip.check(hip.load().vps_flow_max_radius(hip.ptr(t), ld, coff, H, W, hip.ptr(out), hip.stream_ptr()), 'vps_flow_max_radius')
    return out


def flow_max_radius(flow, out=None):
    """max sqrt(u*u + v*v) over the frame in fp64 (unknown flow, u or v > 1e9, counts as 0) -> device float64 [1], on the current stream,
    no sync (`vps_flow_max_radius`). `out`: caller-owned device float64 [1]."""
    return _max_radius(_flow_view(flow), out)


def max_rad_scalar(max_rad, device='cuda'):
    """a normaliser for `flow_colour` as the device float64 [1] the kernel reads. A float is uploaded from pageable host memory, which
    waits for the copy: make the scalar once per clip, not once per frame."""
    if torch.is_tensor(max_rad):
        assert max_rad.is_cuda and max_rad.dtype == torch.float64 and max_rad.numel() == 1, 'max_rad: a float or a device float64 scalar'
        return max_rad.reshape(1)
    return torch.tensor([float(max_rad)], dtype=torch.float64, device=device)


def flow_colour(flow, max_rad=None, out=None):
    """the reference's `vis_flow(flow.astype(np.float64))` -> device RGB uint8 [H,W,3], on the current stream (`vps_flow_colour`).
    max_rad None: the frame's own maximum radius normalises it (the reference); no sync. A device float64 scalar fixes the normaliser,
    so that the colours of a clip do not flicker from frame to frame, also without a sync; a float does the same but is uploaded on
    every call, which synchronises (`max_rad_scalar` makes the device scalar once). Pixels beyond the normaliser are darkened (x 0.75).
    `out`: caller-owned contiguous device uint8 [H,W,3]."""
    view = _flow_view(flow)
    t, ld, coff, H, W = view
    rad = _max_radius(view) if max_rad is None else max_rad_scalar(max_rad, t.device)
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=t.device)
    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (H, W, 3)
    hip.check(hip.load().vps_flow_colour(hip.ptr(t), ld, coff, H, W, hip.ptr(rad), hip.ptr(out), hip.stream_ptr()), 'vps_flow_colour')
    return out


# ------------------------------------------------------------------------------------------------------------------
# Middlebury .flo: float32 tag 202021.25, int32 width, int32 height, rows of interleaved float32 (u, v), little-endian
# ------------------------------------------------------------------------------------------------------------------
def _flo_header(H, W):
    return struct.pack('<fii', FLO_TAG, W, H)


def _host_hw2(flow):
    """any flow (host array [H,W,2], or what `_flow_view` takes) -> contiguous host float32 [H,W,2]; a device flow is downloaded"""
    if isinstance(flow, np.ndarray) or (torch.is_tensor(flow) and not flow.is_cuda):
        a = np.asarray(flow.numpy() if torch.is_tensor(flow) else flow)
        if a.ndim == 4:
            assert a.shape[0] == 1 and a.shape[1] == 2, a.shape
            a = a[0].transpose(1, 2, 0)
        assert a.ndim == 3 and a.shape[2] == 2, 'flow is [H,W,2] or [1,2,H,W], got %s' % (a.shape,)
        return np.ascontiguousarray(a, dtype='<f4')
    t, ld, coff, H, W = _flow_view(flow)
    return np.ascontiguousarray(t.view(H, W, ld)[:, :, coff:coff + 2].cpu().numpy(), dtype='<f4')


def flo_bytes(flow):
    """the bytes of the .flo file the reference's `writeFlow(name, flow)` writes (host array, or a device flow, which is downloaded)"""
    a = _host_hw2(flow)
    return _flo_header(a.shape[0], a.shape[1]) + a.tobytes()


def write_flo(flow, name):
    os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
    with open(name, 'wb') as f:
        f.write(flo_bytes(flow))
    return name


def read_flo(name):
    """the reference's `readFlow`: float32 [H,W,2]; a wrong tag or a short file raises"""
    with open(name, 'rb') as f:
        data = f.read()
    if len(data) < 12 or struct.unpack('<f', data[:4])[0] != FLO_TAG:
        raise ValueError('%s: not a .flo file (tag 202021.25 missing)' % name)
    W, H = struct.unpack('<ii', data[4:12])
    if W <= 0 or H <= 0 or len(data) != 12 + 8 * W * H:
        raise ValueError('%s: %d x %d flow needs %d bytes, the file has %d' % (name, W, H, 12 + 8 * W * H, len(data)))
    return np.frombuffer(data, dtype='<f4', offset=12).reshape(H, W, 2).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
class _FloSlot:
    def __init__(self):
        self.raw = None
        self.event = torch.cuda.Event()

    def fit(self, nelem):
        if self.raw is None or self.raw.numel() < nelem:
            self.raw = torch.empty(nelem, dtype=torch.float32).pin_memory()


class FlowWriter:
    """`DeviceJpegWriter`'s surface for flow fields: `submit(flow, name)` reads the flow on the CURRENT stream before it returns - the
    caller's buffer (a ring slot of the detector) may be overwritten right after - and leaves the rest to worker threads; it never
    synchronises the caller's stream and blocks only while every slot is busy.
      fmt 'jpg'  `flow_colour` into a fresh image, handed to a `DeviceJpegWriter` of its own (which keeps the image alive); `entropy`
                 ('host' or 'device') is that writer's: where the Huffman coding runs, the files are the same
      fmt 'png'  `flow_colour` into a fresh image, handed to a `DevicePngWriter` of its own
      fmt 'flo'  a stream-ordered copy of the two channels into one of `slots` pinned slots; a worker writes header + field
      fmt 'kitti' the KITTI devkit's 16-bit PNG (vps_amd/kittiflow.py), every pixel valid: `kitti_flow_encode` + `png_deflate_bpp` into one
                 of `slots` ring slots on the current stream; a worker copies the stream on its own copy stream and writes the file
    max_rad (jpg / png): None = each frame's own maximum (the reference); a float or device float64 scalar = one normaliser for all
    frames. Counters: `submitted`; after `close()`, which joins and re-raises a worker's exception: `written`, `bytes_written`."""

    def __init__(self, device='cuda', workers=2, slots=4, fmt='jpg', quality=90, max_rad=None, entropy='host', huffman='fixed'):
        if fmt not in FORMATS:
            raise ValueError('fmt is one of %s, got %r' % (FORMATS, fmt))
        pp.png_huffman(huffman)
        self.huffman = huffman                           # png / kitti: the Huffman code of the deflate stage ('fixed' | 'dynamic')
        self.device = torch.device(device)
        self.fmt = fmt
        self.max_rad = None if max_rad is None else max_rad_scalar(max_rad, self.device)
        self.images = self.pool = None
        if fmt == 'jpg':
            self.images = pp.DeviceJpegWriter(self.device, workers=workers, slots=slots, quality=quality, entropy=entropy)
        elif fmt == 'png':
            self.images = pp.DevicePngWriter(self.device, workers=workers, slots=slots, huffman=huffman)
        else:
            import queue
            import threading
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=workers)
            self.futures = []
            self.free = queue.Queue()
            self.local = threading.local()
            for _ in range(slots):
                self.free.put(_FloSlot() if fmt == 'flo' else pp._PngSlot(self.device))
        self.submitted = 0
        self.written = 0
        self.bytes_written = 0

    def _finish_flo(self, slot, name, H, W):
        try:
            slot.event.synchronize()                     # the worker waits, not the caller
            os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
            with open(name, 'wb') as f:
                f.write(_flo_header(H, W))
                f.write(memoryview(slot.raw[:H * W * 2].numpy()))
        finally:
            self.free.put(slot)
        return name

    def _finish_kitti(self, slot, name, H, W):
        from . import kittiflow
        try:
            slot.event.synchronize()                     # the worker waits, not the caller
            n = int(slot.size_host[0])
            if n < 0:
                raise hip.VpsHipError('vps_png_deflate_bpp: the stream did not fit its worst-case bound')
            if not hasattr(self.local, 'stream'):
                self.local.stream = torch.cuda.Stream(self.device)
            with torch.cuda.stream(self.local.stream):
                host = slot.staging(n)
                host.copy_(slot.out[:n], non_blocking=True)
                self.local.stream.synchronize()
                data = kittiflow.png16_container(host.numpy().tobytes(), H, W)
        finally:
            slot.image = None
            self.free.put(slot)
        os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
        with open(name, 'wb') as f:
            f.write(data)
        return name

    def _submit_kitti(self, flow, name, H, W):
        from . import kittiflow
        slot = self.free.get()                           # blocks only when every slot is in flight
        try:
            slot.fit(*kittiflow.png_encode_bound_bpp(H, 6 * W, 6))
            slot.image = kittiflow.kitti_flow_encode(flow)               # reads the flow on the current stream; alive until the worker is done
            kittiflow.png_deflate_bpp(slot.image, 6, slot.out, slot.ws, slot.size, huffman=self.huffman)
            slot.size_host.copy_(slot.size, non_blocking=True)
            slot.event.record()
        except BaseException:
            slot.image = None
            self.free.put(slot)
            raise
        self.futures.append(self.pool.submit(self._finish_kitti, slot, name, H, W))

    def submit(self, flow, name):
        view = _flow_view(flow)
        t, ld, coff, H, W = view
        if self.fmt == 'kitti':
            self._submit_kitti(flow, name, H, W)
        elif self.fmt != 'flo':
            rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=t.device)
            rad = _max_radius(view) if self.max_rad is None else self.max_rad
            hip.check(hip.load().vps_flow_colour(hip.ptr(t), ld, coff, H, W, hip.ptr(rad), hip.ptr(rgb), hip.stream_ptr()), 'vps_flow_colour')
            self.images.submit(rgb, name)
        else:
            slot = self.free.get()                       # blocks only when every slot is in flight
            try:
                slot.fit(H * W * 2)
                slot.raw[:H * W * 2].view(H, W, 2).copy_(t.view(H, W, ld)[:, :, coff:coff + 2], non_blocking=True)
                slot.event.record()
            except BaseException:
                self.free.put(slot)
                raise
            self.futures.append(self.pool.submit(self._finish_flo, slot, name, H, W))
        self.submitted += 1

    def close(self):
        if self.images is not None:
            names = self.images.close()
        else:
            futures, self.futures = self.futures, []
            try:
                names = [f.result() for f in futures]    # re-raises a worker's exception
            finally:
                self.pool.shutdown()
        self.written += len(names)
        self.bytes_written += sum(os.path.getsize(n) for n in names)
        return names


def flow_name(save_folder, name, fmt='jpg'):
    """output file of the flow of an input image name: DIR/<name without its extension>.<fmt>; a KITTI flow file is a .png"""
    return os.path.join(save_folder, os.path.splitext(os.path.basename(name))[0] + '.' + ('png' if fmt == 'kitti' else fmt))


def write_flows(flows, names, out_dir, device='cuda', fmt='jpg', quality=90, max_rad=None, writer=None, entropy='host'):
    """a file per frame, `out_dir/<name>.<fmt>`, through a `FlowWriter` (the caller's, or one made and closed here). `flows`: device
    flows in the order of `names`. Returns the file names."""
    assert len(flows) == len(names)
    own = writer is None
    writer = FlowWriter(device, fmt=fmt, quality=quality, max_rad=max_rad, entropy=entropy) if own else writer
    out = []
    for flow, name in zip(flows, names):
        out.append(flow_name(out_dir, name, writer.fmt))
        writer.submit(flow, out[-1])
    if own:
        writer.close()
    return out
