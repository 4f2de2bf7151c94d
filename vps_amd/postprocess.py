"""Device-side panoptic post-processing behind the reference's own method signature.

`PanopticUnifier.get_unified_pan_result(segs, pans, cls_inds, obj_ids, stuff_area_limit, names)` takes what
`tools/test_vpq.py:51-63` collects per frame (`fcn_outputs`, `panoptic_outputs`, `panoptic_cls_inds`,
`panoptic_det_obj_ids`) and returns what `tools/dataset/cityscapes_vps.py:162-226` returns — `{name: uint8 [H,W,3]}` with
channels (pan_seg, pan_ins, pan_obj) — but the maps stay on the GPU until the 3-channel result is ready: one histogram pass,
the reference's per-instance decisions on one wavefront, one table-lookup pass (`vps_unify_*`, `csrc/post_ops.hip`).
The only host work is the object-id de-duplication (`:170-181`, <= 100 integers, and stateful across frames).
No CPU path: maps must be (or are uploaded to) device tensors and the HIP library must load."""
import json
import os
from collections import Counter

import numpy as np
import torch

from . import hip


def dedup_obj_ids(obj_id, max_oid):
    """cityscapes_vps.py:170-181: of every repeated object id, the LAST occurrence keeps it and the others get fresh ids
    max_oid, max_oid+1, ... handed out from the end of the list backwards; repeated values are treated in ascending order.
    Returns (ids, max_oid)."""
    orig = [int(v) for v in obj_id]
    work = orig[::-1]                                    # the reference edits a reversed copy
    counts = Counter(orig)
    for red in sorted(v for v, c in counts.items() if c > 1):
        fresh = [red] + [max_oid + i for i in range(counts[red] - 1)]
        max_oid += counts[red] - 1
        where = [i for i, v in enumerate(work) if v == red]
        if len(where) != len(fresh):                     # a fresh id collided with an existing one: numpy raises here too
            raise ValueError('NumPy boolean array indexing assignment cannot assign %d input values to the %d output values '
                             'where the mask is true' % (len(fresh), len(where)))
        for i, v in zip(where, fresh):
            work[i] = v
    return np.asarray(work[::-1], dtype=np.int64), max_oid


# class tables of the datasets the reference's post-processing is configured for: `config.dataset.num_seg_classes / num_classes`
# (stuff classes = ids 0 .. num_seg_classes - num_classes - 1 of the semantic map, things behind them) and the categories the
# evaluation leaves out of the PQ average. tools/dataset/cityscapes_vps.py + configs/cityscapes/test_cityscapes_1gpu.yaml:7-8;
# tools/dataset/viper.py:93-130 (23 / 11: ids 0..12 stuff, 13..22 things + the void instance) and :74-76 (`#### exclude
# "mobilebarrier"`, category 11)
DATASETS = {
    'cityscapes_vps': dict(num_seg_classes=19, num_classes=9, pq_exclude=()),
    'viper': dict(num_seg_classes=23, num_classes=11, pq_exclude=(11,)),
}


class PanopticUnifier:
    def __init__(self, device='cuda', num_seg_classes=19, num_classes=9):
        self.device = torch.device(device)
        self.id_last_stuff = num_seg_classes - num_classes          # config.dataset.* (cityscapes_vps.py:186)
        self.hist = torch.empty(256 * 256, dtype=torch.int32, device=self.device)
        self.pan_count = torch.empty(256, dtype=torch.int32, device=self.device)
        self.tables = torch.empty(3 * 256, dtype=torch.uint8, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _map(self, m):
        t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
        t = t.to(self.device)
        if t.dtype != torch.uint8:
            t = t.to(torch.uint8)                        # test_vpq.py:53,56 `.astype(np.uint8)`
        return t.contiguous()

    def unify_frame(self, seg, pan, cls_ind, obj_id, stuff_area_limit=4 * 64 * 64):
        """one frame, object ids already de-duplicated. Returns a device uint8 tensor [H,W,3]."""
        lib = hip.load()
        seg, pan = self._map(seg), self._map(pan)
        assert seg.shape == pan.shape and pan.dim() == 2
        npix = pan.numel()
        cls_t = torch.as_tensor(np.asarray(cls_ind.cpu() if torch.is_tensor(cls_ind) else cls_ind), dtype=torch.int32).to(self.device)
        obj_t = None
        if obj_id is not None:
            obj_t = torch.as_tensor(np.asarray(obj_id), dtype=torch.int32).to(self.device)
        out = torch.empty(pan.shape[0], pan.shape[1], 3, dtype=torch.uint8, device=self.device)
        s = hip.stream_ptr()
        hip.check(lib.vps_unify_hist(hip.ptr(pan), hip.ptr(seg), npix, self.id_last_stuff, hip.ptr(self.hist), hip.ptr(self.pan_count), s),
                  'vps_unify_hist')
        hip.check(lib.vps_unify_tables(hip.ptr(self.hist), hip.ptr(self.pan_count), hip.ptr(cls_t) if cls_t.numel() else None,
                                       cls_t.numel(), hip.ptr(obj_t) if (obj_t is not None and obj_t.numel()) else None,
                                       0 if obj_t is None else obj_t.numel(), self.id_last_stuff, int(stuff_area_limit),
                                       hip.ptr(self.tables), hip.ptr(self.status), s), 'vps_unify_tables')
        hip.check(lib.vps_unify_write(hip.ptr(pan), npix, hip.ptr(self.tables), hip.ptr(out), s), 'vps_unify_write')
        self._keep = (seg, pan, cls_t, obj_t)            # alive until the stream has consumed them
        return out

    def get_unified_pan_result(self, segs, pans, cls_inds, obj_ids=None, stuff_area_limit=4 * 64 * 64, names=None):
        if obj_ids is None:
            obj_ids = [None for _ in range(len(cls_inds))]
        results, outs = {}, []
        max_oid = 100
        for seg, pan, cls_ind, obj_id, name in zip(segs, pans, cls_inds, obj_ids, names):
            if obj_id is not None:
                obj_id = obj_id.cpu().numpy() if torch.is_tensor(obj_id) else np.asarray(obj_id)
                obj_id, max_oid = dedup_obj_ids(obj_id, max_oid)
            out = self.unify_frame(seg, pan, cls_ind, obj_id, stuff_area_limit)
            st = int(self.status.item())                 # also orders the reuse of hist / tables by the next frame
            if st:
                raise IndexError('instance id without %s entry (cityscapes_vps.py:%s)' % (('cls_ind', '197') if st == 1 else ('obj_id', '201')))
            outs.append((name, out))
        for name, out in outs:
            results[name] = out.cpu().numpy()
        return results


def _rgb2id(color):
    return int(color[0]) + 256 * int(color[1]) + 256 * 256 * int(color[2])        # panopticapi.utils.rgb2id for one colour


class TrackConverter:
    """Device-side body of `converter_2ch_track_core(proc_id, pan_2ch_set, color_generator)` (cityscapes_vps.py:97-159): same
    result — (annotations, pan_all) — from one statistics pass and one painting pass per frame instead of a boolean mask per
    segment. Colours come from the caller's generator exactly as in the reference (one call per stuff segment and frame, one
    per new (class, object id) pair and clip), in ascending order of 1000*seg + obj."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        self.stats = torch.empty(65536 * 5, dtype=torch.int32, device=self.device)
        self.lut = torch.zeros(65536 * 3, dtype=torch.uint8, device=self.device)

    def convert(self, pan_2ch_set, color_generator):
        annotations, pan_dev, _ = self.convert_device(pan_2ch_set, color_generator)
        return annotations, [p.cpu().numpy() for p in pan_dev]

    def convert_device(self, pan_2ch_set, color_generator):
        """as `convert`, but the painted maps stay on the device: (annotations, pan_pred device tensors, pan_2ch device tensors)"""
        lib = hip.load()
        annotations, pan_all, two_all = [], [], []
        inst2color = {}
        self.frame_stats = []                                   # per frame (keys, rows) of the present segments, for tubes.TubeCollector
        for pan_2ch in pan_2ch_set:
            t = torch.from_numpy(np.ascontiguousarray(pan_2ch)) if isinstance(pan_2ch, np.ndarray) else pan_2ch
            t = t.to(self.device).contiguous()
            assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
            H, W = int(t.shape[0]), int(t.shape[1])
            hip.check(lib.vps_segment_stats(hip.ptr(t), H, W, hip.ptr(self.stats), hip.stream_ptr()), 'vps_segment_stats')
            st = self.stats.view(65536, 5)
            keys = torch.nonzero(st[:, 0] > 0).flatten()
            rows = st[keys].cpu().numpy()                       # a few dozen present segments
            keys = keys.cpu().numpy()
            self.frame_stats.append((keys, rows))
            seg, obj = keys >> 8, keys & 255
            order = np.argsort(1000 * seg + obj, kind='stable')  # np.unique(1000*seg + obj) ascending
            lut = np.zeros((65536, 3), dtype=np.uint8)
            segm_info, painted = {}, {}
            for i in order:
                sem, ob = int(seg[i]), int(obj[i])
                if sem == 255:
                    continue
                el = 1000 * sem + ob
                if ob > 0:
                    if el in inst2color:
                        color = inst2color[el]
                    else:
                        color = color_generator.get_color(sem)
                        inst2color[el] = color
                else:
                    color = color_generator.get_color(sem)
                lut[keys[i]] = color
                cnt, x0, y0, x1, y1 = (int(v) for v in rows[i])
                sid = _rgb2id(color)
                segm_info[sid] = {"category_id": sem, "iscrowd": 0, "id": sid, "bbox": [x0, y0, x1 - x0, y1 - y0], "area": cnt}
                painted[sid] = painted.get(sid, 0) + cnt    # areas are re-counted per COLOUR (two segments may share one)
            for sid, area in painted.items():
                if sid != 0:
                    segm_info[sid]["area"] = area
            self.lut.copy_(torch.from_numpy(lut.reshape(-1)), non_blocking=False)
            out = torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
            hip.check(lib.vps_segment_paint(hip.ptr(t), H * W, hip.ptr(self.lut), hip.ptr(out), hip.stream_ptr()), 'vps_segment_paint')
            pan_all.append(out)
            two_all.append(t)
            annotations.append({"segments_info": [v for k, v in segm_info.items()]})
        return annotations, pan_all, two_all


# ------------------------------------------------------------------------------------------------------------------
# Output side of tools/test_vpq.py:194-198 — `inference_panoptic_video` (cityscapes_vps.py:27-94): sample the labelled frames,
# convert the 2-channel maps (TrackConverter above), write pan_2ch / pan_pred PNGs and pred.json.
# ------------------------------------------------------------------------------------------------------------------
class AsyncPngWriter:
    """PNG encoding off the critical path: a small thread pool (zlib releases the GIL) fed with host arrays; `close()` joins.
    The reference encodes inside multiprocessing pools after ALL frames are done (base_dataset.py:434-447); here frame t is
    encoded while frame t+1 runs on the GPU. Same file bytes' CONTENT (PIL `Image.fromarray(image).save(name)`)."""

    def __init__(self, workers=4):
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.futures = []

    @staticmethod
    def _save(image, name, palette=None):
        from PIL import Image
        os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
        im = Image.fromarray(image)
        if palette is not None:
            im.putpalette(np.asarray(palette, dtype=np.uint8).reshape(-1))
        im.save(name)
        return name

    def submit(self, image, name):
        self.futures.append(self.pool.submit(self._save, np.ascontiguousarray(image), name))

    def close(self):
        names = [f.result() for f in self.futures]       # re-raises a worker's exception
        self.pool.shutdown()
        self.futures = []
        return names


def _png_view(t):
    """device uint8 [H,W] / [H,W,3] with unit-stride pixels (rows may be strided) -> (tensor, H, W, C, row stride in bytes)"""
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8, 'png_deflate takes a device uint8 tensor'
    assert t.dim() == 2 or (t.dim() == 3 and t.shape[2] in (1, 3)), 'shape [H,W] or [H,W,3], got %s' % (tuple(t.shape),)
    C = 1 if t.dim() == 2 else int(t.shape[2])
    H, W = int(t.shape[0]), int(t.shape[1])
    dense = (t.stride(1) == 1) if t.dim() == 2 else (t.stride(2) == 1 and t.stride(1) == C)
    if not (dense and t.stride(0) >= W * C):
        t = t.contiguous()
    return t, H, W, C, int(t.stride(0)) if H > 1 else W * C


def png_encode_bound(H, W, channels):
    """(worst-case stream bytes, workspace bytes) of `vps_png_deflate` for one image size"""
    import ctypes
    cap, wsb = ctypes.c_int64(0), ctypes.c_int64(0)
    hip.check(hip.load().vps_png_encode_bound(H, W, channels, ctypes.byref(cap), ctypes.byref(wsb)), 'vps_png_encode_bound')
    return cap.value, wsb.value


PNG_HUFFMAN = {'fixed': 0, 'dynamic': 1}


def png_huffman(huffman):
    """'fixed' | 'dynamic' -> the `huffman` argument of `vps_png_deflate_h`"""
    if huffman not in PNG_HUFFMAN:
        raise ValueError("huffman must be 'fixed' or 'dynamic', got %r" % (huffman,))
    return PNG_HUFFMAN[huffman]


def png_deflate(t, out=None, ws=None, size=None, huffman='fixed'):
    """Filter + deflate a device uint8 [H,W,3] / [H,W] map on the device (`vps_png_deflate_h`: literals and distance-1 runs, DESIGN.md 6
    row 2b) on the current stream, no sync. huffman 'fixed' = every segment in the fixed Huffman code (the bytes of `vps_png_deflate`);
    'dynamic' = a segment in a code of its own where that is shorter (dense images). Returns (device uint8 buffer, device int64 [1]
    size): the zlib stream is buffer[:size]; size -1 = `out` was too small. `out` / `ws` / `size`: caller-owned buffers (default: fresh
    worst-case ones; the bound is the same for both codes)."""
    huffman = png_huffman(huffman)
    t, H, W, C, stride = _png_view(t)
    if out is None or ws is None:
        cap, wsb = png_encode_bound(H, W, C)
        out = torch.empty(cap, dtype=torch.uint8, device=t.device) if out is None else out
        ws = torch.empty(wsb, dtype=torch.uint8, device=t.device) if ws is None else ws
    if size is None:
        size = torch.empty(1, dtype=torch.int64, device=t.device)
    hip.check(hip.load().vps_png_deflate_h(hip.ptr(t), H, W, C, stride, hip.ptr(out), out.numel(), hip.ptr(size), hip.ptr(ws), ws.numel(),
                                           hip.stream_ptr(), huffman), 'vps_png_deflate_h')
    return out, size


def png_container(stream_bytes, H, W, channels, palette=None):
    """the PNG file around one zlib stream: signature, IHDR (8 bit, grey or RGB, no interlace), one IDAT, IEND. The CRCs are zlib.crc32
    on the host: the compressed data is ~100 KB. `palette` (uint8 [256][3], single-channel images only): colour type 3 with a PLTE
    chunk in front of the same IDAT stream - the file `Image.putpalette(palette)` + `save` gives in content."""
    import struct
    import zlib

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    plte = b''
    ctype = {1: 0, 3: 2}[channels]
    if palette is not None:
        pal = np.ascontiguousarray(np.asarray(palette, dtype=np.uint8).reshape(-1))
        assert channels == 1 and pal.size == 768, 'a palette is 256 x 3 uint8 and goes with a single-channel image'
        ctype, plte = 3, chunk(b'PLTE', pal.tobytes())
    ihdr = struct.pack('>IIBBBBB', W, H, 8, ctype, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) + plte + chunk(b'IDAT', bytes(stream_bytes)) + chunk(b'IEND', b'')


class _PngSlot:
    def __init__(self, device):
        self.device = device
        self.cap = self.wsb = 0
        self.out = self.ws = self.host = self.image = None
        self.size = torch.empty(1, dtype=torch.int64, device=device)
        self.size_host = torch.empty(1, dtype=torch.int64).pin_memory()
        self.event = torch.cuda.Event()

    def fit(self, cap, wsb):
        if cap > self.cap:
            self.out, self.cap = torch.empty(cap, dtype=torch.uint8, device=self.device), cap
        if wsb > self.wsb:
            self.ws, self.wsb = torch.empty(wsb, dtype=torch.uint8, device=self.device), wsb

    def staging(self, n):
        if self.host is None or self.host.numel() < n:
            self.host = torch.empty(max(1 << 16, 1 << (n - 1).bit_length()), dtype=torch.uint8).pin_memory()
        return self.host[:n]


class DevicePngWriter:
    """`AsyncPngWriter`'s surface with the encoding on the device: `submit(device tensor, name)` enqueues `png_deflate` on the CURRENT
    stream into one of `slots` ring slots (output + workspace, sized by `vps_png_encode_bound` from the first image and grown if a
    larger one comes), copies the size to pinned memory, records an event and returns - it never synchronises the caller's stream and
    blocks only while every slot is busy. A worker thread waits for the event, copies exactly `size` bytes on its own copy stream,
    wraps them (`png_container`) and writes the file. Host arrays - and an image whose stream did not fit (size -1) - go through PIL
    like `AsyncPngWriter`. Counters: `device_encoded`, `fallback_encoded`. `close()` joins and re-raises a worker's exception."""
    accepts_device = True

    def __init__(self, device='cuda', workers=2, slots=8, huffman='fixed'):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        png_huffman(huffman)
        self.huffman = huffman       # 'fixed' | 'dynamic': the Huffman code of `png_deflate`
        self.device = torch.device(device)
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.futures = []
        self.free = queue.Queue()
        for _ in range(slots):
            self.free.put(_PngSlot(self.device))
        self.local = threading.local()
        self.lock = threading.Lock()
        self.device_encoded = 0      # files whose stream came from vps_png_deflate
        self.fallback_encoded = 0    # files PIL encoded (host input, or a stream that did not fit)

    def _count(self, device):
        with self.lock:
            if device:
                self.device_encoded += 1
            else:
                self.fallback_encoded += 1

    def _save_host(self, image, name, palette=None):
        AsyncPngWriter._save(image, name, palette)
        self._count(False)
        return name

    def _finish(self, slot, name, H, W, C, palette=None):
        try:
            slot.event.synchronize()                     # the worker waits, not the caller
            n = int(slot.size_host[0])
            if not hasattr(self.local, 'stream'):
                self.local.stream = torch.cuda.Stream(self.device)
            with torch.cuda.stream(self.local.stream):
                if n < 0:
                    host = slot.image.cpu().numpy()
                else:
                    host = slot.staging(n)
                    host.copy_(slot.out[:n], non_blocking=True)
                    self.local.stream.synchronize()
                    data = png_container(host.numpy().tobytes(), H, W, C, palette)
        finally:
            slot.image = None
            self.free.put(slot)
        if n < 0:
            return self._save_host(host, name, palette)
        os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
        with open(name, 'wb') as f:
            f.write(data)
        self._count(True)
        return name

    def submit(self, image, name, palette=None):
        """`palette` (uint8 [256][3], optional, [H,W] maps only): a palette PNG, as `putpalette` + `save`"""
        if not (torch.is_tensor(image) and image.is_cuda):
            image = image.numpy() if torch.is_tensor(image) else image
            self.futures.append(self.pool.submit(self._save_host, np.ascontiguousarray(image), name, palette))
            return
        t, H, W, C, _ = _png_view(image)
        assert palette is None or C == 1, 'a palette goes with a single-channel map'
        slot = self.free.get()                           # blocks only when every slot is in flight
        try:
            slot.fit(*png_encode_bound(H, W, C))
            slot.image = t                               # alive until the worker is done with it
            png_deflate(t, slot.out, slot.ws, slot.size, huffman=self.huffman)
            slot.size_host.copy_(slot.size, non_blocking=True)
            slot.event.record()
        except BaseException:
            slot.image = None
            self.free.put(slot)
            raise
        self.futures.append(self.pool.submit(self._finish, slot, name, H, W, C, palette))

    def close(self):
        futures, self.futures = self.futures, []
        try:
            names = [f.result() for f in futures]        # re-raises a worker's exception
        finally:
            self.pool.shutdown()
        return names


# ------------------------------------------------------------------------------------------------------------------
# Overlay images: the panoptic result blended over the input frame, written as a baseline JPEG. Blend, colour conversion, chroma
# down-sampling, forward DCT and quantisation on the device (csrc/jpeg_enc_ops.hip), Huffman coding and the container on the host
# without the interpreter lock (csrc/jpeg_enc_host.cpp): the JPEG input path of pipeline.py in the other direction. The files are the
# ones libjpeg's default compressor (PIL's `save(format='JPEG', quality=q, subsampling=s)`) writes for the same pixels, scan byte for
# scan byte. entropy='device' (opt-in) moves the Huffman coding to the device as well (csrc/jpeg_scan_ops.hip): the host copies the scan,
# about the size of the file, and writes the container round it (`vps_jpeg_wrap`); the files are the same.
# ------------------------------------------------------------------------------------------------------------------
JPEG_SUBSAMPLING = {'4:2:0': 2, '4:4:4': 0, 2: 2, 0: 0}                         # the numbers are PIL's `subsampling=` values
_jpeg_qt_cache = {}


def _subsampling(s):
    if s not in JPEG_SUBSAMPLING:
        raise ValueError("subsampling is '4:2:0' or '4:4:4', got %r" % (s,))
    return JPEG_SUBSAMPLING[s]


def jpeg_quant_tables(quality):
    """uint16 [2][64] (luma, chroma; natural order): the Annex K tables scaled by libjpeg's quality rule, baseline forced"""
    import ctypes
    qt = np.zeros((2, 64), dtype=np.uint16)
    hip.check(hip.load_host().vps_jpeg_quant_tables(int(quality), qt.ctypes.data_as(ctypes.c_void_p)), 'vps_jpeg_quant_tables')
    return qt


def _jpeg_qt(quality, device):
    """(host tables, the same on `device`), made once per quality and device"""
    key = (int(quality), str(device))
    if key not in _jpeg_qt_cache:
        qt = jpeg_quant_tables(quality)
        _jpeg_qt_cache[key] = (qt, torch.from_numpy(qt.view(np.int16)).to(device))
    return _jpeg_qt_cache[key]


def jpeg_encode_bound(H, W, subsampling='4:2:0'):
    """(block grid [(rows, columns)] x 3, bytes of the coefficient array, worst-case bytes of the file) of one image size"""
    import ctypes
    sub = _subsampling(subsampling)
    host = hip.load_host()
    grid, nb, cap = (ctypes.c_int32 * 6)(), ctypes.c_int64(0), ctypes.c_int64(0)
    hip.check(host.vps_jpeg_encode_bound(H, W, sub, grid, ctypes.byref(nb)), 'vps_jpeg_encode_bound')
    hip.check(host.vps_jpeg_write_bound(H, W, sub, ctypes.byref(cap)), 'vps_jpeg_write_bound')
    return [(grid[2 * c], grid[2 * c + 1]) for c in range(3)], nb.value, cap.value


def _device_u8(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, 'uint8 [H,W,3], got %s %s' % (t.dtype, tuple(t.shape))
    return t.to(device)


def render_overlay(frame, colour, alpha=128):
    """`frame` BGR uint8 [H,W,3] (as the clip feeder decodes it), `colour` RGB uint8 [H,W,3] (as `TrackConverter.convert_device` paints
    it; 0,0,0 = void), alpha 0..256 -> device RGB uint8 [H,W,3] on the current stream, no sync (`vps_overlay_render`): void pixels keep
    the frame, the others are (frame * (256 - alpha) + colour * alpha + 128) >> 8, and a pixel whose right or lower neighbour has another
    colour is white. Host arrays are uploaded to the other argument's device (both on the host: 'cuda')."""
    dev = next((t.device for t in (colour, frame) if torch.is_tensor(t) and t.is_cuda), torch.device('cuda'))
    frame, colour = _device_u8(frame, dev).contiguous(), _device_u8(colour, dev).contiguous()
    assert frame.shape == colour.shape, (tuple(frame.shape), tuple(colour.shape))
    if not 0 <= int(alpha) <= 256:
        raise ValueError('alpha is 0..256, got %r' % (alpha,))
    out = torch.empty_like(colour)
    hip.check(hip.load().vps_overlay_render(hip.ptr(frame), hip.ptr(colour), int(frame.shape[0]), int(frame.shape[1]), int(alpha), hip.ptr(out),
                                            hip.stream_ptr()), 'vps_overlay_render')
    return out


def jpeg_encode_coef(rgb, quality=90, subsampling='4:2:0', out=None):
    """device RGB uint8 [H,W,3] (rows may be strided) -> device int16 quantised coefficients [component][block row][block column][64] in
    natural order - the array `vps_jpeg_decode_coef` reads from the file libjpeg writes for these pixels - on the current stream, no sync
    (`vps_jpeg_encode_coef`). `out`: caller-owned int16 buffer of at least `jpeg_encode_bound(..)[1] / 2` elements."""
    t, H, W, C, stride = _png_view(rgb)
    assert C == 3, 'jpeg_encode_coef takes an RGB image [H,W,3]'
    sub = _subsampling(subsampling)
    _, nb, _ = jpeg_encode_bound(H, W, sub)
    if out is None:
        out = torch.empty(nb // 2, dtype=torch.int16, device=t.device)
    assert out.dtype == torch.int16 and out.is_cuda and out.numel() * 2 >= nb
    _, qt_dev = _jpeg_qt(quality, t.device)
    hip.check(hip.load().vps_jpeg_encode_coef(hip.ptr(t), H, W, stride, sub, hip.ptr(qt_dev), hip.ptr(out), out.numel() * 2, hip.stream_ptr()),
              'vps_jpeg_encode_coef')
    return out[:nb // 2]


def jpeg_write(coef, H, W, quality=90, subsampling='4:2:0', out=None):
    """HOST int16 coefficients (numpy, or a CPU tensor such as pinned staging) -> the bytes of the baseline JFIF file (`vps_jpeg_write`,
    no interpreter lock while it runs). `out`: reusable uint8 numpy buffer; it is grown to the worst case when the file does not fit."""
    import ctypes
    sub = _subsampling(subsampling)
    qt = jpeg_quant_tables(quality)
    _, nb, cap = jpeg_encode_bound(H, W, sub)
    if torch.is_tensor(coef):
        assert not coef.is_cuda and coef.dtype == torch.int16 and coef.is_contiguous() and coef.numel() * 2 >= nb
        cptr = ctypes.c_void_p(coef.data_ptr())
    else:
        coef = np.ascontiguousarray(coef, dtype=np.int16)
        assert coef.size * 2 >= nb
        cptr = coef.ctypes.data_as(ctypes.c_void_p)
    if out is None:
        out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_int64(0)
    hip.check(hip.load_host().vps_jpeg_write(cptr, H, W, sub, qt.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), out.size,
                                             ctypes.byref(n)), 'vps_jpeg_write')
    return out[:n.value].tobytes()


JPEG_ENTROPY = ('host', 'device')
JPEG_SCAN_OK, JPEG_SCAN_SHORT, JPEG_SCAN_RANGE = 0, 1, 2                        # result[1] of `vps_jpeg_encode_scan`


def _entropy(e):
    if e not in JPEG_ENTROPY:
        raise ValueError("entropy is 'host' or 'device', got %r" % (e,))
    return e


def jpeg_scan_bound(H, W, subsampling='4:2:0'):
    """(workspace bytes, worst-case scan bytes) of `vps_jpeg_encode_scan` for one image size (`vps_jpeg_scan_bound`)"""
    import ctypes
    wsb, cap = ctypes.c_int64(0), ctypes.c_int64(0)
    hip.check(hip.load_host().vps_jpeg_scan_bound(H, W, _subsampling(subsampling), ctypes.byref(wsb), ctypes.byref(cap)), 'vps_jpeg_scan_bound')
    return wsb.value, cap.value


def jpeg_encode_scan(coef, H, W, subsampling='4:2:0', out=None, ws=None, result=None):
    """Huffman-code device coefficients (as `jpeg_encode_coef` wrote them) on the device (`vps_jpeg_encode_scan`) on
    the current stream, no sync. Returns (device uint8 buffer, device int64 [2] = bytes, status): with status JPEG_SCAN_OK the scan
    between the SOS header and EOI is buffer[:bytes]; JPEG_SCAN_SHORT = `out` holds only its first `out.numel()` bytes of `bytes`;
    JPEG_SCAN_RANGE = a coefficient the baseline tables have no code for. `out` / `ws` / `result`: caller-owned buffers (default:
    fresh ones, `out` of the worst-case size)."""
    assert torch.is_tensor(coef) and coef.is_cuda and coef.dtype == torch.int16 and coef.is_contiguous(), 'device int16 coefficients'
    sub = _subsampling(subsampling)
    assert coef.numel() * 2 >= jpeg_encode_bound(H, W, sub)[1]
    if out is None or ws is None:
        wsb, cap = jpeg_scan_bound(H, W, sub)
        out = torch.empty(cap, dtype=torch.uint8, device=coef.device) if out is None else out
        ws = torch.empty(wsb, dtype=torch.uint8, device=coef.device) if ws is None else ws
    if result is None:
        result = torch.empty(2, dtype=torch.int64, device=coef.device)
    hip.check(hip.load().vps_jpeg_encode_scan(hip.ptr(coef), H, W, sub, hip.ptr(out), out.numel(), hip.ptr(result), hip.ptr(ws), ws.numel(),
                                              hip.stream_ptr()), 'vps_jpeg_encode_scan')
    return out, result


def jpeg_wrap(scan, H, W, quality=90, subsampling='4:2:0', out=None):
    """HOST scan bytes (uint8 numpy, or a CPU tensor such as pinned staging) -> the bytes of the baseline JFIF file: the header
    `jpeg_write` writes, the scan, EOI (`vps_jpeg_wrap`, no interpreter lock). `out`: reusable uint8 numpy buffer, grown when too small."""
    import ctypes
    if torch.is_tensor(scan):
        assert not scan.is_cuda and scan.dtype == torch.uint8 and scan.is_contiguous()
        sptr, n = ctypes.c_void_p(scan.data_ptr()), scan.numel()
    else:
        scan = np.ascontiguousarray(scan, dtype=np.uint8)
        sptr, n = scan.ctypes.data_as(ctypes.c_void_p), scan.size
    qt = jpeg_quant_tables(quality)
    if out is None or out.size < n + 1024:
        out = np.empty(n + 1024, dtype=np.uint8)                                 # the header and EOI are 625 bytes
    nb = ctypes.c_int64(0)
    hip.check(hip.load_host().vps_jpeg_wrap(sptr, n, H, W, _subsampling(subsampling), qt.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p), out.size, ctypes.byref(nb)), 'vps_jpeg_wrap')
    return out[:nb.value].tobytes()


def jpeg_encode(rgb, quality=90, subsampling='4:2:0', entropy='host'):
    """device RGB uint8 [H,W,3] -> bytes of a baseline JPEG, the file PIL's `save(format='JPEG', quality=quality, subsampling=subsampling)`
    writes from the SOS marker on. Synchronises; `DeviceJpegWriter` is the asynchronous form. entropy 'host': one download of the
    coefficients, `vps_jpeg_write`. 'device': `jpeg_encode_scan` into a buffer of an eighth of the coefficients' size - repeated once
    with the exact size when the scan is longer - and one download of the scan; the same bytes."""
    t, H, W, _, _ = _png_view(rgb)
    coef = jpeg_encode_coef(t, quality, subsampling)
    if _entropy(entropy) == 'host':
        return jpeg_write(coef.cpu().numpy(), H, W, quality, subsampling)
    ws = torch.empty(jpeg_scan_bound(H, W, subsampling)[0], dtype=torch.uint8, device=t.device)
    out = torch.empty(max(4096, coef.numel() // 4), dtype=torch.uint8, device=t.device)
    out, result = jpeg_encode_scan(coef, H, W, subsampling, out, ws)
    n, status = (int(v) for v in result.cpu())
    if status == JPEG_SCAN_SHORT:
        out, result = jpeg_encode_scan(coef, H, W, subsampling, torch.empty(n, dtype=torch.uint8, device=t.device), ws)
        n, status = (int(v) for v in result.cpu())
    if status != JPEG_SCAN_OK:
        raise hip.VpsHipError('vps_jpeg_encode_scan: status %d (a coefficient outside the range of 8-bit baseline data)' % status)
    return jpeg_wrap(out[:n].cpu().numpy(), H, W, quality, subsampling)


class _JpegSlot:
    def __init__(self, device):
        self.device = device
        self.coef = self.host = self.image = None
        self.scan = self.ws = self.scan_host = None      # entropy 'device' only
        self.event = torch.cuda.Event()

    def fit(self, nelem, pinned=True):
        if self.coef is None or self.coef.numel() < nelem:
            self.coef = torch.empty(nelem, dtype=torch.int16, device=self.device)
            self.host = torch.empty(nelem, dtype=torch.int16).pin_memory() if pinned else None

    def fit_scan(self, cap, wsb):
        """scan buffer + pinned staging of `cap` bytes, workspace, result (device and pinned)"""
        if self.scan is None:
            self.result = torch.empty(2, dtype=torch.int64, device=self.device)
            self.result_host = torch.empty(2, dtype=torch.int64).pin_memory()
        if self.scan is None or self.scan.numel() < cap:
            self.scan = torch.empty(cap, dtype=torch.uint8, device=self.device)
            self.scan_host = torch.empty(cap, dtype=torch.uint8).pin_memory()
        if self.ws is None or self.ws.numel() < wsb:
            self.ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)


class DeviceJpegWriter:
    """`DevicePngWriter`'s shape for JPEG files: `submit(device RGB uint8 [H,W,3], name)` enqueues `jpeg_encode_coef` on the CURRENT stream
    into one of `slots` ring slots (coefficients on the device + pinned staging of the same size, grown if a larger image comes), records
    an event and returns - it never synchronises the caller's stream and blocks only while every slot is busy. A worker thread waits for
    the event, downloads the coefficients on its own copy stream, runs `vps_jpeg_write` (no interpreter lock) into a buffer it keeps, and
    writes the file. Host arrays are uploaded first: there is no host encoder here. Counters: `submitted`, `device_encoded`,
    `bytes_written`, `bytes_downloaded`. `close()` joins and re-raises a worker's exception.
    entropy='device' (default 'host', the above): `submit` also enqueues `jpeg_encode_scan` and the copy of its 16-byte result; the slot
    holds a scan buffer of `scan_capacity` bytes (default: a quarter of the coefficients' bytes, 2 bits per coefficient), the workspace
    and pinned staging for the scan in place of the staging for the coefficients. The worker copies exactly the scan's bytes and puts
    the container round them (`vps_jpeg_wrap`): the same file. A scan that does not fit the slot, or a coefficient out of range, sends
    that frame through the host coder as above (unpinned download) and is counted in `fallback_encoded`; the others in `scan_encoded`."""
    accepts_device = True

    def __init__(self, device='cuda', workers=2, slots=4, quality=90, subsampling='4:2:0', entropy='host', scan_capacity=None):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        self.device = torch.device(device)
        self.quality, self.subsampling = int(quality), _subsampling(subsampling)
        self.entropy, self.scan_capacity = _entropy(entropy), scan_capacity
        jpeg_quant_tables(self.quality)                  # a bad quality raises here, not in a worker
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.futures = []
        self.free = queue.Queue()
        for _ in range(slots):
            self.free.put(_JpegSlot(self.device))
        self.local = threading.local()
        self.lock = threading.Lock()
        self.submitted = 0           # images handed to submit()
        self.device_encoded = 0      # files written from device coefficients
        self.scan_encoded = 0        # ... of them: files whose scan came from vps_jpeg_encode_scan
        self.fallback_encoded = 0    # entropy 'device' frames the host coder wrote (scan slot too small, coefficient out of range)
        self.bytes_written = 0
        self.bytes_downloaded = 0    # device -> host, coefficients or scan + result

    def _host_coded(self, coef_host, H, W):
        cap = jpeg_encode_bound(H, W, self.subsampling)[2]
        if self.local.out is None or self.local.out.size < cap:
            self.local.out = np.empty(cap, dtype=np.uint8)    # pages of the worst case that no file reaches are never touched
        return jpeg_write(coef_host, H, W, self.quality, self.subsampling, self.local.out)

    def _finish(self, slot, name, H, W, nelem):
        scanned = False
        try:
            slot.event.synchronize()                     # the worker waits, not the caller
            if not hasattr(self.local, 'stream'):
                self.local.stream = torch.cuda.Stream(self.device)
                self.local.out = None
            if self.entropy == 'device':
                n, status = int(slot.result_host[0]), int(slot.result_host[1])
                scanned = status == JPEG_SCAN_OK
                down = 16
            if scanned:
                with torch.cuda.stream(self.local.stream):
                    slot.scan_host[:n].copy_(slot.scan[:n], non_blocking=True)
                    self.local.stream.synchronize()
                if self.local.out is None or self.local.out.size < n + 1024:
                    self.local.out = np.empty(max(1 << 16, 1 << (n + 1024).bit_length()), dtype=np.uint8)
                data = jpeg_wrap(slot.scan_host[:n], H, W, self.quality, self.subsampling, self.local.out)
                down += n
            elif self.entropy == 'device':
                with torch.cuda.stream(self.local.stream):
                    coef_host = slot.coef[:nelem].cpu()
                data = self._host_coded(coef_host, H, W)
                down += 2 * nelem
            else:
                with torch.cuda.stream(self.local.stream):
                    slot.host[:nelem].copy_(slot.coef[:nelem], non_blocking=True)
                    self.local.stream.synchronize()
                data = self._host_coded(slot.host, H, W)
                down = 2 * nelem
        finally:
            slot.image = None
            self.free.put(slot)
        os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
        with open(name, 'wb') as f:
            f.write(data)
        with self.lock:
            self.device_encoded += 1
            self.bytes_written += len(data)
            self.bytes_downloaded += down
            if self.entropy == 'device':
                self.scan_encoded += scanned
                self.fallback_encoded += not scanned
        return name

    def submit(self, image, name):
        if not (torch.is_tensor(image) and image.is_cuda):
            image = _device_u8(image, self.device)
        t, H, W, C, _ = _png_view(image)
        assert C == 3, 'a JPEG overlay is an RGB image [H,W,3]'
        nelem = jpeg_encode_bound(H, W, self.subsampling)[1] // 2
        slot = self.free.get()                           # blocks only when every slot is in flight
        try:
            slot.fit(nelem, pinned=self.entropy == 'host')
            slot.image = t                               # alive until the worker is done with it
            jpeg_encode_coef(t, self.quality, self.subsampling, slot.coef)
            if self.entropy == 'device':
                cap = nelem // 2 if self.scan_capacity is None else int(self.scan_capacity)
                slot.fit_scan(max(cap, 1), jpeg_scan_bound(H, W, self.subsampling)[0])
                jpeg_encode_scan(slot.coef[:nelem], H, W, self.subsampling, slot.scan, slot.ws, slot.result)
                slot.result_host.copy_(slot.result, non_blocking=True)
            slot.event.record()
        except BaseException:
            slot.image = None
            self.free.put(slot)
            raise
        self.submitted += 1
        self.futures.append(self.pool.submit(self._finish, slot, name, H, W, nelem))

    def close(self):
        futures, self.futures = self.futures, []
        try:
            names = [f.result() for f in futures]        # re-raises a worker's exception
        finally:
            self.pool.shutdown()
        return names


def overlay_name(save_folder, name):
    """output file of the overlay of an input image name: DIR/<name without its extension>.jpg"""
    return os.path.join(save_folder, os.path.splitext(os.path.basename(name))[0] + '.jpg')


def write_overlays(pred_pans_2ch, frames, names, out_dir, color_generator, nframes_per_video, device='cuda', alpha=128, quality=90,
                   writer=None, entropy='host', video=None, video_sampling='420jpeg', video_fps=(30, 1), video_files=None):
    """an overlay JPEG of EVERY frame: `pred_pans_2ch` (the unified 3-channel maps, host or device) are painted per video by
    `TrackConverter.convert_device` (a track keeps its colour through its video), blended over `frames` (BGR uint8 [H,W,3], host or
    device, same order) by `render_overlay` and written as `out_dir/<name>.jpg` through a `DeviceJpegWriter` (the caller's, or one made
    and closed here, with `entropy` 'host' or 'device'). `color_generator`: its own instance - the colours of pred.json are not touched.
    Returns the file names.
    video='FILE.y4m' (default None: nothing else happens): the same images also go, video by video, to one Y4M stream each through a
    `y4m.Y4mWriter` (`video_sampling`, `video_fps`; limited range, bt601): `video` itself for a single video, else the video's name
    (`video_name_of` its frames' names) inserted in front of the extension, `overlay_video_name`. `video_files`: a list that receives
    the streams' names. With `out_dir=None` only the streams are written and the return value is their names."""
    assert len(pred_pans_2ch) == len(frames) == len(names)
    jpegs = out_dir is not None
    assert jpegs or video is not None, 'nothing to write: out_dir and video are both None'
    own = writer is None and jpegs
    writer = DeviceJpegWriter(device, quality=quality, entropy=entropy) if own else writer
    conv = TrackConverter(device)
    out, videos = [], [] if video_files is None else video_files
    nvideos = (len(pred_pans_2ch) + nframes_per_video - 1) // nframes_per_video
    for v0 in range(0, len(pred_pans_2ch), nframes_per_video):
        _, pans_dev, _ = conv.convert_device(pred_pans_2ch[v0:v0 + nframes_per_video], color_generator)
        vw = None
        try:
            for j, pan in enumerate(pans_dev):
                img = render_overlay(frames[v0 + j], pan, alpha)
                if jpegs:
                    out.append(overlay_name(out_dir, names[v0 + j]))
                    writer.submit(img, out[-1])
                if video is not None:
                    if vw is None:
                        from .y4m import Y4mWriter
                        vname = video_name_of(names[v0:v0 + nframes_per_video], v0 // nframes_per_video)
                        videos.append(overlay_video_name(video, vname, nvideos, taken=videos))
                        vw = Y4mWriter(videos[-1], int(img.shape[1]), int(img.shape[0]), fps=video_fps, sampling=video_sampling, device=img.device,
                                       order='rgb')
                    vw.submit(img)
        finally:
            if vw is not None:
                vw.close()
    if own:
        writer.close()
    return out if jpegs else videos


def video_name_of(names, k):
    """the name of video k from the names of its frames: what their base names have in common, cut back to a whole `_` / `-` separated
    field ('0005_0025_frankfurt_..', '0005_0026_frankfurt_..' -> '0005'); 'v<k, three digits>' when they share no whole field"""
    stems = [os.path.splitext(os.path.basename(n))[0] for n in names]
    common = os.path.commonprefix(stems)
    if not all(s == common or s[len(common)] in '_-' for s in stems):     # the prefix ends inside a field
        cut = max(common.rfind('_'), common.rfind('-'))
        common = common[:cut] if cut > 0 else ''
    return common.rstrip('_-') or 'v%03d' % k


def overlay_video_name(video, vname, nvideos, taken=()):
    """the Y4M file of the video called `vname`: `video` itself for a single video, else DIR/<stem>.<vname><ext> (with a counter behind
    the name when an earlier video of the call has the same one)"""
    if nvideos <= 1:
        return video
    stem, ext = os.path.splitext(video)
    name, n = '%s.%s%s' % (stem, vname, ext), 1
    while name in taken:
        n += 1
        name = '%s.%s-%d%s' % (stem, vname, n, ext)
    return name


def png_name(save_folder, name):
    """cityscapes_vps.py:73 (save_image): output file name of an input image name"""
    return os.path.join(save_folder, name.replace('_leftImg8bit', '').replace('_newImg8bit', '').replace('jpg', 'png').replace('jpeg', 'png'))


def inference_panoptic_video(pred_pans_2ch, output_dir, categories, names, n_video=0, color_generator=None, device='cuda',
                             labeled_fid=20, lambda_=5, nframes_per_video=6, writer=None, tubes=None):
    """`CityscapesVps.inference_panoptic_video` (cityscapes_vps.py:27-94) with the conversion on the device and asynchronous PNG
    writing: same arguments and return value `(pred_pans, pred_json)`, same files (`pan_2ch/`, `pan_pred/`, `pred.json`).
    `pred_pans_2ch`: per-frame uint8 [H,W,3] maps (host arrays or device tensors, e.g. straight from PanopticUnifier);
    `names`: the image file names of the SAMPLED frames (the reference passes them already sampled, test_vpq.py:186-197).
    color_generator: panopticapi's IdGenerator(categories) by default (imported lazily, like the reference); colours are handed
    out per video in the reference's order — one converter state per video, as `np.array_split(.., nprocs)` over whole videos
    gives when nprocs == number of videos.
    tubes: a `tubes.TubeCollector`; every sampled frame is added to it under its video's index (with the segment statistics the
    converter has already downloaded) and `tubes.json` is written beside `pred.json`. None: nothing else happens."""
    pred_pans_2ch = pred_pans_2ch[(labeled_fid // lambda_)::lambda_]            # only frames with GT annotations (:36)
    if color_generator is None:
        from panopticapi.utils import IdGenerator
        color_generator = IdGenerator({el['id']: el for el in categories})
    own = writer is None
    writer = AsyncPngWriter() if own else writer
    conv = TrackConverter(device)
    on_device = bool(getattr(writer, 'accepts_device', False))     # DevicePngWriter: hand over the device maps, not host copies
    annotations, pan_all = [], []
    for v0 in range(0, len(pred_pans_2ch), nframes_per_video):
        chunk = pred_pans_2ch[v0:v0 + nframes_per_video]
        ann, pans_dev, twos_dev = conv.convert_device(chunk, color_generator)
        for j, (a, pan_dev) in enumerate(zip(ann, pans_dev)):
            i = v0 + j
            annotations.append(a)
            if tubes is not None:
                tubes.add(v0 // nframes_per_video, names[i] if names is not None else '%d' % i, twos_dev[j], stats=conv.frame_stats[j])
            if names is not None and on_device:
                writer.submit(twos_dev[j], png_name(os.path.join(output_dir, 'pan_2ch'), names[i]))
                writer.submit(pan_dev, png_name(os.path.join(output_dir, 'pan_pred'), names[i]))
            pan = pan_dev.cpu().numpy()                            # part of the return value: downloaded once either way
            pan_all.append(pan)
            if names is not None and not on_device:
                two = chunk[j]
                two = two.cpu().numpy() if torch.is_tensor(two) else np.asarray(two)
                writer.submit(two, png_name(os.path.join(output_dir, 'pan_2ch'), names[i]))
                writer.submit(pan, png_name(os.path.join(output_dir, 'pan_pred'), names[i]))
    pred_json = {'annotations': annotations}
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, 'pred.json'), 'w') as f:
        json.dump(pred_json, f)
    if tubes is not None:
        tubes.write(os.path.join(output_dir, 'tubes.json'))
    if own:
        writer.close()
    return pan_all, pred_json
