"""Track tubes: the mask of every tracked segment over time, as COCO run-length encodings, from the final panoptic map.

`simple_test` returns boxes and labels per object id and `pred.json` lists `category_id / id / bbox / area` per frame; the masks of
a track are only in the panoptic maps. This module encodes them without a host copy of the maps: `vps_rle_runs` (csrc/rle_ops.hip)
lists the runs of a unified `(pan_seg, pan_ins, pan_obj)` map in column-major order on the device - one pass over the pixels - and
`vps_rle_strings` (csrc/rle_host.cpp) turns the list into the `counts` string of every segment in a pass over the runs on the host.
Only the run list is downloaded. Every mask is by construction the one the panoptic PNG shows: no resize, no floating point.

  rle_runs        device map -> (run_start, run_key, count) on the device
  segment_rles    device map -> {key: {'size': [H, W], 'counts': bytes}}; key = pan_seg * 256 + id (as `vps_segment_stats`)
  rle_decode      an encoding -> uint8 [H, W] mask (host NumPy; pycocotools is not needed)
  TubeCollector   frames of videos -> tubes.json: per video and track the encoding, box and area in every frame, null where absent

Boxes in tubes.json are COCO boxes, `[x, y, w, h]` with `w = xmax - xmin + 1` (pycocotools' `toBbox` of the mask). This DIFFERS from
`pred.json`, which keeps the reference's `[x, y, xmax - x, ymax - y]` (cityscapes_vps.py:147). Area and box are those of
`vps_segment_stats`; `inference_panoptic_video` hands the collector the rows its TrackConverter has already downloaded.

No CPU path for the run list: maps must be device tensors. `rle_strings`, `rle_decode` and `TubeCollector.add_runs` are host code."""
import json
import os

import numpy as np
import torch

from . import hip

BAND_ROWS = 32                         # rows of one band of vps_rle_runs' sweeps (`vps_rle_band_rows`): a run may cross a band edge
VOID_CLASS = 255


def _map_view(pan_2ch):
    if not (torch.is_tensor(pan_2ch) and pan_2ch.is_cuda):
        raise hip.VpsHipError('vps_rle_runs needs a device map; there is no CPU path')
    assert pan_2ch.dtype == torch.uint8 and pan_2ch.dim() == 3 and pan_2ch.shape[2] == 3, 'uint8 [H,W,3], got %s %s' % (pan_2ch.dtype, tuple(pan_2ch.shape))
    t = pan_2ch.contiguous()
    return t, int(t.shape[0]), int(t.shape[1])


def rle_runs_ws(H, W):
    """workspace bytes of `vps_rle_runs` for one map size"""
    return int(hip.load().vps_rle_runs_ws(H, W))


def rle_runs_async(pan_2ch, id_channel=2, cap=None, ws=None):
    """`vps_rle_runs` on the current stream, no sync: (run_start int32 [cap], run_key int16 [cap], nruns int32 [1]), all on the device;
    the bit patterns are uint32 / uint16. nruns is the true number of runs, the lists hold the first min(nruns, cap)."""
    t, H, W = _map_view(pan_2ch)
    cap = H * W // 8 if cap is None else int(cap)
    run_start = torch.empty(max(cap, 1), dtype=torch.int32, device=t.device)
    run_key = torch.empty(max(cap, 1), dtype=torch.int16, device=t.device)
    nruns = torch.empty(1, dtype=torch.int32, device=t.device)
    if ws is None:
        ws = torch.empty(rle_runs_ws(H, W), dtype=torch.uint8, device=t.device)
    hip.check(hip.load().vps_rle_runs(hip.ptr(t), H, W, int(id_channel), hip.ptr(run_start), hip.ptr(run_key), cap, hip.ptr(nruns), hip.ptr(ws),
                                      ws.numel(), hip.stream_ptr()), 'vps_rle_runs')
    return run_start[:cap], run_key[:cap], nruns


def rle_runs(pan_2ch, id_channel=2, cap=None):
    """The run list of a device uint8 [H,W,3] map in column-major order: (run_start, run_key, n). run_start int32 [n] and run_key
    int16 [n] are device tensors holding uint32 positions `x * H + y` and uint16 keys `ch0 * 256 + ch[id_channel]`. Reads the count,
    which waits for the stream; if it exceeds `cap` (default H * W // 8) the kernel runs once more with the exact size."""
    t, H, W = _map_view(pan_2ch)
    run_start, run_key, nruns = rle_runs_async(t, id_channel, cap)
    n = int(nruns.item())
    if n > run_start.numel():
        run_start, run_key, nruns = rle_runs_async(t, id_channel, n)
        assert int(nruns.item()) == n
    return run_start[:n], run_key[:n], n


def runs_to_host(run_start, run_key):
    """device lists -> (uint32, uint16) NumPy arrays"""
    return run_start.cpu().numpy().view(np.uint32), run_key.cpu().numpy().view(np.uint16)


def rle_strings_bound(nruns, nkeys):
    return int(hip.load_host().vps_rle_strings_bound(int(nruns), int(nkeys)))


def rle_strings(run_start, run_key, npix, keys, capacity=None):
    """`vps_rle_strings` on host arrays: the run list of a map of npix pixels -> [counts bytes of every key in `keys`] (sorted, unique).
    The call holds no interpreter lock. `capacity`: size of the string buffer (default: the bound)."""
    run_start = np.ascontiguousarray(run_start, dtype=np.uint32)
    run_key = np.ascontiguousarray(run_key, dtype=np.uint16)
    keys = np.ascontiguousarray(keys, dtype=np.uint16)
    n, nk = int(run_start.size), int(keys.size)
    assert run_key.size == n
    cap = rle_strings_bound(n, nk) if capacity is None else int(capacity)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offset, length, scratch = np.zeros(max(nk, 1), np.int64), np.zeros(max(nk, 1), np.int64), np.empty(4 * max(nk, 1), np.int64)
    hip.check(hip.load_host().vps_rle_strings(run_start.ctypes.data, run_key.ctypes.data, n, int(npix), keys.ctypes.data, nk, out.ctypes.data, cap,
                                              offset.ctypes.data, length.ctypes.data, scratch.ctypes.data), 'vps_rle_strings')
    return [out[offset[i]:offset[i] + length[i]].tobytes() for i in range(nk)]


def default_keys(run_key):
    """every present key whose class is not 255 (void), ascending"""
    keys = np.unique(np.asarray(run_key).view(np.uint16))
    return keys[(keys >> 8) != VOID_CLASS]


def segment_rles(pan_2ch, id_channel=2, keys=None):
    """{key: {'size': [H, W], 'counts': bytes}} of a device uint8 [H,W,3] map: the COCO encoding of `key_map == key` for every key in
    `keys` (default: every present key whose class is not 255). A key that is absent encodes the empty mask."""
    H, W = int(pan_2ch.shape[0]), int(pan_2ch.shape[1])
    run_start, run_key = runs_to_host(*rle_runs(pan_2ch, id_channel)[:2])
    keys = default_keys(run_key) if keys is None else np.unique(np.asarray(keys, dtype=np.uint16))
    strings = rle_strings(run_start, run_key, H * W, keys)
    return {int(k): {'size': [H, W], 'counts': s} for k, s in zip(keys, strings)}


def rle_counts(rle):
    """the counts of an encoding (COCO's rleFrString)"""
    s = rle['counts']
    s = s.encode('ascii') if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(rle):
    """{'size': [H, W], 'counts': str or bytes} -> uint8 [H, W] mask (host NumPy)"""
    H, W = (int(v) for v in rle['size'])
    counts = np.asarray(rle_counts(rle), dtype=np.int64)
    if (counts < 0).any() or int(counts.sum()) != H * W:
        raise ValueError('the counts do not add up to %d x %d' % (H, W))
    flat = np.repeat((np.arange(counts.size) & 1).astype(np.uint8), counts)
    return flat.reshape((H, W), order='F')


class TubeCollector:
    """Collects the frames of videos and builds `tubes.json`:

        {"videos": [{"video_id", "file_names": [...], "height", "width",
                     "tracks": [{"track_id": 1000 * sem + obj, "category_id": sem, "segmentations": [rle | null per frame],
                                 "bboxes": [[x, y, w, h] | null], "areas": [int | null]}]}]}

    A track is a (class, id) pair of the map; the same pair in two frames of a video is the same track. `counts` is an ASCII string.
    Videos appear in the order of their first frame, tracks in ascending track_id. Class 255 is never a track. things_only: only
    the instances. With id_last_stuff (PanopticUnifier's: num_seg_classes - num_classes, 10 for Cityscapes-VPS) those are the
    segments of a class above it; without it the rule of the reference's converter holds, an id > 0 (cityscapes_vps.py:130) - in a
    unified video map a stuff segment carries its class as pan_obj, so every stuff class but 0 passes that rule. id_channel 2 for video maps (pan_obj), 1 for image-level maps
    (pan_ins). workers > 0: the host coding of a frame runs in a thread pool (`vps_rle_strings` holds no interpreter lock) while the
    caller goes on; `result` waits for it."""

    def __init__(self, things_only=True, id_channel=2, workers=0, device='cuda', id_last_stuff=None):
        self.things_only = bool(things_only)
        self.id_last_stuff = id_last_stuff
        self.id_channel = int(id_channel)
        self.device = device
        self.videos = {}                                 # video_id -> dict(file_names, height, width, frames: [future or dict])
        self.pool = None
        if workers > 0:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=workers)
        self._stats = None

    def _stat_rows(self, t, H, W):
        """(keys, rows) of the present segments from `vps_segment_stats_ch`"""
        if self._stats is None:
            self._stats = torch.empty(65536 * 5, dtype=torch.int32, device=t.device)
        hip.check(hip.load().vps_segment_stats_ch(hip.ptr(t), H, W, self.id_channel, hip.ptr(self._stats), hip.stream_ptr()), 'vps_segment_stats_ch')
        st = self._stats.view(65536, 5)
        keys = torch.nonzero(st[:, 0] > 0).flatten()
        return keys.cpu().numpy(), st[keys].cpu().numpy()

    @staticmethod
    def _rows_of(stats):
        """stats: (keys, rows [n,5]) of the present segments, or the whole int32 [65536,5] table (device tensor or array)"""
        if isinstance(stats, (tuple, list)) and len(stats) == 2:
            return np.asarray(stats[0]).astype(np.int64), np.asarray(stats[1]).astype(np.int64)
        st = stats.cpu().numpy() if torch.is_tensor(stats) else np.asarray(stats)
        st = st.reshape(65536, 5)
        keys = np.flatnonzero(st[:, 0] > 0)
        return keys.astype(np.int64), st[keys].astype(np.int64)

    def _encode(self, run_start, run_key, H, W, keys, rows):
        sel = (keys >> 8) != VOID_CLASS
        if self.things_only:
            sel &= ((keys & 255) > 0) if self.id_last_stuff is None else ((keys >> 8) > self.id_last_stuff)
        keys, rows = keys[sel], rows[sel]
        order = np.argsort(keys, kind='stable')
        keys, rows = keys[order], rows[order]
        strings = rle_strings(run_start, run_key, H * W, keys)
        frame = {}
        for k, row, s in zip(keys, rows, strings):
            cnt, x0, y0, x1, y1 = (int(v) for v in row)
            sem, obj = int(k) >> 8, int(k) & 255
            frame[(sem, obj)] = ({'size': [H, W], 'counts': s.decode('ascii')}, [x0, y0, x1 - x0 + 1, y1 - y0 + 1], cnt)
        return frame

    def add_runs(self, video_id, file_name, H, W, run_start, run_key, stats):
        """one frame from a host run list (uint32 starts, uint16 keys) and its segment statistics; host code only"""
        keys, rows = self._rows_of(stats)
        v = self.videos.setdefault(video_id, dict(file_names=[], height=int(H), width=int(W), frames=[]))
        assert (v['height'], v['width']) == (int(H), int(W)), 'the frames of a video have one size'
        v['file_names'].append(file_name)
        if self.pool is not None:
            v['frames'].append(self.pool.submit(self._encode, run_start, run_key, int(H), int(W), keys, rows))
        else:
            v['frames'].append(self._encode(run_start, run_key, int(H), int(W), keys, rows))

    def add(self, video_id, file_name, pan_2ch, stats=None):
        """one frame: pan_2ch device uint8 [H,W,3] (a host array is uploaded). stats: what `vps_segment_stats` gave for this map -
        (keys, rows) of the present segments as TrackConverter keeps them, or the [65536,5] table; None: computed here."""
        t = torch.from_numpy(np.ascontiguousarray(pan_2ch)).to(self.device) if isinstance(pan_2ch, np.ndarray) else pan_2ch
        t, H, W = _map_view(t)
        if stats is None:
            stats = self._stat_rows(t, H, W)
        run_start, run_key = runs_to_host(*rle_runs(t, self.id_channel)[:2])
        self.add_runs(video_id, file_name, H, W, run_start, run_key, stats)

    def result(self):
        videos = []
        for vid, v in self.videos.items():
            frames = [f.result() if hasattr(f, 'result') else f for f in v['frames']]
            v['frames'] = frames
            tracks = []
            for sem, obj in sorted(set(k for f in frames for k in f), key=lambda k: (1000 * k[0] + k[1], k)):
                per = [f.get((sem, obj)) for f in frames]
                tracks.append({'track_id': 1000 * sem + obj, 'category_id': sem,
                               'segmentations': [None if p is None else p[0] for p in per],
                               'bboxes': [None if p is None else p[1] for p in per],
                               'areas': [None if p is None else p[2] for p in per]})
            videos.append({'video_id': vid, 'file_names': list(v['file_names']), 'height': v['height'], 'width': v['width'], 'tracks': tracks})
        return {'videos': videos}

    def write(self, path):
        res = self.result()
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
        with open(path, 'w') as f:
            json.dump(res, f)
        return res

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None
