"""Temporal consistency (TC) without ground truth: the agreement of a frame's unified map with the previous frame's map warped to it by
the detector's own FlowNet2 flow, with the per-pixel counting on the device.

The video-segmentation literature reports such a figure beside accuracy (Liu et al., "Efficient semantic video segmentation with
per-frame inference", ECCV 2020, warp with FlowNet2 and score the mIoU of the warped and the current prediction). The reference has no
TC. The definition below is RESTATED FROM MEMORY of that publication and EXTENDED to track ids; no implementation of it is available
where this was written. It is pinned only by hand-derived answers (tests/test_tc.py) and by an independent per-pixel restatement
(tests/tc_restate.py), not by a run of an original.

One pair: frame t is "cur", its reference frame (frame t-1 of the same video in these tools) is "prev"; a video's first frame has no
pair. cur, prev: unified maps uint8 [H][W][3] = (pan_seg, pan_ins, pan_obj). flow: fp32 [H][W][2], channel 0 = x, 1 = y, in the
direction the detector computes it: FlowNet2 gets (img, ref) and its stages sample the SECOND image at p + flow(p) (flownet2.py
`run`: x6 = img | ref, every `vps_flow_stage_full` warps ref; `vps_resample2d`: out(p) = in(p + flow(p))), so
    warped(p) = prev(p + flow(p))
and `pano_results['flow']` of frame t (`keep_flow`) is the flow of this pair as it stands.

Warp, per pixel p = (x, y) of cur, all in fp32:
    sx = float(x) + u, sy = float(y) + v (one add each);  qx = floorf(sx + 0.5f), qy = floorf(sy + 0.5f)
    in view iff 0 <= qx <= W-1 and 0 <= qy <= H-1, compared as floats before any conversion to int: NaN, +-inf, 1e30 fall out
    not in view: outside += 1 and nothing else
Semantic table: class index c(.) = seg_class[pan_seg] (uint8 [256] from the host), a value >= C is void = index C. In view, a = cur[p],
b = prev[q]: conf[c(b)][c(a)] += 1, conf is [C+1][C+1].
    IoU_c = conf[c][c] / (row_c + col_c - conf[c][c]) over the full table (a pixel that was road and became void costs road)
    TC_sem = mean of IoU_c over the classes c < C whose union is non-zero (0 when there is none)
Track tables: key = pan_seg * 256 + map[.., id_channel] (the key of `vps_segment_stats_ch`; id_channel 2 = pan_obj for video maps). The
host lists the sorted unique uint16 keys of the video's thing segments. In view: cur_size[k] += 1 when cur's key is listed,
prev_size[k] += 1 when the warped key is listed, same[k] += 1 when both are listed and equal.
    IoU_k = sum same / sum (prev_size + cur_size - same), summed over the video's pairs (a tube-style sum, like VPQ)
    TC_track = mean over the keys whose union is non-zero (0 when there is none: a video without tracks has TC 0, read TC_sem then)
    TC = sqrt(TC_sem * TC_track)
Over several videos: conf is summed, the tracks of all videos are averaged together.

Known limits: occluded pixels are NOT excluded, so a perfect prediction scores below 1 wherever the flow is wrong; a track that enters
or leaves the view is charged for it; the figure rates the flow as much as the maps.

Occlusion (opt-in: `TcEvaluator(occlusion=True)`, `flow_occlusion`) removes the first of these limits with a
forward-backward check. The definition is RESTATED FROM MEMORY of Sundaram et al. ("Dense point trajectories by GPU-accelerated large
displacement optical flow", ECCV 2010) as used by UnFlow (Meister et al., AAAI 2018), with alpha = 0.01 and beta = 0.5; no
implementation of it is available where this was written. It is pinned only by hand-derived answers (tests/test_flow_occ.py) and by an
independent per-pixel restatement (tests/flow_occ_restate.py). `fwd` is the flow above (on the grid of cur, pointing into prev), `back`
is the flow on the grid of prev pointing into cur: FlowNet2 run with the two images swapped (`flow_between(ref_img, img)` of the
detector). Per pixel p = (x, y), everything fp32 and every operation rounded on its own, in the order written:
    u, v = fwd(p).
    sx = float(x) + u, sy = float(y) + v.
    In view: exactly the rule above. qx = floorf(sx + 0.5f) and qy likewise. 0 <= qx <= W-1 and 0 <= qy <= H-1, compared as floats before
    any conversion to int. NaN, +-inf and 1e30 fall out.
    Not in view: code 2, counts[2] += 1, and back is not read.
    Corners: x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1. Both x0 and x1 are clamped to [0, W-1] after conversion to int. The same holds
    for y.
    With b00 at (y0, x0), b01 at (y0, x1), b10 at (y1, x0), b11 at (y1, x1), for each channel: top = b00 + wx*(b01 - b00),
    bot = b10 + wx*(b11 - b10), bt = top + wy*(bot - top).
    dx = u + bt_u, dy = v + bt_v.
    d2 = dx*dx + dy*dy.
    m = (u*u + v*v) + (bt_u*bt_u + bt_v*bt_v).
    thr = alpha*m + beta.
    Visible (code 0, counts[0]) iff d2 <= thr is true. Otherwise occluded (code 1, counts[1]). A NaN anywhere therefore gives occluded.
The check flags disocclusions: pixels of cur that were hidden in prev (behind a moving object, beyond the frame edge) and so have no
true correspondence; the backward flow of the place the forward flow points to leads somewhere else. The counting then skips them: an
in-view pixel with a non-zero mask byte adds 1 to the pair's `masked` cell and to nothing else (inconsistency code 4), a pixel that is
not in view stays `outside` whatever the mask says, so in_view + outside + masked grows by H*W per pair. `occluded` is the sum of the
masked cells and `occluded_share` its share of ALL pixels; `in_view` then counts the visible in-view pixels only and `in_view_share` is
their share of all pixels. Memory: a second 8 bytes per pixel and frame (the backward flow) until the pair is counted, and one byte
per pixel for the mask of the pair being counted. What remains a limit: a flow that is wrong but self-consistent in both directions
is still trusted - unless the photometric flag is on too (opt-in: `TcEvaluator(occlusion=True, photometric=THR)`, DESIGN.md 6 row 3h,
vps_amd/flowphoto.py): the pair's mask then passes through `vps_flow_photo` in place, which gives code 3 to the visible in-view pixels
whose previous frame, sampled where the flow points, differs from the current frame by more than THR grey levels on average, and the
counting skips those as well. The `masked` cell then holds occluded plus flagged pixels; the table layout does not change.

`tc_from_tables`, `TcStats` and `tc_text` are NumPy / Python only. The counting (`TcEvaluator`) is `vps_tc_accumulate`
(csrc/tc_ops.hip): no CPU path, the HIP library must load and a device must be present; host arrays are uploaded, device tensors are
used as they are. Memory: the evaluator keeps nothing but its tables; a caller that collects the flows of a clip before its maps are
unified (the tools do) holds 8 bytes per pixel and frame, 16.8 MB per frame at 1024x2048, each until its pair has been counted."""
import ctypes
import math

import numpy as np
import torch

from . import hip

MAX_CLASSES = 63
MAX_KEYS = 65536
FLICKER_PALETTE = ((0, 0, 0), (255, 0, 0), (255, 200, 0), (0, 90, 255), (128, 128, 128))     # RGB of codes 0..4 (4, grey: occluded, with the occlusion option only); 0,0,0 = the overlay keeps the frame
OCC_ALPHA, OCC_BETA = 0.01, 0.5


def table_sizes(num_classes, nkeys, occlusion=False):
    """cells of (conf, prev_size, cur_size, same, misc) as they lie in one int64 block; occlusion=True: the masked cell behind them"""
    sizes = [(num_classes + 1) ** 2, nkeys, nkeys, nkeys, 2]
    return sizes + [1] if occlusion else sizes


def _iou_mean(inter, union):
    iou = np.zeros(len(union), dtype=np.float64)
    nz = union > 0
    iou[nz] = inter[nz].astype(np.float64) / union[nz].astype(np.float64)
    n = int(nz.sum())
    return (float(iou[nz].sum() / n) if n else 0.0), iou, n


def tc_from_tables(conf, prev_size, cur_size, same, misc, masked=None):
    """One pair's, one video's or one set's tables -> {'tc', 'tc_sem', 'tc_track', 'n_classes', 'n_tracks', 'class_iou', 'class_inter',
    'class_union' [C], 'track_iou', 'track_union' [n], 'in_view', 'outside'}. conf [C+1][C+1], the others [n], misc [2], integers.
    masked (the occlusion option's cell, [1]): also 'occluded' and 'occluded_share' (of in_view + outside + occluded)."""
    conf = np.asarray(conf, dtype=np.int64)
    if conf.ndim == 1:                                   # as it lies in a block of tables
        conf = conf.reshape(math.isqrt(len(conf)), -1)
    C = conf.shape[0] - 1
    assert conf.shape == (C + 1, C + 1) and C >= 1
    prev_size, cur_size, same = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (prev_size, cur_size, same))
    assert len(prev_size) == len(cur_size) == len(same)
    misc = np.asarray(misc, dtype=np.int64).reshape(2)
    inter = np.diag(conf)[:C].copy()
    union = (conf.sum(1) + conf.sum(0))[:C] - inter
    tc_sem, class_iou, n_classes = _iou_mean(inter, union)
    t_union = prev_size + cur_size - same
    tc_track, track_iou, n_tracks = _iou_mean(same, t_union)
    out = {'tc': math.sqrt(tc_sem * tc_track), 'tc_sem': tc_sem, 'tc_track': tc_track, 'n_classes': n_classes, 'n_tracks': n_tracks,
           'class_iou': class_iou, 'class_inter': inter, 'class_union': union, 'track_iou': track_iou, 'track_union': t_union,
           'in_view': int(misc[0]), 'outside': int(misc[1])}
    if masked is not None:
        occ = int(np.asarray(masked, dtype=np.int64).reshape(1)[0])
        out.update(occluded=occ, occluded_share=_share(occ, out['in_view'] + out['outside']))
    return out


def _share(in_view, outside):
    return in_view / (in_view + outside) if in_view + outside else 0.0


class TcStats:
    """Host side of the evaluation: collects the downloaded tables of every video and turns them into the result. No device."""

    def __init__(self, seg_class, num_classes):
        self.seg_class = np.ascontiguousarray(np.asarray(seg_class, dtype=np.uint8).reshape(-1))
        if len(self.seg_class) != 256:
            raise ValueError('seg_class is uint8 [256], one class index per pan_seg value; got %d entries' % len(self.seg_class))
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError('TC takes 1..%d classes, got %r' % (MAX_CLASSES, num_classes))
        self.num_classes = int(num_classes)
        self.videos = []

    def add_tables(self, video_id, keys, conf, prev_size, cur_size, same, misc, pairs=None, masked=None):
        """one video's tables; `pairs`: None or the video's per-pair tables, int64 [npairs][cells] in the order of `table_sizes`;
        `masked`: None or the masked cell of a video counted with the occlusion option (`pairs` then has that cell too) - all videos
        of a set with it or none"""
        C, keys = self.num_classes, np.asarray(keys, dtype=np.uint16).reshape(-1)
        conf = np.asarray(conf, dtype=np.int64).reshape(C + 1, C + 1)
        occ = masked is not None
        if self.videos and occ != ('occluded' in self.videos[0]):
            raise ValueError('a set is counted with the occlusion option or without it, not both')
        st = tc_from_tables(conf, prev_size, cur_size, same, misc, masked)
        st.update(video=len(self.videos) if video_id is None else video_id, keys=keys, conf=conf, prev_size=np.asarray(prev_size, dtype=np.int64),
                  cur_size=np.asarray(cur_size, dtype=np.int64), same=np.asarray(same, dtype=np.int64), pairs=None)
        if pairs is not None:
            pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, sum(table_sizes(C, len(keys), occ)))
            st['pairs'] = [tc_from_tables(*np.split(row, np.cumsum(table_sizes(C, len(keys), occ))[:-1])) for row in pairs]
        self.videos.append(st)
        return st

    def result(self):
        """{'tc', 'tc_sem', 'tc_track', 'n_classes', 'n_tracks', 'in_view', 'outside', 'in_view_share', 'conf' (the summed matrix), 'per_class':
        [{'class', 'iou', 'inter', 'union'}], 'per_video': [{'video', 'tc', 'tc_sem', 'tc_track', 'n_tracks', 'in_view_share'}], 'tracks': [{'video',
        'key', 'pan_seg', 'id', 'iou', 'same', 'prev_size', 'cur_size'}] (every listed key with pixels, per video in ascending key),
        'per_pair': [{'video', 'pair', 'tc', 'tc_sem', 'tc_track', 'in_view_share'}] (videos counted with per-pair tables)}:
        plain Python numbers, lists and strings, so that it survives JSON unchanged. A set counted with the occlusion option: also
        'occluded' and 'occluded_share' (of all pixels), 'occluded_share' in every 'per_video' and 'per_pair' row, and every
        'in_view_share' is the share of all pixels too (in_view / (in_view + outside + occluded))"""
        C = self.num_classes
        conf = np.zeros((C + 1, C + 1), dtype=np.int64)
        same, union, in_view, outside = [], [], 0, 0
        per_video, tracks, per_pair = [], [], []
        occ = bool(self.videos) and 'occluded' in self.videos[0]
        occluded = 0
        with_occ = lambda row, t: dict(row, in_view_share=_share(t['in_view'], t['outside'] + t['occluded']), occluded_share=t['occluded_share']) if occ else row
        for st in self.videos:
            conf += st['conf']; in_view += st['in_view']; outside += st['outside']; occluded += st.get('occluded', 0)
            same.append(st['same']); union.append(st['track_union'])
            per_video.append(with_occ({'video': st['video'], 'tc': st['tc'], 'tc_sem': st['tc_sem'], 'tc_track': st['tc_track'], 'n_tracks': st['n_tracks'],
                                       'in_view_share': _share(st['in_view'], st['outside'])}, st))
            for k in np.nonzero(st['track_union'] > 0)[0]:
                key = int(st['keys'][k])
                tracks.append({'video': st['video'], 'key': key, 'pan_seg': key >> 8, 'id': key & 255, 'iou': float(st['track_iou'][k]),
                               'same': int(st['same'][k]), 'prev_size': int(st['prev_size'][k]), 'cur_size': int(st['cur_size'][k])})
            for i, p in enumerate(st['pairs'] or []):
                per_pair.append(with_occ({'video': st['video'], 'pair': i + 1, 'tc': p['tc'], 'tc_sem': p['tc_sem'], 'tc_track': p['tc_track'],
                                          'in_view_share': _share(p['in_view'], p['outside'])}, p))
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        tot = tc_from_tables(conf, [], [], [], [in_view, outside])                              # the classes of the summed matrix
        tc_track, _, n_tracks = _iou_mean(cat(same), cat(union))                                # the tracks of all videos together
        res = {'tc': math.sqrt(tot['tc_sem'] * tc_track), 'tc_sem': tot['tc_sem'], 'tc_track': tc_track, 'n_classes': tot['n_classes'],
               'n_tracks': n_tracks, 'in_view': in_view, 'outside': outside, 'in_view_share': _share(in_view, outside), 'conf': conf.tolist(),
               'per_class': [{'class': c, 'iou': float(tot['class_iou'][c]), 'inter': int(tot['class_inter'][c]), 'union': int(tot['class_union'][c])}
                             for c in range(C)],
               'per_video': per_video, 'tracks': tracks, 'per_pair': per_pair}
        if occ:
            res.update(in_view_share=_share(in_view, outside + occluded), occluded=occluded, occluded_share=_share(occluded, in_view + outside))
        return res


def tc_text(result):
    """the text of tc.txt: the set's TC / TC_sem / TC_track x100 with the number of tracks and the in-view share, the per-class IoU
    rows, the per-video rows. A result of the occlusion option (it has 'occluded_share'): one more column, OCC, the occluded share x100"""
    if 'occluded_share' in result:
        return _tc_text_occ(result)
    out = []
    out.append('=' * 56 + '\n')
    out.append('{:10s}| {:>5s}  {:>6s}  {:>8s} {:>5s} {:>7s}\n'.format('', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW'))
    out.append('-' * 56 + '\n')
    row = '{:10s}| {:5.1f}  {:6.1f}  {:8.1f} {:5d} {:7.2f}\n'
    out.append(row.format('All', 100 * result['tc'], 100 * result['tc_sem'], 100 * result['tc_track'], result['n_tracks'], 100 * result['in_view_share']))
    out.append('{:4s}| {:>5s} {:>11s} {:>11s}\n'.format('IDX', 'IoU', 'INTER', 'UNION'))
    for r in result['per_class']:
        out.append('{:4d}| {:5.1f} {:11d} {:11d}\n'.format(r['class'], 100 * r['iou'], r['inter'], r['union']))
    out.append('{:10s}| {:>5s}  {:>6s}  {:>8s} {:>5s} {:>7s}\n'.format('VIDEO', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW'))
    for r in result['per_video']:
        out.append(row.format(str(r['video']), 100 * r['tc'], 100 * r['tc_sem'], 100 * r['tc_track'], r['n_tracks'], 100 * r['in_view_share']))
    return ''.join(out)


def _tc_text_occ(result):
    """`tc_text` with the OCC column"""
    out = []
    out.append('=' * 64 + '\n')
    out.append('{:10s}| {:>5s}  {:>6s}  {:>8s} {:>5s} {:>7s} {:>7s}\n'.format('', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW', 'OCC'))
    out.append('-' * 64 + '\n')
    row = '{:10s}| {:5.1f}  {:6.1f}  {:8.1f} {:5d} {:7.2f} {:7.2f}\n'
    out.append(row.format('All', 100 * result['tc'], 100 * result['tc_sem'], 100 * result['tc_track'], result['n_tracks'], 100 * result['in_view_share'],
                          100 * result['occluded_share']))
    out.append('{:4s}| {:>5s} {:>11s} {:>11s}\n'.format('IDX', 'IoU', 'INTER', 'UNION'))
    for r in result['per_class']:
        out.append('{:4d}| {:5.1f} {:11d} {:11d}\n'.format(r['class'], 100 * r['iou'], r['inter'], r['union']))
    out.append('{:10s}| {:>5s}  {:>6s}  {:>8s} {:>5s} {:>7s} {:>7s}\n'.format('VIDEO', 'TC', 'TC_sem', 'TC_track', 'N', 'INVIEW', 'OCC'))
    for r in result['per_video']:
        out.append(row.format(str(r['video']), 100 * r['tc'], 100 * r['tc_sem'], 100 * r['tc_track'], r['n_tracks'], 100 * r['in_view_share'],
                              100 * r['occluded_share']))
    return ''.join(out)


def tc_tracks_json(result):
    """the content of tc-tracks.json: every track with its IoU and sizes, the per-pair series, the summed class matrix and the counts
    ('occluded' and 'occluded_share' too for a result of the occlusion option)"""
    doc = {'tc': result['tc'], 'tc_sem': result['tc_sem'], 'tc_track': result['tc_track'], 'in_view': result['in_view'], 'outside': result['outside'],
           'in_view_share': result['in_view_share'], 'conf': result['conf'], 'tracks': result['tracks'], 'per_pair': result['per_pair']}
    if 'occluded_share' in result:
        doc.update(occluded=result['occluded'], occluded_share=result['occluded_share'])
    return doc


def flicker_colour(flicker):
    """the inconsistency map uint8 [H,W] (device) painted with `FLICKER_PALETTE`: RGB uint8 [H,W,3] for `render_overlay`, where 0,0,0
    (agreement) keeps the frame"""
    lut = torch.tensor(FLICKER_PALETTE, dtype=torch.uint8, device=flicker.device)
    return lut[flicker.to(torch.int64)]


def _flow_layout(f, device):
    """(tensor kept alive, ld): a dense NHWC view [H,W,2] of a wider map (stride W*ld, ld, 1) is used where it lies"""
    t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 2):
        raise ValueError('flow as fp32 [H,W,2], got %s %s' % (getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
    t = t.to(device)
    sh, sw, sc = t.stride()
    if not (sc == 1 and sw >= 2 and sh == sw * t.shape[1]):
        t = t.contiguous()
    return t, int(t.stride(1))


def flow_occlusion(fwd, back, alpha=OCC_ALPHA, beta=OCC_BETA, out=None, counts=None):
    """The forward-backward check of the module docstring (`vps_flow_occlusion`, csrc/flow_occ_ops.hip; no CPU path). fwd, back: device
    fp32 [H,W,2] tensors (a view of a wider NHWC map is read where it lies), fwd on the grid of cur pointing into prev, back on the grid
    of prev pointing into cur. -> the device uint8 [H,W] mask: 0 visible, 1 occluded, 2 not in view (`out` if given: contiguous).
    counts: None or a device int64 [3] tensor the call ADDS the number of pixels of each code to. On the current stream, nothing is
    downloaded or synchronised."""
    if not (torch.is_tensor(fwd) and fwd.is_cuda and torch.is_tensor(back) and back.is_cuda):
        raise hip.VpsHipError('flow_occlusion runs on the device (vps_flow_occlusion); there is no CPU path')
    dev = fwd.device
    fwd, fld = _flow_layout(fwd, dev)
    back, bld = _flow_layout(back, dev)
    H, W = int(fwd.shape[0]), int(fwd.shape[1])
    if (int(back.shape[0]), int(back.shape[1])) != (H, W):
        raise ValueError('both flows must have equal H, W: fwd %s, back %s' % (tuple(fwd.shape), tuple(back.shape)))
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (H, W)):
        raise ValueError('out is a contiguous device uint8 [H,W] tensor')
    if counts is not None and not (torch.is_tensor(counts) and counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()
                                   and counts.numel() == 3):
        raise ValueError('counts is a contiguous device int64 [3] tensor')
    hip.check(hip.load().vps_flow_occlusion(hip.ptr(fwd), fld, 0, hip.ptr(back), bld, 0, H, W, float(alpha), float(beta), hip.ptr(out),
                                            hip.ptr(counts), hip.stream_ptr()), 'vps_flow_occlusion')
    return out


class TcEvaluator(TcStats):
    """The device side. `add_video(maps, flows)` counts one video into tables that stay on the device until its last pair is enqueued
    (`vps_tc_accumulate` per pair, no synchronisation between pairs, ONE download per video). per_pair=True: the video gets
    [npairs][cells] tables and every pair its own slice (still one download); the video's tables are their sum and `result()['per_pair']`
    is the series that shows where a clip flickers. `add_pair` / `end_video` are the same in steps, for a caller that releases each flow
    once its pair is counted. id_channel 2 = pan_obj (video maps), 1 = pan_ins. The keys default to the thing keys that
    `vps_segment_stats_ch` finds in the video's maps (`video_keys`): class not 255 and, with id_last_stuff (PanopticUnifier's), a
    class above it, else an id > 0.
    occlusion=True (module docstring): every pair needs its backward flow (`add_pair(.., back_flow=)`, `add_video(.., back_flows=)`);
    the pair's mask is made by `vps_flow_occlusion` with (alpha, beta) and the pair is counted by `vps_tc_accumulate_masked`. Every
    table row has one more cell (`table_sizes(C, n, occlusion=True)`), still one download per video.
    photometric=THR (with occlusion=True only; vps_amd/flowphoto.py): every pair also needs its two frames
    (`add_pair(.., frames=(prev_bgr, cur_bgr))`, `add_video(.., frames=)`); between the two launches above the pair's mask goes through
    `vps_flow_photo` in place, which turns the visible in-view pixels whose photometric warp error is above THR grey levels into code 3,
    so they are left out of the counts as well: the flow that is wrong but self-consistent in both directions. The tables keep their
    layout; the masked cell (`occluded`) then holds occluded plus flagged pixels.
    census=THR[, census_eps=] (with occlusion=True only): the same with `vps_flow_census` in the place of
    `vps_flow_photo` - the visible in-view pixels whose ternary census residual is above THR percent become code 3, which brightness
    changes do not trigger. It takes the two frames of every pair as photometric= does and may be combined with it: the absolute pass
    runs first, then the census in place."""

    def __init__(self, seg_class, num_classes, id_channel=2, device='cuda', per_pair=False, id_last_stuff=None, occlusion=False, alpha=OCC_ALPHA,
                 beta=OCC_BETA, photometric=None, census=None, census_eps=None):
        super().__init__(seg_class, num_classes)
        if census is not None and not occlusion:
            raise ValueError('census= flags pixels in the mask of the occlusion option: it needs occlusion=True')
        if census is None and census_eps is not None:
            raise ValueError('census_eps= belongs to census=')
        self.census = self.census_eps = self._census = None
        if census is not None:
            from .flowphoto import CENSUS_EPS, _census_args
            self.census, self.census_eps = _census_args(census, CENSUS_EPS if census_eps is None else census_eps)
        if photometric is not None and not occlusion:
            raise ValueError('photometric= flags pixels in the mask of the occlusion option: it needs occlusion=True')
        if photometric is not None and not float(photometric) >= 0:
            raise ValueError('photometric is a threshold in grey levels, not negative, got %r' % (photometric,))
        self.photometric = None if photometric is None else float(photometric)
        self._photo = None
        if id_channel not in (1, 2):
            raise ValueError('id_channel is 1 or 2, got %r' % (id_channel,))
        if not (alpha >= 0 and beta >= 0):
            raise ValueError('alpha and beta are not negative, got %r, %r' % (alpha, beta))
        self.id_channel, self.per_pair, self.id_last_stuff = int(id_channel), bool(per_pair), id_last_stuff
        self.occlusion, self.alpha, self.beta = bool(occlusion), float(alpha), float(beta)
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise hip.VpsHipError('TcEvaluator counts on the device (vps_tc_accumulate); there is no CPU path and no device is present')
        self.lib = hip.load()
        self._stats = None
        self._open = None

    def _map(self, m):
        t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
        if not (t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3):
            raise ValueError('unified map as uint8 [H,W,3], got %s %s' % (t.dtype, tuple(t.shape)))
        return t.to(self.device).contiguous()

    def _flow(self, f):
        """(tensor kept alive, flow_ld): a dense NHWC view [H,W,2] of a wider map (stride W*ld, ld, 1) is used where it lies"""
        return _flow_layout(f, self.device)

    def video_keys(self, maps):
        """sorted unique uint16 keys of the thing segments of `maps` (one `vps_segment_stats_ch` per map, one download)"""
        present = torch.zeros(65536, dtype=torch.bool, device=self.device)
        if self._stats is None:
            self._stats = torch.empty(65536 * 5, dtype=torch.int32, device=self.device)
        for m in maps:
            t = self._map(m)
            hip.check(self.lib.vps_segment_stats_ch(hip.ptr(t), int(t.shape[0]), int(t.shape[1]), self.id_channel, hip.ptr(self._stats),
                                                    hip.stream_ptr()), 'vps_segment_stats_ch')
            present |= self._stats.view(65536, 5)[:, 0] > 0
        keys = torch.nonzero(present).flatten().cpu().numpy()
        sel = (keys >> 8) != 255
        sel &= ((keys & 255) > 0) if self.id_last_stuff is None else ((keys >> 8) > self.id_last_stuff)
        return keys[sel].astype(np.uint16)

    def _begin(self, keys, npairs):
        keys = np.unique(np.asarray(keys, dtype=np.int64).reshape(-1))
        if len(keys) and not (0 <= keys[0] and keys[-1] < MAX_KEYS):
            raise ValueError('keys are pan_seg * 256 + id, 0 .. 65535')
        keys = keys.astype(np.uint16)
        cells = sum(table_sizes(self.num_classes, len(keys), self.occlusion))
        self._open = dict(keys=keys, d_keys=torch.from_numpy(keys.view(np.int16)).to(self.device) if len(keys) else None, cells=cells,
                          tables=[torch.zeros((npairs if self.per_pair else 1, cells), dtype=torch.int64, device=self.device)] if npairs else [],
                          npairs=0)

    def _slice(self):
        o = self._open
        if not self.per_pair:
            if not o['tables']:
                o['tables'].append(torch.zeros((1, o['cells']), dtype=torch.int64, device=self.device))
            return o['tables'][0][0]
        rows = sum(int(t.shape[0]) for t in o['tables'])
        if o['npairs'] >= rows:                          # pairs added one by one: rows in blocks, still one download per video
            o['tables'].append(torch.zeros((16, o['cells']), dtype=torch.int64, device=self.device))
            rows += 16
        i = o['npairs']
        for t in o['tables']:
            if i < t.shape[0]:
                return t[i]
            i -= int(t.shape[0])

    def _frame(self, f, H, W):
        t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
        if not (torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (H, W, 3)):
            raise ValueError('frames are uint8 [%d,%d,3] like the maps, got %s %s' % (H, W, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
        return t.to(self.device).contiguous()

    def add_pair(self, prev, cur, flow, keys=None, flicker=None, back_flow=None, frames=None):
        """count one pair into the open video (opened by the first pair; `keys` then fixes the video's list, None = the thing keys of
        these two maps). flicker: None or a device uint8 [H,W] tensor that receives the inconsistency map. back_flow: the flow from
        prev to cur, fp32 [H,W,2] - required by an evaluator with occlusion=True, refused by one without. frames: (prev_bgr, cur_bgr),
        the two frames as uint8 [H,W,3] - required by an evaluator with photometric=, refused by one without. Nothing is downloaded."""
        census = getattr(self, 'census', None)
        if (self.photometric is not None or census is not None) != (frames is not None):
            raise ValueError('photometric= and census= need the two frames of every pair (frames=(prev_bgr, cur_bgr))' if frames is None
                             else 'frames are given but the evaluator was made without photometric= or census=')
        if self.occlusion != (back_flow is not None):
            raise ValueError('occlusion=True needs the backward flow of every pair (back_flow=)' if self.occlusion
                             else 'back_flow is given but the evaluator was made without occlusion=True')
        prev, cur = self._map(prev), self._map(cur)
        flow, ld = self._flow(flow)
        H, W = int(cur.shape[0]), int(cur.shape[1])
        if self.occlusion:
            back_flow, bld = self._flow(back_flow)
            if (int(back_flow.shape[0]), int(back_flow.shape[1])) != (H, W):
                raise ValueError('maps and flows must have equal H, W: cur %s, back_flow %s' % (tuple(cur.shape), tuple(back_flow.shape)))
        if tuple(prev.shape) != tuple(cur.shape) or (int(flow.shape[0]), int(flow.shape[1])) != (H, W):
            raise ValueError('maps and flow must have equal H, W: prev %s, cur %s, flow %s' % (tuple(prev.shape), tuple(cur.shape), tuple(flow.shape)))
        if flicker is not None and not (torch.is_tensor(flicker) and flicker.is_cuda and flicker.dtype == torch.uint8 and flicker.is_contiguous()
                                        and tuple(flicker.shape) == (H, W)):
            raise ValueError('flicker is a contiguous device uint8 [H,W] tensor')
        if frames is not None:
            fprev, fcur = self._frame(frames[0], H, W), self._frame(frames[1], H, W)
        if self._open is None:
            self._begin(self.video_keys([prev, cur]) if keys is None else keys, 0)
        elif keys is not None and not np.array_equal(np.unique(np.asarray(keys)), self._open['keys']):
            raise ValueError('the keys of a video are fixed by its first pair')
        o, C = self._open, self.num_classes
        n = len(o['keys'])
        if self.occlusion:
            conf, psz, csz, same, misc, masked = torch.split(self._slice(), table_sizes(C, n, True))
            mask = torch.empty((H, W), dtype=torch.uint8, device=self.device)      # (stream-ordered: the allocator hands the block on only behind its last use)
            hip.check(self.lib.vps_flow_occlusion(hip.ptr(flow), ld, 0, hip.ptr(back_flow), bld, 0, H, W, self.alpha, self.beta, hip.ptr(mask), None,
                                                  hip.stream_ptr()), 'vps_flow_occlusion')
            if self.photometric is not None:             # in place: the visible pixels that are photometrically wrong become code 3
                nbytes = int(self.lib.vps_flow_photo_ws_bytes(H, W))
                hip.check(min(nbytes, 0), 'vps_flow_photo_ws_bytes')
                if self._photo is None:                  # tables nobody reads: the call wants somewhere to add to
                    self._photo = (torch.zeros(21, dtype=torch.int64, device=self.device), torch.zeros(4, dtype=torch.float64, device=self.device))
                ws = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
                hip.check(self.lib.vps_flow_photo(hip.ptr(fcur), hip.ptr(fprev), H, W, hip.ptr(flow), ld, 0, hip.ptr(mask), self.photometric,
                                                  hip.ptr(self._photo[0]), hip.ptr(self._photo[1]), hip.ptr(mask), None, hip.ptr(ws), nbytes,
                                                  hip.stream_ptr()), 'vps_flow_photo')
            if census is not None:                       # in place as well, behind the absolute pass: code 3 for the visible pixels the census flags
                nbytes = int(self.lib.vps_flow_census_ws_bytes(H, W))
                hip.check(min(nbytes, 0), 'vps_flow_census_ws_bytes')
                if self._census is None:                 # a table nobody reads
                    self._census = torch.zeros(26, dtype=torch.int64, device=self.device)
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
                hip.check(self.lib.vps_flow_census(hip.ptr(fcur), hip.ptr(fprev), H, W, hip.ptr(flow), ld, 0, hip.ptr(mask), census, self.census_eps,
                                                   hip.ptr(self._census), hip.ptr(mask), None, hip.ptr(ws), nbytes, hip.stream_ptr()),
                          'vps_flow_census')
            hip.check(self.lib.vps_tc_accumulate_masked(hip.ptr(prev), hip.ptr(cur), H, W, hip.ptr(flow), ld, 0, self.id_channel,
                                                        self.seg_class.ctypes.data_as(ctypes.c_void_p), C, hip.ptr(o['d_keys']) if n else None, n,
                                                        hip.ptr(conf), hip.ptr(psz) if n else None, hip.ptr(csz) if n else None,
                                                        hip.ptr(same) if n else None, hip.ptr(misc), hip.ptr(flicker), hip.ptr(mask), hip.ptr(masked),
                                                        hip.stream_ptr()), 'vps_tc_accumulate_masked')
            o['npairs'] += 1
            return
        conf, psz, csz, same, misc = torch.split(self._slice(), table_sizes(C, n))
        hip.check(self.lib.vps_tc_accumulate(hip.ptr(prev), hip.ptr(cur), H, W, hip.ptr(flow), ld, 0, self.id_channel,
                                             self.seg_class.ctypes.data_as(ctypes.c_void_p), C, hip.ptr(o['d_keys']) if n else None, n, hip.ptr(conf),
                                             hip.ptr(psz) if n else None, hip.ptr(csz) if n else None, hip.ptr(same) if n else None, hip.ptr(misc),
                                             hip.ptr(flicker), hip.stream_ptr()), 'vps_tc_accumulate')
        o['npairs'] += 1

    def end_video(self, video_id=None):
        """the one download (and synchronisation) of the open video; returns its entry (`tc_from_tables` of its tables and the tables)"""
        o, C = self._open, self.num_classes
        assert o is not None, 'no video is open'
        self._open = None
        host = np.zeros((0, o['cells']), dtype=np.int64)
        if o['tables']:
            host = (torch.cat(o['tables']) if len(o['tables']) > 1 else o['tables'][0]).cpu().numpy()
        host = host[:o['npairs'] if self.per_pair else 1]
        pairs = host if self.per_pair else None
        total = host.sum(0)
        parts = np.split(total, np.cumsum(table_sizes(C, len(o['keys']), self.occlusion))[:-1])
        return self.add_tables(video_id, o['keys'], *parts[:5], pairs=pairs, masked=parts[5] if self.occlusion else None)

    def add_video(self, maps, flows, video_id=None, keys=None, flickers=None, back_flows=None, frames=None):
        """maps: the unified maps of one video in order, uint8 [H,W,3] host arrays or device tensors; flows: one per map, flows[t] the
        flow of frame t to frame t-1, fp32 [H,W,2] (flows[0] is not used and may be None); flickers: None or one device uint8 [H,W]
        tensor (or None) per map; back_flows (occlusion=True): one per map, back_flows[t] the flow of frame t-1 to frame t (the first
        is not used); frames (photometric=): one uint8 [H,W,3] frame per map. Returns the video's entry."""
        assert self._open is None, 'a video opened by add_pair is not ended'
        if len(flows) != len(maps):
            raise ValueError('one flow per map (the first is not used): %d maps, %d flows' % (len(maps), len(flows)))
        if self.occlusion != (back_flows is not None) or (back_flows is not None and len(back_flows) != len(maps)):
            raise ValueError('occlusion=True takes one backward flow per map (the first is not used), an evaluator without it takes none')
        if (self.photometric is not None or getattr(self, 'census', None) is not None) != (frames is not None) or \
                (frames is not None and len(frames) != len(maps)):
            raise ValueError('photometric= and census= take one frame per map, an evaluator without them takes none')
        maps = [self._map(m) for m in maps]
        self._begin(self.video_keys(maps) if keys is None else keys, max(len(maps) - 1, 0))
        for t in range(1, len(maps)):                    # no synchronisation between pairs
            kw = dict(back_flow=back_flows[t]) if self.occlusion else {}
            if frames is not None:
                kw['frames'] = (frames[t - 1], frames[t])
            self.add_pair(maps[t - 1], maps[t], flows[t], flicker=None if flickers is None else flickers[t], **kw)
        return self.end_video(video_id)

    def result(self):
        assert self._open is None, 'a video opened by add_pair is not ended'
        return super().result()


def score_videos(evaluator, maps, flows, names, nframes_per_video, map_dir=None, frames=None, alpha=128, quality=90, entropy='host', back_flows=None):
    """What `--tc` of the tools does with a run's unified maps (host or device, videos one after the other, `nframes_per_video` each) and
    the flows kept for them (`flows[i]` = `pano_results['flow']` of frame i): every video through `add_pair`, one download per video.
    `flows` is EMPTIED as it goes - entry i is set to None once its pair is counted (a video's first frame at once), so each flow
    lives on the device only until then. map_dir (`--tc-map`): the inconsistency map of every pair, painted with `FLICKER_PALETTE`,
    blended over `frames[i]` (BGR uint8 [H,W,3]) by `render_overlay` and written as map_dir/<name>.jpg by a `DeviceJpegWriter`.
    back_flows (an evaluator with occlusion=True): `back_flows[i]` = `flow_between(ref_img, img)` of frame i, emptied entry by entry as
    `flows` is; occluded pixels are grey in the inconsistency maps. An evaluator with photometric= gets `frames[i - 1]` and `frames[i]`
    with every pair (`frames` is then required); the flagged pixels are grey too. Returns the written file names."""
    from .postprocess import DeviceJpegWriter, overlay_name, render_overlay, video_name_of
    assert len(maps) == len(flows) == len(names) and (map_dir is None or (frames is not None and len(frames) == len(maps)))
    assert back_flows is None or len(back_flows) == len(maps)
    photo = getattr(evaluator, 'photometric', None) is not None or getattr(evaluator, 'census', None) is not None
    assert not photo or (frames is not None and len(frames) == len(maps))
    writer = DeviceJpegWriter(evaluator.device, quality=quality, entropy=entropy) if map_dir is not None else None
    out = []
    try:
        for v0 in range(0, len(maps), nframes_per_video):
            vm = [evaluator._map(m) for m in maps[v0:v0 + nframes_per_video]]
            keys = evaluator.video_keys(vm)
            flows[v0] = None
            if back_flows is not None:
                back_flows[v0] = None
            for j in range(1, len(vm)):
                fl = torch.empty(vm[j].shape[:2], dtype=torch.uint8, device=evaluator.device) if writer is not None else None
                if back_flows is None:
                    evaluator.add_pair(vm[j - 1], vm[j], flows[v0 + j], keys=keys, flicker=fl)
                else:
                    kw = dict(frames=(frames[v0 + j - 1], frames[v0 + j])) if photo else {}
                    evaluator.add_pair(vm[j - 1], vm[j], flows[v0 + j], keys=keys, flicker=fl, back_flow=back_flows[v0 + j], **kw)
                    back_flows[v0 + j] = None
                flows[v0 + j] = None
                if writer is not None:
                    out.append(overlay_name(map_dir, names[v0 + j]))
                    writer.submit(render_overlay(frames[v0 + j], flicker_colour(fl), alpha), out[-1])
            if len(vm) > 1:
                evaluator.end_video(video_name_of(names[v0:v0 + nframes_per_video], v0 // nframes_per_video))
    finally:
        if writer is not None:
            writer.close()
    return out


def write_outputs(result, out_dir):
    """tc.txt and tc-tracks.json in `out_dir`"""
    import json
    import os
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'tc.txt'), 'w') as f:
        f.write(tc_text(result))
    with open(os.path.join(out_dir, 'tc-tracks.json'), 'w') as f:
        json.dump(tc_tracks_json(result), f, indent=1)
