"""PanopticFuseTrack on libvpship — the drop-in for mmdet/models/detectors/panoptic_fusetrack.py (inference path).

Same registry name, constructor kwargs (configs/cityscapes/fusetrack.py model dict), `state_dict` key families,
call signature `model(return_loss=False, rescale=True, img=[T], img_meta=[[meta]], ref_img=[T])` and return
structure `(bbox_results, mask_results, pano_results)` as the reference, so tools/test_vpq.py:129-149,46-63 runs
unchanged. Everything below the Python glue is a HIP kernel call through the C-ABI; there is no torch.nn compute
and no CPU fallback.

MI355X-first differences (results identical by construction):
  * activations are NHWC slices of persistent concat buffers; BN/bias/activation/residual fused into the convs;
  * the reference-frame features are NOT recomputed: frame t's gathered pre-neck feature is frame t-1's (cached);
  * fcn_output [1,19,H,W], mask_energy/seg_inst/panoptic_logits [1,k,H,W] are never materialised;
  * track-memory embeddings are cached instead of re-running the track FCs on all stored RoI features each frame.
"""
import os
import os.path as osp
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import hip, nhwc, panoptic_ops
from . import registry as R
from .base import HipModule
from .flownet2 import FlowNet2
from .panoptic_ops import MaskRemoval, MaskROI, panoptic_combine

# The announcement board (round 6): the (img, ref_img) device-tensor pairs of the frames that FOLLOW the one the next `simple_test`
# call is made with, posted by a caller-side component that knows them when the call itself cannot say (`vps_amd.dataloader.
# LookaheadLoader` around the unmodified tools/test_vpq.py loop). `simple_test(..., prefetch=None)` reads it as its `prefetch`.
_BOARD = []


def announce(pairs):
    """pairs: list of (img, ref_img) tensors in frame order (at most two are used); [] clears the board"""
    _BOARD[:] = [(a, b) for a, b in pairs][:2]



def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def bbox2result(bboxes, labels, num_classes):
    """core/bbox/transforms.py:142-157: per-class list of [n, 5] arrays"""
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes - 1)]
    bboxes = _np(bboxes); labels = _np(labels)
    return [bboxes[labels == i, :] for i in range(num_classes - 1)]


def bbox2result_with_id(bboxes, labels, obj_ids, num_classes):
    """core/bbox/transforms.py:159-180"""
    if bboxes.shape[0] == 0:
        return dict()
    bboxes = _np(bboxes); labels = _np(labels)
    return {obj_id: {'bbox': bbox, 'label': label} for bbox, label, obj_id in zip(bboxes, labels, obj_ids) if obj_id >= 0}


@R.DETECTORS.register_module
class PanopticFuseTrack(HipModule):
    # the two sibling detectors of the reference reuse this class with one branch switched off (bottom of the file)
    with_fusion = True        # FlowNet2 + flow-guided BFP-TCEA temporal fusion neck (panoptic_fusetrack.py:506-518)
    keep_flow = False         # True: pano_results['flow'] = the frame's full-resolution FlowNet2 flow, device fp32 [h,w,2] (flowvis.py)
    with_track = True         # TrackHead + instance-id assignment (panoptic_fusetrack.py:400-469)

    def __init__(self, backbone, rpn_head, bbox_roi_extractor, bbox_head, mask_roi_extractor, mask_head, train_cfg,
                 test_cfg, neck=None, extra_neck=None, panoptic=None, track_head=None, shared_head=None, pretrained=None,
                 flownet_checkpoint=None):
        super().__init__()
        assert shared_head is None
        # attribute names follow two_stage.py:31-64 (they are the state_dict prefixes)
        self.backbone = R.build_backbone(backbone)
        self.neck = R.build_neck(neck)
        self.extra_neck = R.build_extra_neck(extra_neck) if self.with_fusion else None
        assert (extra_neck is not None) == self.with_fusion and (track_head is not None) == self.with_track, \
            '%s: extra_neck / track_head do not match the detector type' % type(self).__name__
        self.panopticFPN = R.build_panoptic(panoptic)
        self.rpn_head = R.build_head(rpn_head)
        self.bbox_roi_extractor = R.build_roi_extractor(bbox_roi_extractor)
        self.bbox_head = R.build_head(bbox_head)
        self.track_head = R.build_head(track_head) if self.with_track else None
        self.mask_roi_extractor = R.build_roi_extractor(mask_roi_extractor)
        self.mask_head = R.build_head(mask_head)
        self.train_cfg = R.ConfigDict.wrap(train_cfg) if train_cfg is not None else None
        self.test_cfg = R.ConfigDict.wrap(test_cfg) if test_cfg is not None else None
        if self.train_cfg is not None and hasattr(self.train_cfg, 'class_mapping'):
            self.class_mapping = self.train_cfg['class_mapping']
        elif self.test_cfg is not None and hasattr(self.test_cfg, 'class_mapping'):
            self.class_mapping = self.test_cfg['class_mapping']
        else:
            self.class_mapping = {1: 11, 2: 12, 3: 13, 4: 14, 5: 15, 6: 16, 7: 17, 8: 18}
        self.class_mapping = {int(k): int(v) for k, v in dict(self.class_mapping).items()}
        self.mask_roi_panoptic = MaskROI(clip_boxes=True, bbox_class_agnostic=False, top_n=100,
                                         num_classes=self.panopticFPN.num_things_classes + 1, nms_thresh=0.5,
                                         class_agnostic=True, score_thresh=0.6)
        self.mask_removal = MaskRemoval(fraction_threshold=0.3)
        has_flow = (self.train_cfg is not None and hasattr(self.train_cfg, 'flownet2')) or \
                   (self.test_cfg is not None and hasattr(self.test_cfg, 'flownet2'))
        self.mean = [123.675, 116.28, 103.53]
        self.std = [58.395, 57.12, 57.375]
        self.flownet2 = None
        if self.with_fusion:
            assert has_flow, 'Feature flow must be implemented.'

            class _Args(object):
                rgb_max = 255.0
                fp16 = False
            self.flownet2 = FlowNet2(_Args())
            # panoptic_fusetrack.py:100-106: FlowNet2 weights come from a separate cwd-relative file, loaded in __init__;
            # load_checkpoint(model, latest.pth) afterwards may overwrite flownet2.* keys (kept: same order).
            ck = flownet_checkpoint or osp.join(os.getcwd(), 'work_dirs', 'flownet', 'FlowNet2_checkpoint.pth.tar')
            if osp.exists(ck):
                self.flownet2.load_state_dict(torch.load(ck, map_location='cpu')['state_dict'])
            else:
                warnings.warn('FlowNet2 checkpoint %s not found: flownet2.* keeps its initial weights until a state_dict is loaded' % ck)
        self.CLASSES = None
        # options
        self.reuse_ref_features = True     # False: recompute extract_feat(ref_img) every frame like the reference
        self.verify_ref_frame = True       # check that ref_img IS the previous call's img before reusing its features
        self.int64_outputs = False         # True: panoptic/semantic maps as int64 like the reference (uint8 values otherwise)
        self.profile = None                # set to {} to collect per-stage hip events (stages then run on one stream)
        self.overlap_streams = True        # independent branches of the frame on two HIP streams, + a prefetch stream (see simple_test)
        self._side = None
        # image-only stages of the NEXT frame: 1 = one prefetch stream (FlowNet2, then ResNet + FPN + gather), 2 = ResNet + FPN + gather
        # on a stream of their own beside FlowNet2, 3 = FlowNetSD beside the FlowNetC -> S -> S chain as well. The branches are
        # independent (they share the input images only), every one of them has long runs of low-resolution layers that launch fewer
        # workgroups than the chip has CUs, and the convolutions are latency- not throughput-bound: side by side they
        # fill each other's gaps. Bitwise the serial schedule (tests/test_fusetrack_gpu.py).
        self.pre_streams = int(os.environ.get('VPS_PRE_STREAMS', '3'))
        # 1: the frame's main chain (neck, heads, the host reads) runs on a HIGH-priority stream of the detector's own, so that its
        # short kernels are not queued behind the prefetched frame's workgroups (A/B switch, off by default)
        self.main_priority = os.environ.get('VPS_MAIN_PRIO', '0') != '0'
        self._hp = None
        self._sd = None
        # 1: ResNet + FPN of the frame after next are enqueued in front of the end-of-frame read instead of behind the neck (they then
        # carry the GPU across the frame boundary: idle 0.57 -> 0.28 ms in the traced frame) - measured SLOWER untraced (52.6 against
        # 53.2 frames/s in one call: they compete with the next frame's neck): off
        self.defer_backbone = os.environ.get('VPS_DEFER_BACKBONE', '0') != '0'
        self._pre_aux = []                 # the extra prefetch streams (pre_streams > 1)
        self._pre = None                   # prefetch stream + its ring of workspaces (clip pipelines)
        self._ring = None
        self._lane = None
        self._slot = 0
        self._ws = None
        self._between_ws = None
        self._flip = 0
        self._cache = None
        self._handoff = None
        self._pf = None
        self.reset_tracker()

    # ------------------------------------------------------------------------------------------------------
    def reset_tracker(self):
        self.prev_bboxes = None
        self.prev_emb = None
        self.prev_det_labels = None
        self._mem_n = 0              # memory entries (host view; exact after every end-of-frame read)
        self._mem_count = None       # the same number on the device, written by vps_track_assign

    def pack(self, device):
        for m in (self.backbone, self.neck, self.extra_neck, self.panopticFPN, self.rpn_head, self.bbox_head,
                  self.track_head, self.mask_head, self.flownet2):
            if m is not None:
                m.ensure_packed(device)
        self._mean_t = torch.tensor(self.mean, dtype=torch.float32, device=device)
        self._std_t = torch.tensor(self.std, dtype=torch.float32, device=device)

    def _mark(self, name):
        if self.profile is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.profile.setdefault('events', []).append((name, ev))

    def stage_times_ms(self):
        """after a frame with self.profile = {}: [(stage, ms)] from the hip events (caller must synchronize first)"""
        ev = self.profile.get('events', [])
        return [(ev[i + 1][0], ev[i][1].elapsed_time(ev[i + 1][1])) for i in range(len(ev) - 1)]

    # ------------------------------------------------------------------------------------------------------
    def extract_feat(self, img):
        """reference API (NCHW in, tuple of NCHW FPN levels out)"""
        ws = nhwc.Workspace(img.device)
        ws.pooling = False                 # one-off API call: plain buffers
        lv = self.neck.run(self.backbone.run(nhwc.from_nchw(img), ws, 'bb.'), ws, 'fpn.')
        return tuple(l.to_nchw() for l in lv)

    def compute_flow(self, img, ref_img, scale_factor=1):
        """panoptic_fusetrack.py:117-143 (NCHW API). Returns (flow [1,2,h,w], None)."""
        ws = nhwc.Workspace(img.device)
        ws.pooling = False
        self.ensure_packed(img.device)
        flow = self.flownet2.run(img, ref_img, self._mean_t, self._std_t, ws)
        if scale_factor != 1:
            Ho, Wo = int(flow.H * scale_factor), int(flow.W * scale_factor)
            flow = nhwc.resize(flow, ws.fmap('flow_s', 1, Ho, Wo, 2), 'bilinear', scale_factor)
        return flow.to_nchw(), None

    @torch.no_grad()
    def flow_between(self, a, b, img_shape=None):
        """FlowNet2 on the pair (a, b): NCHW [1,3,H,W] normalised device tensors, as the detector gets them (a list holding one is
        taken as that one). -> device fp32 [h,w,2], a contiguous copy of the caller's own: the flow on the grid of `a` that points into
        `b` (b sampled at p + flow(p) lies over a(p)), cropped to img_shape[:2] (a frame's img_meta['img_shape']: without the
        Pad-to-32 rows) when that is given. `pano_results['flow']` of a frame (`keep_flow`) is flow_between(img, ref_img);
        flow_between(ref_img, img) is the backward flow of that pair, what the occlusion option of vps_amd.tc needs.
        Call it after the frame's `model(...)` call. It runs on the current stream, in a workspace and a block pool of its own and
        under buffer names of its own, so it touches nothing of the detector's schedule: not the prefetch records, not the ring or
        lane workspaces, not the addresses the main workspace's temporaries get. The price is a second set of FlowNet2 buffers
        (`workspace_bytes` counts them) and one more FlowNet2 pass per call."""
        if not self.with_fusion:
            raise hip.VpsHipError('flow_between: %s computes no optical flow (no FlowNet2 on its path)' % type(self).__name__)
        a = a[0] if isinstance(a, (list, tuple)) else a
        b = b[0] if isinstance(b, (list, tuple)) else b
        if not (a.is_cuda and b.is_cuda):
            raise hip.VpsHipError('PanopticFuseTrack runs on the device only (no CPU path)')
        if a.shape != b.shape:
            raise ValueError('flow_between takes two images of one size, got %s and %s' % (tuple(a.shape), tuple(b.shape)))
        dev = a.device
        self.ensure_packed(dev)
        if self._between_ws is None or self._between_ws.device != dev:
            self._between_ws = nhwc.Workspace(dev)
        flow = self.flownet2.run(a, b, self._mean_t, self._std_t, self._between_ws, tag='between.fn2.')
        h, w = (flow.H, flow.W) if img_shape is None else (int(img_shape[0]), int(img_shape[1]))
        return flow.t[0, :h, :w, flow.coff:flow.coff + 2].clone(memory_format=torch.contiguous_format)

    # ------------------------------------------------------------------------------------------------------
    def forward(self, img, img_meta, return_loss=True, **kwargs):
        if return_loss:
            raise NotImplementedError('vps_amd implements the inference path (return_loss=False) only')
        return self.forward_test(img, img_meta, **kwargs)

    def forward_test(self, imgs, img_metas, **kwargs):
        """base.py:79-97: single-scale, batch 1"""
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        if len(imgs) != len(img_metas) or len(imgs) != 1:
            raise ValueError('only single-scale testing (1 augmentation) is on the path')
        assert imgs[0].size(0) == 1
        return self.simple_test(imgs[0], img_metas[0], **kwargs)

    @torch.no_grad()
    def simple_test(self, img, img_meta, proposals=None, rescale=False, ref_img=None, inject=None, ref_feature=None,
                    defer_tracking=False, prefetch=None):
        """panoptic_fusetrack.py:502-606 (see `_simple_test_once`). f16x3 arithmetic only: a layer that staged an activation
        beyond the fp16 range (|x| > 65504; reported per layer through vps_conv_desc.status, read with the frame's end-of-frame
        read) is switched to bf16x6 for good and the frame is computed again from the state it started in — no exception, no
        wrong result; `nhwc.F16_FALLBACKS` counts the switched layers."""
        if self.main_priority and img.is_cuda and self.overlap_streams and self.profile is None:
            # the whole call on the detector's high-priority stream, ordered behind / in front of the caller's stream
            cur = torch.cuda.current_stream(img.device)
            if self._hp is None or self._hp.device != img.device:
                self._hp = torch.cuda.Stream(device=img.device, priority=-1)
            if cur != self._hp:
                self._hp.wait_stream(cur)
                try:
                    with torch.cuda.stream(self._hp):
                        return self._simple_test_guarded(img, img_meta, proposals, rescale, ref_img, inject, ref_feature, defer_tracking, prefetch)
                finally:
                    cur.wait_stream(self._hp)
        return self._simple_test_guarded(img, img_meta, proposals, rescale, ref_img, inject, ref_feature, defer_tracking, prefetch)

    def _simple_test_guarded(self, img, img_meta, proposals, rescale, ref_img, inject, ref_feature, defer_tracking, prefetch):
        if self.keep_flow and (not self.with_fusion or (inject is not None and 'neck_out' in inject)):
            raise hip.VpsHipError('keep_flow: %s computes no optical flow (no FlowNet2 on its path)'
                                  % (type(self).__name__ if not self.with_fusion else 'a frame with an injected neck output'))
        if img.is_cuda:
            self.ensure_packed(img.device)      # a lazily packed model registers its f16x3 layers here: `guard` must see them
        guard = nhwc._F16_NEXT[0] > 1 and img.is_cuda
        if self._mem_n is None:
            # an exception between the tracker kernels and the end-of-frame read of an earlier call left the host's view of the memory
            # size unset: the device word is authoritative
            self._mem_n = int(self._mem_count.item()) if self._mem_count is not None else 0
        for attempt in range(4):
            snap = self._tracker_snapshot() if guard and self.with_track and not defer_tracking else None
            out = self._simple_test_once(img, img_meta, proposals, rescale, ref_img, inject, ref_feature, defer_tracking,
                                         prefetch if attempt == 0 else None)
            if out is not None:
                return out
            nhwc.f16_fallback(img.device)
            # back to the state the frame started in: tracker memory, no cached / prefetched features (they may come from the
            # layer that overflowed: the reference-frame features are recomputed like the reference does)
            if snap is not None:
                self._tracker_restore(snap)
            pf, self._pf = self._pf, None
            for r in pf or []:
                self._finish_backbone(r)
                r['event'].synchronize()
                if r['event2'] is not None:
                    r['event2'].synchronize()
            self._cache = None
            self._handoff = None
        raise hip.VpsHipError('f16x3: the frame still overflows the fp16 range after three rounds of per-layer bf16x6 fallback')

    def _tracker_snapshot(self):
        if self.prev_emb is None or not self._mem_n:
            return (0, None, None, None)
        M = self._mem_n
        return (M, self.prev_emb[:M].clone(), self.prev_bboxes[:M].clone(), self.prev_det_labels[:M].clone())

    def _tracker_restore(self, snap):
        M, emb, box, lab = snap
        self._mem_n = M
        if M:
            self.prev_emb[:M] = emb; self.prev_bboxes[:M] = box; self.prev_det_labels[:M] = lab
            self._mem_count.fill_(M)

    def _simple_test_once(self, img, img_meta, proposals=None, rescale=False, ref_img=None, inject=None, ref_feature=None,
                          defer_tracking=False, prefetch=None):
        """panoptic_fusetrack.py:502-606. `inject` (tests/bench only): dict overriding head inputs at the operator
        boundaries of SURVEY §8d config 2 (fcn_score, proposals, cls_score, bbox_pred, mask_score).
        ref_feature / defer_tracking (clip_shard.py): gathered pre-neck feature of the previous frame received from the
        neighbouring GPU, and postponing the sequential id assignment to the clip-level replay.
        prefetch (clip pipelines): (next_img, next_ref_img), the device tensors the NEXT call will be made with. Their
        FlowNet2 + ResNet/FPN/gather — which depend on the images alone — are enqueued on a third (prefetch) stream, into a ring
        of private workspaces, BEFORE this frame's neck: they run beside this frame's neck, semantic head and detection heads
        and keep the GPU fed while the host waits for this frame's two small reads. The next call picks the results up (matched
        by tensor identity); outputs are bitwise those of the unpipelined schedule."""
        assert proposals is None
        if not img.is_cuda:
            raise hip.VpsHipError('PanopticFuseTrack runs on the device only (no CPU path)')
        if prefetch is None and _BOARD and inject is None:
            prefetch = [p for p in _BOARD if p[0].is_cuda and p[0].device == img.device and p[0].shape == img.shape] or None        # (module docstring of dataloader.py)
        dev = img.device
        self.ensure_packed(dev)
        ws = self._workspace(dev)
        if self.profile is not None:
            self.profile['events'] = []
        self._mark('start')
        if ref_img is not None and isinstance(ref_img, (list, tuple)):
            ref_img = ref_img[0]
        meta = img_meta[0]
        if self.with_track:
            # (the reference's check that it is fed Cityscapes-VPS frames; a clip that has no such file names says so: meta['dataset'])
            assert ('city' in meta['filename'] or meta.get('dataset') == 'cityscapes_vps') and 'iid' in meta
        iid = meta.get('iid', -1)          # PanopticFuse runs on image pairs without a video index
        is_first = (iid % 10000) == 1
        _, _, H, W = img.shape
        im_info = np.array([[float(H), float(W), 1.0]])

        # Two independent pairs of branches run on two HIP streams (self.overlap_streams): FlowNet2 || backbone+FPN (both need
        # only the images) and semantic head || RPN + box/track/mask heads (both need only the neck output). Their
        # low-resolution layers launch fewer workgroups than the chip has CUs; side by side they fill it. Every branch is
        # enqueued completely before the next one starts (the host only waits inside the detection branch), the side
        # stream is ordered after the main stream at the fork and the main stream after the side stream at the join.
        main, side = None, None
        if self.overlap_streams and self.profile is None:
            main = torch.cuda.current_stream(dev)
            if self._side is None or self._side.device != dev:
                self._side = torch.cuda.Stream(device=dev)
            side = self._side
        flow = cat = aux = levels = kept_flow = None
        late = []
        if inject is not None and 'neck_out' in inject:
            # tests: the neck output itself is injected (five NCHW levels) — the image-only stages and the neck are skipped
            x = [nhwc.from_nchw(l.to(dev), ws, 'inj.neck%d' % i) for i, l in enumerate(inject['neck_out'])]
        elif not self.with_fusion:
            # PanopticTrack (panoptic_track.py:447): the FPN outputs feed the heads directly
            with ws.scope():
                levels = self.neck.run(self.backbone.run(nhwc.from_nchw(img, ws, 'img_nhwc'), ws, 'bb.'), ws, 'fpn.')
            x = levels
            self._mark('backbone_fpn')
        else:
            pending, self._pf = self._pf or [], None
            late = []
            pf = None
            if side is not None:
                # (1) flow + (2) backbone / FPN / gather of THIS frame: enqueued on the prefetch streams during an earlier call
                # (matched by tensor identity), or now - through the same machinery (the image-stage streams, the lane workspace
                # whose temporaries all ring slots share, a ring slot for the outputs), ahead of the announced frames'.
                # `prefetch`: one (next_img, its ref) pair or a list of them in frame order. The FIRST announced frame is enqueued
                # here, at the start of the call; a SECOND one behind this frame's neck, so that the GPU has the next
                # frames' image-only stages queued through the tail of this frame and across the frame boundary (round 5: the
                # frame's last third ran on one or two streams and the boundary was a 0.2 - 0.3 ms bubble; ring of three slots: frame t+2 goes where frame t-1 was, whose
                # gathered feature neck(t) has read by then).
                # (the same storage in the same state: a scatter that re-wraps a device tensor keeps the match; a record holds its
                # tensors, so an address cannot be re-used by another frame while the record waits)
                same = lambda r, a, b: (r['img'].data_ptr() == a.data_ptr() and r['ref'].data_ptr() == b.data_ptr() and r['img'].shape == a.shape
                                        and r['version'] == (a._version, b._version))
                announced = [] if prefetch is None else ([prefetch] if torch.is_tensor(prefetch[0]) else list(prefetch))
                pf = next((r for r in pending if same(r, img, ref_img)), None)
                keep = [r for r in pending if r is not pf and any(same(r, a, b) for a, b in announced)]
                for r in pending:
                    if r is not pf and r not in keep:
                        # an unused prefetch (the caller announced other tensors than it now passes): the prefetch streams may still be
                        # reading those tensors, which the caller is now free to rewrite on the main stream - so the main stream orders
                        # itself behind them. Its results sit in a ring slot nobody reads.
                        self._finish_backbone(r)
                        main.wait_event(r['event'])
                        if r['event2'] is not None:
                            main.wait_event(r['event2'])
                # (ring slots a new frame must not take: those of the records this call still consumes - `busy` - and the one that
                # holds the cached reference feature neck(t) reads, `_enqueue_image_stages`)
                if pf is None:
                    pf = self._enqueue_image_stages(img, ref_img, main, busy=keep)
                is_pending = lambda a, b: any(same(r, a, b) for r in keep)
                if announced and not is_pending(*announced[0]):
                    keep.append(self._enqueue_image_stages(announced[0][0], announced[0][1], main, busy=[pf] + keep))       # the NEXT frame: now
                late = [(a, b) for a, b in announced[1:2] if not is_pending(a, b)]                        # the one after: before the tail read
                self._pf = keep or None
                self._finish_backbone(pf)                 # (a record whose backbone was deferred and never placed: now)
                main.wait_event(pf['event'])
                if pf['event2'] is not None:
                    main.wait_event(pf['event2'])
                flow, levels, cat = pf['flow'], pf['levels'], pf['cat']
                self._mark('flownet2')
            else:
                for r in pending:
                    self._finish_backbone(r)
                    r['event'].synchronize()
                    if r['event2'] is not None:
                        r['event2'].synchronize()
                # one stream (profiling, overlap_streams off): the serial schedule in the main workspace
                flow = self.flownet2.run(img, ref_img, self._mean_t, self._std_t, ws)
                self._mark('flownet2')
                levels, cat = self._backbone_fpn_gather(img, ws)
            C = self.extra_neck.in_channels
            # flowR2T = F.interpolate(flow, 0.25, bilinear) * 0.25 written straight into the LiteFlowNet input buffer
            nhwc.resize(flow, cat.window(C + 81, 2), 'bilinear', 0.25)
            if self.keep_flow:
                # a copy of its own, made on the frame's stream: the flow lives in a ring workspace that the frame after next rewrites.
                # Cropped to the image: without the Pad-to-32 rows (FlowNet2.run has already trimmed its own 64-multiple padding)
                kept_flow = flow.t[0, :meta['img_shape'][0], :meta['img_shape'][1], flow.coff:flow.coff + 2].clone(memory_format=torch.contiguous_format)
            self._mark('backbone_fpn')
            # reference-frame gathered feature: cached from the previous call when the frames are consecutive
            cache = self._cache
            if ref_feature is not None:
                ref_bsf = nhwc.FMap(ref_feature.view(1, cat.H, cat.W, C))
            elif (self.reuse_ref_features and iid >= 0 and cache is not None and cache['iid'] + 1 == iid and not is_first and cache['shape'] == (H, W)
                  and self._same_frame(ref_img, cache['probe'])):
                ref_bsf = cache['cat'].window(0, C)
            elif self.reuse_ref_features and iid >= 0 and is_first:
                ref_bsf = cat.window(0, C)        # datasets/cityscapes_vps.py:137-148: the first frame's ref is itself
            else:
                with ws.scope():
                    rl = self.neck.run(self.backbone.run(nhwc.from_nchw(ref_img, ws, 'ref_nhwc'), ws, 'rbb.'), ws, 'rfpn.')
                ref_bsf = self.extra_neck.gather(rl, ws, 'neck.refcat').window(0, C)
                self._mark('ref_backbone_fpn')
            self._cache = dict(iid=iid, cat=cat, shape=(H, W), probe=self._probe(img), slot=None if pf is None else pf.get('slot'))
            # (3) temporal fusion neck -------------------------------------------------------------------------------
            x, aux = self.extra_neck.run(levels, cat, ref_bsf, ws, 'neck.')
            self._mark('extra_neck')
        # (4) semantic head --------------------------------------------------------------------------------------
        sem_done = None
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                fcn_score = self.panopticFPN.run(x[0:self.panopticFPN.num_levels], ws)
                sem_done = torch.cuda.Event()
                sem_done.record(side)
        else:
            fcn_score = self.panopticFPN.run(x[0:self.panopticFPN.num_levels], ws)
        if inject is not None and 'fcn_score' in inject:
            fcn_score = nhwc.from_nchw(inject['fcn_score'].to(dev), ws, 'inj.fcn_score')
        self._mark('semantic_head')
        if self.with_fusion and late and main is not None:
            # the frame after next (see `prefetch` above): its image-only stages go out HERE, behind the neck - the prefetch streams
            # order themselves behind what the main stream holds now (the neck: the last reader of the ring slot they rewrite) and then
            # run beside everything that follows: the RPN / box head / MaskROI chain of mostly single-workgroup kernels, the two host
            # reads, the mask head, MaskRemoval's dependency chain, the combine and the next call's first launches - the two thirds of
            # a frame in which the GPU had least to do (idle 0.72 -> 0.38 ms per traced frame, profiles/r05_frame_occupancy_traced.json)
            # ... FlowNet2 (the long chain) here; its ResNet + FPN + gather (~4 ms on one stream) are placed in front of the end-of-frame read
            # instead: they carry the GPU across the frame boundary (host read, result assembly, the next call's first launches)
            # (the neck is enqueued: the slot of the OLD cached feature is free again; `_cache` already names this frame's slot)
            self._pf = (self._pf or []) + [self._enqueue_image_stages(late[0][0], late[0][1], main, defer_backbone=self.defer_backbone)]
        # (5) RPN ------------------------------------------------------------------------------------------------
        nprop = None                          # device int32 [1]: rows of `proposals` that exist (None = all)
        if inject is not None and 'proposals' in inject:
            proposals = inject['proposals'].to(dev)
        else:
            proposals, nprop = self.rpn_head.run(x, ws, meta['img_shape'], self.test_cfg.rpn)
        self._mark('rpn')
        # (6) bbox head + MaskROI + tracking ---------------------------------------------------------------------
        det = self.simple_test_bboxes(x, meta, proposals, im_info, is_first, ws, inject, defer_tracking, nprop)
        self._mark('bbox_track')

        det_bboxes, det_labels = det['det_bboxes'], det['det_labels']
        cls_prob, mask_rois, cls_idx = det['cls_prob'], det['det_rois'], det['cls_idx']
        mask_results = [[] for _ in range(self.mask_head.num_classes - 1)]       # simple_test_mask: `or True` stub
        # (8) mask head ------------------------------------------------------------------------------------------
        mask_feats = self.mask_roi_extractor.run(x, mask_rois)
        logits = self.mask_head.run(mask_feats, ws)
        nc = self.mask_head.num_classes
        if inject is not None and 'mask_score' in inject:
            # a bank of >= K rows: the number of detections is decided by MaskROI
            all_scores = inject['mask_score'][:mask_rois.size(0)].to(dev).permute(0, 2, 3, 1).contiguous()       # [K,28,28,nc]
        else:
            all_scores = logits.t[..., :nc]
        S = all_scores.shape[1]
        mask_score = all_scores.gather(3, cls_idx.view(-1, 1, 1, 1).expand(-1, S, S, 1)).squeeze(3).contiguous()
        self._mark('mask_head')
        # (9)-(11) MaskRemoval + SegTerm + combine: the kept list stays on the device -------------------------------
        last = self.mask_roi_panoptic.last
        K = mask_rois.size(0)
        has_ids = self.with_track and not defer_tracking
        for mr_try in (0, 1):
            # second pass only after an expired dependency wait of the one-launch MaskRemoval (below): the per-level launches
            removal = self.mask_removal(last['rows_h'], last['rows_d'], mask_score, (H, W), ws, self.class_mapping, force_level=mr_try == 1)
            if side is not None:
                main.wait_event(sem_done)  # the combine kernel reads fcn_score; MaskRemoval's dependency chain above does not: it may
                                           # run beside the end of the semantic head (prefetched work behind the event is not waited for)
            pan, sem = panoptic_combine(fcn_score, removal, mask_score, self.panopticFPN.num_stuff_classes, self.panopticFPN.num_classes,
                                        (H, W), ws)
            h0, w0 = meta['img_shape'][0], meta['img_shape'][1]
            pan = pan[:, 0:h0, 0:w0].clone(); sem = sem[:, 0:h0, 0:w0].clone()     # fresh tensors: the workspace is reused next frame
            if self.int64_outputs:
                pan, sem = pan.long(), sem.long()
            self._mark('panoptic_combine')
            # ---- the frame's END-OF-FRAME host read: kept list, ids, tracker memory size, fp16-range words (one D2H) ----------
            tail = ws.get('frame.tail', (2 * MaskROI.KCAP + 8,), dtype=torch.int32, zero=False)
            for r in self._pf or []:
                self._finish_backbone(r)
            st16 = nhwc.f16_status(dev)
            hip.check(hip.load().vps_frame_tail(hip.ptr(removal['kinfo']), hip.ptr(removal['keep']), hip.ptr(det['ids_dev']) if has_ids else None,
                                                hip.ptr(self._mem_count) if has_ids else None, hip.ptr(st16), st16.numel(), K, MaskROI.KCAP,
                                                hip.ptr(tail), hip.stream_ptr()), 'vps_frame_tail')
            th = tail.cpu().numpy()
            if th[5]:
                return None              # f16x3: a layer overflowed the fp16 range -> simple_test falls back and recomputes the frame
            k, masks_valid, cstat = int(th[0]), bool(th[1]), int(th[2])
            if cstat & 1:
                raise hip.VpsHipError('vps_panoptic_combine: %d kept instances do not fit the uint8 panoptic map (at most %d)'
                                      % (k, 255 - self.panopticFPN.num_stuff_classes))
            if not (cstat & 4):
                break
            # vps_mask_removal_dep: a box gave up waiting for a box it depends on (bounded spin: a wedged GPU is not an option - the
            # API promises neither the dispatch order nor progress of the lower workgroups while three prefetch streams hold the CUs).
            # The kept list of that pass is not valid: MaskRemoval + combine + the read are repeated through the per-level launches,
            # which need no cross-workgroup waits (nothing else of the frame depends on them; `panoptic_ops.MR_RECOVERIES` counts)
            if mr_try == 1:
                raise hip.VpsHipError('MaskRemoval: status %d from the per-level launches' % cstat)
            panoptic_ops.MR_RECOVERIES[0] += 1
        keep_inds = th[8:8 + k].astype(np.int64)
        det_obj_ids = None
        if has_ids:
            det_obj_ids = th[8 + MaskROI.KCAP:8 + MaskROI.KCAP + K].astype(np.int64)
            self._mem_n = int(th[4])
        det['det_obj_ids'] = det_obj_ids
        keep_t = removal['keep'][:k].long()
        # boxes / labels of the result lists come from the host copy of the detection list (no further D2H)
        boxes_h = last['rows_h'][:, 1:5].astype(np.float32); labels_h = last['rows_h'][:, 6].astype(np.int64) - 1
        if not self.with_track:
            bbox_results = bbox2result(boxes_h, labels_h, self.bbox_head.num_classes)      # panoptic_fuse.py:425-426
        else:
            ids_out = np.full((K,), -1, dtype=np.int64) if defer_tracking else det_obj_ids
            bbox_results = bbox2result_with_id(boxes_h, labels_h, ids_out, self.bbox_head.num_classes)
        pano_results = {
            'fcn_outputs': sem,
            'panoptic_cls_inds': cls_idx[keep_t],
            'panoptic_cls_prob': cls_prob[keep_t],
            'panoptic_outputs': pan,
        }
        if self.with_track:                                    # panoptic_fuse.py:467-472 returns the four keys above only
            pano_results['panoptic_det_labels'] = det_labels[keep_t]
            ids_t = det['ids_dev'][:K].long() if has_ids else torch.full((K,), -1, dtype=torch.long, device=dev)
            pano_results['panoptic_det_obj_ids'] = ids_t[keep_t]
        if self.keep_flow:
            pano_results['flow'] = kept_flow
        self._track_record = dict(det_bboxes=det_bboxes, det_labels=det_labels, cls_prob=cls_prob, emb=det['emb'],
                                  keep_inds=keep_inds)
        self._aux = dict(flow=flow, levels=levels, cat=cat, neck_out=x, neck_aux=aux, fcn_score=fcn_score, det=det,
                         mask_score=mask_score, keep_inds=keep_inds, proposals=proposals[:last['nrois']], masks_valid=masks_valid)
        return bbox_results, mask_results, pano_results

    # ------------------------------------------------------------------------------------------------------
    def _workspace(self, dev):
        """main workspace (neck, heads, results), the LANE workspace of the image-only stages (FlowNet2, ResNet + FPN: their persistent
        internals - the zero-padded concat buffers - exist once, not once per ring slot) and the ring of three OUTPUT workspaces
        (flow, FPN levels, gathered feature of a prefetched frame). One block pool (per stream) serves all of them."""
        if self._ws is None or self._ws.device != dev:
            self._ws = nhwc.Workspace(dev)
            self._lane = nhwc.Workspace(dev, pool=self._ws.pool)
            self._ring = [nhwc.Workspace(dev, pool=self._ws.pool) for _ in range(3)]
        return self._ws

    def workspace_bytes(self):
        """device bytes held by the detector's workspaces: persistent buffers of the main / lane / ring workspaces + the block pool"""
        if self._ws is None:
            return 0
        between = 0 if self._between_ws is None else self._between_ws.nbytes() + self._between_ws.pool.total
        return sum(w.nbytes() for w in [self._ws, self._lane] + self._ring) + self._ws.pool.total + between

    def _enqueue_image_stages(self, nimg, nref, main, defer_backbone=False, busy=()):
        """The image-only stages (FlowNet2, ResNet + FPN + gather) of a frame go to the prefetch streams: for the frame the NEXT call
        will be made with, before anything of the current frame is enqueued, so they run beside the current frame's neck and heads, not
        behind its semantic head - they are the longest chain (~16 ms of the frame's ~22 ms of kernel time) and the main / side
        streams fill the CUs their low-resolution layers leave idle. With `pre_streams` > 1 the chain itself is split over independent
        streams (ResNet + FPN + gather beside FlowNet2, FlowNetSD beside FlowNetC -> S -> S). Internals live in the lane workspace
        (shared by all frames: a prefetch stream runs one frame after the other), outputs in a ring of three: slot (t+1) % 3 was last
        written for frame t-2, whose flow / levels were read by neck(t-2) and whose gathered feature was last read by neck(t-1) as
        ref_bsf - both enqueued on the main stream in earlier calls, which the waits below order every prefetch stream behind. The
        images may have been produced on the main stream too. Every auxiliary stream is joined into the first one before the event the
        consumer waits for is recorded. -> the record the consuming call matches by tensor identity.
        defer_backbone: only FlowNet2 (the long chain) is enqueued now; ResNet + FPN + gather of that frame follow with
        `_finish_backbone` - the caller places them where the GPU would otherwise run dry (the end of the current frame). They wait for
        an EVENT recorded on the main stream now, not for whatever the main stream holds when they are enqueued."""
        dev = nimg.device
        self._workspace(dev)
        if self._pre is None or self._pre.device != dev:
            self._pre = torch.cuda.Stream(device=dev)
            self._pre_aux = [torch.cuda.Stream(device=dev) for _ in range(2)]
        self._pre.wait_stream(main)
        # the next ring slot that nothing still reads: not the slot of a record that waits for its consumer (`self._pf`, `busy` = the
        # records the running call holds), and not the slot whose gathered feature is the cached reference feature the next neck reads
        # (`_cache`: the prefetch streams are ordered behind what the main stream holds NOW - a neck enqueued later is not in that).
        # The announced-clip schedule never finds its slot taken (ring of three: frame t+2 goes where frame t-1 was, behind neck(t));
        # a caller whose announcements do not match what it passes can enqueue three frames in one call - the ring then grows.
        taken = {r.get('slot') for r in list(self._pf or []) + list(busy) if r is not None}
        if self._cache is not None:
            taken.add(self._cache.get('slot'))
        n = len(self._ring)
        slot = next(((self._slot + i) % n for i in range(1, n + 1) if (self._slot + i) % n not in taken), None)
        if slot is None:
            self._ring.append(nhwc.Workspace(dev, pool=self._ws.pool))
            slot = n
        self._slot = slot
        lws = self._lane.with_out(self._ring[self._slot])
        bb_stream = self._pre_aux[0] if self.pre_streams >= 2 else self._pre
        sd_stream = self._pre_aux[1] if self.pre_streams >= 3 else None
        defer_backbone = defer_backbone and bb_stream is not self._pre
        rec = dict(img=nimg, ref=nref, version=(nimg._version, nref._version), levels=None, cat=None, event2=None, bb_pending=None, slot=self._slot)
        if defer_backbone:
            after = torch.cuda.Event()
            after.record(main)
            rec['bb_pending'] = (lws, after)
        elif bb_stream is not self._pre:
            bb_stream.wait_stream(main)
            with torch.cuda.stream(bb_stream):
                rec['levels'], rec['cat'] = self._backbone_fpn_gather(nimg, lws, ring=True)
        with torch.cuda.stream(self._pre):
            rec['flow'] = self.flownet2.run(nimg, nref, self._mean_t, self._std_t, lws, sd_stream=sd_stream)
            if bb_stream is self._pre:
                rec['levels'], rec['cat'] = self._backbone_fpn_gather(nimg, lws, ring=True)
            elif not defer_backbone:
                self._pre.wait_stream(bb_stream)
            ev = torch.cuda.Event()
            ev.record(self._pre)
        rec['event'] = ev
        return rec

    def _finish_backbone(self, rec):
        """ResNet + FPN + gather of a record whose backbone was deferred (`_enqueue_image_stages(defer_backbone=True)`)"""
        if rec.get('bb_pending') is None:
            return
        lws, after = rec['bb_pending']
        rec['bb_pending'] = None
        bb_stream = self._pre_aux[0]
        bb_stream.wait_event(after)
        with torch.cuda.stream(bb_stream):
            rec['levels'], rec['cat'] = self._backbone_fpn_gather(rec['img'], lws, ring=True)
            rec['event2'] = torch.cuda.Event()
            rec['event2'].record(bb_stream)

    @torch.no_grad()
    def prime(self, img, ref_img):
        """Enqueue the image-only stages of the frame the next `simple_test(img, ..., ref_img=ref_img)` call will process, now: a rank
        that owns a later shard of a clip (clip_shard.py) calls this BEFORE it waits for the previous rank's feature hand-off, so
        its first frame's FlowNet2 + ResNet / FPN run while the hand-off is in flight instead of behind it. No-op without the
        stream schedule (profiling, overlap_streams off) or without the fusion neck."""
        if not (self.with_fusion and self.overlap_streams and self.profile is None and img.is_cuda):
            return False
        self.ensure_packed(img.device)
        pf, self._pf = self._pf, None
        for r in pf or []:
            self._finish_backbone(r)
            r['event'].synchronize()
            if r['event2'] is not None:
                r['event2'].synchronize()
        self._pf = [self._enqueue_image_stages(img, ref_img, torch.cuda.current_stream(img.device))]
        return True

    def _sd_stream(self, dev):
        """the stream FlowNetSD runs on beside the FlowNetC -> S -> S chain of an UNprefetched frame (first frame of a clip, a caller
        that owns the loop); None with fewer than three image-stage streams"""
        if self.pre_streams < 3:
            return None
        if self._sd is None or self._sd.device != dev:
            self._sd = torch.cuda.Stream(device=dev)
        return self._sd

    @staticmethod
    def _probe(img):
        """a 3 x 16 x 32 strided sample of a frame (device tensor, no sync): the fingerprint `reuse_ref_features` checks"""
        return img[0, :, ::max(img.shape[2] // 16, 1), ::max(img.shape[3] // 32, 1)].clone()

    def _same_frame(self, ref_img, probe):
        """is `ref_img` the frame whose features are cached? The reference's test dataset guarantees it (ref = previous frame,
        cityscapes_vps.py:137-148) but a custom caller may pass any pair: compare the strided sample (one tiny D2H at the start of
        the frame, when the main stream is idle). On a mismatch the reference features are recomputed like the reference does."""
        if not self.verify_ref_frame:
            return True
        p = self._probe(ref_img)
        return p.shape == probe.shape and bool(torch.equal(p, probe))

    def _backbone_fpn_gather(self, img, ws, ring=False):
        """ResNet + FPN + gather of one frame -> (levels, cat). In the main workspace the gathered feature alternates between the
        'neck.catA' / 'neck.catB' buffers (frame t's is frame t+1's `ref_bsf`); a slot of the prefetch ring is rewritten every third
        frame only and has ONE buffer (the A/B pair there was 0.4 GB of dead memory at 1024x2048: ADVICE r3)"""
        if ring:
            tag = 'R'
        else:
            self._flip ^= 1
            tag = 'AB'[self._flip]
        pre = self._handoff
        if pre is not None and pre['img'] is img and pre['version'] == img._version:
            # clip sharding: this frame's ResNet+FPN+gather already ran for the hand-off to the next GPU (gathered_feature)
            self._handoff = None
            return pre['levels'], pre['cat']
        with ws.scope():          # the stage outputs C2..C5 (temporaries the backbone leaves to its caller) go back when the levels exist
            levels = self.neck.run(self.backbone.run(nhwc.from_nchw(img, ws, 'img_nhwc'), ws, 'bb.'), ws, 'fpn.')
        return levels, self.extra_neck.gather(levels, ws, 'neck.cat' + tag)

    def gathered_feature(self, img):
        """gather(FPN(ResNet(img))) (bfp_tcea.py:96-109,117): the tensor the NEXT frame needs as ref_bsf; [1,H/4,W/4,C]"""
        dev = img.device
        self.ensure_packed(dev)
        ws = self._workspace(dev)
        with ws.scope():
            lv = self.neck.run(self.backbone.run(nhwc.from_nchw(img, ws, 'ho_nhwc'), ws, 'hbb.'), ws, 'hfpn.')
        cat = self.extra_neck.gather(lv, ws, 'neck.handoff')
        C = self.extra_neck.in_channels
        # kept for this frame's own simple_test call (its buffers have their own workspace names): the sender does not run
        # ResNet+FPN on its last frame twice
        # (matched by tensor IDENTITY: a data_ptr can be recycled by the allocator for a different frame)
        self._handoff = dict(img=img, version=img._version, levels=lv, cat=cat)
        return cat.t[..., :C].contiguous()

    def track_assign(self, rec, is_first):
        """sequential tracker step on a deferred record (clip_shard.py) -> ids (host array: the replay is the consumer)"""
        dev = rec['emb'].device
        ids, _ = self._assign_ids(rec['det_bboxes'], rec['det_labels'], rec['cls_prob'], rec['emb'], is_first, self._workspace(dev))
        K = rec['det_bboxes'].size(0)
        buf = torch.cat([ids[:K], self._mem_count])
        h = buf.cpu().numpy()
        self._mem_n = int(h[K])
        return h[:K].astype(np.int64)

    def _mem_reserve(self, dev, need, E):
        """tracker memory = fixed-capacity device buffers (embeddings [cap,E], boxes [cap,4], labels [cap]); grown by doubling"""
        cap = 0 if self.prev_emb is None else self.prev_emb.size(0)
        if cap >= need and self.prev_emb.device == dev:
            return
        new = max(1024, 2 * cap, need)
        emb = torch.zeros(new, E, device=dev); box = torch.zeros(new, 4, device=dev); lab = torch.zeros(new, dtype=torch.long, device=dev)
        if cap and self._mem_n:
            emb[:self._mem_n] = self.prev_emb[:self._mem_n]; box[:self._mem_n] = self.prev_bboxes[:self._mem_n]
            lab[:self._mem_n] = self.prev_det_labels[:self._mem_n]
        self.prev_emb, self.prev_bboxes, self.prev_det_labels = emb, box, lab

    def _assign_ids(self, det_bboxes, det_labels, cls_prob, emb, is_first, ws):
        """panoptic_fusetrack.py:400-469 (tracking block of simple_test_bboxes), device-resident: the comprehensive scores, their
        row arg-max, the greedy assignment (undo branch included) and the memory update are kernels; ids and the new memory size
        stay on the device (`self._mem_count`) until the frame's end-of-frame read. `self._mem_n` = memory size known to the host
        (it sizes the launches). -> (ids int32 [K] device, comp_scores or None)"""
        lib = hip.load()
        dev = emb.device
        K, E = det_bboxes.size(0), emb.size(1)
        comp_scores = None
        if self._mem_count is None or self._mem_count.device != dev:
            self._mem_count = torch.zeros(1, dtype=torch.int32, device=dev)
        ids = ws.get('trk.ids', (MaskROI.KCAP,), dtype=torch.int32, zero=False)
        if is_first or self.prev_emb is None or self._mem_n == 0:
            self._mem_n = 0
            self._mem_reserve(dev, 2 * K, E)
            ids[:K].copy_(torch.arange(K, dtype=torch.int32, device=dev))
            self.prev_emb[:K] = emb; self.prev_bboxes[:K] = det_bboxes[:, :4]; self.prev_det_labels[:K] = det_labels
            self._mem_n = K
            self._mem_count.fill_(K)
        else:
            M = self._mem_n
            self._mem_reserve(dev, M + K, E)
            pb = self.prev_bboxes[:M]
            match_score = self.track_head.match_scores(emb, self.prev_emb[:M], ws).contiguous()
            match_logprob = torch.empty_like(match_score)
            hip.check(lib.vps_row_softmax(hip.ptr(match_score), hip.ptr(match_logprob), K, M + 1, 1, hip.stream_ptr()), 'log_softmax')
            label_delta = (self.prev_det_labels[:M] == det_labels.view(-1, 1)).float()
            db = det_bboxes.contiguous()
            bbox_ious = torch.empty(K, M, device=dev)
            hip.check(lib.vps_bbox_overlaps(hip.ptr(db), db.shape[1], K, hip.ptr(pb), pb.shape[1], M, hip.ptr(bbox_ious),
                                            hip.stream_ptr()), 'vps_bbox_overlaps')
            comp_scores = self.track_head.compute_comp_scores(match_logprob, cls_prob.view(-1, 1), bbox_ious, label_delta,
                                                              add_bbox_dummy=True).contiguous()
            scratch = ws.get('trk.scratch', (self.prev_emb.size(0) + 3 * MaskROI.KCAP + 1,), dtype=torch.int32, zero=False)
            embc = emb.contiguous(); lab = det_labels.contiguous()
            hip.check(lib.vps_track_assign(hip.ptr(comp_scores), K, M, hip.ptr(embc), E, hip.ptr(db), db.shape[1], hip.ptr(lab),
                                           hip.ptr(self.prev_emb), hip.ptr(self.prev_bboxes), hip.ptr(self.prev_det_labels),
                                           hip.ptr(scratch), hip.ptr(ids), hip.ptr(self._mem_count), hip.stream_ptr()), 'vps_track_assign')
            self._mem_n = None           # unknown to the host until the end-of-frame read (simple_test / track_assign) delivers it
        return ids, comp_scores

    # ------------------------------------------------------------------------------------------------------
    def simple_test_bboxes(self, x, meta, proposals, im_info, is_first, ws, inject=None, defer_tracking=False, nprop=None):
        """panoptic_fusetrack.py:358-471"""
        lib = hip.load()
        dev = proposals.device
        rois = torch.cat([proposals.new_zeros(proposals.size(0), 1), proposals[:, :4]], dim=-1).contiguous()   # bbox2roi
        roi_feats = self.bbox_roi_extractor.run(x, rois)
        cls_score, bbox_pred = self.bbox_head.run(roi_feats, ws)
        if inject is not None and 'cls_score' in inject:
            cls_score, bbox_pred = inject['cls_score'].to(dev).contiguous(), inject['bbox_pred'].to(dev).contiguous()
        cls_prob_all = torch.empty_like(cls_score)
        hip.check(lib.vps_row_softmax(hip.ptr(cls_score), hip.ptr(cls_prob_all), cls_score.shape[0], cls_score.shape[1], 0,
                                      hip.stream_ptr()), 'vps_row_softmax')
        cls_prob, det_rois, cls_idx = self.mask_roi_panoptic(rois, bbox_pred, cls_prob_all, im_info, ws, nprop)
        det_labels = cls_idx - 1
        det_roi_feats = self.bbox_roi_extractor.run(x, det_rois)
        det_bboxes = det_rois[:, 1:]
        ids_dev, comp_scores, emb = None, None, None
        if self.with_track:
            emb = self.track_head.embed(det_roi_feats, ws)
        if self.with_track and not defer_tracking:
            ids_dev, comp_scores = self._assign_ids(det_bboxes, det_labels, cls_prob, emb, is_first, ws)
        return dict(det_bboxes=det_bboxes, det_labels=det_labels, det_obj_ids=None, ids_dev=ids_dev, cls_score=cls_score,
                    bbox_pred=bbox_pred, cls_prob=cls_prob, det_rois=det_rois, cls_idx=cls_idx, comp_scores=comp_scores,
                    det_roi_feats=det_roi_feats, emb=emb)


@R.DETECTORS.register_module
class PanopticFuse(PanopticFuseTrack):
    """mmdet/models/detectors/panoptic_fuse.py: the same path without the track head — per-class box
    lists instead of id-keyed boxes, `pano_results` without `panoptic_det_labels` / `panoptic_det_obj_ids`
    (panoptic_fuse.py:399-472). It runs on image pairs whose reference frame is arbitrary, so the reference-feature cache
    is off by default."""
    with_track = False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.reuse_ref_features = False


@R.DETECTORS.register_module
class PanopticTrack(PanopticFuseTrack):
    """mmdet/models/detectors/panoptic_track.py: no FlowNet2 and no temporal fusion neck — the FPN
    outputs feed the semantic / RPN / box / track / mask heads directly (panoptic_track.py:443-536); tracking as in
    PanopticFuseTrack (the two `simple_test_bboxes` are identical)."""
    with_fusion = False
