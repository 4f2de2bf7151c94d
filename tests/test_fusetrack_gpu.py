"""GPU: end-to-end parity of the HIP PanopticFuseTrack against the CPU oracle and against the golden vectors produced
by the real reference code (tests/golden/fusetrack_clip.npz), on a 3-frame synthetic clip, plus stage-level checks.

Tolerance (fp32 path, exact-fp32 MFMA; differences come from summation order only, amplified through ~100 layers):
  stage tensors: |err| <= 2e-3 * max|ref| (max-norm relative); final maps: identical ids and <= 0.1 % differing pixels
  (argmax flips at exact-tie-level logit differences), identical instance ids / classes.
"""
import os

import numpy as np
import pytest
import torch

import golden_npz
import tolerances as T
import vps_amd
from vps_amd import nhwc, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'fusetrack_clip.npz')


def _relmax(got, ref):
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-12))


@pytest.fixture(scope='module', params=['f32', 'bf16x6', 'f16x3'])
def setup(dev, request):
    """every test of this module runs in ALL fp32-grade arithmetic modes: the exact-fp32 MFMA kernels (library default), the
    split-bf16x6 kernels and the split-fp16x3 kernels (VPS_PREC=bf16x6 / f16x3)"""
    from vps_amd import hip, nhwc
    gold = golden_npz.load(GOLD)
    H, W, n, seed = [int(v) for v in gold['meta']]
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    old = nhwc.DEFAULT_PREC
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[request.param]
    try:
        model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        sd = synth.load_synth(model, seed)
        model.to(dev)
        model.ensure_packed(dev)             # weights are packed under this mode (PackedConv reads DEFAULT_PREC at pack time)
    finally:
        nhwc.DEFAULT_PREC = old
    frames = synth.synth_clip(H, W, n, seed)
    return dict(gold=gold, model=model, sd=sd, frames=frames, H=H, W=W, n=n, dev=dev, prec=request.param)


@pytest.fixture(scope='module')
def oracle_clip():
    """the oracle on the golden clip, computed once for both arithmetic modes"""
    from oracle.fusetrack import FuseTrackOracle
    gold = golden_npz.load(GOLD)
    H, W, n, seed = [int(v) for v in gold['meta']]
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    sd = synth.synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed)
    o = FuseTrackOracle(sd)
    fr = synth.synth_clip(H, W, n, seed)
    ora = []
    with torch.no_grad():
        for t in range(n):
            ora.append(o.simple_test(fr[t], fr[t - 1 if t else 0], t == 0, return_aux=True))
    return ora


@pytest.fixture(scope='module')
def runs(setup, oracle_clip):
    """HIP path (with the cached reference features, the product default) and the oracle on the same clip"""
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W = setup['H'], setup['W']
    hip_res, aux = [], []
    for t in range(setup['n']):
        meta = synth.img_meta(H, W, 10000 + t + 1)
        out = m(return_loss=False, rescale=True, img=[fr[t].to(dev)], img_meta=[[meta]], ref_img=[fr[t - 1 if t else 0].to(dev)])
        torch.cuda.synchronize()
        hip_res.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out[2].items()})
        a = m._aux
        aux.append(dict(flow=a['flow'].to_nchw().cpu(), fpn=[l.to_nchw().cpu() for l in a['levels']],
                        neck=[l.to_nchw().cpu() for l in a['neck_out']], fcn_score=a['fcn_score'].to_nchw().cpu(),
                        proposals=a['proposals'].cpu(), cls_score=a['det']['cls_score'].cpu(), bbox_pred=a['det']['bbox_pred'].cpu(),
                        det_rois=a['det']['det_rois'].cpu(), ids=np.asarray(a['det']['det_obj_ids']), bbox_ids=sorted(out[0].keys())))
    return hip_res, aux, oracle_clip


@pytest.mark.parametrize('t', [0, 1, 2])
def test_stage_tensors_match_oracle(setup, runs, t):
    _, aux, ora = runs
    a, r = aux[t], ora[t]
    # proposals are score-sorted; rows whose scores differ by less than the fp32 noise may swap -> align rows by box
    ph, po = a['proposals'], r['det']['proposals']
    assert ph.shape == po.shape
    # clamped boxes can coincide (several anchors decode to the same clipped box): match on box AND score
    dist = torch.maximum((ph[:, None, :4] - po[None, :, :4]).abs().amax(2), 500.0 * (ph[:, None, 4] - po[None, :, 4]).abs())
    match = dist.argmin(1)
    # an NMS decision with IoU within fp32 noise of the 0.7 threshold may flip: allow <= 1 % unmatched proposals
    dmin = dist.gather(1, match[:, None])[:, 0]
    good = dmin < 0.05
    assert int((~good).sum()) <= ph.shape[0] // 100, 'proposal sets differ: %d unmatched' % int((~good).sum())
    assert float((ph[good, 4] - po[match[good], 4]).abs().max()) < 1e-4
    nswap = int((match != torch.arange(ph.shape[0])).sum())
    errs = dict(
        flow=_relmax(a['flow'], r['flow_full']),
        fpn_p2=_relmax(a['fpn'][0], r['pre_neck'][0]), fpn_p6=_relmax(a['fpn'][4], r['pre_neck'][4]),
        neck_p2=_relmax(a['neck'][0], r['feats'][0]), neck_p6=_relmax(a['neck'][4], r['feats'][4]),
        fcn_score=_relmax(a['fcn_score'], r['fcn_score']),
        cls_score=_relmax(a['cls_score'][good], r['det']['cls_score'][match][good]),
        bbox_pred=_relmax(a['bbox_pred'][good], r['det']['bbox_pred'][match][good]),
    )
    print('[%s] frame %d stage max-norm relative errors: %s (score-tie row swaps: %d)' % (setup['prec'], t, {k: '%.2e' % v for k, v in errs.items()}, nswap))
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    with open(os.path.join(ROOT, 'gpurun_out', 'stage_errors.txt'), 'a') as f:
        f.write('%s frame %d %s swaps %d\n' % (setup['prec'], t, errs, nswap))
    for k, v in errs.items():
        assert v < T.stage_tol(k), (k, v, errs)


@pytest.mark.parametrize('t', [0, 1, 2])
def test_outputs_match_oracle_and_reference_golden(setup, runs, t):
    hip_res, aux, ora = runs
    g = setup['gold']; p = 'f%d.' % t
    h, r = hip_res[t], ora[t]
    for key in ('panoptic_cls_inds', 'panoptic_det_labels', 'panoptic_det_obj_ids'):
        assert np.array_equal(h[key].numpy(), r[key].numpy()), (key, h[key], r[key])
        assert np.array_equal(h[key].numpy(), g[p + key]), (key, h[key], g[p + key])
    assert np.allclose(h['panoptic_cls_prob'].numpy(), g[p + 'panoptic_cls_prob'], rtol=1e-3, atol=1e-4)
    assert [int(k) for k in aux[t]['bbox_ids']] == [int(k) for k in g[p + 'bbox_ids']]
    pan = h['panoptic_outputs'].numpy().astype(np.uint8); sem = h['fcn_outputs'].numpy().astype(np.uint8)
    for name, got, ref_o, ref_g in (('pan', pan, r['panoptic_outputs'].numpy(), g[p + 'panoptic_outputs']),
                                    ('sem', sem, r['fcn_outputs'].numpy(), g[p + 'fcn_outputs'])):
        d_o = float((got != ref_o.astype(np.uint8)).mean()); d_g = float((got != ref_g).mean())
        print('frame %d %s: differing pixels vs oracle %.5f%%, vs reference golden %.5f%%' % (t, name, 100 * d_o, 100 * d_g))
        assert d_o < 1e-3 and d_g < 1e-3, (name, d_o, d_g)


@pytest.mark.parametrize('t', [0, 1, 2])
def test_stage_tensors_match_reference_golden(setup, runs, t):
    """the HIP path against the golden FILE (the real reference detector's own tensors), head inputs included"""
    _, aux, _ = runs
    a, g, p = aux[t], setup['gold'], 'f%d.' % t
    errs = dict(flow=_relmax(a['flow'][0][:, ::2, ::2], g[p + 'flow_full']), fpn_p2=_relmax(a['fpn'][0][0, :8], g[p + 'fpn_p2']),
                fpn_p5=_relmax(a['fpn'][3][0], g[p + 'fpn_p5']), neck_p2=_relmax(a['neck'][0][0, :8], g[p + 'neck_out_p2']),
                neck_p6=_relmax(a['neck'][4][0], g[p + 'neck_out_p6']), fcn_score=_relmax(a['fcn_score'][0], g[p + 'fcn_score']))
    ph, pg = a['proposals'], torch.from_numpy(g[p + 'proposals'])
    assert ph.shape == pg.shape
    dist = torch.maximum((ph[:, None, :4] - pg[None, :, :4]).abs().amax(2), 500.0 * (ph[:, None, 4] - pg[None, :, 4]).abs())
    match = dist.argmin(1)
    good = dist.gather(1, match[:, None])[:, 0] < 0.05
    assert int((~good).sum()) <= ph.shape[0] // 100, 'proposal sets differ from the golden file: %d unmatched' % int((~good).sum())
    errs['cls_score'] = _relmax(a['cls_score'][good], torch.from_numpy(g[p + 'cls_score'])[match][good])
    errs['bbox_pred'] = _relmax(a['bbox_pred'][good], torch.from_numpy(g[p + 'bbox_pred'])[match][good])
    print('[%s] frame %d vs golden file: %s' % (setup['prec'], t, {k: '%.2e' % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < T.stage_tol(k), (k, v, errs)


def test_reference_feature_cache_equals_recompute(setup):
    """frame t's ref features taken from the cache (product default) == recomputing extract_feat(ref_img) (reference)"""
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W = setup['H'], setup['W']
    outs = {}
    for reuse in (True, False):
        m.reuse_ref_features = reuse
        m._cache = None
        res = []
        for t in range(2):
            out = m(return_loss=False, rescale=True, img=[fr[t].to(dev)], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                    ref_img=[fr[t - 1 if t else 0].to(dev)])
            res.append((out[2]['panoptic_outputs'].cpu().numpy().copy(), out[2]['panoptic_det_obj_ids'].cpu().numpy().copy(),
                        m._aux['neck_out'][0].to_nchw().cpu()))
        outs[reuse] = res
    m.reuse_ref_features = True
    for t in range(2):
        assert np.array_equal(outs[True][t][0], outs[False][t][0])
        assert np.array_equal(outs[True][t][1], outs[False][t][1])
        assert torch.equal(outs[True][t][2], outs[False][t][2])


def test_operator_api_matches_reference_signatures(setup):
    """module-level NCHW APIs (reference call signatures): backbone/neck extract_feat and compute_flow"""
    from oracle.fusetrack import FuseTrackOracle
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    o = FuseTrackOracle(setup['sd'])
    feats = m.extract_feat(fr[1].to(dev))
    with torch.no_grad():
        ref = o.extract_feat(fr[1])
    assert len(feats) == 5
    for a, b in zip(feats, ref):
        assert _relmax(a.cpu(), b) < 1e-3
    flow, _ = m.compute_flow(fr[1].to(dev), fr[0].to(dev), scale_factor=0.25)
    with torch.no_grad():
        rf = o.compute_flow(fr[1], fr[0], 0.25)
    assert _relmax(flow.cpu(), rf) < 2 * T.STAGE['flow']


def test_cached_reference_features_are_only_used_for_the_previous_frame(setup):
    """with consecutive iids but a ref_img that is NOT the previous call's img (a custom pair), the cached features
    must not be used — the result equals the reference's per-frame recomputation"""
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W = setup['H'], setup['W']
    if setup['prec'] != 'f16x3':
        pytest.skip('one arithmetic mode is enough for the cache logic')
    outs = {}
    for reuse in (True, False):
        m.reuse_ref_features = reuse; m.verify_ref_frame = True
        m._cache = None; m.reset_tracker()
        m(return_loss=False, rescale=True, img=[fr[0].to(dev)], img_meta=[[synth.img_meta(H, W, 10001)]], ref_img=[fr[0].to(dev)])
        # frame 2 with frame 2 (not frame 1's img = frame 0) as its reference
        out = m(return_loss=False, rescale=True, img=[fr[1].to(dev)], img_meta=[[synth.img_meta(H, W, 10002)]], ref_img=[fr[2].to(dev)])
        outs[reuse] = (out[2]['panoptic_outputs'].cpu().numpy().copy(), m._aux['neck_out'][0].to_nchw().cpu())
    m.reuse_ref_features = True
    m._cache = None; m.reset_tracker()
    assert np.array_equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])


def test_compute_flow_pads_and_trims_like_the_reference(setup):
    """panoptic_fusetrack.py:125-138: 200x400 (and 800x1600) inputs are zero-padded to a multiple of 64 for FlowNet2 and the flow
    is trimmed back; any other size must already be a multiple of 64"""
    from oracle.fusetrack import FuseTrackOracle
    m, dev = setup['model'], setup['dev']
    if setup['prec'] != 'f16x3':
        pytest.skip('one arithmetic mode is enough for the padding logic')
    fr = synth.synth_clip(200, 400, 2, 3)
    o = FuseTrackOracle(setup['sd'])
    with torch.no_grad():
        ref = o.compute_flow(fr[1], fr[0], 0.25)
        full = o.last_flow_full
    flow, _ = m.compute_flow(fr[1].to(dev), fr[0].to(dev), scale_factor=0.25)
    assert tuple(flow.shape) == (1, 2, 50, 100) == tuple(ref.shape) and tuple(full.shape) == (1, 2, 200, 400)
    assert _relmax(flow.cpu(), ref) < 2 * T.STAGE['flow']
    flow1, _ = m.compute_flow(fr[1].to(dev), fr[0].to(dev))
    assert _relmax(flow1.cpu(), full) < 2 * T.STAGE['flow']
    with pytest.raises(AssertionError):
        m.compute_flow(fr[1][..., :200, :336].to(dev), fr[0][..., :200, :336].to(dev))      # 200x336: not a special case, not /64


def test_clip_shard_backend_and_handoff_feature(setup):
    """(a) ClipShardRunner + DetectorBackend (deferred tracking + sequential replay) == plain sequential calls;
    (b) frame 1 fed with the hand-off feature gathered_feature(frame 0) (what a neighbouring GPU would send) == the
    cached-feature path."""
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W, n = setup['H'], setup['W'], setup['n']
    m._cache = None; m.reset_tracker()
    seq = []
    for t in range(n):
        out = m(return_loss=False, rescale=True, img=[fr[t].to(dev)], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                ref_img=[fr[t - 1 if t else 0].to(dev)])
        seq.append({k: v.cpu().numpy().copy() for k, v in out[2].items()})
    frd = [f.to(dev) for f in fr]            # the runner's frames must be stable objects: the cross-frame prefetch matches by identity
    for prefetch in (True, False):
        m._cache = None; m._pf = None; m.reset_tracker()
        outs = ClipShardRunner(DetectorBackend(m, H, W, prefetch=prefetch), 0, 1, None, dev).run(lambda t: frd[t], n)
        for t in range(n):
            # the pipelined schedule (next frame's FlowNet2 / ResNet / FPN on the prefetch stream beside this frame's neck and
            # heads, in a ring of three workspaces) is bitwise the sequential one
            assert np.array_equal(np.asarray(outs[t]['panoptic_det_obj_ids']), seq[t]['panoptic_det_obj_ids']), (prefetch, t)
            assert np.array_equal(outs[t]['panoptic_outputs'].cpu().numpy(), seq[t]['panoptic_outputs']), (prefetch, t)
            assert np.array_equal(outs[t]['fcn_outputs'].cpu().numpy(), seq[t]['fcn_outputs']), (prefetch, t)
            assert np.array_equal(outs[t]['panoptic_cls_prob'].cpu().numpy(), seq[t]['panoptic_cls_prob']), (prefetch, t)
        assert (m._pf is None)
    # (b)
    m._cache = None; m.reset_tracker()
    m(return_loss=False, rescale=True, img=[fr[0].to(dev)], img_meta=[[synth.img_meta(H, W, 10001)]], ref_img=[fr[0].to(dev)])
    feat = m.gathered_feature(fr[0].to(dev)).clone()
    m._cache = None
    out = m.simple_test(fr[1].to(dev), [synth.img_meta(H, W, 10002)], ref_img=[fr[0].to(dev)], ref_feature=feat)
    assert np.array_equal(out[2]['panoptic_outputs'].cpu().numpy(), seq[1]['panoptic_outputs'])
    assert np.array_equal(out[2]['panoptic_det_obj_ids'].cpu().numpy(), seq[1]['panoptic_det_obj_ids'])


def test_image_stage_stream_fan_out_is_bitwise_the_single_prefetch_stream(setup):
    """detector.pre_streams (VPS_PRE_STREAMS): the next frame's image-only stages on one prefetch stream (1), with ResNet + FPN + gather
    beside FlowNet2 (2), with FlowNetSD beside the FlowNetC -> S -> S chain as well (3, the default), the main chain on a
    high-priority stream (main_priority), one or two frames announced ahead (prefetch_depth), the second one's backbone deferred to the end of the frame (defer_backbone) - all bitwise equal, over a clip long enough to reuse every ring slot (10 frames, ring of 3)"""
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W, n = setup['H'], setup['W'], setup['n']
    frd = [fr[t % n].to(dev).clone() for t in range(10)]
    runs = []
    old, oldp, oldd = m.pre_streams, m.main_priority, m.defer_backbone
    try:
        for streams, prio, depth, defer in ((1, False, 1, False), (2, False, 1, False), (3, False, 1, False), (3, True, 2, False), (3, False, 2, False),
                                            (3, False, 2, True), (1, False, 2, True)):
            m.pre_streams, m.main_priority, m.defer_backbone = streams, prio, defer
            m._cache = None; m._pf = None; m.reset_tracker()
            be = DetectorBackend(m, H, W, prefetch=True)
            be.prefetch_depth = depth          # 2: the frame after next is announced too and enqueued before the end-of-frame read
            outs = ClipShardRunner(be, 0, 1, None, dev).run(lambda t: frd[t], len(frd))
            assert m._pf is None               # every announced frame was consumed
            runs.append([{k: (v.cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v).copy()) for k, v in o.items()
                          if k in ('panoptic_det_obj_ids', 'panoptic_outputs', 'fcn_outputs', 'panoptic_cls_prob')} for o in outs])
    finally:
        m.pre_streams, m.main_priority, m.defer_backbone = old, oldp, oldd
    for r in runs[1:]:
        for t in range(len(frd)):
            for k in runs[0][t]:
                assert np.array_equal(runs[0][t][k], r[t][k]), (t, k)


def test_unmatched_announcements_do_not_overwrite_the_cached_reference_feature(setup):
    """a caller that announces tensors it then does NOT pass (it re-uploads per call: here the announced pair is a clone)
    makes every call enqueue its own frame, the announced next frame and the one after - three ring slots in one call, while the
    slot of frame t-1 still holds the cached reference feature neck(t) reads. The slot chooser must leave that slot (and the slots
    of records still to be consumed) alone - the ring grows instead - and the outputs must be bitwise the serial schedule's."""
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W, n = setup['H'], setup['W'], setup['n']
    nf = 7
    frd = [fr[t % n].to(dev).clone() for t in range(nf)]

    def run(announce):
        m._cache = None; m._pf = None; m.reset_tracker()
        outs = []
        for t in range(nf):
            pf = None
            if announce:
                # the next two frames, as tensors the following calls will NOT be made with
                pf = [(frd[min(t + 1 + j, nf - 1)].clone(), frd[min(t + j, nf - 1)].clone()) for j in range(2)]
            out = m.simple_test(frd[t], [synth.img_meta(H, W, 10000 + t + 1)], ref_img=[frd[t - 1 if t else 0]], prefetch=pf)
            outs.append({k: v.cpu().numpy().copy() for k, v in out[2].items()})
        torch.cuda.synchronize()
        return outs

    serial = run(False)
    assert m._ring is not None and len(m._ring) == 3
    noisy = run(True)
    for t in range(nf):
        for k in ('panoptic_det_obj_ids', 'panoptic_outputs', 'fcn_outputs', 'panoptic_cls_prob'):
            assert np.array_equal(serial[t][k], noisy[t][k]), (t, k)
    # every record that is waiting names a slot of its own, none of them the cached feature's
    slots = [r['slot'] for r in (m._pf or [])] + [m._cache['slot']]
    assert len(set(slots)) == len(slots), slots
    m._cache = None; m._pf = None; m._ws = None; m.reset_tracker()          # fresh (three-slot) workspaces for the tests that follow


def test_pooled_workspace_is_bitwise_the_buffer_per_activation_workspace(setup):
    """nhwc.Workspace temporaries (liveness-based reuse of activation blocks per stream, round 5) against one persistent buffer per
    activation (VPS_WS_POOL=0, the round-4 workspace): bitwise equal outputs over a clip long enough to recycle every ring slot, in the
    pipelined schedule; and every temporary is back in its pool at the end of a frame"""
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W, n = setup['H'], setup['W'], setup['n']
    frd = [fr[t % n].to(dev).clone() for t in range(8)]
    runs, sizes = [], []
    old = nhwc.POOLING
    try:
        for pooling in (True, False):
            nhwc.POOLING = pooling
            m._ws = None; m._cache = None; m._pf = None; m.reset_tracker()          # fresh workspaces in that mode
            outs = ClipShardRunner(DetectorBackend(m, H, W, prefetch=True), 0, 1, None, dev).run(lambda t: frd[t], len(frd))
            torch.cuda.synchronize()
            assert m._ws.pooling == pooling and not m._ws._live and not m._lane._live
            sizes.append(m.workspace_bytes())
            runs.append([{k: (v.cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v).copy()) for k, v in o.items()
                          if k in ('panoptic_det_obj_ids', 'panoptic_outputs', 'fcn_outputs', 'panoptic_cls_prob')} for o in outs])
    finally:
        nhwc.POOLING = old
        m._ws = None; m._cache = None; m._pf = None; m.reset_tracker()
    for t in range(len(frd)):
        for k in runs[0][t]:
            assert np.array_equal(runs[0][t][k], runs[1][t][k]), (t, k)
    # (at this frame size the fixed-size scratch buffers dominate both; the full-size figure is asserted in tests/test_fullsize_gpu.py)
    print('workspace bytes pooled %.1f MB, one buffer per activation %.1f MB' % (sizes[0] / 1e6, sizes[1] / 1e6))
    assert sizes[0] < sizes[1]


def test_streamed_records_of_another_rank_replay_to_the_sequential_ids(setup):
    """what rank r > 0 does in vps_amd/clip_shard.py, in one process: every frame is computed with deferred tracking, its detection
    record + maps are packed into the fixed-layout tensors that travel to rank 0, unpacked there and assigned in clip order
    (`track_assign`) — ids, maps and per-instance vectors must equal the inline sequential run"""
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    m, fr, dev = setup['model'], setup['frames'], setup['dev']
    H, W, n = setup['H'], setup['W'], setup['n']
    m._cache = None; m._pf = None; m.reset_tracker()
    seq = []
    for t in range(n):
        out = m(return_loss=False, rescale=True, img=[fr[t].to(dev)], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                ref_img=[fr[t - 1 if t else 0].to(dev)])
        seq.append({k: v.cpu().numpy().copy() for k, v in out[2].items()})
    be = DetectorBackend(m, H, W, prefetch=False)
    be.inline_ids = False                                  # a rank that does not own the head of the clip
    runner = ClipShardRunner(be, 0, 1, None, dev)
    cap, lay, nrec = runner._layout()
    m._cache = None; m._pf = None; m.reset_tracker()
    frd = [f.to(dev) for f in fr]
    wire = []
    for t in range(n):
        rec = be.process(frd[t], frd[t - 1 if t else 0], None, 10000 + t + 1, t == 0)
        buf = runner._pack(rec, torch.zeros(nrec, dtype=torch.float32, device=dev))
        maps = torch.stack([rec['panoptic_outputs'][0], rec['fcn_outputs'][0]]).to(torch.uint8).contiguous()
        wire.append((buf.clone(), maps.clone()))
    m.reset_tracker()                                      # "rank 0": only the tracker state matters from here on
    for t, (buf, maps) in enumerate(wire):
        rec = runner._unpack(buf, maps, t)
        out = be.finalize(rec, be.assign(rec, t == 0))
        assert np.array_equal(np.asarray(out['panoptic_det_obj_ids']), seq[t]['panoptic_det_obj_ids']), t
        assert np.array_equal(out['panoptic_cls_inds'].cpu().numpy(), seq[t]['panoptic_cls_inds']), t
        assert np.array_equal(out['panoptic_det_labels'].cpu().numpy(), seq[t]['panoptic_det_labels']), t
        assert np.array_equal(out['panoptic_cls_prob'].cpu().numpy(), seq[t]['panoptic_cls_prob']), t
        assert np.array_equal(out['panoptic_outputs'].cpu().numpy(), seq[t]['panoptic_outputs']), t
        assert np.array_equal(out['fcn_outputs'].cpu().numpy(), seq[t]['fcn_outputs']), t
    m._cache = None; m.reset_tracker()


@pytest.mark.parametrize('prec_name', ['bf16x3'])
def test_split_bf16_arithmetic_end_to_end(setup, runs, prec_name):
    """the split-bf16 matrix-core modes on the whole path: bf16x6 (fp32-grade) must reproduce ids/classes exactly; bf16x3
    is reported (stage errors, pixel mismatch) and must stay within 1e-2 stage error"""
    from vps_amd import hip, nhwc
    if setup['prec'] != 'f32':
        pytest.skip('the optional bf16x3 mode is reported once')
    _, _, ora = runs
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    old = nhwc.DEFAULT_PREC
    nhwc.DEFAULT_PREC = {'bf16x3': hip.PREC_BF16X3, 'bf16x6': hip.PREC_BF16X6}[prec_name]
    try:
        m = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        synth.load_synth(m, 0)
        fr, dev, H, W = setup['frames'], setup['dev'], setup['H'], setup['W']
        lines = []
        for t in range(setup['n']):
            out = m(return_loss=False, rescale=True, img=[fr[t].to(dev)], img_meta=[[synth.img_meta(H, W, 10000 + t + 1)]],
                    ref_img=[fr[t - 1 if t else 0].to(dev)])
            a, r = m._aux, ora[t]
            e = dict(flow=_relmax(a['flow'].to_nchw().cpu(), r['flow_full']), fpn_p2=_relmax(a['levels'][0].to_nchw().cpu(), r['pre_neck'][0]),
                     neck_p2=_relmax(a['neck_out'][0].to_nchw().cpu(), r['feats'][0]), fcn_score=_relmax(a['fcn_score'].to_nchw().cpu(), r['fcn_score']))
            pan = out[2]['panoptic_outputs'].cpu().numpy(); sem = out[2]['fcn_outputs'].cpu().numpy()
            dp = float((pan != r['panoptic_outputs'].numpy().astype(np.uint8)).mean()); ds = float((sem != r['fcn_outputs'].numpy().astype(np.uint8)).mean())
            same_ids = np.array_equal(out[2]['panoptic_det_obj_ids'].cpu().numpy(), r['panoptic_det_obj_ids'].numpy())
            same_cls = np.array_equal(out[2]['panoptic_cls_inds'].cpu().numpy(), r['panoptic_cls_inds'].numpy())
            lines.append('%s frame %d: %s pan_mismatch %.5f sem_mismatch %.5f ids_equal %s cls_equal %s' % (
                prec_name, t, {k: '%.2e' % v for k, v in e.items()}, dp, ds, same_ids, same_cls))
            print(lines[-1])
            with open(os.path.join(ROOT, 'gpurun_out', 'prec_report.txt'), 'a') as f:
                f.write(lines[-1] + '\n')
            tol = 2e-3 if prec_name == 'bf16x6' else 2e-2
            for k, v in e.items():
                assert v < tol, (k, v)
            if prec_name == 'bf16x6':
                assert same_ids and same_cls and dp < 1e-3 and ds < 1e-3
    finally:
        nhwc.DEFAULT_PREC = old
