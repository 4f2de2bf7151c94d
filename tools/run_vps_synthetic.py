"""End-to-end run of the whole drop-in on a synthetic video set — the flow of the reference's tools/test_vpq.py:93-198 followed by
tools/eval_vpq.py:261-330, with every device-side stage of this package in place of the reference's:

    decoded uint8 frames -> DeviceImagePrep / PairFeeder (Normalize, Pad, ImageToTensor; ref_img = previous frame, prepared once)
    -> build_detector(cfg.model) + synthetic checkpoint -> model(return_loss=False, rescale=True, img=[..], img_meta=[..], ref_img=[..])
    -> the pano_results bookkeeping of single_gpu_test (test_vpq.py:28-69), maps kept on the device
    -> PanopticUnifier.get_unified_pan_result (cityscapes_vps.py:162-226)
    -> inference_panoptic_video: labelled-frame sampling, 2-channel -> colour PNG + segments_info, pan_2ch/ pan_pred/ pred.json
    -> vpq_compute_single_core for the window lengths of eval_vpq.py (k = 0, 5, 10, 15 <-> nframes 1..4) against a ground truth

There is no dataset offline, so the "ground truth" is the prediction itself (VPQ must come out as exactly 100 for every class
present), or the prediction of a second run in another arithmetic mode (`--gt-prec`): the VPQ between two fp32-grade modes is
the end-to-end parity number in the reference's own metric.

    python tools/run_vps_synthetic.py --videos 2 --frames 30 --height 256 --width 512 --out gpurun_out/vps_synth [--prec f16x3 --gt-prec f32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CATEGORIES = [{'id': c, 'name': 'class%d' % c, 'isthing': 1 if c >= 11 else 0, 'color': [(37 * c) % 256, (91 * c) % 256, (53 * c + 80) % 256]}
              for c in range(19)]


class ColorGenerator:
    """stand-in for panopticapi.utils.IdGenerator (absent offline): distinct colours per call, deterministic"""

    def __init__(self, categories):
        self.categories = categories
        self.taken = set([0])

    def get_color(self, cat_id):
        base = self.categories[cat_id]['color']
        k = 0
        while True:
            c = [(base[0] + 7 * k) % 256, (base[1] + 13 * k) % 256, (base[2] + 29 * k) % 256]
            key = c[0] + 256 * c[1] + 65536 * c[2]
            if key not in self.taken:
                self.taken.add(key)
                return c
            k += 1


def uint8_frame(H, W, seed, shift):
    from vps_amd import synth
    return synth.synth_frame(H, W, seed=seed, shift=shift, noise=2.0 if shift != (0, 0) else 0.0).astype(np.uint8)


def run_model(prec, videos, nframes, H, W, dev, separated=False, flow=None, jpeg_entropy='host', keep_flows=False, back_flows=False, png_huffman='fixed'):
    """test_vpq.py:129-149 + single_gpu_test (:28-69) on `videos` synthetic clips -> pano_results with DEVICE maps.
    `flow` = (directory, format, max_rad): the FlowNet2 flow of EVERY frame as DIR/<name>.<format> (flowvis.FlowWriter).
    `keep_flows` (--tc): the device flow of every frame in res['all_flows'], 8 bytes per pixel and frame until `tc` has counted its pair.
    `back_flows` (--tc-occlusion): after every frame but a video's first, `model.flow_between(ref, img)` - the flow from the previous
    frame to this one, a second FlowNet2 pass - in res['all_back_flows'] (None for a first frame), the same 8 bytes again"""
    import vps_amd
    from vps_amd import nhwc, synth
    from vps_amd.pipeline import DeviceImagePrep, PairFeeder
    old = nhwc.DEFAULT_PREC
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[prec]
    try:
        cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
        model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        over = synth.separated_overrides(os.path.join(ROOT, 'tests', 'golden', 'separated_fc_cls.npz')) if separated else None
        synth.load_synth(model, 0, overrides=over)
        model.ensure_packed(dev)
    finally:
        nhwc.DEFAULT_PREC = old
    prep = DeviceImagePrep(**cfg.img_norm_cfg, size_divisor=32, img_scale=(max(H, W), min(H, W)), device=dev)
    feed = PairFeeder(prep)
    res = dict(all_names=[], all_ssegs=[], all_panos=[], all_pano_cls_inds=[], all_pano_obj_ids=[], all_frames=[], flow_files=[])
    flow_writer = None
    if flow:
        from vps_amd.flowvis import FlowWriter, flow_name
        model.keep_flow = True
        flow_writer = FlowWriter(dev, fmt=flow[1], max_rad=flow[2], entropy=jpeg_entropy, huffman=png_huffman)
    if keep_flows:
        model.keep_flow = True
        res['all_flows'] = []
    if back_flows:
        res['all_back_flows'] = []
    decoded = [[uint8_frame(H, W, seed=v, shift=(2 * f, f)) for f in range(nframes)] for v in range(videos)]   # "cv2.imread" results (BGR uint8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for v in range(videos):
        feed.reset()
        for f in range(nframes):
            img, ref = feed(decoded[v][f])                                         # 6 MB upload + Normalize / Pad / ToTensor on the device
            name = '%04d_%04d_city_%06d_%06d_newImg8bit.png' % (v, f, v, f)
            meta = dict(filename=name, iid=v * 10000 + f + 1, img_shape=(H, W, 3), ori_shape=(H, W, 3), pad_shape=tuple(img.shape[2:]) + (3,),
                        scale_factor=1.0, flip=False)
            with torch.no_grad():
                result = model(return_loss=False, rescale=True, img=[img], img_meta=[[meta]], ref_img=[ref])
            res['all_ssegs'].append(result[2]['fcn_outputs'][0])                   # device uint8 maps (test_vpq.py:51-56 moves them to the host)
            res['all_panos'].append(result[2]['panoptic_outputs'][0])
            res['all_pano_cls_inds'].append(result[2]['panoptic_cls_inds'].cpu().numpy())
            res['all_pano_obj_ids'].append(result[2]['panoptic_det_obj_ids'].cpu().numpy())
            res['all_names'].append(name)
            res['all_frames'].append(decoded[v][f])                                # the decoded frame itself: what --overlay draws on
            if flow_writer is not None:
                flow_writer.submit(result[2]['flow'], flow_name(flow[0], name, flow[1]))
            if keep_flows:
                res['all_flows'].append(result[2]['flow'])
            if back_flows:
                res['all_back_flows'].append(model.flow_between(ref, img, img_shape=meta['img_shape']) if f > 0 else None)
    if flow_writer is not None:
        res['flow_files'] = flow_writer.close()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def postprocess(res, out_dir, videos, dev, labeled_fid, lambda_, nper, device_png=False, overlay=None, tubes=False, jpeg_entropy='host',
                overlay_video=None, tc=None, flow_photo=None, flow_census=None, png_huffman='fixed'):
    """test_vpq.py:178-198 with the device-side unifier / converter / asynchronous writer (`device_png`: the PNGs are filtered and
    deflated on the device too, postprocess.DevicePngWriter). `overlay` = (directory, quality, alpha): an overlay JPEG of EVERY frame,
    blended and transformed on the device (postprocess.write_overlays). `tubes`: tubes.json beside pred.json, the COCO run-length
    encoding, box and area of every tracked instance in every labelled frame (vps_amd.tubes). `overlay_video` = (FILE.y4m, sampling):
    the same overlays as one Y4M stream per video (y4m.Y4mWriter), beside the JPEGs or, without `overlay`, instead of them; its
    'files' entry receives the streams' names. `tc` = dict(map_dir, alpha, quality): the temporal consistency of EVERY video's consecutive
    frames from res['all_flows'] (vps_amd.tc; tc.txt and tc-tracks.json beside pred.json, the inconsistency overlays in map_dir if it
    is given; with 'occlusion' the forward-backward check on res['all_back_flows'] first; with 'photometric' = THR the photometric flag of
    vps_amd.flowphoto on top of it); its 'result' entry receives the figures. `flow_photo` = dict(map_dir, thr, alpha, quality): the
    photometric warp error of the run's own flows between the decoded frames (vps_amd.flowphoto; flow-photo.txt and flow-photo.json
    beside pred.json, the residual overlays in map_dir if it is given), before `tc` lets the flows go; its 'result' entry likewise.
    `flow_census` = dict(map_dir, thr, eps, alpha, quality): the same with the ternary census residual (flow-census.txt and
    flow-census.json); tc['census'] = THR is the census flag of the temporal consistency"""
    from vps_amd.postprocess import DevicePngWriter, PanopticUnifier, inference_panoptic_video, write_overlays
    unifier = PanopticUnifier(dev, 19, 9)
    two = unifier.get_unified_pan_result(res['all_ssegs'], res['all_panos'], res['all_pano_cls_inds'], obj_ids=res['all_pano_obj_ids'],
                                         stuff_area_limit=2048, names=res['all_names'])
    keys = sorted(two.keys())
    pred_pans_2ch = [two[k] for k in keys]
    if flow_photo is not None:
        flow_photo['result'] = photo_score(pred_pans_2ch, res, keys, len(keys) // max(videos, 1), dev, out_dir, flow_photo, jpeg_entropy)
    if flow_census is not None:
        flow_census['result'] = census_score(pred_pans_2ch, res, keys, len(keys) // max(videos, 1), dev, out_dir, flow_census, jpeg_entropy)
    if tc is not None:
        tc['result'] = tc_score(pred_pans_2ch, res, keys, len(keys) // max(videos, 1), dev, out_dir, unifier.id_last_stuff, tc, jpeg_entropy)
    names = keys[(labeled_fid // lambda_)::lambda_]                               # names of the labelled frames (im_jsons['images'])
    cats = {c['id']: c for c in CATEGORIES}
    writer = DevicePngWriter(dev, huffman=png_huffman) if device_png else None
    collector = None
    if tubes:
        from vps_amd.tubes import TubeCollector
        collector = TubeCollector(things_only=True, device=dev, id_last_stuff=unifier.id_last_stuff)
    pans, pj = inference_panoptic_video(pred_pans_2ch, out_dir, CATEGORIES, names, n_video=videos, color_generator=ColorGenerator(cats), device=dev,
                                        labeled_fid=labeled_fid, lambda_=lambda_, nframes_per_video=nper, writer=writer, tubes=collector)
    if collector is not None:
        collector.close()
    if writer is not None:
        writer.close()
    if overlay or overlay_video:
        # (synth_frame crops the late, far-shifted frames of a clip at the edge of its noise field while img_meta keeps the nominal
        # size: such a frame is padded back to the size of its map with its edge pixels)
        frames = {n: np.pad(f, ((0, two[n].shape[0] - f.shape[0]), (0, two[n].shape[1] - f.shape[1]), (0, 0)), mode='edge')
                  for n, f in zip(res['all_names'], res['all_frames'])}
        ov = overlay or (None, 90, overlay_video['alpha'])
        vkw = dict(video=overlay_video['file'], video_sampling=overlay_video['sampling'], video_files=overlay_video['files']) if overlay_video else {}
        write_overlays(pred_pans_2ch, [frames[k] for k in keys], keys, ov[0], ColorGenerator(cats), len(keys) // max(videos, 1), device=dev,
                       quality=ov[1], alpha=ov[2], entropy=jpeg_entropy, **vkw)
    return names, pans, pj


def padded_frames(res, names, maps):
    """the decoded frames in the order of `names`, each padded with its edge pixels to the size of its map (synth_frame crops the late,
    far-shifted frames of a clip at the edge of its noise field while img_meta keeps the nominal size)"""
    at = {n: i for i, n in enumerate(res['all_names'])}
    return [np.pad(res['all_frames'][at[n]], ((0, m.shape[0] - res['all_frames'][at[n]].shape[0]), (0, m.shape[1] - res['all_frames'][at[n]].shape[1]),
                                               (0, 0)), mode='edge') for n, m in zip(names, maps)]


def photo_score(maps, res, names, nframes_per_video, dev, out_dir, opt, jpeg_entropy='host'):
    """--flow-photo: the photometric warp error of every frame's flow between the frame and its predecessor (vps_amd.flowphoto); with the
    backward flows of --tc-occlusion the occlusion mask splits the pixels into a visible and a masked group. The flows stay where they are"""
    from vps_amd import flowphoto
    at = {n: i for i, n in enumerate(res['all_names'])}
    ev = flowphoto.PhotoEvaluator(dev, thr=opt['thr'], per_pair=True)
    back = [res['all_back_flows'][at[n]] for n in names] if res.get('all_back_flows') is not None else None
    files = flowphoto.score_videos(ev, padded_frames(res, names, maps), [res['all_flows'][at[n]] for n in names], names, nframes_per_video, back_flows=back,
                                   map_dir=opt.get('map_dir'), alpha=opt.get('alpha', 128), quality=opt.get('quality', 90), entropy=jpeg_entropy)
    result = ev.result()
    flowphoto.write_outputs(result, out_dir)
    result['map_files'] = files
    return result


def census_score(maps, res, names, nframes_per_video, dev, out_dir, opt, jpeg_entropy='host'):
    """--flow-census: `photo_score` with the ternary census residual (`flowphoto.CensusEvaluator`) in the place of the photometric error"""
    from vps_amd import flowphoto
    at = {n: i for i, n in enumerate(res['all_names'])}
    ev = flowphoto.CensusEvaluator(dev, thr=opt['thr'], eps=opt['eps'], per_pair=True)
    back = [res['all_back_flows'][at[n]] for n in names] if res.get('all_back_flows') is not None else None
    files = flowphoto.score_videos(ev, padded_frames(res, names, maps), [res['all_flows'][at[n]] for n in names], names, nframes_per_video, back_flows=back,
                                   map_dir=opt.get('map_dir'), alpha=opt.get('alpha', 128), quality=opt.get('quality', 90), entropy=jpeg_entropy)
    result = ev.result()
    flowphoto.write_census_outputs(result, out_dir)
    result['map_files'] = files
    return result


def census_report(r):
    """the 'flow_census' entry of the report from the result of `flowphoto.CensusEvaluator`"""
    a = r['all']
    out = dict(thr=r['thr'], eps=r['eps'], pairs=r['pairs'], ce_warp=round(a['ce_warp'], 6), ce_static=round(a['ce_static'], 6), ratio=round(a['ratio'], 6),
               gain=round(a['gain'], 6), flagged_share=round(a['flagged_share'], 6), outside_share=round(a['outside_share'], 6),
               map_files=len(r['map_files']))
    if r['masked']['n']:
        out.update(ce_warp_visible=round(r['visible']['ce_warp'], 6), ce_warp_masked=round(r['masked']['ce_warp'], 6))
    return out


def tc_score(maps, res, names, nframes_per_video, dev, out_dir, id_last_stuff, opt, jpeg_entropy='host'):
    """--tc: the unified maps of every frame (in the order of `names`) against their predecessors warped by the run's own flows. The 19
    classes of CATEGORIES are the class indices, every other pan_seg value is void; tracks are keyed by pan_obj (channel 2)"""
    from vps_amd import tc
    seg_class = np.full(256, 255, dtype=np.uint8)
    seg_class[:len(CATEGORIES)] = np.arange(len(CATEGORIES))
    kw = {}
    if opt.get('census') is not None:                     # --tc-census: occluded pixels and pixels the census flags are left out of the counts
        ev = tc.TcEvaluator(seg_class, len(CATEGORIES), id_channel=2, device=dev, per_pair=True, id_last_stuff=id_last_stuff, occlusion=True,
                            photometric=opt.get('photometric'), census=opt['census'], census_eps=opt.get('census_eps'))
    elif opt.get('photometric') is not None:              # --tc-photometric: occluded and photometrically wrong pixels are left out of the counts
        ev = tc.TcEvaluator(seg_class, len(CATEGORIES), id_channel=2, device=dev, per_pair=True, id_last_stuff=id_last_stuff, occlusion=True,
                            photometric=opt['photometric'])
    elif opt.get('occlusion'):                            # --tc-occlusion: occluded pixels are left out of the counts
        ev = tc.TcEvaluator(seg_class, len(CATEGORIES), id_channel=2, device=dev, per_pair=True, id_last_stuff=id_last_stuff, occlusion=True)
    else:
        ev = tc.TcEvaluator(seg_class, len(CATEGORIES), id_channel=2, device=dev, per_pair=True, id_last_stuff=id_last_stuff)
    at = {n: i for i, n in enumerate(res['all_names'])}
    flows = [res['all_flows'][at[n]] for n in names]
    res['all_flows'] = None                               # `flows` holds them now and lets each one go once its pair is counted
    if opt.get('occlusion'):
        kw['back_flows'] = [res['all_back_flows'][at[n]] for n in names]
        res['all_back_flows'] = None
    frames = None
    if opt.get('map_dir') or opt.get('photometric') is not None or opt.get('census') is not None:
        frames = padded_frames(res, names, maps)
    files = tc.score_videos(ev, maps, flows, names, nframes_per_video, map_dir=opt.get('map_dir'), frames=frames, alpha=opt.get('alpha', 128),
                            quality=opt.get('quality', 90), entropy=jpeg_entropy, **kw)
    result = ev.result()
    tc.write_outputs(result, out_dir)
    result['map_files'] = files
    return result


def photo_report(r):
    """the 'flow_photo' entry of the report from the result of vps_amd.flowphoto"""
    a = r['all']
    out = dict(thr=r['thr'], pairs=r['pairs'], mae_warp=round(a['mae_warp'], 6), mae_static=round(a['mae_static'], 6), ratio=round(a['ratio'], 6),
               psnr_warp=round(a['psnr_warp'], 4), psnr_static=round(a['psnr_static'], 4), gain_db=round(a['gain_db'], 4),
               flagged_share=round(a['flagged_share'], 6), outside_share=round(r['outside_share'], 6), map_files=len(r['map_files']))
    if r['masked']['n']:
        out.update(mae_warp_visible=round(r['visible']['mae_warp'], 6), mae_warp_masked=round(r['masked']['mae_warp'], 6))
    return out


def vpq(gt, pred, videos, nper, dev):
    """eval_vpq.py:261-330: per video, window lengths 1..4, PQ averaged over the categories with support; VPQ = mean over k"""
    from vps_amd.evaluate import vpq_compute_single_core
    cats = {c['id']: c for c in CATEGORIES}
    out = {}
    for nf in (1, 2, 3, 4):
        from vps_amd.evaluate import PQStat
        stat = PQStat()
        for v in range(videos):
            sl = slice(v * nper, (v + 1) * nper)
            clip = [(g, p, gp, pp, {}) for g, p, gp, pp in zip(gt[1]['annotations'][sl], pred[1]['annotations'][sl], gt[0][sl], pred[0][sl])]
            stat += vpq_compute_single_core(clip, cats, nframes=nf, device=dev)
        res, _ = stat.pq_average(cats, isthing=None)
        out[nf] = res
    out['vpq'] = float(np.mean([100 * out[nf]['pq'] for nf in (1, 2, 3, 4)]))
    return out


def stq(gt_dir, gt_json, pred_dir, names, out, nper, dev):
    """tools/eval_stq_device.py on the files of this run: the ground truth (the `pan_pred/` PNGs and annotations of `gt_dir`) is laid
    out as that tool reads it under `out`/stq_truth/; stq.txt and stq-tracks.json go beside pred.json"""
    import shutil
    import eval_stq_device
    truth = os.path.join(out, 'stq_truth')
    os.makedirs(truth, exist_ok=True)
    images = [dict(id=n.replace('_newImg8bit.png', ''), file_name=n) for n in names]
    for im in images:
        shutil.copy(os.path.join(gt_dir, 'pan_pred', im['id'] + '.png'), os.path.join(truth, im['file_name'].replace('_newImg8bit.png', '_final_mask.png')))
    gt_file = os.path.join(out, 'stq_gt.json')
    with open(gt_file, 'w') as f:
        json.dump(dict(annotations=gt_json['annotations'], categories=CATEGORIES, images=images), f)
    return eval_stq_device.main(['--submit_dir', pred_dir, '--truth_dir', truth, '--pan_gt_json_file', gt_file, '--nframes_per_video', str(nper),
                                 '--device', str(dev)])


def bvpq(gt, pred, videos, nper, dev, out_dir, ratio):
    """boundary VPQ of the same clips (vps_amd.boundary): bvpq-<k>.txt and bvpq-final.txt go beside pred.json"""
    from vps_amd import boundary
    cats = {c['id']: c for c in CATEGORIES}
    clips = []
    for v in range(videos):
        sl = slice(v * nper, (v + 1) * nper)
        clips.append([(g, p, gp, pp, {}) for g, p, gp, pp in zip(gt[1]['annotations'][sl], pred[1]['annotations'][sl], gt[0][sl], pred[0][sl])])
    return boundary.bvpq_compute(clips, cats, out_dir, device=dev, boundary_ratio=ratio)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--videos', type=int, default=2)
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--prec', default='f16x3')
    ap.add_argument('--gt-prec', default=None, help='take the "ground truth" from a second run in this arithmetic mode (default: the prediction itself)')
    ap.add_argument('--separated', action='store_true', help='box classification layer of tests/golden/separated_fc_cls.npz (few, well-separated detections)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'gpurun_out', 'vps_synth'))
    ap.add_argument('--device-png', action='store_true', help='encode the result PNGs on the device (postprocess.DevicePngWriter) instead of PIL threads')
    ap.add_argument('--png-huffman', default='fixed', choices=['fixed', 'dynamic'], help="--device-png, --flow-format png|kitti and PNG error maps: the Huffman code of the device deflate stage. fixed (default): the fixed code, right for label maps; dynamic: a code per 8 KiB segment where that is shorter, for dense images")
    ap.add_argument('--overlay', default=None, metavar='DIR', help='write DIR/<name>.jpg for every frame: the panoptic result blended over the frame (off by default)')
    ap.add_argument('--overlay-quality', type=int, default=90)
    ap.add_argument('--overlay-alpha', type=int, default=128, help='weight of the colour map, 0..256')
    ap.add_argument('--overlay-video', default=None, metavar='FILE.y4m', help='write the overlays of every video as one Y4M stream (YUV4MPEG2; with several '
                    'videos the video\'s name goes in front of the extension), beside --overlay or without it (off by default)')
    ap.add_argument('--overlay-video-sampling', default='420jpeg', choices=['420jpeg', '420mpeg2', '444'])
    ap.add_argument('--jpeg-entropy', default='host', choices=['host', 'device'],
                    help='where the JPEG files of --overlay and --flow are Huffman-coded; the files are the same (default host)')
    ap.add_argument('--tubes', action='store_true', help='write pred/tubes.json: run-length encoded masks, boxes and areas of every tracked instance (off by default)')
    ap.add_argument('--flow', default=None, metavar='DIR', help='write DIR/<name>.<ext> for every frame: the FlowNet2 flow of the frame (off by default)')
    ap.add_argument('--flow-format', default='jpg', choices=['jpg', 'png', 'flo', 'kitti'], help="colour image (jpg, png), the raw Middlebury field (flo) or the KITTI devkit's 16-bit PNG (kitti)")
    ap.add_argument('--flow-max-rad', type=float, default=None, metavar='X', help='one normaliser of the flow colours for all frames (default: each frame its own maximum)')
    ap.add_argument('--stq', action='store_true', help='after the VPQ step, score the same files with tools/eval_stq_device.py: pred/stq.txt and '
                    'pred/stq-tracks.json (off by default)')
    ap.add_argument('--boundary', action='store_true', help='after the VPQ step, score the same clips with boundary VPQ (vps_amd.boundary): pred/bvpq-<k>.txt '
                    'and pred/bvpq-final.txt (off by default)')
    ap.add_argument('--boundary-ratio', type=float, default=0.02, help='--boundary: width of the band as a fraction of the image diagonal')
    ap.add_argument('--tc', action='store_true', help='temporal consistency without ground truth (vps_amd.tc): every frame against the previous one warped by '
                    'the detector\'s own flow; pred/tc.txt and pred/tc-tracks.json (keeps the flow of every frame on the device until its pair is counted; '
                    'off by default)')
    ap.add_argument('--tc-map', default=None, metavar='DIR', help='--tc: write DIR/<name>.jpg for every frame but a video\'s first, the inconsistency map '
                    'blended over the frame (red: class differs, amber: track differs, blue: not in view)')
    ap.add_argument('--tc-occlusion', action='store_true', help='--tc with a forward-backward flow check: a second FlowNet2 pass per frame gives the flow from '
                    'the previous frame to this one, pixels where the two flows do not cancel (disocclusions) are left out of the counts and reported '
                    'as the occluded share (OCC in pred/tc.txt; grey in the --tc-map images; off by default)')
    ap.add_argument('--flow-photo', action='store_true', help='flow quality without ground truth (vps_amd.flowphoto): the photometric warp error of every '
                    'frame\'s flow between the frame and the previous one, beside the static error of not warping; pred/flow-photo.txt and '
                    'pred/flow-photo.json (keeps the flow of every frame on the device; with --tc-occlusion the occlusion mask splits the pixels into a '
                    'visible and a masked group; flagged above --tc-photometric if given, else %g grey levels; off by default)' % 16.0)
    ap.add_argument('--flow-photo-map', default=None, metavar='DIR', help='--flow-photo: write DIR/<name>.jpg for every frame but a video\'s first, the '
                    'photometric residual blended over the frame')
    ap.add_argument('--tc-photometric', type=float, default=None, metavar='THR', help='--tc-occlusion, and pixels that are in view and not occluded but whose '
                    'photometric warp error is above THR grey levels are left out of the counts too (they are part of OCC then; off by default)')
    ap.add_argument('--flow-census', action='store_true', help='illumination-robust flow quality without ground truth (vps_amd.flowphoto, DESIGN.md 6 row '
                    '3i): the ternary census residual of every frame\'s flow between the frame and the previous one, beside the static one of not '
                    'warping; pred/flow-census.txt and pred/flow-census.json (as --flow-photo; flagged above --tc-census if given, else 25 percent; '
                    'off by default)')
    ap.add_argument('--flow-census-map', default=None, metavar='DIR', help='--flow-census: write DIR/<name>.jpg for every frame but a video\'s first, the '
                    'census residual blended over the frame')
    ap.add_argument('--tc-census', type=int, default=None, metavar='THR', help='--tc-occlusion, and pixels that are in view and not occluded but whose '
                    'census residual is above THR percent of their counted neighbours are left out of the counts too (they are part of OCC then; may '
                    'be combined with --tc-photometric; off by default)')
    ap.add_argument('--flow-census-eps', type=float, default=None, metavar='EPS', help='--flow-census / --tc-census: the dead zone of the ternary code in '
                    'thousandths of a grey level (default 2000 = two grey levels)')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    dev = torch.device('cuda:0')
    labeled_fid, lambda_ = 20, 5
    overlay = (args.overlay, args.overlay_quality, args.overlay_alpha) if args.overlay else None
    overlay_video = dict(file=args.overlay_video, sampling=args.overlay_video_sampling, files=[], alpha=args.overlay_alpha) if args.overlay_video else None
    nper = len(range(labeled_fid // lambda_, args.frames, lambda_))
    flow = (args.flow, args.flow_format, args.flow_max_rad) if args.flow else None
    if args.tc_photometric is not None or args.tc_census is not None:
        args.tc_occlusion = True
    tc = dict(map_dir=args.tc_map, alpha=args.overlay_alpha, quality=args.overlay_quality) if (args.tc or args.tc_map or args.tc_occlusion) else None
    if tc and args.tc_occlusion:
        tc['occlusion'] = True
    if tc and args.tc_photometric is not None:
        tc['photometric'] = args.tc_photometric
    if tc and args.tc_census is not None:
        tc['census'], tc['census_eps'] = args.tc_census, args.flow_census_eps
    flow_census = None
    if args.flow_census or args.flow_census_map:
        from vps_amd.flowphoto import CENSUS_EPS, CENSUS_THR
        flow_census = dict(map_dir=args.flow_census_map, thr=CENSUS_THR if args.tc_census is None else args.tc_census,
                           eps=CENSUS_EPS if args.flow_census_eps is None else args.flow_census_eps, alpha=args.overlay_alpha, quality=args.overlay_quality)
    flow_photo = None
    if args.flow_photo or args.flow_photo_map:
        from vps_amd.flowphoto import PHOTO_THR
        flow_photo = dict(map_dir=args.flow_photo_map, thr=PHOTO_THR if args.tc_photometric is None else args.tc_photometric, alpha=args.overlay_alpha,
                          quality=args.overlay_quality)
    res, dt = run_model(args.prec, args.videos, args.frames, args.height, args.width, dev, args.separated, flow, args.jpeg_entropy,
                        keep_flows=tc is not None or flow_photo is not None or flow_census is not None, back_flows=args.tc_occlusion,
                        png_huffman=args.png_huffman)
    t0 = time.perf_counter()
    names, pans, pj = postprocess(res, os.path.join(args.out, 'pred'), args.videos, dev, labeled_fid, lambda_, nper, args.device_png, overlay, args.tubes,
                                  args.jpeg_entropy, overlay_video, tc, flow_photo, flow_census, png_huffman=args.png_huffman)
    dpost = time.perf_counter() - t0
    pred = (pans, pj)
    gt = pred
    if args.gt_prec:
        res2, _ = run_model(args.gt_prec, args.videos, args.frames, args.height, args.width, dev, args.separated)
        _, pans2, pj2 = postprocess(res2, os.path.join(args.out, 'gt'), args.videos, dev, labeled_fid, lambda_, nper, args.device_png, png_huffman=args.png_huffman)
        gt = (pans2, pj2)
    t0 = time.perf_counter()
    score = vpq(gt, pred, args.videos, nper, dev)
    deval = time.perf_counter() - t0
    files = sorted(os.listdir(os.path.join(args.out, 'pred', 'pan_pred')))
    report = dict(videos=args.videos, frames_per_video=args.frames, size=[args.height, args.width], prec=args.prec, gt=args.gt_prec or 'self', weights='synthetic seed 0' + (' + separated fc_cls' if args.separated else ''),
                  labelled_frames=len(names), png_files=len(files), overlay_files=len(os.listdir(args.overlay)) if args.overlay else 0,
                  flow_files=len(res['flow_files']), vpq=round(score['vpq'], 4),
                  pq_per_window={str(k): round(100 * score[k]['pq'], 4) for k in (1, 2, 3, 4)},
                  seconds=dict(model=round(dt, 3), postprocess_and_png=round(dpost, 3), eval=round(deval, 3)),
                  frames_per_s_upload_prep_model_sequential=round(args.videos * args.frames / dt, 2))
    if args.stq:                                        # a key of its own: without the option the report is what it was
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        r = stq(os.path.join(args.out, 'gt' if args.gt_prec else 'pred'), gt[1], os.path.join(args.out, 'pred'), names, args.out, nper, dev)
        report['stq'] = dict(stq=round(100 * r['stq'], 4), aq=round(100 * r['aq'], 4), sq=round(100 * r['sq'], 4), tracks=r['n'])
        print('STQ %.4f  AQ %.4f  SQ %.4f' % (100 * r['stq'], 100 * r['aq'], 100 * r['sq']))
    if args.boundary:                                   # a key of its own: without the option the report is what it was
        r = bvpq(gt, pred, args.videos, nper, dev, os.path.join(args.out, 'pred'), args.boundary_ratio)
        report['bvpq'] = dict(bvpq=round(r['All'], 4), ratio=args.boundary_ratio,
                              pq_per_window={str(k): round(100 * r['per_window'][k]['All']['pq'], 4) for k in (1, 2, 3, 4)},
                              biou_per_window={str(k): round(100 * r['per_window'][k]['All']['biou'], 4) for k in (1, 2, 3, 4)})
        print('boundary VPQ %.4f (VPQ %.4f)' % (r['All'], score['vpq']))
    if tc:                                              # a key of its own: without the option the report is what it was
        r = tc['result']
        report['tc'] = dict(tc=round(100 * r['tc'], 4), tc_sem=round(100 * r['tc_sem'], 4), tc_track=round(100 * r['tc_track'], 4), tracks=r['n_tracks'],
                            in_view_share=round(r['in_view_share'], 6), pairs=len(r['per_pair']), map_files=len(r['map_files']))
        if 'occluded_share' in r:
            report['tc']['occluded_share'] = round(r['occluded_share'], 6)
        print('TC %.4f  TC_sem %.4f  TC_track %.4f' % (100 * r['tc'], 100 * r['tc_sem'], 100 * r['tc_track']))
    if tc and args.tc_photometric is not None:          # a key of its own: without the option the report is what it was
        report['tc_photometric'] = dict(thr=args.tc_photometric)
    if flow_photo:                                      # a key of its own: without the option the report is what it was
        report['flow_photo'] = photo_report(flow_photo['result'])
        print('flow photo  MAE warped %.4f  static %.4f  ratio %.4f' % tuple(report['flow_photo'][k] for k in ('mae_warp', 'mae_static', 'ratio')))
    if tc and args.tc_census is not None:               # a key of its own: without the option the report is what it was
        from vps_amd.flowphoto import CENSUS_EPS
        report['tc_census'] = dict(thr=args.tc_census, eps=CENSUS_EPS if args.flow_census_eps is None else args.flow_census_eps)
    if flow_census:                                     # a key of its own: without the option the report is what it was
        report['flow_census'] = census_report(flow_census['result'])
        print('flow census  CE warped %.4f  static %.4f  ratio %.4f' % tuple(report['flow_census'][k] for k in ('ce_warp', 'ce_static', 'ratio')))
    if overlay_video:                                   # a key of its own: without the option the report is what it was
        report['overlay_video'] = dict(files=overlay_video['files'], sampling=args.overlay_video_sampling)
    with open(os.path.join(args.out, 'report.json'), 'w') as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main()
