"""BASELINE config 3 in one command: the released checkpoint + the Cityscapes-VPS val videos through the whole drop-in, the flow of
tools/test_vpq.py:93-198 (then tools/eval_vpq.py when the ground truth is given) with this package in the reference's place:

    python tools/run_config3.py --config configs/cityscapes/fusetrack.py \\
        --checkpoint work_dirs/cityscapes_vps/fusetrack_vpct/latest.pth --flownet-checkpoint work_dirs/flownet/FlowNet2_checkpoint.pth.tar \\
        --data-root data/cityscapes_vps --out work_dirs/cityscapes_vps/fusetrack_vpct/val.pkl [--truth-dir data/cityscapes_vps/val/panoptic_video]

    file / directory                                   reference                                  read by
    <data-root>/im_all_info_val_city_vps.json           configs/cityscapes/fusetrack.py:216-222    frame list, ids (iid = video*10000 + frame + 1)
    <data-root>/val/img_all/<file_name>                 img_prefix == ref_prefix                   vps_amd.pipeline.ClipFeeder (every file decoded once)
    <data-root>/panoptic_im_val_city_vps.json           test_vpq.py:86,165-169                     labelled-frame names + categories
    <checkpoint>  ('state_dict' / 'meta', 'module.')    test_vpq.py:135-143                        vps_amd.load_checkpoint (mmcv semantics)
    <flownet-checkpoint> ('state_dict')                 panoptic_fusetrack.py:100-106              detector constructor
    <truth-dir>, <data-root>/panoptic_gt_val_city_vps.json   eval_vpq.py:251-330                   tools/eval_vpq_device.py (vpq-*.txt)

Outputs (test_vpq.py:150-198): <out>_pans_unified/{pan_2ch,pan_pred}/*.png + pred.json, and the VPQ tables when --truth-dir is given.
The artefacts do not exist offline (no weights, no dataset). `--dry-run` writes a synthetic checkpoint pair IN THE
REFERENCE'S FILE LAYOUT ('module.'-prefixed state_dict + meta; FlowNet2 'state_dict') and a synthetic dataset tree (PNG frames, the
two json files, ground truth = the run's own prediction) into a scratch directory and runs the same code on it;
`--check-only` stops after the model is built, the checkpoints are loaded (missing / unexpected keys reported) and the dataset is
listed - no GPU needed. One JSON report line on stdout.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='VPSNet FuseTrack test on Cityscapes-VPS (vps_amd)')
    ap.add_argument('--config', default=os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    ap.add_argument('--checkpoint', default='work_dirs/cityscapes_vps/fusetrack_vpct/latest.pth')
    ap.add_argument('--flownet-checkpoint', default='work_dirs/flownet/FlowNet2_checkpoint.pth.tar')
    ap.add_argument('--data-root', default='data/cityscapes_vps')
    ap.add_argument('--out', default='work_dirs/cityscapes_vps/fusetrack_vpct/val.pkl', help='like test_vpq.py --out: <out minus .pkl>_pans_unified/ receives the results')
    ap.add_argument('--mode', default='val', choices=['val', 'test'])
    ap.add_argument('--n-video', type=int, default=50)
    ap.add_argument('--nframes-span-test', type=int, default=30)
    ap.add_argument('--stuff-area-limit', type=int, default=2048, help='configs/cityscapes/test_cityscapes_1gpu.yaml:29')
    ap.add_argument('--truth-dir', default=None, help='ground-truth PNG directory: evaluate with tools/eval_vpq_device.py afterwards')
    ap.add_argument('--pan-gt-json', default=None)
    ap.add_argument('--prec', default='f16x3', choices=['f32', 'bf16x6', 'f16x3'])
    ap.add_argument('--strict', action='store_true', help='load_checkpoint(strict=True): missing / unexpected keys are fatal')
    ap.add_argument('--png-workers', type=int, default=6)
    ap.add_argument('--device-png', action='store_true', help='encode the result PNGs on the device (postprocess.DevicePngWriter) instead of PIL threads')
    ap.add_argument('--png-huffman', default='fixed', choices=['fixed', 'dynamic'], help="--device-png, --flow-format png|kitti and PNG error maps: the Huffman code of the device deflate stage. fixed (default): the fixed code, right for label maps; dynamic: a code per 8 KiB segment where that is shorter, for dense images")
    ap.add_argument('--overlay', default=None, metavar='DIR', help='write DIR/<name>.jpg for every frame: the panoptic result blended over the frame (off by default; '
                    'keeps every decoded frame on the device until the maps are unified, 6 MB per frame at 1024x2048)')
    ap.add_argument('--overlay-quality', type=int, default=90)
    ap.add_argument('--overlay-video', default=None, metavar='FILE.y4m', help='write the overlays of every video as one Y4M stream (YUV4MPEG2; with several '
                    'videos the video\'s name goes in front of the extension), beside --overlay or without it (off by default)')
    ap.add_argument('--overlay-video-sampling', default='420jpeg', choices=['420jpeg', '420mpeg2', '444'])
    ap.add_argument('--video', default=None, metavar='FILE.y4m', help='run ONE clip from a Y4M file (ffmpeg -i in.mp4 -f yuv4mpegpipe in.y4m) instead of the '
                    'dataset\'s image list: every frame is a result frame (no labelled-frame selection), the dataset files and the evaluation are not '
                    'used; with --dry-run a synthetic clip of --dry-frames frames is written to a file of that name in the scratch directory')
    ap.add_argument('--video-matrix', default='bt601', choices=['bt601', 'bt709'], help='--video: the colour matrix of the clip (Y4M has no tag for it)')
    ap.add_argument('--jpeg-entropy', default='host', choices=['host', 'device'],
                    help='where the JPEG files of --overlay and --flow are Huffman-coded; the files are the same (default host)')
    ap.add_argument('--overlay-alpha', type=int, default=128, help='weight of the colour map, 0..256')
    ap.add_argument('--flow', default=None, metavar='DIR', help='write DIR/<name>.<ext> for every frame: the FlowNet2 flow of the frame (off by default)')
    ap.add_argument('--flow-format', default='jpg', choices=['jpg', 'png', 'flo', 'kitti'], help="colour image (jpg, png), the raw Middlebury field (flo) or the KITTI devkit's 16-bit PNG (kitti)")
    ap.add_argument('--flow-max-rad', type=float, default=None, metavar='X', help='one normaliser of the flow colours for all frames (default: each frame its own maximum)')
    ap.add_argument('--tubes', action='store_true', help='write tubes.json beside pred.json: the COCO run-length encoding, box and area of every tracked instance in '
                    'every labelled frame (vps_amd.tubes; off by default)')
    ap.add_argument('--stq', action='store_true', help='after the VPQ step, score the same files with tools/eval_stq_device.py: stq.txt and stq-tracks.json '
                    'beside the vpq-*.txt files (needs the ground truth; off by default)')
    ap.add_argument('--boundary', action='store_true', help='with the VPQ step: also write bvpq-<k>.txt and bvpq-final.txt, boundary VPQ (vps_amd.boundary; needs '
                    'the ground truth; off by default)')
    ap.add_argument('--boundary-ratio', type=float, default=0.02, help='--boundary: width of the band as a fraction of the image diagonal')
    ap.add_argument('--tc', action='store_true', help='temporal consistency without ground truth (vps_amd.tc): every frame against the previous one of its '
                    'video warped by the detector\'s own flow; tc.txt and tc-tracks.json beside pred.json, also with --video (keeps the flow of every frame '
                    'on the device until the maps are unified and its pair is counted, 16.8 MB per frame at 1024x2048; off by default)')
    ap.add_argument('--tc-map', default=None, metavar='DIR', help='--tc: write DIR/<name>.jpg for every frame but a video\'s first, the inconsistency map '
                    'blended over the frame (red: class differs, amber: track differs, blue: not in view); keeps the decoded frames like --overlay')
    ap.add_argument('--tc-occlusion', action='store_true', help='--tc with a forward-backward flow check, also with --video and --tc-map: a second FlowNet2 '
                    'pass behind every frame gives the flow from the previous frame to this one (another 16.8 MB per frame at 1024x2048 until its pair is '
                    'counted); pixels where the two flows do not cancel (disocclusions) are left out of the counts and reported as the occluded share '
                    '(OCC in tc.txt, grey in the --tc-map images; off by default)')
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--flow-photo', action='store_true', help='flow quality without ground truth (vps_amd.flowphoto), also with --video: the photometric warp '
                    'error of every frame\'s flow between the frame and the previous one of its video, beside the static error of not warping; '
                    'flow-photo.txt and flow-photo.json beside pred.json (keeps the flow and the decoded frame of every frame; with --tc-occlusion the '
                    'occlusion mask splits the pixels into a visible and a masked group; flagged above --tc-photometric if given, else 16 grey levels; '
                    'off by default)')
    ap.add_argument('--flow-photo-map', default=None, metavar='DIR', help='--flow-photo: write DIR/<name>.jpg for every frame but a video\'s first, the '
                    'photometric residual blended over the frame')
    ap.add_argument('--tc-photometric', type=float, default=None, metavar='THR', help='--tc-occlusion, and pixels that are in view and not occluded but whose '
                    'photometric warp error is above THR grey levels are left out of the counts too (they are part of OCC then; off by default)')
    ap.add_argument('--flow-census', action='store_true', help='illumination-robust flow quality without ground truth (vps_amd.flowphoto, DESIGN.md 6 row '
                    '3i), also with --video: the ternary census residual of every frame\'s flow between the frame and the previous one of its video, '
                    'beside the static one of not warping; flow-census.txt and flow-census.json beside pred.json (as --flow-photo; flagged above '
                    '--tc-census if given, else 25 percent; off by default)')
    ap.add_argument('--flow-census-map', default=None, metavar='DIR', help='--flow-census: write DIR/<name>.jpg for every frame but a video\'s first, the '
                    'census residual blended over the frame')
    ap.add_argument('--tc-census', type=int, default=None, metavar='THR', help='--tc-occlusion, and pixels that are in view and not occluded but whose '
                    'census residual is above THR percent of their counted neighbours are left out of the counts too (they are part of OCC then; may '
                    'be combined with --tc-photometric; off by default)')
    ap.add_argument('--dry-size', default='128x256'); ap.add_argument('--dry-videos', type=int, default=1); ap.add_argument('--dry-frames', type=int, default=16)
    ap.add_argument('--check-only', action='store_true')
    return ap.parse_args(argv)


def make_dry_run_artefacts(args, tmp):
    """synthetic artefacts in the layout of download_weights.sh / the dataset README: returns the patched args"""
    import vps_amd
    from PIL import Image
    from vps_amd import synth
    H, W = [int(v) for v in args.dry_size.split('x')]
    cfg = vps_amd.Config.fromfile(args.config)
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    sd = synth.synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, 0)
    os.makedirs(os.path.join(tmp, 'work_dirs', 'flownet'), exist_ok=True)
    os.makedirs(os.path.join(tmp, 'work_dirs', 'cityscapes_vps', 'fusetrack_vpct'), exist_ok=True)
    fn = {k[len('flownet2.'):]: v for k, v in sd.items() if k.startswith('flownet2.')}
    args.flownet_checkpoint = os.path.join(tmp, 'work_dirs', 'flownet', 'FlowNet2_checkpoint.pth.tar')
    torch.save({'epoch': 0, 'state_dict': fn}, args.flownet_checkpoint)
    # latest.pth as mmcv's save_checkpoint writes it from a MMDistributedDataParallel model: 'module.' prefix, 'meta', an optimizer blob
    from collections import OrderedDict
    args.checkpoint = os.path.join(tmp, 'work_dirs', 'cityscapes_vps', 'fusetrack_vpct', 'latest.pth')
    torch.save({'meta': {'epoch': 12, 'CLASSES': ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')},
                'state_dict': OrderedDict(('module.' + k, v) for k, v in sd.items()), 'optimizer': {}}, args.checkpoint)
    root = os.path.join(tmp, 'data', 'cityscapes_vps')
    img_dir = os.path.join(root, args.mode, 'img_all')
    os.makedirs(img_dir, exist_ok=True)
    images, labelled = [], []
    for v in range(args.dry_videos):
        for f in range(args.dry_frames):
            name = '%04d_%04d_frankfurt_%06d_%06d_newImg8bit.png' % (v, f, v, f)
            fr = synth.synth_frame(H, W, seed=v, shift=(2 * f, f), noise=2.0 if f else 0.0).astype(np.uint8)       # BGR
            Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(os.path.join(img_dir, name))
            images.append(dict(id=v * 10000 + f + 1, file_name=name, height=H, width=W))
            if f % 5 == args.dry_label_first % 5 and f >= args.dry_label_first:
                # panoptic_im_*.json: id = the frame's base name (eval_vpq.py:280 opens pan_pred/<id>.png), file_name = the image name
                labelled.append(dict(id=name.replace('_newImg8bit.png', ''), file_name=name, height=H, width=W))
    cats = [{'id': c, 'name': 'class%d' % c, 'isthing': 1 if c >= 11 else 0, 'color': [(37 * c) % 256, (91 * c) % 256, (53 * c + 80) % 256]} for c in range(19)]
    json.dump(dict(images=images, categories=cats), open(os.path.join(root, 'im_all_info_%s_city_vps.json' % args.mode), 'w'))
    json.dump(dict(images=labelled, categories=cats), open(os.path.join(root, 'panoptic_im_%s_city_vps.json' % args.mode), 'w'))
    args.data_root = root
    args.out = os.path.join(tmp, 'work_dirs', 'cityscapes_vps', 'fusetrack_vpct', args.mode + '.pkl')
    args.n_video, args.nframes_span_test = args.dry_videos, args.dry_frames
    if args.video and not torch.cuda.is_available() and not args.check_only:
        raise SystemExit('--dry-run --video writes its clip through Y4mWriter, which converts on the device: no device here (only --check-only runs without one)')
    if args.video and torch.cuda.is_available():
        # the clip of --video: the frames of video 0 through the product's own writer (converted on the device, so only with one)
        from vps_amd.y4m import Y4mWriter
        args.video = os.path.join(tmp, os.path.basename(args.video))
        w = Y4mWriter(args.video, W, H, fps=(17, 1), sampling='420jpeg')
        for f in range(args.dry_frames):
            fr = synth.synth_frame(H, W, seed=0, shift=(2 * f, f), noise=2.0 if f else 0.0).astype(np.uint8)
            fr = np.pad(fr, ((0, H - fr.shape[0]), (0, W - fr.shape[1]), (0, 0)), mode='edge')      # late frames are cropped at the noise field's edge
            w.submit(torch.from_numpy(np.ascontiguousarray(fr)).cuda())
        w.close()
    return args


def main(argv=None):
    args = parse_args(argv)
    args.dry_label_first = 0
    tmp = None
    if args.dry_run:
        import tempfile
        tmp = tempfile.mkdtemp(prefix='vps_config3_')
    try:
        return run(args, tmp)
    finally:
        if tmp and not os.environ.get('VPS_KEEP_DRY_RUN'):
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)


def run(args, tmp):
    report = dict(config=args.config, dry_run=bool(args.dry_run), prec=args.prec)
    if args.dry_run:
        args = make_dry_run_artefacts(args, tmp)
    import vps_amd
    from vps_amd import nhwc
    dataset_files = [os.path.join(args.data_root, 'im_all_info_%s_city_vps.json' % args.mode), os.path.join(args.data_root, 'panoptic_im_%s_city_vps.json' % args.mode)]
    if args.video:
        dataset_files = [args.video] if not (args.dry_run and args.check_only) else []
    for f in [args.checkpoint, args.flownet_checkpoint] + dataset_files:
        if not os.path.exists(f):
            print(json.dumps(dict(report, error='missing artefact: %s (the reference fetches it with download_weights.sh / the dataset README; '
                                                'use --dry-run for synthetic stand-ins)' % f)))
            return 2
    # ---- test_vpq.py:129-143: build, load, classes ---------------------------------------------------------------------------
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[args.prec]
    cfg = vps_amd.Config.fromfile(args.config)
    cfg.model['pretrained'] = None
    model = vps_amd.build_detector(dict(cfg.model, flownet_checkpoint=args.flownet_checkpoint), train_cfg=None, test_cfg=cfg.test_cfg)
    checkpoint = vps_amd.load_checkpoint(model, args.checkpoint, map_location='cpu', strict=args.strict)
    rep = checkpoint.get('_vps_load_report', {})
    model.CLASSES = checkpoint.get('meta', {}).get('CLASSES', ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle'))
    report['checkpoint'] = dict(file=args.checkpoint, loaded=rep.get('loaded'), missing=rep.get('missing'), unexpected=rep.get('unexpected'),
                                classes=list(model.CLASSES))
    # ---- the dataset list (cityscapes_vps.py:137-148: the previous frame is the reference, a video's first frame its own) -----------
    reader = None
    if args.video:
        # ONE clip from a Y4M file: frame f is '<stem>_<f, six digits>.png' in every output, every frame is a result frame, one video
        from run_vps_synthetic import CATEGORIES
        from vps_amd.y4m import Y4mReader
        stem, nfr = os.path.splitext(os.path.basename(args.video))[0], 0
        if os.path.exists(args.video):
            reader = Y4mReader(args.video)
            nfr = len(reader)
            report['video'] = dict(file=args.video, frames=nfr, size=[reader.info.H, reader.info.W], sampling=reader.info.sampling, range=reader.info.range,
                                   fps=list(reader.info.fps), dropped_partial_frames=reader.dropped, matrix=args.video_matrix)
        info = [dict(id=f + 1, file_name='%s_%06d.png' % (stem, f)) for f in range(nfr)]
        img_prefix, categories = os.path.dirname(os.path.abspath(args.video)), CATEGORIES
        im_jsons = dict(images=[dict(id=x['file_name'][:-4], file_name=x['file_name']) for x in info], categories=categories)
        args.n_video, args.nframes_span_test = 1, max(nfr, 1)
    else:
        info = json.load(open(os.path.join(args.data_root, 'im_all_info_%s_city_vps.json' % args.mode)))['images']
        img_prefix = os.path.join(args.data_root, args.mode, 'img_all')
        im_jsons = json.load(open(os.path.join(args.data_root, 'panoptic_im_%s_city_vps.json' % args.mode)))
        categories = im_jsons['categories']
    names = sorted(x['file_name'] for x in im_jsons['images'])
    span = args.nframes_span_test
    report['dataset'] = dict(frames=len(info), videos=len(info) // max(span, 1), labelled_frames=len(names), img_prefix=img_prefix)
    if args.check_only:
        print(json.dumps(report))
        return 0
    assert torch.cuda.is_available(), 'the run needs the MI355X (there is no CPU path); --check-only stops before it'
    dev = torch.device('cuda:0')
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    from vps_amd.postprocess import PanopticUnifier, inference_panoptic_video
    model.ensure_packed(dev)
    prep = DeviceImagePrep(**cfg.img_norm_cfg, size_divisor=32, img_scale=(2048, 1024), device=dev)
    files = [os.path.join(img_prefix, x['file_name']) for x in info]
    if args.tc_photometric is not None or args.tc_census is not None:
        args.tc_occlusion = True
    with_photo = bool(args.flow_photo or args.flow_photo_map)
    with_census = bool(args.flow_census or args.flow_census_map)
    keep = bool(args.overlay or args.overlay_video or args.tc_map or with_photo or with_census or args.tc_photometric is not None
                or args.tc_census is not None)
    with_tc = bool(args.tc or args.tc_map or args.tc_occlusion)
    if reader is not None:
        assert len(reader) > 0, '%s holds no complete frame' % args.video
        feeder = ClipFeeder(reader, prep, workers=args.png_workers, keep_frames=keep, y4m_matrix=args.video_matrix).start()
    else:
        feeder = ClipFeeder(files, prep, workers=args.png_workers, keep_frames=keep).start()
    res = dict(all_names=[], all_ssegs=[], all_panos=[], all_pano_cls_inds=[], all_pano_obj_ids=[], all_frames=[])
    flow_writer = None
    if args.flow:
        from vps_amd.flowvis import FlowWriter, flow_name
        model.keep_flow = True
        flow_writer = FlowWriter(dev, fmt=args.flow_format, max_rad=args.flow_max_rad, entropy=args.jpeg_entropy, huffman=args.png_huffman)
    if with_tc or with_photo or with_census:
        model.keep_flow = True
        res['all_flows'] = []
    if args.tc_occlusion:
        res['all_back_flows'] = []
    t0 = time.perf_counter()
    with torch.no_grad():
        for idx, im in enumerate(info):
            img = feeder(idx)
            ref = feeder(idx - 1) if idx % span > 0 else img
            nxt = idx + 1 if idx + 1 < len(info) else None
            meta = dict(feeder.meta(idx), iid=im['id'])       # filename, ori_shape, img_shape, pad_shape, scale_factor, flip + the video index
            if reader is not None:
                meta['dataset'] = 'cityscapes_vps'       # the tracking detector checks for Cityscapes-VPS file names otherwise; the clip's is '<path>#<t>'
            # the next pair is known: its image-only stages are announced to the detector (the drop-in's own clip pipelining)
            pf = (feeder(nxt), img) if (nxt is not None and nxt % span > 0) else None
            result = model.simple_test(img, [meta], rescale=True, ref_img=[ref], prefetch=pf)
            res['all_ssegs'].append(result[2]['fcn_outputs'][0]); res['all_panos'].append(result[2]['panoptic_outputs'][0])
            res['all_pano_cls_inds'].append(result[2]['panoptic_cls_inds'].cpu().numpy())
            res['all_pano_obj_ids'].append(result[2]['panoptic_det_obj_ids'].cpu().numpy())
            res['all_names'].append(os.path.basename(files[idx]))
            if keep:
                res['all_frames'].append(feeder.frame(idx))       # the decoded BGR frame the feeder holds anyway
            if flow_writer is not None:
                flow_writer.submit(result[2]['flow'], flow_name(args.flow, files[idx], args.flow_format))
            if with_tc or with_photo or with_census:
                res['all_flows'].append(result[2]['flow'])
            if args.tc_occlusion:                            # the flow from the previous frame to this one: a second FlowNet2 pass, behind the frame
                res['all_back_flows'].append(model.flow_between(ref, img, img_shape=meta['img_shape']) if idx % span > 0 else None)
    torch.cuda.synchronize()
    if flow_writer is not None:
        flow_files = flow_writer.close()
        report['flow'] = dict(dir=args.flow, files=len(flow_files), format=args.flow_format, max_rad=args.flow_max_rad, bytes=flow_writer.bytes_written)
    dt = time.perf_counter() - t0
    feeder.close()
    # ---- test_vpq.py:150-198 ------------------------------------------------------------------------------------------------------
    output_dir = args.out.replace('.pkl', '_pans_unified/')
    unifier = PanopticUnifier(dev, 19, 9)
    two = unifier.get_unified_pan_result(res['all_ssegs'], res['all_panos'], res['all_pano_cls_inds'], obj_ids=res['all_pano_obj_ids'],
                                         stuff_area_limit=args.stuff_area_limit, names=res['all_names'])
    pred_pans_2ch = [two[k] for k in sorted(two.keys())]
    try:
        from panopticapi.utils import IdGenerator
        gen = IdGenerator({c['id']: c for c in categories})
    except ImportError:
        from run_vps_synthetic import ColorGenerator          # stand-in with the same get_color(cat_id) contract (panopticapi is absent offline)
        gen = ColorGenerator({c['id']: c for c in categories})
    kw = {}
    if args.video:
        kw = dict(labeled_fid=0, lambda_=1, nframes_per_video=len(names))                  # every frame, one video
    elif args.dry_run:
        kw = dict(labeled_fid=args.dry_label_first, lambda_=5, nframes_per_video=len(names) // max(args.n_video, 1))
    if args.device_png:
        from vps_amd.postprocess import DevicePngWriter
        kw['writer'] = DevicePngWriter(dev, huffman=args.png_huffman)
    if args.tubes:
        from vps_amd.tubes import TubeCollector
        kw['tubes'] = TubeCollector(things_only=True, device=dev, id_last_stuff=unifier.id_last_stuff)
    pans, pj = inference_panoptic_video(pred_pans_2ch, output_dir, categories, names, n_video=args.n_video, color_generator=gen, device=dev, **kw)
    if args.device_png:
        kw['writer'].close()
    if args.tubes:
        tb = kw['tubes'].result()
        report['tubes'] = dict(file=os.path.join(output_dir, 'tubes.json'), videos=len(tb['videos']), tracks=sum(len(v['tracks']) for v in tb['videos']))
        kw['tubes'].close()
    if with_photo:                                          # a key of its own: without the options the report is what it was
        from run_vps_synthetic import photo_report
        from vps_amd import flowphoto
        order = sorted(range(len(res['all_names'])), key=lambda i: res['all_names'][i])                # the order of pred_pans_2ch
        pev = flowphoto.PhotoEvaluator(dev, thr=flowphoto.PHOTO_THR if args.tc_photometric is None else args.tc_photometric, per_pair=True)
        pfiles = flowphoto.score_videos(pev, [res['all_frames'][i] for i in order], [res['all_flows'][i] for i in order], [res['all_names'][i] for i in order],
                                        span, back_flows=[res['all_back_flows'][i] for i in order] if args.tc_occlusion else None,
                                        map_dir=args.flow_photo_map, alpha=args.overlay_alpha, quality=args.overlay_quality, entropy=args.jpeg_entropy)
        pr = pev.result()
        flowphoto.write_outputs(pr, output_dir)
        pr['map_files'] = pfiles
        report['flow_photo'] = dict(photo_report(pr), file=os.path.join(output_dir, 'flow-photo.txt'))
        print('flow photo  MAE warped %.4f  static %.4f  ratio %.4f' % tuple(report['flow_photo'][k] for k in ('mae_warp', 'mae_static', 'ratio')))
    if with_census:                                         # a key of its own: without the options the report is what it was
        from run_vps_synthetic import census_report
        from vps_amd import flowphoto
        order = sorted(range(len(res['all_names'])), key=lambda i: res['all_names'][i])                # the order of pred_pans_2ch
        cev = flowphoto.CensusEvaluator(dev, thr=flowphoto.CENSUS_THR if args.tc_census is None else args.tc_census, per_pair=True)
        cfiles = flowphoto.score_videos(cev, [res['all_frames'][i] for i in order], [res['all_flows'][i] for i in order], [res['all_names'][i] for i in order],
                                        span, back_flows=[res['all_back_flows'][i] for i in order] if args.tc_occlusion else None,
                                        map_dir=args.flow_census_map, alpha=args.overlay_alpha, quality=args.overlay_quality, entropy=args.jpeg_entropy)
        cr = cev.result()
        flowphoto.write_census_outputs(cr, output_dir)
        cr['map_files'] = cfiles
        report['flow_census'] = dict(census_report(cr), file=os.path.join(output_dir, 'flow-census.txt'))
        print('flow census  CE warped %.4f  static %.4f  ratio %.4f' % tuple(report['flow_census'][k] for k in ('ce_warp', 'ce_static', 'ratio')))
    if with_tc:                                             # a key of its own: without the options the report is what it was
        from vps_amd import tc
        nseg = 19                                           # PanopticUnifier(dev, 19, 9): the 19 classes are their own indices, the rest is void
        seg_class = np.full(256, 255, dtype=np.uint8)
        seg_class[:nseg] = np.arange(nseg)
        okw = {}
        if args.tc_census is not None:
            ev = tc.TcEvaluator(seg_class, nseg, id_channel=2, device=dev, per_pair=True, id_last_stuff=unifier.id_last_stuff, occlusion=True,
                                photometric=args.tc_photometric, census=args.tc_census)
            report['tc_census'] = dict(thr=args.tc_census, eps=ev.census_eps)
            if args.tc_photometric is not None:
                report['tc_photometric'] = dict(thr=args.tc_photometric)
        elif args.tc_photometric is not None:
            ev = tc.TcEvaluator(seg_class, nseg, id_channel=2, device=dev, per_pair=True, id_last_stuff=unifier.id_last_stuff, occlusion=True,
                                photometric=args.tc_photometric)
            report['tc_photometric'] = dict(thr=args.tc_photometric)
        elif args.tc_occlusion:
            ev = tc.TcEvaluator(seg_class, nseg, id_channel=2, device=dev, per_pair=True, id_last_stuff=unifier.id_last_stuff, occlusion=True)
        else:
            ev = tc.TcEvaluator(seg_class, nseg, id_channel=2, device=dev, per_pair=True, id_last_stuff=unifier.id_last_stuff)
        order = sorted(range(len(res['all_names'])), key=lambda i: res['all_names'][i])                # the order of pred_pans_2ch
        flows = [res['all_flows'][i] for i in order]
        res['all_flows'] = None                             # `flows` holds them now and lets each one go once its pair is counted
        if args.tc_occlusion:
            okw['back_flows'] = [res['all_back_flows'][i] for i in order]
            res['all_back_flows'] = None
        tfiles = tc.score_videos(ev, pred_pans_2ch, flows, [res['all_names'][i] for i in order], span, map_dir=args.tc_map,
                                 frames=[res['all_frames'][i] for i in order] if (args.tc_map or args.tc_photometric is not None or args.tc_census is not None) else None,
                                 alpha=args.overlay_alpha,
                                 quality=args.overlay_quality, entropy=args.jpeg_entropy, **okw)
        r = ev.result()
        tc.write_outputs(r, output_dir)
        report['tc'] = dict(tc=round(100 * r['tc'], 4), tc_sem=round(100 * r['tc_sem'], 4), tc_track=round(100 * r['tc_track'], 4), tracks=r['n_tracks'],
                            in_view_share=round(r['in_view_share'], 6), pairs=len(r['per_pair']), map_files=len(tfiles), file=os.path.join(output_dir, 'tc.txt'))
        if 'occluded_share' in r:
            report['tc']['occluded_share'] = round(r['occluded_share'], 6)
        print('TC %.4f  TC_sem %.4f  TC_track %.4f' % (100 * r['tc'], 100 * r['tc_sem'], 100 * r['tc_track']))
    if keep and (args.overlay or args.overlay_video):
        from run_vps_synthetic import ColorGenerator
        from vps_amd.postprocess import write_overlays
        order = sorted(range(len(res['all_names'])), key=lambda i: res['all_names'][i])                # the order of pred_pans_2ch
        vfiles = []
        vkw = dict(video=args.overlay_video, video_sampling=args.overlay_video_sampling, video_files=vfiles) if args.overlay_video else {}
        ov = write_overlays(pred_pans_2ch, [res['all_frames'][i] for i in order], [res['all_names'][i] for i in order], args.overlay,
                            ColorGenerator({c['id']: c for c in categories}), span, device=dev, quality=args.overlay_quality, alpha=args.overlay_alpha,
                            entropy=args.jpeg_entropy, **vkw)
    if args.overlay_video:                                  # keys of their own: without the options the report is what it was
        report['overlay_video'] = dict(files=vfiles, sampling=args.overlay_video_sampling, bytes=sum(os.path.getsize(f) for f in vfiles))
    if args.overlay:
        report['overlay'] = dict(dir=args.overlay, files=len(ov), quality=args.overlay_quality, alpha=args.overlay_alpha, entropy=args.jpeg_entropy)
    if reader is not None:
        report['video']['native_y4m'] = feeder.native_y4m
    report['run'] = dict(frames=len(info), seconds=round(dt, 3), frames_per_s=round(len(info) / dt, 2), decodes=feeder.decodes, output_dir=output_dir,
                         png_files=len(os.listdir(os.path.join(output_dir, 'pan_pred'))))
    truth_dir, gt_json = (None, None) if args.video else (args.truth_dir, args.pan_gt_json)       # a clip from a file has no ground truth
    if args.dry_run and not args.video:
        # ground truth = this run's own prediction, written in the ground-truth layout: the reference's metric must come out as 100
        truth_dir = os.path.join(args.data_root, args.mode, 'panoptic_video')
        os.makedirs(truth_dir, exist_ok=True)
        import shutil
        ims = sorted(im_jsons['images'], key=lambda x: x['file_name'])
        for im in ims:          # eval_vpq.py:272-276: ground-truth PNG = <image name> with _newImg8bit.png -> _final_mask.png
            shutil.copy(os.path.join(output_dir, 'pan_pred', im['id'] + '.png'), os.path.join(truth_dir, im['file_name'].replace('_newImg8bit.png', '_final_mask.png')))
        gt_json = os.path.join(args.data_root, 'panoptic_gt_%s_city_vps.json' % args.mode)
        json.dump(dict(annotations=pj['annotations'], categories=categories, images=ims), open(gt_json, 'w'))
    if truth_dir:
        import eval_vpq_device
        ev = ['--submit_dir', output_dir, '--truth_dir', truth_dir, '--pan_gt_json_file', gt_json or os.path.join(args.data_root, 'panoptic_gt_%s_city_vps.json' % args.mode)]
        if args.dry_run:
            ev += ['--nframes_per_video', str(len(names) // max(args.n_video, 1))]
        eval_vpq_device.main(ev + (['--boundary', '--boundary-ratio', str(args.boundary_ratio)] if args.boundary else []))
        fin = os.path.join(output_dir, 'vpq-final.txt')
        report['vpq_final'] = open(fin).read().strip().splitlines()[-3:] if os.path.exists(fin) else None
        if args.boundary:                                   # a key of its own: without the option the report is what it was
            report['bvpq_final'] = open(os.path.join(output_dir, 'bvpq-final.txt')).read().strip().splitlines()[-3:]
        if args.stq:                                        # a key of its own: without the option the report is what it was
            import eval_stq_device
            r = eval_stq_device.main(ev + ['--device', str(dev)])
            report['stq'] = dict(stq=round(100 * r['stq'], 4), aq=round(100 * r['aq'], 4), sq=round(100 * r['sq'], 4), tracks=r['n'],
                                 file=os.path.join(output_dir, 'stq.txt'))
            print('STQ %.4f  AQ %.4f  SQ %.4f' % (100 * r['stq'], 100 * r['aq'], 100 * r['sq']))
    print(json.dumps(report))
    return 0


if __name__ == '__main__':
    sys.exit(main())
