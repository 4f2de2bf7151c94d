"""Image-level evaluation in one command: the flow of the reference's tools/test_eval_ipq.py:78-180 with this package in its place:
detector (PanopticFuse) -> collect fcn_outputs / panoptic_outputs / panoptic_cls_inds -> evaluate_ssegs (palette PNGs, mIoU) ->
get_unified_pan_result -> evaluate_panoptic (pan_2ch/, pan/, gt.json, pred.json, pq.txt), all of it on the device (vps_amd/ipq.py).

    python tools/run_ipq.py --config configs/cityscapes/fuse.py --checkpoint work_dirs/cityscapes/fuse_vpct/latest.pth \\
        --flownet-checkpoint work_dirs/flownet/FlowNet2_checkpoint.pth.tar --data-root data/cityscapes --out work_dirs/cityscapes/fuse_vpct/val.pkl

    <data-root>/annotations/cityscapes_fine_val.json    cityscapes.py:45-47      images (file names), annotations, categories
    <data-root>/images/<file_name>                      cityscapes.py:34-38      the *_leftImg8bit.png inputs
    <data-root>/labels/*_gtFine_labelTrainIds.png       cityscapes.py:122        semantic ground truth
    <data-root>/panoptic/<file_name>                    cityscapes.py:48         panoptic ground-truth PNGs
Outputs (test_eval_ipq.py:146-180): <out>_ssegs/*.png and <out>_pans_unified/{pan_2ch,pan}/*.png, gt.json, pred.json, pq.txt.

`--dry-run` builds synthetic images and a synthetic PanopticFuse checkpoint pair in that layout under a temporary directory, runs
the detector once to write the labels and the panoptic ground truth from its own outputs, then runs the whole flow on the tree: PQ
must come out as 100 and the IoU of every class present as 1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='PanopticFuse image-level evaluation (vps_amd)')
    ap.add_argument('--config', default=os.path.join(ROOT, 'configs', 'cityscapes', 'fuse.py'))
    ap.add_argument('--checkpoint', default='work_dirs/cityscapes/fuse_vpct/latest.pth')
    ap.add_argument('--flownet-checkpoint', default='work_dirs/flownet/FlowNet2_checkpoint.pth.tar')
    ap.add_argument('--data-root', default='data/cityscapes')
    ap.add_argument('--out', default='work_dirs/cityscapes/fuse_vpct/val.pkl')
    ap.add_argument('--stuff-area-limit', type=int, default=2048, help='configs/cityscapes/test_cityscapes_1gpu.yaml:29')
    ap.add_argument('--prec', default='f16x3', choices=['f32', 'bf16x6', 'f16x3'])
    ap.add_argument('--tubes', action='store_true', help='write <out>_pans_unified/tubes.json: the COCO run-length encoding, box and area of every instance of every '
                    'image (vps_amd.tubes; one "video" of one frame per image; off by default)')
    ap.add_argument('--boundary', action='store_true', help='also write <out>_pans_unified/bpq.txt: boundary PQ (vps_amd.boundary; off by default)')
    ap.add_argument('--boundary-ratio', type=float, default=0.02, help='--boundary: width of the band as a fraction of the image diagonal')
    ap.add_argument('--dry-run', action='store_true')
    ap.add_argument('--height', type=int, default=128); ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--dry-images', type=int, default=3)
    ap.add_argument('--work-dir', default=None, help='--dry-run: where the synthetic tree goes (default: a temporary directory, removed afterwards)')
    return ap.parse_args(argv)


def color_generator(categories):
    try:
        from panopticapi.utils import IdGenerator
        return IdGenerator(categories)
    except ImportError:
        from run_vps_synthetic import ColorGenerator          # same get_color(cat_id) contract (panopticapi is absent offline)
        return ColorGenerator(categories)


def make_dry_run_tree(args, tmp):
    import vps_amd
    from collections import OrderedDict
    from PIL import Image
    from vps_amd import synth
    H, W = args.height, args.width
    cfg = vps_amd.Config.fromfile(args.config)
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    sd = synth.synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, 0)
    wd = os.path.join(tmp, 'work_dirs')
    os.makedirs(wd, exist_ok=True)
    args.flownet_checkpoint = os.path.join(wd, 'FlowNet2_checkpoint.pth.tar')
    torch.save({'epoch': 0, 'state_dict': {k[len('flownet2.'):]: v for k, v in sd.items() if k.startswith('flownet2.')}}, args.flownet_checkpoint)
    args.checkpoint = os.path.join(wd, 'latest.pth')
    torch.save({'meta': {'epoch': 12, 'CLASSES': ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')},
                'state_dict': OrderedDict(('module.' + k, v) for k, v in sd.items()), 'optimizer': {}}, args.checkpoint)
    root = os.path.join(tmp, 'data', 'cityscapes')
    for d in ('images', 'labels', 'panoptic', 'annotations'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    images = []
    for i in range(args.dry_images):
        name = 'frankfurt_%06d_%06d_leftImg8bit.png' % (i, 19)
        fr = synth.synth_frame(H, W, seed=i, shift=(0, 0), noise=0.0).astype(np.uint8)                 # BGR
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(os.path.join(root, 'images', name))
        images.append(dict(id=name.replace('_leftImg8bit.png', ''), file_name=name, height=H, width=W))
    cats = [{'id': c, 'name': 'class%d' % c, 'isthing': 1 if c >= 11 else 0, 'color': [(37 * c) % 256, (91 * c) % 256, (53 * c + 80) % 256]} for c in range(19)]
    json.dump(dict(images=images, annotations=[], categories=cats), open(os.path.join(root, 'annotations', 'cityscapes_fine_val.json'), 'w'))
    args.data_root = root
    args.out = os.path.join(wd, 'val.pkl')
    return args


def detect(args, dev, gt_json):
    """test_eval_ipq.py:92-127: the detector over the image list; the maps stay on the device"""
    import vps_amd
    from vps_amd import nhwc
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[args.prec]
    cfg = vps_amd.Config.fromfile(args.config)
    cfg.model['pretrained'] = None
    model = vps_amd.build_detector(dict(cfg.model, flownet_checkpoint=args.flownet_checkpoint), train_cfg=None, test_cfg=cfg.test_cfg)
    checkpoint = vps_amd.load_checkpoint(model, args.checkpoint, map_location='cpu')
    model.CLASSES = checkpoint.get('meta', {}).get('CLASSES', ())
    model.ensure_packed(dev)
    scale = (args.width, args.height) if args.dry_run else (2048, 1024)
    prep = DeviceImagePrep(**cfg.img_norm_cfg, size_divisor=32, img_scale=scale, device=dev)
    files = [os.path.join(args.data_root, 'images', x['file_name']) for x in gt_json['images']]
    feeder = ClipFeeder(files, prep, workers=2).start()
    res = dict(all_names=[], all_ssegs=[], all_panos=[], all_pano_cls_inds=[])
    with torch.no_grad():
        for idx in range(len(files)):
            img = feeder(idx)
            meta = dict(feeder.meta(idx), iid=idx + 1)
            result = model.simple_test(img, [meta], rescale=True, ref_img=[img])       # an image is its own reference frame
            res['all_ssegs'].append(result[2]['fcn_outputs'][0].to(torch.uint8).clone())
            res['all_panos'].append(result[2]['panoptic_outputs'][0].to(torch.uint8).clone())
            res['all_pano_cls_inds'].append(result[2]['panoptic_cls_inds'].cpu().numpy())
            res['all_names'].append(os.path.basename(files[idx]))
    torch.cuda.synchronize()
    feeder.close()
    return res


def label_path(data_root, name):
    return os.path.join(data_root, 'labels', name.replace('leftImg8bit.png', 'gtFine_labelTrainIds.png'))      # cityscapes.py:122


def run(args, tmp):
    from PIL import Image
    from vps_amd import ipq
    if args.dry_run:
        args = make_dry_run_tree(args, tmp)
    assert torch.cuda.is_available(), 'the run needs the MI355X (there is no CPU path)'
    dev = torch.device('cuda:0')
    gt_file = os.path.join(args.data_root, 'annotations', 'cityscapes_fine_val.json')
    gt_json = json.load(open(gt_file))
    categories = {el['id']: el for el in gt_json['categories']}
    outputs_pano = detect(args, dev, gt_json)
    unifier = ipq.ImagePanopticUnifier(dev, 19, 9)
    if args.dry_run:
        # ground truth = this run's own outputs, written in the ground-truth layout
        two = unifier.get_unified_pan_result_device(outputs_pano['all_ssegs'], outputs_pano['all_panos'], outputs_pano['all_pano_cls_inds'],
                                                    stuff_area_limit=args.stuff_area_limit, names=outputs_pano['all_names'])
        ann, pans = ipq.ImageConverter(dev).convert([two[k] for k in sorted(two)], color_generator(categories))
        for item, a, pan, seg in zip(gt_json['images'], ann, pans, outputs_pano['all_ssegs']):
            a['image_id'] = item['id']; a['file_name'] = item['file_name']
            Image.fromarray(pan).save(os.path.join(args.data_root, 'panoptic', item['file_name']))
            Image.fromarray(seg.cpu().numpy()).save(label_path(args.data_root, item['file_name']))
        gt_json['annotations'] = ann
        json.dump(gt_json, open(gt_file, 'w'))
    # EVAL: SEMANTIC SEGMENTATION (test_eval_ipq.py:146-153)
    print("==> Semantic Segmentation PNGs will be saved at:")
    print("---", args.out.split('.pkl')[0] + '_ssegs/')
    sem = ipq.SemanticEvaluator(19, dev)
    res = sem.evaluate_ssegs(outputs_pano['all_ssegs'], args.out.replace('.pkl', '_ssegs'), outputs_pano['all_names'],
                             [label_path(args.data_root, n) for n in outputs_pano['all_names']])
    cm = res['confusion_matrix']
    present = (cm.sum(0) + cm.sum(1)) > 0
    print('meanIU over the classes present: %.5f' % res['IU_array'][present].mean())
    # EVAL: IMAGE PANOPTIC SEGMENTATION (:155-180)
    print("==> Image Panoptic Segmentation PNGs and PQ.TXT will be saved at:")
    print("---", args.out.split('.pkl')[0] + '_pans_unified/')
    two = unifier.get_unified_pan_result_device(outputs_pano['all_ssegs'], outputs_pano['all_panos'], outputs_pano['all_pano_cls_inds'],
                                                stuff_area_limit=args.stuff_area_limit, names=outputs_pano['all_names'])
    pred_pans_2ch = [two[k] for k in sorted(two)]
    ipq.evaluate_panoptic(pred_pans_2ch, args.out.replace('.pkl', '_pans_unified'), gt_file, os.path.join(args.data_root, 'panoptic'),
                          None, color_generator(categories), device=dev)
    if args.boundary:                       # from the files evaluate_panoptic has just written: gt.json, pred.json and pan/
        from vps_amd import boundary
        out_dir = args.out.replace('.pkl', '_pans_unified')
        gt_all, pred_all = json.load(open(os.path.join(out_dir, 'gt.json'))), json.load(open(os.path.join(out_dir, 'pred.json')))
        gt_pans = [np.array(Image.open(os.path.join(args.data_root, 'panoptic', item['file_name']))) for item in gt_all['images']]
        pred_pans = [np.array(Image.open(ipq.ipq_png_name(os.path.join(out_dir, 'pan'), item['file_name']))) for item in gt_all['images']]
        boundary.bpq_compute(gt_all, pred_all, gt_pans, pred_pans, categories, out_dir, device=dev, boundary_ratio=args.boundary_ratio)
    if args.tubes:
        from vps_amd.tubes import TubeCollector
        col = TubeCollector(things_only=True, id_channel=1, device=dev)       # image-level maps: the instance id is pan_ins, 0 for stuff
        for i, name in enumerate(sorted(two)):
            col.add(i, name, two[name])
        col.write(os.path.join(args.out.replace('.pkl', '_pans_unified'), 'tubes.json'))
        col.close()
    return 0


def main(argv=None):
    args = parse_args(argv)
    tmp, own = None, False
    if args.dry_run:
        import tempfile
        tmp, own = (args.work_dir, False) if args.work_dir else (tempfile.mkdtemp(prefix='vps_ipq_'), True)
        os.makedirs(tmp, exist_ok=True)
    try:
        return run(args, tmp)
    finally:
        if own:
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
