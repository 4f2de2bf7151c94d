"""Optical-flow accuracy of a directory of flow files against ground truth: end-point error, Fl outlier rate, Sintel's speed bins, the
shares within 1 / 3 / 5 px and, with ground-truth occlusions, EPE noc / occ. Every pair is counted on the device into tables that stay
there (vps_amd.floweval.FlowEvaluator -> vps_flow_error), one download at the end.

    python tools/run_config3.py ... --flow work_dirs/flow --flow-format flo
    python tools/eval_flow_device.py --pred work_dirs/flow --gt data/sintel/flow [--mask data/sintel/invalid] [--occ-mask data/sintel/occlusions]
                                     [--error-map work_dirs/flow_err [--format jpg|png]] [--out work_dirs/flow]
    python tools/eval_flow_device.py --pred work_dirs/flow --gt data/kitti/flow_occ [--gt-noc data/kitti/flow_noc]

Files are matched by stem. A prediction or a ground truth is NAME.flo (Middlebury) or NAME.png (the KITTI devkit's 16-bit PNG,
vps_amd/kittiflow.py: decoded on the device), chosen per file by its extension; a directory that holds both for one stem is refused.
.flo ground truth: --mask names 8-bit PNGs, non-zero = invalid (Sintel's `invalid`), --occ-mask 8-bit PNGs, non-zero = occluded in the
ground truth (Sintel's `occlusions`); the two are combined into the kernel's mask byte: 0 invalid, 1 valid and not occluded, 2 valid and
occluded. KITTI ground truth carries its own validity: --gt names the flow_occ directory (every labelled pixel), --gt-noc the flow_noc
directory (the non-occluded ones), which gives the same mask byte; --mask and --occ-mask are refused with it. An invalid pixel of a
KITTI PREDICTION becomes NaN, the kernel's "bad" class. Frames of any size (375 x 1242) work: only files are scored.
Writes to --out (default: --pred): flow-eval.txt (one row per pair and a total row) and flow-eval.json; with --error-map the error
image of every pair (KITTI-style colours, black = invalid, magenta = unusable prediction) through the device JPEG / PNG writers.

Not here: angular error, and FlowNet2 on frames whose size is no multiple of 64. The definitions are in vps_amd/floweval.py, restated
from memory of the KITTI, Sintel and Middlebury kits."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='optical-flow accuracy (device-side counting)')
    ap.add_argument('--pred', required=True, help='directory of predicted flows: .flo, or KITTI 16-bit .png')
    ap.add_argument('--gt', required=True, help='directory of ground-truth flows, the same stems: .flo, or KITTI .png (flow_occ)')
    ap.add_argument('--gt-noc', default=None, help="directory of KITTI's flow_noc files (the non-occluded pixels), with KITTI ground truth")
    ap.add_argument('--mask', default=None, help='directory of 8-bit PNGs, non-zero = invalid (Sintel invalid)')
    ap.add_argument('--occ-mask', default=None, help='directory of 8-bit PNGs, non-zero = occluded (Sintel occlusions)')
    ap.add_argument('--error-map', default=None, help='directory for the error images')
    ap.add_argument('--format', default='jpg', choices=('jpg', 'png'), help='format of the error images')
    ap.add_argument('--png-huffman', default='fixed', choices=('fixed', 'dynamic'), help='--format png: the Huffman code of the device deflate stage; dynamic = a code per 8 KiB segment where that is shorter (dense images)')
    ap.add_argument('--out', default=None, help='directory for flow-eval.txt and flow-eval.json (default: --pred)')
    ap.add_argument('--device', default='cuda')
    args = ap.parse_args(argv)
    if args.gt_noc is not None and (args.mask is not None or args.occ_mask is not None):
        ap.error("--gt-noc goes with KITTI ground truth, which carries its own validity: --mask and --occ-mask are for .flo ground truth")
    return args


FLOW_EXTS = ('.flo', '.png')


def flow_files(d):
    """{stem: path} of the flow files of a directory; a stem with both a .flo and a .png is refused"""
    out = {}
    for f in sorted(os.listdir(d)):
        stem, ext = os.path.splitext(f)
        if ext.lower() in FLOW_EXTS:
            if stem in out:
                raise SystemExit('%s holds both %s and %s' % (d, os.path.basename(out[stem]), f))
            out[stem] = os.path.join(d, f)
    return out


def is_kitti(path):
    return path.lower().endswith('.png')


def match_files(args):
    """-> [(stem, prediction, ground truth, flow_noc file or None)], every refusal of the file layout made before any device work"""
    for d in (args.pred, args.gt, args.gt_noc, args.mask, args.occ_mask):
        if d is not None and not os.path.isdir(d):
            raise SystemExit("%s doesn't exist" % d)
    pred, gt = flow_files(args.pred), flow_files(args.gt)
    if not pred:
        raise SystemExit('no .flo or .png flow files in %s' % args.pred)
    missing = [s for s in sorted(pred) if s not in gt]
    if missing:
        raise SystemExit('%d of %d files have no ground truth in %s, the first: %s' % (len(missing), len(pred), args.gt, missing[0]))
    def kitti_header(path):
        from vps_amd.kittiflow import png16_info
        with open(path, 'rb') as f:
            if png16_info(f.read(33)) is None:
                raise SystemExit('%s is no non-interlaced 16-bit RGB PNG (the KITTI flow flavour)' % path)
    out = []
    for s in sorted(pred):
        noc = None
        for path in (pred[s], gt[s]):
            if is_kitti(path):
                kitti_header(path)
        if is_kitti(gt[s]):
            if args.mask is not None or args.occ_mask is not None:
                raise SystemExit('%s is KITTI ground truth and carries its own validity: --mask / --occ-mask are for .flo ground truth' % gt[s])
            if args.gt_noc is not None:
                noc = os.path.join(args.gt_noc, s + '.png')
                if not os.path.isfile(noc):
                    raise SystemExit('%s has no flow_noc file %s' % (gt[s], noc))
                kitti_header(noc)
        elif args.gt_noc is not None:
            raise SystemExit('--gt-noc goes with KITTI ground truth, %s is a .flo' % gt[s])
        out.append((s, pred[s], gt[s], noc))
    return out


def read_mask(path, shape):
    """an 8-bit PNG -> bool [H,W]: non-zero"""
    from vps_amd.pipeline import imread
    img = np.asarray(imread(path))
    nz = img.any(axis=2) if img.ndim == 3 else img != 0
    if nz.shape != shape:
        raise SystemExit('%s is %s, the flow is %s' % (path, nz.shape, shape))
    return nz


def mask_byte(shape, invalid=None, occluded=None):
    """the kernel's mask byte from Sintel's two masks (bool [H,W] or None)"""
    m = np.ones(shape, dtype=np.uint8)
    if occluded is not None:
        m[occluded] = 2
    if invalid is not None:
        m[invalid] = 0
    return m


def main(argv=None):
    import torch
    from vps_amd import floweval, postprocess
    from vps_amd.flowvis import read_flo
    from vps_amd.kittiflow import read_kitti_flow
    args = parse_args(argv)
    pairs = match_files(args)
    t0 = time.time()
    ev = floweval.FlowEvaluator(args.device, per_pair=True)
    writer = None
    if args.error_map is not None:
        writer = postprocess.DeviceJpegWriter(ev.device) if args.format == 'jpg' else postprocess.DevicePngWriter(ev.device, huffman=args.png_huffman)
    written = []
    try:
        for s, pred_path, gt_path, noc_path in pairs:
            if is_kitti(pred_path):
                pred, pmask = read_kitti_flow(pred_path, device=ev.device)
                pred.masked_fill_((pmask == 0).unsqueeze(-1), float('nan'))        # an invalid predicted pixel: the kernel's "bad" class
            else:
                pred = read_flo(pred_path)
            mask = None
            if is_kitti(gt_path):
                gt, mask = read_kitti_flow(gt_path, noc_path, device=ev.device)
            else:
                gt = read_flo(gt_path)
            if tuple(pred.shape) != tuple(gt.shape):
                raise SystemExit('%s: the prediction is %s, the ground truth %s' % (s, tuple(pred.shape[:2]), tuple(gt.shape[:2])))
            if args.mask is not None or args.occ_mask is not None:
                mask = mask_byte(gt.shape[:2], None if args.mask is None else read_mask(os.path.join(args.mask, s + '.png'), gt.shape[:2]),
                                 None if args.occ_mask is None else read_mask(os.path.join(args.occ_mask, s + '.png'), gt.shape[:2]))
            img = ev.add_pair(pred, gt, mask=mask, err_rgb=True if writer is not None else None, name=s)
            if writer is not None:
                written.append(os.path.join(args.error_map, s + '.' + args.format))
                writer.submit(img, written[-1])
    finally:
        if writer is not None:
            writer.close()
    result = ev.result()
    out_dir = args.pred if args.out is None else args.out
    floweval.write_outputs(result, out_dir)
    torch.cuda.synchronize()
    print('==> flow: %.2f sec  EPE %.4f  (noc %.4f, occ %.4f)  Fl-all %.3f%%  s0-10 %.4f  s10-40 %.4f  s40+ %.4f  (%d pairs, %d error maps)' % (
        time.time() - t0, result['epe_all'], result['epe_noc'], result['epe_occ'], result['fl_all'], result['s0_10'], result['s10_40'], result['s40plus'],
        result['pairs'], len(written)))
    return result


if __name__ == '__main__':
    main()
