"""Optical-flow accuracy of a directory of .flo files against ground truth: end-point error, Fl outlier rate, Sintel's speed bins, the
shares within 1 / 3 / 5 px and, with ground-truth occlusions, EPE noc / occ. Every pair is counted on the device into tables that stay
there (vps_amd.floweval.FlowEvaluator -> vps_flow_error), one download at the end.

    python tools/run_config3.py ... --flow work_dirs/flow --flow-format flo
    python tools/eval_flow_device.py --pred work_dirs/flow --gt data/sintel/flow [--mask data/sintel/invalid] [--occ-mask data/sintel/occlusions]
                                     [--error-map work_dirs/flow_err [--format jpg|png]] [--out work_dirs/flow]

Files are matched by stem: every NAME.flo of --pred needs a NAME.flo in --gt (and a NAME.png in --mask / --occ-mask when those are
given). --mask: 8-bit PNGs, non-zero = invalid (Sintel's `invalid`). --occ-mask: 8-bit PNGs, non-zero = occluded in the ground truth
(Sintel's `occlusions`). The two are combined into the kernel's mask byte: 0 invalid, 1 valid and not occluded, 2 valid and occluded.
Writes to --out (default: --pred): flow-eval.txt (one row per pair and a total row) and flow-eval.json; with --error-map the error
image of every pair (KITTI-style colours, black = invalid, magenta = unusable prediction) through the device JPEG / PNG writers.

Not here: KITTI's 16-bit PNG ground truth (the host PNG decoder is 8-bit only), angular error, and FlowNet2 on frames whose size is no
multiple of 64. The definitions are in vps_amd/floweval.py, restated from memory of the KITTI, Sintel and Middlebury kits."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='optical-flow accuracy (device-side counting)')
    ap.add_argument('--pred', required=True, help='directory of predicted .flo files')
    ap.add_argument('--gt', required=True, help='directory of ground-truth .flo files, the same stems')
    ap.add_argument('--mask', default=None, help='directory of 8-bit PNGs, non-zero = invalid (Sintel invalid)')
    ap.add_argument('--occ-mask', default=None, help='directory of 8-bit PNGs, non-zero = occluded (Sintel occlusions)')
    ap.add_argument('--error-map', default=None, help='directory for the error images')
    ap.add_argument('--format', default='jpg', choices=('jpg', 'png'), help='format of the error images')
    ap.add_argument('--out', default=None, help='directory for flow-eval.txt and flow-eval.json (default: --pred)')
    ap.add_argument('--device', default='cuda')
    return ap.parse_args(argv)


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
    args = parse_args(argv)
    for d in (args.pred, args.gt, args.mask, args.occ_mask):
        if d is not None and not os.path.isdir(d):
            raise SystemExit("%s doesn't exist" % d)
    stems = sorted(os.path.splitext(f)[0] for f in os.listdir(args.pred) if f.lower().endswith('.flo'))
    if not stems:
        raise SystemExit('no .flo files in %s' % args.pred)
    missing = [s for s in stems if not os.path.isfile(os.path.join(args.gt, s + '.flo'))]
    if missing:
        raise SystemExit('%d of %d files have no ground truth in %s, the first: %s.flo' % (len(missing), len(stems), args.gt, missing[0]))
    t0 = time.time()
    ev = floweval.FlowEvaluator(args.device, per_pair=True)
    writer = None
    if args.error_map is not None:
        writer = postprocess.DeviceJpegWriter(ev.device) if args.format == 'jpg' else postprocess.DevicePngWriter(ev.device)
    written = []
    try:
        for s in stems:
            pred, gt = read_flo(os.path.join(args.pred, s + '.flo')), read_flo(os.path.join(args.gt, s + '.flo'))
            if pred.shape != gt.shape:
                raise SystemExit('%s.flo: the prediction is %s, the ground truth %s' % (s, pred.shape[:2], gt.shape[:2]))
            mask = None
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
