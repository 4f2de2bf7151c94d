"""STQ (Segmentation and Tracking Quality) of a result directory: the command line and the input files of tools/eval_vpq_device.py
(pred.json + pan_pred/*.png of tools/test_vpq.py, the ground-truth json + *_final_mask.png / *_gtFine_color.png), scored over whole
videos instead of windows of at most four labelled frames. Every frame is counted on the device into tables that stay there for the
whole video (vps_amd.stq.StqEvaluator -> vps_stq_accumulate), one download per video.

    python tools/eval_stq_device.py --submit_dir work_dirs/.../val_pans_unified --truth_dir data/cityscapes_vps/val/panoptic_video \\
        --pan_gt_json_file data/cityscapes_vps/panoptic_gt_val_city_vps.json

Writes to the submit directory: stq.txt (STQ / AQ / SQ x100 of the set, per-class IoU, one row per video) and stq-tracks.json (every
ground-truth track: video, id, category, size, association score, overlapping predicted ids, the predicted id it shares most pixels
with). The reference has no STQ; the definition is the one in vps_amd/stq.py, restated from memory of the published implementation."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='STQ eval (device-side counting)')
    ap.add_argument('--submit_dir', type=str, default='work_dirs/cityscapes_vps/fusetrack_vpct/val_pans_unified/', help='test output directory')
    ap.add_argument('--truth_dir', type=str, default='data/cityscapes_vps/val/panoptic_video', help='ground truth directory')
    ap.add_argument('--pan_gt_json_file', type=str, default='data/cityscapes_vps/panpotic_gt_val_city_vps.json', help='ground truth json')
    ap.add_argument('--nframes_per_video', type=int, default=6)
    ap.add_argument('--device', type=str, default='cuda')
    # the command line of tools/eval_vpq_device.py is taken whole: its boundary options are accepted and ignored (STQ has no boundary form)
    ap.add_argument('--boundary', action='store_true', help='accepted for tools/eval_vpq_device.py\'s command line; no effect here')
    ap.add_argument('--boundary-ratio', type=float, default=0.02, help='accepted for tools/eval_vpq_device.py\'s command line; no effect here')
    return ap.parse_args(argv)


def write_outputs(result, output_dir):
    """stq.txt and stq-tracks.json of a `StqStats.result()`"""
    from vps_amd.stq import stq_text
    with open(os.path.join(output_dir, 'stq.txt'), 'w') as f:
        f.write(stq_text(result))
    with open(os.path.join(output_dir, 'stq-tracks.json'), 'w') as f:
        json.dump({'stq': result['stq'], 'aq': result['aq'], 'sq': result['sq'], 'per_video': result['per_video'], 'tracks': result['tracks']},
                  f, indent=1)


def main(argv=None):
    from PIL import Image
    from vps_amd.stq import StqEvaluator
    args = parse_args(argv)
    submit_dir, truth_dir, output_dir = args.submit_dir, args.truth_dir, args.submit_dir
    if not os.path.isdir(submit_dir):
        raise SystemExit("%s doesn't exist" % submit_dir)
    t_all = time.time()
    with open(os.path.join(submit_dir, 'pred.json')) as f:
        pred_jsons = json.load(f)
    with open(args.pan_gt_json_file) as f:
        gt_jsons = json.load(f)
    categories = {el['id']: el for el in gt_jsons['categories']}
    gt_files = sorted(item['file_name'].replace('_newImg8bit.png', '_final_mask.png').replace('_leftImg8bit.png', '_gtFine_color.png')
                      for item in gt_jsons['images'])
    gt_pans = [np.array(Image.open(os.path.join(truth_dir, fn))) for fn in gt_files]
    pred_pans = [np.array(Image.open(os.path.join(submit_dir, 'pan_pred', item['id'] + '.png'))) for item in gt_jsons['images']]
    assert len(gt_pans) == len(pred_pans), 'number of prediction does not match with the groud truth.'
    print('==> gt_pans / pred_pans: %d // %.2f sec' % (len(gt_pans), time.time() - t_all))
    gt_ann, pred_ann, images = gt_jsons['annotations'], pred_jsons['annotations'], gt_jsons['images']
    assert len(gt_ann) == len(pred_ann) == len(gt_pans)
    nvid = len(gt_ann) // args.nframes_per_video
    videos = [[(gt_ann[i], pred_ann[i], gt_pans[i], pred_pans[i], images[i]) for i in range(v * len(gt_ann) // nvid, (v + 1) * len(gt_ann) // nvid)]
              for v in range(nvid)]
    t0 = time.time()
    ev = StqEvaluator(categories, args.device)
    for v, clip in enumerate(videos):
        ev.add_video(clip, video_id=v)
    result = ev.result()
    write_outputs(result, output_dir)
    print('==> stq: %.2f sec  STQ %.4f  AQ %.4f  SQ %.4f  (%d tracks in %d videos)' % (time.time() - t0, 100 * result['stq'], 100 * result['aq'],
                                                                                     100 * result['sq'], result['n'], nvid))
    print('==> All: %.2f sec' % (time.time() - t_all))
    return result


if __name__ == '__main__':
    main()
