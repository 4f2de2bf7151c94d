"""Times one image's evaluation at 1024x2048 on the image-level path (vps_amd/ipq.py): semantic confusion matrix, unify, converter
and PQ pair counts on the device against the NumPy restatement (tests/ipq_restate.py) on the host, and the `vps_sseg_confusion`
kernel alone on a uniform map and on a noisy one (HIP events, warm-up first, median of the repeats; bytes read / time against the
HBM roof). Writes profiles/ipq_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.
    python tools/bench_ipq.py [--reps 20] [--out profiles/ipq_pipeline.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_ROOF_GBS = 8000.0          # MI355X HBM3E peak


def event_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ipq_pipeline.json'))
    args = ap.parse_args()
    import ipq_cases
    import ipq_restate as R
    import png_cases
    from vps_amd import hip, ipq
    dev = torch.device('cuda:0')
    H, W, C = 1024, 2048, 19
    lm = png_cases.label_map(H, W, seed=2, n_things=45)
    seg = np.ascontiguousarray(lm[..., 0]); seg[seg > 18] = 18
    pan = np.where(lm[..., 1] > 0, 10 + lm[..., 1], np.minimum(seg, 10)).astype(np.uint8)
    cls_ind = (np.arange(45) % 8).astype(np.int64)
    gt = np.roll(seg, 3, 1).copy(); gt[:40] = 255
    rng = np.random.default_rng(0)
    noisy_gt = rng.integers(0, C, (H, W)).astype(np.uint8); noisy_pr = rng.integers(0, C, (H, W)).astype(np.uint8)
    uni = np.full((H, W), 5, np.uint8)
    d = lambda a: torch.from_numpy(a).to(dev)                                     # noqa: E731
    ev = ipq.SemanticEvaluator(C, dev)
    kernel = {}
    for name, g, p in (('uniform', d(uni), d(uni)), ('noisy', d(noisy_gt), d(noisy_pr)), ('label_map', d(gt), d(seg))):
        med, best = event_ms(lambda: ev.add(g, p), args.reps)
        kernel[name] = dict(median_ms=round(med, 4), min_ms=round(best, 4), bytes_read=2 * H * W,
                            gb_per_s=round(2 * H * W / (med * 1e-3) / 1e9, 1), fraction_of_hbm_roof=round(2 * H * W / (med * 1e-3) / 1e9 / HBM_ROOF_GBS, 4))
    half = d(np.ascontiguousarray(seg[::2, ::2]))
    gt_d, seg_d, pan_d = d(gt), d(seg), d(pan)
    med, best = event_ms(lambda: ev.add(gt_d, half), args.reps)
    kernel['label_map_from_half_size'] = dict(median_ms=round(med, 4), min_ms=round(best, 4))

    # one image through the device path: confusion + unify + convert + PQ pair counts against itself (wall clock, synchronised)
    uni_d, conv = ipq.ImagePanopticUnifier(dev), ipq.ImageConverter(dev)
    cats = {c: {'id': c, 'isthing': 1 if c >= 11 else 0} for c in range(19)}

    def device_image():
        e = ipq.SemanticEvaluator(C, dev)
        e.add(gt_d, seg_d)
        r = e.result()
        two = uni_d.get_unified_pan_result_device([seg_d], [pan_d], [cls_ind], 2048, ['a'])['a']
        ann, pans, _ = conv.convert_device([two], ipq_cases.DistinctColors())
        import copy
        st = ipq.pq_compute_single_core(copy.deepcopy(ann), ann, pans, pans, [{}], cats, dev)
        torch.cuda.synchronize()
        return r, two, ann, st

    def host_image():
        r = R.miou(R.confusion_matrix(gt, seg, C))
        two = R.get_unified_pan_result([seg], [pan], [cls_ind], 2048, ['a'])['a']
        ann, pans = R.converter_2ch_single_core([two], ipq_cases.DistinctColors())
        st = R.pq_compute_single_core(ann, ann, pans, pans, [{}], cats)
        return r, two, ann, st

    for _ in range(3):
        dres = device_image()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); device_image(); ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); hres = host_image(); host_s = time.perf_counter() - t0
    assert np.array_equal(dres[0]['confusion_matrix'], hres[0]['confusion_matrix']) and np.array_equal(dres[1].cpu().numpy(), hres[1])
    assert dres[2] == hres[2]
    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], reps=args.reps,
               vps_sseg_confusion=kernel, hbm_roof_gb_per_s=HBM_ROOF_GBS,
               kernel_note='events around SemanticEvaluator.add: one launch of a 4 MB pass, so the launch latency is most of the time',
               one_image=dict(device_ms_median=round(1e3 * statistics.median(ts), 3), device_ms_min=round(1e3 * min(ts), 3),
                              numpy_restatement_ms=round(1e3 * host_s, 1), segments=len(dres[2][0]['segments_info']),
                              note='device: wall clock with a synchronisation per image, uploads excluded; restatement: one run on the host'))
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
