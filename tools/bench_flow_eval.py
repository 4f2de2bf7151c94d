"""Times the optical-flow accuracy pass at 1024x2048 on synthetic flows (vps_amd/floweval.py over csrc/flow_err_ops.hip) and writes
profiles/flow_eval_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.

  1. `vps_flow_error` (both launches) by HIP events round one call (warm-up first; median, min and max of the repeats), in four variants -
     flows only, with the mask, with mask and occ_pred, with mask, occ_pred and the error image - each on inputs that stay in the Infinity
     Cache (4 pairs, cycled: 134 MB of flows) and on a pool that does not (20 distinct pairs, 671 MB, walked in order, so a pair has
     left the 256 MiB cache when its turn comes again). Bytes per pixel are stated from the shapes: 16 for the two flows, + 1 mask,
     + 1 occ_pred, + 3 image.
  2. `FlowEvaluator.add_pair` per pair (flows on the device, as the detector holds them; one download per set) against the only other way
     to the same figures: downloading both fields of every pair and counting in float64 NumPy on the host (the rules of tests/flow_err_restate.py with
     bincount and np.sum). Same process, alternating windows, median of 3 windows.

    python tools/bench_flow_eval.py [--reps 30] [--out profiles/flow_eval_pipeline.json]"""
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

HBM_ROOF_GBS = 8000.0          # MI355X HBM3E peak


def make_pair(H, W, seed):
    """(pred, gt, mask, occ_pred): a smooth ground truth with speeds in all three bins, a prediction with a smooth error of a few pixels
    and some noise, a mask with an occluded band and invalid speckle, an occ_pred that overlaps the band"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.stack([45 * np.sin(xs / 301 + seed) * np.cos(ys / 173), 12 * np.cos(ys / 97 + 0.3 * seed) - 0.004 * xs], axis=-1).astype(np.float32)
    pred = (gt + np.stack([2.5 * np.sin(xs / 41 + ys / 59), 1.5 * np.cos(xs / 67)], axis=-1) + rng.standard_normal((H, W, 2)) * 0.4).astype(np.float32)
    mask = np.ones((H, W), dtype=np.uint8)
    mask[:, W // 3:W // 3 + 90] = 2
    mask[rng.random((H, W)) < 0.01] = 0
    occ = np.zeros((H, W), dtype=np.uint8)
    occ[:, W // 3 + 20:W // 3 + 120] = 1
    occ[:, :6] = 2
    return pred, gt, mask, occ


def host_pair(pred, gt, mask, occ):
    """the tables of one pair in NumPy float64, as a user would write them: the rules of tests/flow_err_restate.py's array form with
    bincount and np.sum (pairwise, not the exact fsum of the restatement, which would take seconds per pair)"""
    u, v, ug, vg = (a.astype(np.float64) for a in (pred[..., 0], pred[..., 1], gt[..., 0], gt[..., 1]))
    with np.errstate(all='ignore'):
        valid = ((mask == 1) | (mask == 2)) & (np.abs(ug) <= 1e9) & (np.abs(vg) <= 1e9)
        good = valid & (np.abs(u) <= 1e9) & (np.abs(v) <= 1e9)
        epe = np.sqrt((u - ug) ** 2 + (v - vg) ** 2)
        mag = np.sqrt(ug * ug + vg * vg)
    counts, sums = np.zeros(25, dtype=np.int64), np.zeros(8)
    counts[24] = valid.size - int(valid.sum())
    bins = np.where(mag < 10, 0, np.where(mag < 40, 1, 2))
    for g in range(2):
        grp = mask == g + 1
        sel = good & grp
        e, b = epe[sel], bins[sel]
        c = counts[12 * g:12 * g + 12]
        c[0], c[1], c[2] = e.size, int((valid & grp).sum()) - e.size, int(((e > 3.0) & (e > 0.05 * mag[sel])).sum())
        c[3], c[4], c[5] = int((e > 1.0).sum()), int((e > 3.0).sum()), int((e > 5.0).sum())
        c[6:9] = np.bincount(b, minlength=3)
        c[9:12] = np.bincount(occ[valid & grp], minlength=4)[:3]
        sums[4 * g] = e.sum()
        sums[4 * g + 1:4 * g + 4] = np.bincount(b, weights=e, minlength=3)
    return counts, sums


def event_stats(fn, reps, warmup=6):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(warmup + i); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--pairs', type=int, default=4, help='pairs per timed window of part 2 (and of the cache-resident set)')
    ap.add_argument('--pool', type=int, default=20, help='pairs of the pool beyond the Infinity Cache')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_eval_pipeline.json'))
    args = ap.parse_args()
    from vps_amd import floweval, hip
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    host = [make_pair(H, W, seed) for seed in range(args.pairs)]
    cached = [tuple(torch.from_numpy(a).to(dev) for a in p) for p in host]
    pool = [((p + 0.01 * k).contiguous(), (g - 0.01 * k).contiguous(), torch.roll(m, k + 1, 1).contiguous(), torch.roll(o, k + 1, 1).contiguous())
            for k in range(args.pool) for p, g, m, o in [cached[k % len(cached)]]]
    nws = int(lib.vps_flow_error_ws_bytes(H, W))
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    counts = torch.zeros(25, dtype=torch.int64, device=dev)
    sums = torch.zeros(8, dtype=torch.float64, device=dev)
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)

    # ---- 1. the kernel alone
    def call(pair, mask, occ, img):
        hip.check(lib.vps_flow_error(hip.ptr(pair[0]), 2, 0, hip.ptr(pair[1]), 2, 0, hip.ptr(pair[2]) if mask else None, hip.ptr(pair[3]) if occ else None,
                                     H, W, hip.ptr(counts), hip.ptr(sums), hip.ptr(rgb) if img else None, hip.ptr(ws), nws, hip.stream_ptr()), 'vps_flow_error')
    kernel = {}
    for name, mask, occ, img in (('flows_only', 0, 0, 0), ('with_mask', 1, 0, 0), ('with_mask_occ_pred', 1, 1, 0), ('with_mask_occ_pred_err_rgb', 1, 1, 1)):
        bpp = 16 + mask + occ + 3 * img
        rec = dict(bytes_per_pixel_expected=bpp, bytes_per_pair=bpp * H * W)
        for where, src in (('infinity_cache_resident_%d_pairs_cycled' % len(cached), cached), ('pool_of_%d_pairs_beyond_the_cache' % len(pool), pool)):
            r = event_stats(lambda i: call(src[i % len(src)], mask, occ, img), args.reps, warmup=len(src))
            r['gb_per_s_at_median'] = round(bpp * H * W / (r['median_ms'] * 1e-3) / 1e9, 1)
            r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
            rec[where] = r
        kernel[name] = rec

    # ---- 2. the evaluator against download + NumPy per pair
    def new_way():
        ev = floweval.FlowEvaluator(dev)
        for p, g, m, o in cached:
            ev.add_pair(p, g, mask=m, occ_pred=o)
        return ev.result()

    def old_way():
        c, s = np.zeros(25, dtype=np.int64), np.zeros(8)
        for p, g, m, o in cached:
            pc, ps = host_pair(p.cpu().numpy(), g.cpu().numpy(), m.cpu().numpy(), o.cpu().numpy())
            c, s = c + pc, s + ps
        return c, s
    res = new_way()                                                             # warm-up, and the same tables
    oc, osum = old_way()
    assert res['counts'] == oc.tolist() and np.allclose(res['sums'], osum, rtol=1e-9, atol=0), 'the two ways disagree'
    windows = {'add_pair': [], 'download_and_numpy': []}
    for _ in range(3):
        for name, fn in (('add_pair', new_way), ('download_and_numpy', old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / len(cached))
    per_pair = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3)) for k, v in windows.items()}
    ratio = statistics.median(windows['download_and_numpy']) / statistics.median(windows['add_pair'])
    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], reps=args.reps,
               hbm_roof_gb_per_s=HBM_ROOF_GBS, cached_bytes_flows=len(cached) * 16 * H * W, pool_bytes_flows=len(pool) * 16 * H * W, ws_bytes=nws,
               vps_flow_error=kernel,
               kernel_note='HIP events round one call = two launches (the counting pass over 16..21 bytes per pixel, then one workgroup that adds the '
                           'partial sums), so two launch latencies are part of every figure; bytes per pixel are the expected values from the shapes, '
                           'not counter readings',
               per_pair=dict(pairs_per_window=len(cached), windows=3, **per_pair, download_and_numpy_over_add_pair=round(ratio, 2),
                             note='wall clock per pair, flows, mask and occ_pred on the device in both ways; add_pair: two launches per pair and one download '
                                  'per set (a fresh evaluator per window); download_and_numpy: 37.7 MB down per pair, then float64 NumPy on the host'),
               synthetic_set={k: round(res[k], 6) for k in floweval.FIGURES + floweval.OCC_FIGURES},
               not_measured=['real benchmark files (Sintel, KITTI, Middlebury: none are available)', 'a profiler trace (rocprofv3: event times include the launches)',
                             'hardware counters for the bytes moved', 'FlowNet2\'s own padded layout (8-byte loads) and the scalar-load layouts',
                             'the tool end to end (file reading dominates it)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
