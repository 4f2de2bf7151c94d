"""Times the boundary band and boundary PQ at 1024x2048 on synthetic panoptic maps of about 45 instances (vps_amd/boundary.py over
csrc/boundary_ops.hip) and writes profiles/boundary_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.

  1. `vps_boundary_band` by HIP events around batches of launches (warm-up first; median, min and max of the per-launch time over the
     batches) at d = 1, 46 (the rule's value at this size) and 128, each on four maps cycled (inputs, outputs and the workspace stay in
     the Infinity Cache) and on a pool of 48 map / output pairs (604 MB, walked in order, so a pair has left the 256 MiB cache when
     its turn comes again). The three d show what the band's width costs: the window is never walked, the halo of d rows and columns
     that every tile reads is.
  2. Whole-image boundary PQ of one image, maps on the host in both ways: `boundary.pq_compute_single_core` (upload, two bands per map
     pair, two pair counts, two downloads) against the host way, the NumPy restatement of tests/boundary_restate.py (one erosion loop
     per segment) on one thread. The two must agree on every statistic.

    python tools/bench_boundary.py [--reps 20] [--batch 10] [--out profiles/boundary_pipeline.json]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM_ROOF_GBS = 8000.0          # MI355X HBM3E peak


def batch_stats(fn, reps, batch, warmup):
    """per-launch milliseconds: events around `batch` launches, `reps` batches"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts, k = [], warmup
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn(k); k += 1
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) / batch)
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--skip-host', action='store_true', help='leave out part 2 (the host way takes about a minute)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'boundary_pipeline.json'))
    args = ap.parse_args()
    import bench_stq
    import boundary_restate as R
    from vps_amd import boundary, hip
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    frames = bench_stq.make_video(H, W, seed=0, nframes=4)
    tile = (hip.c_int32 * 2)()
    hip.check(lib.vps_boundary_tile(tile), 'vps_boundary_tile')

    # ---- 1. the kernel alone
    cached = [torch.from_numpy(f[2]).to(dev) for f in frames]
    outs4 = [torch.empty_like(m) for m in cached]
    pool = [(torch.roll(cached[k % 4], k + 1, 1).contiguous(), torch.empty_like(cached[0])) for k in range(48)]
    pool_bytes = sum(a.numel() + b.numel() for a, b in pool)
    ws = torch.empty(boundary.band_workspace_bytes(H, W, 1), dtype=torch.uint8, device=dev)
    kernel = {}
    for d in (1, 46, 128):
        def call(src, dst):
            hip.check(lib.vps_boundary_band(hip.ptr(src), H, W, d, hip.ptr(dst), hip.ptr(ws), ws.numel(), hip.stream_ptr()), 'vps_boundary_band')
        rec = dict(bytes_per_call=dict(map_read=3 * H * W, keys_written_and_read=2 * 4 * H * W, band_written=3 * H * W),
                   halo=dict(row_pass_columns_read_per_column_written=round((tile[1] + 2 * d) / tile[1], 3),
                             column_pass_rows_walked_per_row_written=round((tile[0] + 2 * d) / tile[0], 3)))
        for name, fn, warm in (('infinity_cache_resident_4_maps_cycled', lambda i: call(cached[i % 4], outs4[i % 4]), 8),
                               ('pool_of_48_maps_beyond_the_cache', lambda i: call(*pool[i % 48]), 48)):
            r = batch_stats(fn, args.reps, args.batch, warm)
            r['gb_per_s_at_median'] = round(14 * H * W / (r['median_ms'] * 1e-3) / 1e9, 1)       # 3 + 4 + 4 + 3 bytes per pixel, halos not counted
            r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
            rec[name] = r
        kernel['d=%d' % d] = rec
    m1, m128 = kernel['d=1']['infinity_cache_resident_4_maps_cycled']['median_ms'], kernel['d=128']['infinity_cache_resident_4_maps_cycled']['median_ms']

    # ---- 2. boundary PQ of one image against the host way
    whole = None
    if not args.skip_host:
        f = frames[1]
        one = ([f[0]], [f[1]], [f[2]], [f[3]], [{}])
        boundary.pq_compute_single_core(*one, bench_stq.CATS, device=dev)                      # warm-up
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stat = boundary.pq_compute_single_core(*one, bench_stq.CATS, device=dev)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        want = R.boundary_pq([f + ({},)])
        host_s = time.perf_counter() - t0
        for c, w in want.cat.items():
            got = stat[c]
            assert (got.tp, got.fp, got.fn, got.iou, got.biou) == (w['tp'], w['fp'], w['fn'], w['iou'], w['biou']), ('the two ways disagree', c)
        tp = sum(w['tp'] for w in want.cat.values())
        whole = dict(d=boundary.dilation(H, W), segments=[len(f[0]['segments_info']), len(f[1]['segments_info'])],
                     device=dict(median_ms=round(1e3 * statistics.median(ts), 3), min_ms=round(1e3 * min(ts), 3), max_ms=round(1e3 * max(ts), 3), runs=5),
                     host_numpy_restatement_one_thread=dict(seconds=round(host_s, 2), runs=1),
                     host_over_device=round(host_s / statistics.median(ts), 1), matched_pairs=tp,
                     mean_boundary_iou_of_matches=round(sum(w['biou'] for w in want.cat.values()) / max(tp, 1), 4),
                     mean_min_iou_of_matches=round(sum(w['iou'] for w in want.cat.values()) / max(tp, 1), 4),
                     note='wall clock, host maps in both ways; the prediction is the ground truth shifted by 3 columns; every statistic of the '
                          'two ways is equal (integers and float64 sums)')
    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], instances=45, reps=args.reps,
               launches_per_batch=args.batch, hbm_roof_gb_per_s=HBM_ROOF_GBS, pool_bytes=pool_bytes, tile_rows_cols=[int(tile[0]), int(tile[1])],
               vps_boundary_band=kernel, d128_over_d1=round(m128 / m1, 3),
               kernel_note='HIP events around a batch of calls, two launches per call (row pass, column pass); per-launch latency is part of every '
                           'figure. No pixel walks its window, but every tile reads a halo of d columns (row pass) and d rows (column pass): '
                           'the halo ratios above are what grows with d',
               boundary_pq_one_image=whole,
               not_measured=['real Cityscapes-VPS files (none are available)', 'the two passes separately under rocprofv3 (event times include the launches)',
                             'boundary VPQ over a whole validation set', 'maps already on the device in part 2', 'a host erosion with cv2 (not installed)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
