"""Times the STQ counting at 1024x2048 on synthetic panoptic maps of about 45 instances, 6 frames per video (vps_amd/stq.py over
csrc/stq_ops.hip), and writes profiles/stq_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.

  1. `vps_stq_accumulate` per frame by HIP events (warm-up first; median, min and max of the repeats), on both table paths (the video's
     own ids: workgroup-private LDS tables; the id lists padded with unpainted ids past the bound: global 64-bit atomics), each on
     inputs that stay in the Infinity Cache (the 6 frame pairs of one video, cycled: 75 MB) and on a pool that does not (48 distinct
     frame pairs, 604 MB, walked in order, so a pair has left the 256 MiB cache when its turn comes again).
  2. `StqEvaluator.add_video` per video (host maps uploaded, one download) against the only way the package offered before to obtain the
     same pair counts: `evaluate.FrameCounts.count` per frame (`vps_pair_count`, a download and a synchronisation per frame) plus the
     host merge of the per-frame pair dicts. Same process, alternating windows, median of 3 windows.

    python tools/bench_stq.py [--reps 30] [--out profiles/stq_pipeline.json]"""
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
CATS = {c: {'id': c, 'name': 'class%d' % c, 'isthing': 1 if c >= 11 else 0} for c in range(19)}


def id_map(lm):
    """segment ids of a png_cases.label_map: stuff band s -> s + 1, thing i -> 1000 + i"""
    return np.where(lm[..., 1] > 0, 1000 + lm[..., 2].astype(np.int64) - 100, lm[..., 0].astype(np.int64) + 1)


def category_of(sid, things):
    return things[sid] if sid >= 1000 else sid - 1


def pan_of(ids):
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def make_video(H, W, seed, nframes=6, n_things=45):
    """frames (gt_ann, pred_ann, gt_pan, pred_pan): the instances drift 4 pixels per frame; the prediction is the ground truth shifted by 3
    columns, with every seventh instance's id switched in the second half of the clip"""
    import png_cases
    lm = png_cases.label_map(H, W, seed=seed, n_things=n_things)
    base = id_map(lm)
    things = {int(1000 + i): int(11 + i % 8) for i in range(n_things)}
    things.update({int(2000 + i): int(11 + i % 8) for i in range(n_things)})
    frames = []
    for t in range(nframes):
        g = np.roll(base, 4 * t, axis=1)
        p = np.roll(g, 3, axis=1)
        if t >= nframes // 2:
            for i in range(0, n_things, 7):
                p[p == 1000 + i] = 2000 + i
        ann = []
        for m in (g, p):
            ids, areas = np.unique(m, return_counts=True)
            ann.append({'segments_info': [{'id': int(s), 'category_id': category_of(int(s), things), 'iscrowd': 0, 'area': int(a)} for s, a in zip(ids, areas)]})
        frames.append((ann[0], ann[1], pan_of(g), pan_of(p)))
    return frames


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
    ap.add_argument('--videos', type=int, default=4, help='videos per timed window of part 2')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stq_pipeline.json'))
    args = ap.parse_args()
    from vps_amd import hip, stq
    from vps_amd.evaluate import FrameCounts
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W, C = 1024, 2048, 19
    videos = [make_video(H, W, seed=v) for v in range(args.videos)]

    # ---- 1. the kernel alone
    frames = videos[0]
    gt_ids, gt_info, pred_ids, pred_info = stq.build_id_tables(frames, CATS)
    kernel = {}
    cached = [(torch.from_numpy(f[2]).to(dev), torch.from_numpy(f[3]).to(dev)) for f in frames]
    pool = []
    for k in range(48):                                        # distinct buffers: rolled copies of the 6 pairs
        g, p = cached[k % 6]
        pool.append((torch.roll(g, k + 1, 1).contiguous(), torch.roll(p, k + 1, 1).contiguous()))
    pool_bytes = sum(g.numel() + p.numel() for g, p in pool)
    for path, pad in (('lds_tables', 0), ('global_atomics', 150)):
        gi = np.concatenate([gt_ids, np.arange(5000, 5000 + pad, dtype=np.uint32)]); gf = np.concatenate([gt_info, np.full(pad, 12 | 64, np.uint8)])
        pi = np.concatenate([pred_ids, np.arange(5000, 5000 + pad, dtype=np.uint32)]); pf = np.concatenate([pred_info, np.full(pad, 12 | 64, np.uint8)])
        ngt, npred = len(gi), len(pi)
        sizes = [C * (C + 1), ngt, npred + 1, ngt * npred]
        assert (sum(sizes) <= lib.vps_stq_lds_cells()) == (path == 'lds_tables')
        d = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in (gi, gf, pi, pf)]
        tables = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)
        conf, gsz, psz, inter = torch.split(tables, sizes)

        def call(pair):
            hip.check(lib.vps_stq_accumulate(hip.ptr(pair[0]), hip.ptr(pair[1]), H * W, hip.ptr(d[0]), hip.ptr(d[1]), ngt, hip.ptr(d[2]), hip.ptr(d[3]),
                                             npred, C, hip.ptr(conf), hip.ptr(gsz), hip.ptr(psz), hip.ptr(inter), hip.stream_ptr()), 'vps_stq_accumulate')
        rec = dict(table_cells=sum(sizes), ngt=ngt, npred=npred, bytes_read_per_frame=6 * H * W)
        for name, src in (('infinity_cache_resident_6_pairs_cycled', cached), ('pool_of_48_pairs_beyond_the_cache', pool)):
            r = event_stats(lambda i: call(src[i % len(src)]), args.reps, warmup=len(src))
            r['gb_per_s_at_median'] = round(6 * H * W / (r['median_ms'] * 1e-3) / 1e9, 1)
            r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
            rec[name] = r
        kernel[path] = rec

    # ---- 2. a video through the evaluator against FrameCounts per frame + the host merge
    fc = FrameCounts(dev)

    def new_way(frames):
        return stq.StqEvaluator(CATS, dev).add_video(frames)

    def old_way(frames):
        clip_ids = sorted({el['id'] for f in frames for el in f[0]['segments_info']})
        merged = {}
        for f in frames:
            _, _, pairs = fc.count(f[0], f[1], f[2], f[3], CATS, clip_ids)
            for k, v in pairs.items():
                merged[k] = merged.get(k, 0) + v
        return merged

    st, merged = new_way(videos[0]), old_way(videos[0])        # warm-up, and the two ways agree on every pair of tracks
    gl, pl = [int(v) for v in st['gt_ids']], [int(v) for v in st['pred_ids']]
    inter = {(gl[r], pl[c]): int(v) for (r, c), v in np.ndenumerate(st['inter']) if v}
    assert inter == {k: v for k, v in merged.items() if k[0] >= 1000 and k[1] >= 1000}, 'the two ways disagree'
    windows = {'add_video': [], 'frame_counts_and_merge': []}
    for _ in range(3):
        for name, fn in (('add_video', new_way), ('frame_counts_and_merge', old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for frames in videos:
                fn(frames)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / len(videos))
    per_video = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3)) for k, v in windows.items()}
    ratio = statistics.median(windows['frame_counts_and_merge']) / statistics.median(windows['add_video'])
    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], frames_per_video=6, reps=args.reps,
               instances=45, hbm_roof_gb_per_s=HBM_ROOF_GBS, pool_bytes=pool_bytes, lds_cells_bound=int(lib.vps_stq_lds_cells()),
               vps_stq_accumulate=kernel,
               kernel_note='HIP events around one call: one launch of a 12.6 MB pass, so the launch latency is part of every figure',
               per_video=dict(videos_per_window=len(videos), windows=3, **per_video, frame_counts_over_add_video=round(ratio, 3),
                              note='wall clock per video with host maps uploaded in both ways; add_video: 6 launches, one download; '
                                   'frame_counts_and_merge: vps_pair_count, download and synchronisation per frame, then the dict merge'),
               not_measured=['real Cityscapes-VPS files (none are available)', 'videos with more than 6 labelled frames', 'maps already on the device',
                             'the kernel under rocprofv3 (event times include the launch)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
