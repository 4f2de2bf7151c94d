"""Times the temporal-consistency counting at 1024x2048 on synthetic unified maps of about 45 instances, 6 frames per video
(vps_amd/tc.py over csrc/tc_ops.hip), and writes profiles/tc_pipeline.json, stamped with the kernel sources' hash. Nothing gates on
these numbers.

  1. `vps_tc_accumulate` per pair by HIP events (warm-up first; median, min and max of the repeats), on both table paths (the video's
     own thing keys: workgroup-private LDS tables; the key list padded with absent keys past the bound: global 64-bit atomics), each
     on inputs that stay in the Infinity Cache (the 5 pairs of one video, cycled) and on a pool that does not (24 distinct pairs,
     walked in order, so a pair has left the 256 MiB cache when its turn comes again); the LDS path also with the inconsistency map.
  2. `TcEvaluator.add_video` per pair (maps and flows on the device, as the tools hold them; one download per video) against the only
     other way to the same numbers: downloading the two maps and the flow of every pair and counting in NumPy (the warp of
     tests/tc_restate.py, the tables by bincount). Same process, alternating windows, median of 3 windows.

    python tools/bench_tc.py [--reps 30] [--out profiles/tc_pipeline.json]"""
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
C = 19
SEG_CLASS = np.full(256, 255, dtype=np.uint8)
SEG_CLASS[:C] = np.arange(C)


def make_video(H, W, seed, nframes=6, n_things=45):
    """(maps, flows): the scene drifts 4 pixels per frame to the right, so the true flow of frame t to frame t-1 is (-4, 0); the flow handed
    over adds a smooth error of up to a pixel, and every seventh instance changes its id in the second half of the clip"""
    import png_cases
    base = png_cases.label_map(H, W, seed=seed, n_things=n_things)           # uint8 [H,W,3]: (class, instance, 100 + index)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    maps, flows = [], []
    for t in range(nframes):
        m = np.roll(base, 4 * t, axis=1).copy()
        if t >= nframes // 2:
            for i in range(0, n_things, 7):
                sel = (m[..., 1] > 0) & (m[..., 2] == 100 + i)
                m[sel, 2] = 200 + i
        maps.append(m)
        flows.append(np.stack([-4 + np.sin(xs / 97 + t) * np.cos(ys / 61), 0.8 * np.sin(ys / 83 + 0.5 * t)], axis=-1).astype(np.float32))
    return maps, flows


def host_pair(prev, cur, flow, keys):
    """the five tables of one pair in NumPy: the warp of tests/tc_restate.py, the counting by bincount"""
    import tc_restate
    inview, ix, iy = tc_restate.warp(flow)
    n, W = len(keys), cur.shape[1]
    a = cur[inview].astype(np.int64)
    b = prev.reshape(-1, 3)[(iy * W + ix)[inview]].astype(np.int64)
    ca, cb = np.minimum(SEG_CLASS[a[:, 0]], C).astype(np.int64), np.minimum(SEG_CLASS[b[:, 0]], C).astype(np.int64)
    conf = np.bincount(cb * (C + 1) + ca, minlength=(C + 1) ** 2)
    index = np.full(65536, n, dtype=np.int64)
    index[keys] = np.arange(n)
    ka, kb = index[a[:, 0] * 256 + a[:, 2]], index[b[:, 0] * 256 + b[:, 2]]
    cur_size, prev_size = np.bincount(ka, minlength=n + 1)[:n], np.bincount(kb, minlength=n + 1)[:n]
    same = np.bincount(ka[(ka == kb) & (ka < n)], minlength=n + 1)[:n]
    return np.concatenate([conf, prev_size, cur_size, same, [len(a), inview.size - len(a)]]).astype(np.int64)


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
    ap.add_argument('--videos', type=int, default=2, help='videos per timed window of part 2')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tc_pipeline.json'))
    args = ap.parse_args()
    import ctypes
    from vps_amd import hip, tc
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    videos = [make_video(H, W, seed=v) for v in range(args.videos)]
    ev = tc.TcEvaluator(SEG_CLASS, C, id_channel=2, device=dev, per_pair=True, id_last_stuff=10)

    # ---- 1. the kernel alone
    maps, flows = videos[0]
    keys = ev.video_keys(maps)
    d_maps = [torch.from_numpy(m).to(dev) for m in maps]
    d_flows = [torch.from_numpy(f).to(dev) for f in flows]
    cached = [(d_maps[t - 1], d_maps[t], d_flows[t]) for t in range(1, len(maps))]
    pool = [(torch.roll(p, k + 1, 1).contiguous(), torch.roll(c, k + 1, 1).contiguous(), (f + 0.01 * k).contiguous())
            for k in range(24) for p, c, f in [cached[k % len(cached)]]]
    pair_bytes = 2 * 3 * H * W + 8 * H * W
    flick = torch.empty(H, W, dtype=torch.uint8, device=dev)
    seg_ptr = SEG_CLASS.ctypes.data_as(ctypes.c_void_p)
    kernel = {}
    for path, pad in (('lds_tables', 0), ('global_atomics', 4100)):
        absent = np.setdiff1d(np.arange(20 * 256, 20 * 256 + 2 * pad), keys)[:pad]
        kk = np.sort(np.concatenate([keys.astype(np.int64), absent])).astype(np.uint16)
        n = len(kk)
        sizes = tc.table_sizes(C, n)
        assert (sum(sizes) <= lib.vps_stq_lds_cells()) == (path == 'lds_tables')
        d_keys = torch.from_numpy(kk.view(np.int16)).to(dev)
        tables = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)
        conf, psz, csz, same, misc = torch.split(tables, sizes)

        def call(pair, out=None):
            hip.check(lib.vps_tc_accumulate(hip.ptr(pair[0]), hip.ptr(pair[1]), H, W, hip.ptr(pair[2]), 2, 0, 2, seg_ptr, C, hip.ptr(d_keys), n, hip.ptr(conf),
                                            hip.ptr(psz), hip.ptr(csz), hip.ptr(same), hip.ptr(misc), hip.ptr(out), hip.stream_ptr()), 'vps_tc_accumulate')
        rec = dict(table_cells=sum(sizes), nkeys=n, bytes_per_pair_maps_and_flow=pair_bytes)
        runs = [('infinity_cache_resident_5_pairs_cycled', cached, None), ('pool_of_24_pairs_beyond_the_cache', pool, None)]
        if path == 'lds_tables':
            runs.append(('infinity_cache_resident_with_map_output', cached, flick))
        for name, src, out in runs:
            r = event_stats(lambda i: call(src[i % len(src)], out), args.reps, warmup=len(src))
            moved = pair_bytes + (H * W if out is not None else 0)
            r['gb_per_s_at_median'] = round(moved / (r['median_ms'] * 1e-3) / 1e9, 1)
            r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
            rec[name] = r
        kernel[path] = rec

    # ---- 2. a video through the evaluator against download + NumPy per pair
    dvideos = [([torch.from_numpy(m).to(dev) for m in ms], [torch.from_numpy(f).to(dev) for f in fs]) for ms, fs in videos]
    vkeys = [ev.video_keys(ms) for ms, _ in dvideos]

    def new_way(v):
        e = tc.TcEvaluator(SEG_CLASS, C, id_channel=2, device=dev, id_last_stuff=10)
        st = e.add_video(dvideos[v][0], dvideos[v][1], keys=vkeys[v])
        return np.concatenate([st['conf'].reshape(-1), st['prev_size'], st['cur_size'], st['same'], [st['in_view'], st['outside']]])

    def old_way(v):
        ms, fs = dvideos[v]
        total = 0
        for t in range(1, len(ms)):
            total = total + host_pair(ms[t - 1].cpu().numpy(), ms[t].cpu().numpy(), fs[t].cpu().numpy(), vkeys[v])
        return total

    assert np.array_equal(new_way(0), old_way(0)), 'the two ways disagree'          # warm-up, and the same tables
    npairs = len(videos[0][0]) - 1
    windows = {'add_video': [], 'download_and_numpy': []}
    for _ in range(3):
        for name, fn in (('add_video', new_way), ('download_and_numpy', old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v in range(len(videos)):
                fn(v)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / (len(videos) * npairs))
    per_pair = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3)) for k, v in windows.items()}
    ratio = statistics.median(windows['download_and_numpy']) / statistics.median(windows['add_video'])
    res = tc.tc_from_tables(*np.split(new_way(0), np.cumsum(tc.table_sizes(C, len(vkeys[0])))[:-1]))
    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], frames_per_video=6, reps=args.reps,
               instances=45, hbm_roof_gb_per_s=HBM_ROOF_GBS, pool_bytes=len(pool) * pair_bytes, lds_cells_bound=int(lib.vps_stq_lds_cells()),
               vps_tc_accumulate=kernel,
               kernel_note='HIP events around one call: one launch of a pass over 29 MB of maps and flow (14 bytes per pixel, 15 with the map output), so the '
                           'launch latency is part of every figure',
               per_pair=dict(videos_per_window=len(videos), pairs_per_video=npairs, windows=3, **per_pair, download_and_numpy_over_add_video=round(ratio, 2),
                             note='wall clock per pair, maps and flows on the device in both ways; add_video: 5 launches and one download per video (the key '
                                  'list is given); download_and_numpy: 29 MB down per pair, then the float32 warp and bincounts on the host'),
               synthetic_clip=dict(tc=round(res['tc'], 6), tc_sem=round(res['tc_sem'], 6), tc_track=round(res['tc_track'], 6), in_view=res['in_view'],
                                   outside=res['outside']),
               not_measured=['real videos (none are available)', 'a detector clip with --tc against the same clip without it',
                             'the kernel under rocprofv3 (event times include the launch)', 'FlowNet2\'s own padded layout (8-byte loads)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
