"""Times the occlusion option of temporal consistency at 1024x2048 on the synthetic clips of tools/bench_tc.py (vps_amd/tc.py over
csrc/flow_occ_ops.hip and csrc/tc_ops.hip) and writes profiles/tc_occlusion_pipeline.json, stamped with the kernel sources' hash.
Nothing gates on these numbers; no threshold is fixed in advance.

  1. `vps_flow_occlusion` per call by HIP events (warm-up first; median, min and max of the repeats) and the GB/s of the 17 bytes per
     pixel it must move (8 fwd + 8 back + 1 mask), on 5 cycled pairs that stay in the Infinity Cache and on a pool of 24 pairs (805 MB)
     that does not; also with FlowNet2's padded layout (ld 4) for both flows.
  2. `vps_tc_accumulate_masked` against `vps_tc_accumulate` on the same pairs, same process, alternating windows (3 windows of the
     repeats each, all samples pooled): the masked call moves 15 bytes per pixel where the other moves 14.
  3. `vps_tc_accumulate` as tools/bench_tc.py times it, beside the figures of profiles/tc_pipeline.json (the commit before the kernel
     became a template instance): is the median inside that file's own min - max?
  4. `TcEvaluator(occlusion=True).add_pair` per pair against the only other way to the same numbers: downloading both maps and both
     flows and running the NumPy restatement (tests/flow_occ_restate.py, tests/tc_restate.py's warp, bincounts). Alternating windows.
  5. tools/run_vps_synthetic.py --tc against --tc --tc-occlusion in frames/s (one video of 21 frames, the clip length the tool's tests use): the price of the second
     FlowNet2 pass. One run is thrown away as warm-up, then the two alternate, three runs each.

    python tools/bench_flow_occ.py [--reps 30] [--skip-tool] [--out profiles/tc_occlusion_pipeline.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_tc import C, HBM_ROOF_GBS, SEG_CLASS, event_stats, make_video      # noqa: E402


def back_flows(flows):
    """a backward flow for every forward flow of `make_video`: its negative, read where it stands (so it is the inverse up to the
    flow's own gradient), plus an error that grows to two pixels in a band: most pixels cancel, the band does not"""
    H, W = flows[0].shape[:2]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    band = (2.0 * np.clip(np.sin(xs / 151 + ys / 233) - 0.8, 0, None) / 0.2).astype(np.float32)
    return [np.stack([-f[..., 0] + band, -f[..., 1]], axis=-1).astype(np.float32) for f in flows]


def host_pair_masked(prev, cur, flow, back, keys):
    """the six tables of one pair in NumPy: the mask of tests/flow_occ_restate.py, the warp of tests/tc_restate.py, bincounts"""
    import flow_occ_restate
    import tc_restate
    codes, _ = flow_occ_restate.occlusion(flow, back)
    inview, ix, iy = tc_restate.warp(flow)
    keep = inview & (codes == 0)
    n, W = len(keys), cur.shape[1]
    a = cur[keep].astype(np.int64)
    b = prev.reshape(-1, 3)[(iy * W + ix)[keep]].astype(np.int64)
    ca, cb = np.minimum(SEG_CLASS[a[:, 0]], C).astype(np.int64), np.minimum(SEG_CLASS[b[:, 0]], C).astype(np.int64)
    conf = np.bincount(cb * (C + 1) + ca, minlength=(C + 1) ** 2)
    index = np.full(65536, n, dtype=np.int64)
    index[keys] = np.arange(n)
    ka, kb = index[a[:, 0] * 256 + a[:, 2]], index[b[:, 0] * 256 + b[:, 2]]
    cur_size, prev_size = np.bincount(ka, minlength=n + 1)[:n], np.bincount(kb, minlength=n + 1)[:n]
    same = np.bincount(ka[(ka == kb) & (ka < n)], minlength=n + 1)[:n]
    return np.concatenate([conf, prev_size, cur_size, same, [len(a), inview.size - int(inview.sum())], [int(inview.sum()) - len(a)]]).astype(np.int64)


def samples(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(warmup + i); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--videos', type=int, default=2, help='videos per timed window of part 4')
    ap.add_argument('--skip-tool', action='store_true', help='leave part 5 (two runs of tools/run_vps_synthetic.py at 1024x2048) out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tc_occlusion_pipeline.json'))
    args = ap.parse_args()
    from vps_amd import hip, tc
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    npix = H * W
    videos = [make_video(H, W, seed=v) for v in range(args.videos)]
    backs = [back_flows(fs) for _, fs in videos]
    ev = tc.TcEvaluator(SEG_CLASS, C, id_channel=2, device=dev, per_pair=True, id_last_stuff=10)
    maps, flows = videos[0]
    keys = ev.video_keys(maps)
    d_maps = [torch.from_numpy(m).to(dev) for m in maps]
    d_flows = [torch.from_numpy(f).to(dev) for f in flows]
    d_backs = [torch.from_numpy(f).to(dev) for f in backs[0]]
    nc = len(maps) - 1

    # ---- 1. vps_flow_occlusion
    fcached = [(d_flows[t], d_backs[t]) for t in range(1, len(maps))]
    fpool = [((f + 0.01 * k).contiguous(), (b - 0.01 * k).contiguous()) for k in range(24) for f, b in [fcached[k % nc]]]
    pad = lambda t: torch.cat([t, torch.zeros_like(t)], dim=2).contiguous()
    fpadded = [(pad(f), pad(b)) for f, b in fcached]
    occ = torch.empty(H, W, dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)

    def occ_call(pair, ld=2, with_counts=True):
        hip.check(lib.vps_flow_occlusion(hip.ptr(pair[0]), ld, 0, hip.ptr(pair[1]), ld, 0, H, W, tc.OCC_ALPHA, tc.OCC_BETA, hip.ptr(occ),
                                         hip.ptr(counts) if with_counts else None, hip.stream_ptr()), 'vps_flow_occlusion')
    occ_rec = dict(bytes_per_call=17 * npix)
    for name, src, ld, wc in (('infinity_cache_resident_5_pairs_cycled', fcached, 2, True), ('pool_of_24_pairs_beyond_the_cache', fpool, 2, True),
                              ('infinity_cache_resident_mask_only', fcached, 2, False), ('infinity_cache_resident_padded_ld4', fpadded, 4, True)):
        r = event_stats(lambda i: occ_call(src[i % len(src)], ld, wc), args.reps, warmup=len(src))
        r['gb_per_s_at_median'] = round(17 * npix / (r['median_ms'] * 1e-3) / 1e9, 1)
        r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
        occ_rec[name] = r
    occ_call(fcached[0])
    torch.cuda.synchronize()
    share = counts.cpu().numpy().astype(np.float64)
    occ_rec['codes_share_of_the_first_pair'] = dict(zip(('visible', 'occluded', 'not_in_view'), np.round(share / share.sum(), 4).tolist()))
    del fpool, fpadded

    # ---- 2. + 3. the counting kernels
    cached = [(d_maps[t - 1], d_maps[t], d_flows[t]) for t in range(1, len(maps))]
    pool = [(torch.roll(p, k + 1, 1).contiguous(), torch.roll(c, k + 1, 1).contiguous(), (f + 0.01 * k).contiguous())
            for k in range(24) for p, c, f in [cached[k % nc]]]
    masks = []
    for t in range(1, len(maps)):
        masks.append(tc.flow_occlusion(d_flows[t], d_backs[t]))
    flick = torch.empty(H, W, dtype=torch.uint8, device=dev)
    seg_ptr = SEG_CLASS.ctypes.data_as(ctypes.c_void_p)
    parent = json.load(open(os.path.join(ROOT, 'profiles', 'tc_pipeline.json')))['vps_tc_accumulate']
    plain_rec, masked_rec = {}, {}
    for path, padn in (('lds_tables', 0), ('global_atomics', 4100)):
        absent = np.setdiff1d(np.arange(20 * 256, 20 * 256 + 2 * padn), keys)[:padn]
        kk = np.sort(np.concatenate([keys.astype(np.int64), absent])).astype(np.uint16)
        n = len(kk)
        sizes = tc.table_sizes(C, n, occlusion=True)
        assert (sum(sizes) <= lib.vps_stq_lds_cells()) == (path == 'lds_tables')
        d_keys = torch.from_numpy(kk.view(np.int16)).to(dev)
        tables = torch.zeros(sum(sizes), dtype=torch.int64, device=dev)
        conf, psz, csz, same, misc, msk = torch.split(tables, sizes)

        def plain(pair, out=None):
            hip.check(lib.vps_tc_accumulate(hip.ptr(pair[0]), hip.ptr(pair[1]), H, W, hip.ptr(pair[2]), 2, 0, 2, seg_ptr, C, hip.ptr(d_keys), n, hip.ptr(conf),
                                            hip.ptr(psz), hip.ptr(csz), hip.ptr(same), hip.ptr(misc), hip.ptr(out), hip.stream_ptr()), 'vps_tc_accumulate')

        def masked(pair, mask, out=None):
            hip.check(lib.vps_tc_accumulate_masked(hip.ptr(pair[0]), hip.ptr(pair[1]), H, W, hip.ptr(pair[2]), 2, 0, 2, seg_ptr, C, hip.ptr(d_keys), n,
                                                   hip.ptr(conf), hip.ptr(psz), hip.ptr(csz), hip.ptr(same), hip.ptr(misc), hip.ptr(out), hip.ptr(mask),
                                                   hip.ptr(msk), hip.stream_ptr()), 'vps_tc_accumulate_masked')
        runs = [('infinity_cache_resident_5_pairs_cycled', cached, None), ('pool_of_24_pairs_beyond_the_cache', pool, None)]
        if path == 'lds_tables':
            runs.append(('infinity_cache_resident_with_map_output', cached, flick))
        plain_rec[path], masked_rec[path] = dict(table_cells=sum(sizes) - 1, nkeys=n), dict(table_cells=sum(sizes), nkeys=n)
        for name, src, out in runs:
            tp, tm = [], []
            for _ in range(3):                                                   # alternating windows
                tp += samples(lambda i: plain(src[i % len(src)], out), args.reps, warmup=len(src))
                tm += samples(lambda i: masked(src[i % len(src)], masks[i % nc], out), args.reps, warmup=len(src))
            p, m = stats(tp), stats(tm)
            was = parent[path][name]
            p['parent'] = dict(median_ms=was['median_ms'], min_ms=was['min_ms'], max_ms=was['max_ms'])
            p['median_within_parent_min_max'] = bool(was['min_ms'] <= p['median_ms'] <= was['max_ms'])
            m['median_over_plain_median'] = round(m['median_ms'] / p['median_ms'], 3)
            plain_rec[path][name], masked_rec[path][name] = p, m
    del pool

    # ---- 4. add_pair with occlusion against download + NumPy
    dvideos = [([torch.from_numpy(m).to(dev) for m in ms], [torch.from_numpy(f).to(dev) for f in fs], [torch.from_numpy(f).to(dev) for f in bs])
               for (ms, fs), bs in zip(videos, backs)]
    vkeys = [ev.video_keys(ms) for ms, _, _ in dvideos]

    def new_way(v):
        e = tc.TcEvaluator(SEG_CLASS, C, id_channel=2, device=dev, id_last_stuff=10, occlusion=True)
        ms, fs, bs = dvideos[v]
        for t in range(1, len(ms)):
            e.add_pair(ms[t - 1], ms[t], fs[t], keys=vkeys[v], back_flow=bs[t])
        st = e.end_video()
        return np.concatenate([st['conf'].reshape(-1), st['prev_size'], st['cur_size'], st['same'], [st['in_view'], st['outside']], [st['occluded']]])

    def old_way(v):
        ms, fs, bs = dvideos[v]
        total = 0
        for t in range(1, len(ms)):
            total = total + host_pair_masked(ms[t - 1].cpu().numpy(), ms[t].cpu().numpy(), fs[t].cpu().numpy(), bs[t].cpu().numpy(), vkeys[v])
        return total

    first = new_way(0)
    assert np.array_equal(first, old_way(0)), 'the two ways disagree'               # warm-up, and the same tables
    npairs = len(videos[0][0]) - 1
    windows = {'add_pair_with_occlusion': [], 'download_and_numpy': []}
    for _ in range(3):
        for name, fn in (('add_pair_with_occlusion', new_way), ('download_and_numpy', old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v in range(len(videos)):
                fn(v)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / (len(videos) * npairs))
    per_pair = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3)) for k, v in windows.items()}
    ratio = statistics.median(windows['download_and_numpy']) / statistics.median(windows['add_pair_with_occlusion'])
    res = tc.tc_from_tables(*np.split(first, np.cumsum(tc.table_sizes(C, len(vkeys[0]), occlusion=True))[:-1]))

    # ---- 5. the tool with and without the second FlowNet2 pass
    tool = None
    if not args.skip_tool:
        import run_vps_synthetic as S
        common = ['--videos', '1', '--frames', '21', '--height', str(H), '--width', str(W)]
        tool = dict(frames=21, size=[H, W], runs=[])
        with tempfile.TemporaryDirectory() as tmp:
            for i, extra in enumerate((['--tc'],) + (['--tc'], ['--tc', '--tc-occlusion']) * 3):
                rep = S.main(common + ['--out', os.path.join(tmp, 'run%d' % i)] + extra)
                if i:                                                            # the first run warms the process up
                    tool['runs'].append(dict(options=' '.join(extra), frames_per_s=rep['frames_per_s_upload_prep_model_sequential'],
                                             model_seconds=rep['seconds']['model'], tc=rep['tc']['tc'], occluded_share=rep['tc'].get('occluded_share')))
        for name, sel in (('tc', tool['runs'][0::2]), ('tc_occlusion', tool['runs'][1::2])):
            fps = [r['frames_per_s'] for r in sel]
            tool[name + '_frames_per_s'] = dict(median=statistics.median(fps), min=min(fps), max=max(fps))
        tool['tc_occlusion_over_tc_frames_per_s'] = round(tool['tc_occlusion_frames_per_s']['median'] / tool['tc_frames_per_s']['median'], 3)
        tool['note'] = ('upload + prep + model per frame, sequential, synthetic weights; the run with --tc-occlusion makes one more FlowNet2 pass per frame '
                        'on the frame\'s own stream, behind the frame; its occluded share is that of a flow from random weights and means nothing')

    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], frames_per_video=6, reps=args.reps,
               instances=45, hbm_roof_gb_per_s=HBM_ROOF_GBS, alpha=tc.OCC_ALPHA, beta=tc.OCC_BETA,
               vps_flow_occlusion=occ_rec, vps_tc_accumulate=plain_rec, vps_tc_accumulate_masked=masked_rec,
               kernel_note='HIP events around one call, so the launch latency is part of every figure. vps_flow_occlusion moves 17 bytes per pixel (8 fwd, 8 '
                           'back, 1 mask; the four bilinear corners of back are neighbours and come from the cache), vps_tc_accumulate 14 (15 with the map '
                           'output), vps_tc_accumulate_masked one more for the mask. The two counting kernels: 3 alternating windows of `reps` calls each, '
                           'all samples pooled; `parent` is profiles/tc_pipeline.json',
               per_pair=dict(videos_per_window=len(videos), pairs_per_video=npairs, windows=3, **per_pair, download_and_numpy_over_add_pair=round(ratio, 2),
                             note='wall clock per pair, maps and flows on the device in both ways; add_pair: 2 launches per pair and one download per video '
                                  '(the key list is given); download_and_numpy: 46 MB down per pair, then the float32 mask, warp and bincounts on the host'),
               synthetic_clip=dict(tc=round(res['tc'], 6), tc_sem=round(res['tc_sem'], 6), tc_track=round(res['tc_track'], 6), in_view=res['in_view'],
                                   outside=res['outside'], occluded=res['occluded'], occluded_share=round(res['occluded_share'], 6)),
               run_vps_synthetic=tool,
               not_measured=['real videos (none are available)',
                             'whether the share of occluded pixels on real footage is plausible (random weights give a meaningless flow)',
                             'the kernels under rocprofv3 (event times include the launch)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
