"""Times the ternary census warp error at 1024x2048 (vps_amd/flowphoto.py over csrc/flow_census_ops.hip) and writes
profiles/flow_census_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.

  1. `vps_flow_census` (both launches: the warp pass and the census pass) by HIP events round one call (warm-up first; median, min and
     max of the repeats), in four variants - frames and flow only, with the mask, with mask and mask_out, with mask, mask_out and
     residual - each on inputs that stay in the Infinity Cache (4 triples, cycled) and on a pool that does not (20 distinct triples,
     walked in order). Bytes per pixel are stated from the shapes: pass 1 reads 14 (cur 3, prev(p) 3, flow 8) and writes 12 (three fp32
     planes), pass 2 reads 12 x 38 * 72 / (32 * 64) = 16.03 (the planes with their halo), + 1 mask, + 1 mask_out, + 1 residual; the
     corner gather of pass 1 comes from the caches and is not counted. `vps_flow_photo` is timed the same way in the same sitting, with
     the ratio to it, and `vps_tc_accumulate_masked` as well, each held against the min - max recorded in
     profiles/flow_photo_pipeline.json and profiles/tc_occlusion_pipeline.json.
  2. `CensusEvaluator.add_pair` per pair against downloading both frames, the flow and the mask of every pair and running the array
     restatement (tests/flow_census_restate.py) on the host. Same process, alternating windows, median of 3 windows.
  3. tools/run_vps_synthetic.py --tc --tc-occlusion with and without --flow-census --tc-census 25 (one video of 21 frames): one run is
     thrown away as warm-up, then the two alternate, three runs each.

    python tools/bench_flow_census.py [--reps 30] [--skip-tool] [--out profiles/flow_census_pipeline.json]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_flow_photo import HBM_ROOF_GBS, event_stats, make_triple, with_rate     # noqa: E402  (the same inputs and the same clock)


def recorded(path, *keys):
    """the {median_ms, min_ms, max_ms} entry under `keys` of a committed profile, or None"""
    try:
        r = json.load(open(os.path.join(ROOT, 'profiles', path)))
        for k in keys:
            r = r[k]
        return {k: r[k] for k in ('median_ms', 'min_ms', 'max_ms')}
    except (OSError, KeyError, TypeError, ValueError):
        return None


def inside(now, rec):
    return None if rec is None else bool(rec['min_ms'] <= now['median_ms'] <= rec['max_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--pairs', type=int, default=4, help='triples of the cache-resident set')
    ap.add_argument('--pool', type=int, default=20, help='triples of the pool beyond the Infinity Cache')
    ap.add_argument('--host-pairs', type=int, default=2, help='pairs per timed window of part 2')
    ap.add_argument('--skip-tool', action='store_true', help='leave part 3 (seven runs of tools/run_vps_synthetic.py at 1024x2048) out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_census_pipeline.json'))
    args = ap.parse_args()
    from vps_amd import flowphoto, hip, tc
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    host = [make_triple(H, W, seed) for seed in range(args.pairs)]
    cached = [tuple(torch.from_numpy(a).to(dev) for a in t) for t in host]
    pool = [(torch.roll(c, k + 1, 1).contiguous(), torch.roll(p, k + 1, 1).contiguous(), (f + 0.01 * k).contiguous(), (b - 0.01 * k).contiguous(),
             torch.roll(m, k + 1, 1).contiguous()) for k in range(args.pool) for c, p, f, b, m in [cached[k % len(cached)]]]
    sets = (('infinity_cache_resident_%d_triples_cycled' % len(cached), cached), ('pool_of_%d_triples_beyond_the_cache' % len(pool), pool))
    nws = int(lib.vps_flow_census_ws_bytes(H, W))
    ws = torch.empty(nws // 4, dtype=torch.float32, device=dev)
    table = torch.zeros((2, 13), dtype=torch.int64, device=dev)
    mout = torch.empty(H, W, dtype=torch.uint8, device=dev)
    resid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    tile = (ctypes.c_int32 * 2)()
    hip.check(lib.vps_flow_census_tile(tile), 'vps_flow_census_tile')
    halo = (tile[0] + 6) * (tile[1] + 8) / float(tile[0] * tile[1])

    # ---- 1. the kernel alone
    def call(t, mask, mo, rs):
        hip.check(lib.vps_flow_census(hip.ptr(t[0]), hip.ptr(t[1]), H, W, hip.ptr(t[2]), 2, 0, hip.ptr(t[4]) if mask else None, flowphoto.CENSUS_THR,
                                      flowphoto.CENSUS_EPS, hip.ptr(table), hip.ptr(mout) if mo else None, hip.ptr(resid) if rs else None, hip.ptr(ws), nws,
                                      hip.stream_ptr()), 'vps_flow_census')
    kernel = {}
    for name, mask, mo, rs in (('frames_and_flow_only', 0, 0, 0), ('with_mask', 1, 0, 0), ('with_mask_mask_out', 1, 1, 0), ('with_mask_mask_out_residual', 1, 1, 1)):
        bpp = round(14 + 12 + 12 * halo + mask + mo + rs, 2)
        rec = dict(bytes_per_pixel_expected=bpp, bytes_per_call=int(bpp * H * W))
        for where, src in sets:
            rec[where] = with_rate(event_stats(lambda i: call(src[i % len(src)], mask, mo, rs), args.reps, warmup=len(src)), bpp * H * W)
        kernel[name] = rec
    first = flowphoto.census_from_tables(flowphoto.flow_census(cached[0][0], cached[0][1], cached[0][2], mask=cached[0][4]).cpu().numpy())

    # ---- the unchanged kernels in the same sitting
    pws_n = int(lib.vps_flow_photo_ws_bytes(H, W))
    pws = torch.empty(pws_n // 8, dtype=torch.float64, device=dev)
    pcounts, psums = torch.zeros(21, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)

    def call_photo(t, mask, mo, rs):
        hip.check(lib.vps_flow_photo(hip.ptr(t[0]), hip.ptr(t[1]), H, W, hip.ptr(t[2]), 2, 0, hip.ptr(t[4]) if mask else None, flowphoto.PHOTO_THR,
                                     hip.ptr(pcounts), hip.ptr(psums), hip.ptr(mout) if mo else None, hip.ptr(resid) if rs else None, hip.ptr(pws), pws_n,
                                     hip.stream_ptr()), 'vps_flow_photo')
    photo = {}
    for name, mask, mo, rs in (('frames_and_flow_only', 0, 0, 0), ('with_mask_mask_out_residual', 1, 1, 1)):
        rec = {}
        for where, src in sets:
            now = event_stats(lambda i: call_photo(src[i % len(src)], mask, mo, rs), args.reps, warmup=len(src))
            was = recorded('flow_photo_pipeline.json', 'vps_flow_photo', name, where)
            rec[where] = dict(now, recorded=was, median_inside_recorded_min_max=inside(now, was),
                              census_over_photo_at_median=round(kernel[name][where]['median_ms'] / now['median_ms'], 2))
        photo[name] = rec

    # vps_tc_accumulate_masked on panoptic-like maps of rectangles, as tools/bench_flow_occ.py has it
    C = 19
    seg_class = np.full(256, 255, dtype=np.uint8); seg_class[:C] = np.arange(C)
    rng = np.random.default_rng(0)
    pan = np.zeros((H, W, 3), dtype=np.uint8)
    for _ in range(60):
        y, x, h, w = rng.integers(0, H - 64), rng.integers(0, W - 64), rng.integers(32, 400), rng.integers(32, 600)
        pan[y:y + h, x:x + w] = (rng.integers(0, C), 0, rng.integers(0, 40))
    dpan = torch.from_numpy(pan).to(dev)
    dpan2 = torch.roll(dpan, (1, 2), (0, 1)).contiguous()
    ev = tc.TcEvaluator(seg_class, C, id_channel=2, device=dev, occlusion=True)
    keys = ev.video_keys([dpan, dpan2])
    n = len(keys)
    dkeys = torch.from_numpy(keys.view(np.int16)).to(dev)
    conf, psz, csz, same, misc, masked = torch.split(torch.zeros(sum(tc.table_sizes(C, n, True)), dtype=torch.int64, device=dev), tc.table_sizes(C, n, True))

    def call_tc(t):
        hip.check(lib.vps_tc_accumulate_masked(hip.ptr(dpan), hip.ptr(dpan2), H, W, hip.ptr(t[2]), 2, 0, 2, seg_class.ctypes.data_as(ctypes.c_void_p), C,
                                               hip.ptr(dkeys) if n else None, n, hip.ptr(conf), hip.ptr(psz) if n else None, hip.ptr(csz) if n else None,
                                               hip.ptr(same) if n else None, hip.ptr(misc), None, hip.ptr(t[4]), hip.ptr(masked), hip.stream_ptr()),
                  'vps_tc_accumulate_masked')
    tc_now = event_stats(lambda i: call_tc(cached[i % len(cached)]), args.reps, warmup=len(cached))
    tc_rec = None
    try:
        doc = json.load(open(os.path.join(ROOT, 'profiles', 'tc_occlusion_pipeline.json')))
        found = []

        def walk(o, path):
            if isinstance(o, dict):
                if all(k in o for k in ('median_ms', 'min_ms', 'max_ms')) and any('masked' in p for p in path):
                    found.append(('/'.join(path), {k: o[k] for k in ('median_ms', 'min_ms', 'max_ms')}))
                for k, v in o.items():
                    walk(v, path + [str(k)])
        walk(doc, [])
        tc_rec = [dict(entry=p, recorded=r, median_inside_recorded_min_max=inside(tc_now, r)) for p, r in found]
    except (OSError, ValueError):
        pass

    # ---- 2. the evaluator against download + the array restatement per pair
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import flow_census_restate as R
    some = cached[:args.host_pairs]

    def new_way():
        e = flowphoto.CensusEvaluator(dev)
        for c, p, f, _, m in some:
            e.add_pair(p, c, f, mask=m)
        e.end_video('clip')
        return e.result()

    def old_way():
        t_ = np.zeros((2, 13), dtype=np.int64)
        for c, p, f, _, m in some:
            t_ = t_ + R.flow_census(c.cpu().numpy(), p.cpu().numpy(), f.cpu().numpy(), m.cpu().numpy(), flowphoto.CENSUS_THR, flowphoto.CENSUS_EPS)['table']
        return t_
    res = new_way()                                                             # warm-up, and the same table
    assert res['table'] == old_way().tolist(), 'the two ways disagree'
    windows = {'add_pair': [], 'download_and_restatement': []}
    for _ in range(3):
        for name, fn in (('add_pair', new_way), ('download_and_restatement', old_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / len(some))
    per_pair = {k: dict(median_ms=round(1e3 * statistics.median(v), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3)) for k, v in windows.items()}
    ratio = statistics.median(windows['download_and_restatement']) / statistics.median(windows['add_pair'])

    # ---- 3. the tool with and without the new flags
    tool = None
    if not args.skip_tool:
        import run_vps_synthetic as S
        common = ['--videos', '1', '--frames', '21', '--height', str(H), '--width', str(W), '--tc', '--tc-occlusion']
        new = ['--flow-census', '--tc-census', '25']
        tool = dict(frames=21, size=[H, W], runs=[])
        with tempfile.TemporaryDirectory() as tmp:
            for i, extra in enumerate([[], [], new, [], new, [], new]):
                rep = S.main(common + ['--out', os.path.join(tmp, 'run%d' % i)] + extra)
                if i:                                                            # the first run warms the process up
                    tool['runs'].append(dict(options=' '.join(extra), frames_per_s=rep['frames_per_s_upload_prep_model_sequential'],
                                             model_seconds=rep['seconds']['model'], postprocess_seconds=rep['seconds']['postprocess_and_png'],
                                             occluded_share=rep['tc'].get('occluded_share'), flow_census=rep.get('flow_census')))
        for name, sel in (('without', tool['runs'][0::2]), ('with_flow_census_tc_census', tool['runs'][1::2])):
            fps, post = [r['frames_per_s'] for r in sel], [r['postprocess_seconds'] for r in sel]
            tool[name + '_frames_per_s'] = dict(median=statistics.median(fps), min=min(fps), max=max(fps))
            tool[name + '_postprocess_seconds'] = dict(median=statistics.median(post), min=min(post), max=max(post))
        tool['with_over_without_frames_per_s'] = round(tool['with_flow_census_tc_census_frames_per_s']['median'] / tool['without_frames_per_s']['median'], 3)
        tool['note'] = ('frames/s: upload + prep + model per frame, sequential, synthetic weights; both new passes (one vps_flow_census per pair for the figures, '
                        'one in place for the mask) run in the post-processing stage, whose seconds also hold the PNG files. The figures are those of a flow '
                        'from random weights and prove plumbing, not plausibility')

    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], reps=args.reps,
               hbm_roof_gb_per_s=HBM_ROOF_GBS, thr=flowphoto.CENSUS_THR, eps=flowphoto.CENSUS_EPS, ws_bytes=nws, tile=[int(tile[0]), int(tile[1])],
               cached_bytes=len(cached) * 14 * H * W, pool_bytes=len(pool) * 14 * H * W,
               vps_flow_census=kernel, vps_flow_photo_same_sitting=photo,
               vps_tc_accumulate_masked_same_sitting=dict(tc_now, recorded=tc_rec),
               kernel_note='HIP events round one call = two launches (the warp pass, then the census pass on tiles), so two launch latencies are part of '
                           'every figure; the passes are not timed apart. Bytes per pixel are the expected values computed from the shapes, not counter '
                           'readings; the 24 bytes per pixel of the three planes go through the workspace, which stays in the Infinity Cache at this size',
               figures_of_the_first_triple={g: {k: round(first[g][k], 4) for k in ('ce_warp', 'ce_static', 'ratio', 'gain', 'flagged_share')}
                                            for g in ('all', 'visible', 'masked')},
               per_pair=dict(pairs_per_window=len(some), windows=3, **per_pair, download_and_restatement_over_add_pair=round(ratio, 2),
                             note='wall clock per pair, frames, flow and mask on the device in both ways; add_pair: two launches per pair and one download '
                                  'per video (a fresh evaluator per window); download_and_restatement: 31.5 MB down per pair, then the array form of '
                                  'tests/flow_census_restate.py on the host'),
               run_vps_synthetic=tool,
               not_measured=['real footage (none is available): the defaults thr = 25 and eps = 2000 are unvalidated, and with random weights the synthetic '
                             'flow is meaningless, so the tool figures prove plumbing, not plausibility',
                             'a profiler trace (rocprofv3: event times include the launches) and the two passes apart',
                             'hardware counters: the bytes moved, LDS bank conflicts, VALU utilisation',
                             'FlowNet2\'s own padded layout (8-byte loads), the scalar-load layouts, maps off a dword boundary and widths that are no multiple of 4',
                             'tools/run_config3.py with the new flags (it needs the dataset or a clip)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
