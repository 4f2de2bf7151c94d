"""Times the photometric warp error at 1024x2048 (vps_amd/flowphoto.py over csrc/flow_photo_ops.hip) and writes
profiles/flow_photo_pipeline.json, stamped with the kernel sources' hash. Nothing gates on these numbers.

  1. `vps_flow_photo` (both launches) by HIP events round one call (warm-up first; median, min and max of the repeats), in four variants -
     frames and flow only, with the mask, with mask and mask_out, with mask, mask_out and residual - each on inputs that stay in the
     Infinity Cache (4 triples, cycled) and on a pool that does not (20 distinct triples, walked in order, so a triple has left the
     256 MiB cache when its turn comes again). Bytes per pixel are stated from the shapes: 14 streamed (cur 3, prev(p) 3, flow 8), + 1 mask,
     + 1 mask_out, + 1 residual; the gather of the four corners re-reads up to 12 bytes of `prev` per pixel that the streamed read of the
     neighbourhood has just brought into the caches, and is not counted. `vps_flow_error` (flows only) and `vps_flow_occlusion` (mask and
     counts) are timed the same way in the same sitting as the yardstick, and `vps_tc_accumulate_masked` is left to tools/bench_flow_occ.py.
  2. `PhotoEvaluator.add_pair` per pair (frames, flow and mask on the device; one download per video) against downloading both frames,
     the flow and the mask of every pair and running the array restatement (tests/flow_photo_restate.py) on the host. Same process,
     alternating windows, median of 3 windows.
  3. tools/run_vps_synthetic.py --tc --tc-occlusion with and without --flow-photo --tc-photometric 16 (one video of 21 frames, the clip
     length the tool's tests use): frames/s of the model stage and the seconds of the post-processing stage, which holds both new
     passes. One run is thrown away as warm-up, then the two alternate, three runs each.

    python tools/bench_flow_photo.py [--reps 30] [--skip-tool] [--out profiles/flow_photo_pipeline.json]"""
import argparse
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

HBM_ROOF_GBS = 8000.0          # MI355X HBM3E peak


def make_triple(H, W, seed):
    """(cur, prev, flow, back, mask): a textured frame, the same texture moved by a smooth flow of a few pixels plus a little noise, the
    flow itself with a small error, its negative as the backward flow, a mask with an occluded band"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    tex = lambda x, y: np.stack([127 + 90 * np.sin(x / 7.0 + seed) * np.cos(y / 11.0), 127 + 100 * np.sin((x + y) / 13.0), 127 + 80 * np.cos(x / 5.0 - y / 17.0)],
                                axis=-1)
    u, v = 4 * np.sin(xs / 301 + seed) * np.cos(ys / 173), 2 * np.cos(ys / 97 + 0.3 * seed)
    prev = np.clip(tex(xs, ys) + rng.standard_normal((H, W, 3)) * 2, 0, 255).astype(np.uint8)
    cur = np.clip(tex(xs + u, ys + v) + rng.standard_normal((H, W, 3)) * 2, 0, 255).astype(np.uint8)
    flow = np.stack([u, v], axis=-1).astype(np.float32) + (rng.standard_normal((H, W, 2)) * 0.1).astype(np.float32)
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[:, W // 3:W // 3 + 90] = 1
    mask[:, :6] = 2
    return cur, prev, flow, (-flow).astype(np.float32), mask


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


def with_rate(r, nbytes):
    r['gb_per_s_at_median'] = round(nbytes / (r['median_ms'] * 1e-3) / 1e9, 1)
    r['fraction_of_hbm_roof'] = round(r['gb_per_s_at_median'] / HBM_ROOF_GBS, 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--pairs', type=int, default=4, help='triples of the cache-resident set')
    ap.add_argument('--pool', type=int, default=20, help='triples of the pool beyond the Infinity Cache')
    ap.add_argument('--host-pairs', type=int, default=2, help='pairs per timed window of part 2')
    ap.add_argument('--skip-tool', action='store_true', help='leave part 3 (seven runs of tools/run_vps_synthetic.py at 1024x2048) out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_photo_pipeline.json'))
    args = ap.parse_args()
    from vps_amd import flowphoto, hip
    assert torch.cuda.is_available(), 'the measurement needs the device'
    dev = torch.device('cuda:0')
    lib = hip.load()
    H, W = 1024, 2048
    host = [make_triple(H, W, seed) for seed in range(args.pairs)]
    cached = [tuple(torch.from_numpy(a).to(dev) for a in t) for t in host]
    pool = [(torch.roll(c, k + 1, 1).contiguous(), torch.roll(p, k + 1, 1).contiguous(), (f + 0.01 * k).contiguous(), (b - 0.01 * k).contiguous(),
             torch.roll(m, k + 1, 1).contiguous()) for k in range(args.pool) for c, p, f, b, m in [cached[k % len(cached)]]]
    nws = int(lib.vps_flow_photo_ws_bytes(H, W))
    ws = torch.empty(nws // 8, dtype=torch.float64, device=dev)
    counts = torch.zeros(21, dtype=torch.int64, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    mout = torch.empty(H, W, dtype=torch.uint8, device=dev)
    resid = torch.empty(H, W, dtype=torch.uint8, device=dev)

    # ---- 1. the kernel alone
    def call(t, mask, mo, rs):
        hip.check(lib.vps_flow_photo(hip.ptr(t[0]), hip.ptr(t[1]), H, W, hip.ptr(t[2]), 2, 0, hip.ptr(t[4]) if mask else None, flowphoto.PHOTO_THR, hip.ptr(counts),
                                     hip.ptr(sums), hip.ptr(mout) if mo else None, hip.ptr(resid) if rs else None, hip.ptr(ws), nws, hip.stream_ptr()),
                  'vps_flow_photo')
    kernel = {}
    for name, mask, mo, rs in (('frames_and_flow_only', 0, 0, 0), ('with_mask', 1, 0, 0), ('with_mask_mask_out', 1, 1, 0), ('with_mask_mask_out_residual', 1, 1, 1)):
        bpp = 14 + mask + mo + rs
        rec = dict(bytes_per_pixel_expected=bpp, bytes_per_call=bpp * H * W)
        for where, src in (('infinity_cache_resident_%d_triples_cycled' % len(cached), cached), ('pool_of_%d_triples_beyond_the_cache' % len(pool), pool)):
            rec[where] = with_rate(event_stats(lambda i: call(src[i % len(src)], mask, mo, rs), args.reps, warmup=len(src)), bpp * H * W)
        kernel[name] = rec
    first = flowphoto.photo_from_tables(*(t.cpu().numpy() for t in flowphoto.flow_photometric(cached[0][0], cached[0][1], cached[0][2], mask=cached[0][4])))

    # ---- the yardsticks of the same sitting
    ews = torch.empty(int(lib.vps_flow_error_ws_bytes(H, W)) // 8, dtype=torch.float64, device=dev)
    ecounts, esums = torch.zeros(25, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
    ocounts = torch.zeros(3, dtype=torch.int64, device=dev)

    def call_err(t):
        hip.check(lib.vps_flow_error(hip.ptr(t[2]), 2, 0, hip.ptr(t[3]), 2, 0, None, None, H, W, hip.ptr(ecounts), hip.ptr(esums), None, hip.ptr(ews), ews.numel() * 8,
                                     hip.stream_ptr()), 'vps_flow_error')

    def call_occ(t):
        hip.check(lib.vps_flow_occlusion(hip.ptr(t[2]), 2, 0, hip.ptr(t[3]), 2, 0, H, W, 0.01, 0.5, hip.ptr(mout), hip.ptr(ocounts), hip.stream_ptr()),
                  'vps_flow_occlusion')
    yard = {}
    for name, fn, bpp in (('vps_flow_error_flows_only', call_err, 16), ('vps_flow_occlusion', call_occ, 17)):
        rec = dict(bytes_per_pixel_expected=bpp, bytes_per_call=bpp * H * W)
        for where, src in (('infinity_cache_resident_%d_triples_cycled' % len(cached), cached), ('pool_of_%d_triples_beyond_the_cache' % len(pool), pool)):
            rec[where] = with_rate(event_stats(lambda i: fn(src[i % len(src)]), args.reps, warmup=len(src)), bpp * H * W)
        yard[name] = rec

    # ---- 2. the evaluator against download + the array restatement per pair
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import flow_photo_restate as R
    some = cached[:args.host_pairs]

    def new_way():
        ev = flowphoto.PhotoEvaluator(dev)
        for c, p, f, _, m in some:
            ev.add_pair(p, c, f, mask=m)
        ev.end_video('clip')
        return ev.result()

    def old_way():
        c_, s_ = np.zeros(21, dtype=np.int64), np.zeros(4)
        for c, p, f, _, m in some:
            w = R.flow_photo(c.cpu().numpy(), p.cpu().numpy(), f.cpu().numpy(), m.cpu().numpy(), flowphoto.PHOTO_THR)
            c_, s_ = c_ + w['counts'], s_ + w['sums']
        return c_, s_
    res = new_way()                                                             # warm-up, and the same tables
    oc, osum = old_way()
    assert res['counts'] == oc.tolist() and np.allclose(res['sums'], osum, rtol=1e-9, atol=0), 'the two ways disagree'
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
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        import run_vps_synthetic as S
        common = ['--videos', '1', '--frames', '21', '--height', str(H), '--width', str(W), '--tc', '--tc-occlusion']
        new = ['--flow-photo', '--tc-photometric', '16']
        tool = dict(frames=21, size=[H, W], runs=[])
        with tempfile.TemporaryDirectory() as tmp:
            for i, extra in enumerate([[], [], new, [], new, [], new]):
                rep = S.main(common + ['--out', os.path.join(tmp, 'run%d' % i)] + extra)
                if i:                                                            # the first run warms the process up
                    tool['runs'].append(dict(options=' '.join(extra), frames_per_s=rep['frames_per_s_upload_prep_model_sequential'],
                                             model_seconds=rep['seconds']['model'], postprocess_seconds=rep['seconds']['postprocess_and_png'],
                                             occluded_share=rep['tc'].get('occluded_share'), flow_photo=rep.get('flow_photo')))
        for name, sel in (('without', tool['runs'][0::2]), ('with_flow_photo_tc_photometric', tool['runs'][1::2])):
            fps, post = [r['frames_per_s'] for r in sel], [r['postprocess_seconds'] for r in sel]
            tool[name + '_frames_per_s'] = dict(median=statistics.median(fps), min=min(fps), max=max(fps))
            tool[name + '_postprocess_seconds'] = dict(median=statistics.median(post), min=min(post), max=max(post))
        tool['with_over_without_frames_per_s'] = round(tool['with_flow_photo_tc_photometric_frames_per_s']['median'] / tool['without_frames_per_s']['median'], 3)
        tool['note'] = ('frames/s: upload + prep + model per frame, sequential, synthetic weights - the new flags add nothing to that stage but keeping the flows, '
                        'which --tc keeps anyway; both new passes (one vps_flow_photo per pair for the figures, one in place for the mask) run in the '
                        'post-processing stage, whose seconds also hold the PNG files. The figures themselves are those of a flow from random weights '
                        'and prove plumbing, not plausibility')

    rec = dict(csrc_sha16=hip.csrc_sha16(), build=hip.build_info(), device=torch.cuda.get_device_name(0), size=[H, W], reps=args.reps,
               hbm_roof_gb_per_s=HBM_ROOF_GBS, thr=flowphoto.PHOTO_THR, ws_bytes=nws,
               cached_bytes=len(cached) * 14 * H * W, pool_bytes=len(pool) * 14 * H * W,
               vps_flow_photo=kernel, yardsticks_same_sitting=yard,
               kernel_note='HIP events round one call = two launches (the counting pass, then one workgroup that adds the partial sums), so two launch '
                           'latencies are part of every figure; bytes per pixel are the expected values computed from the shapes (14 streamed + the optional '
                           'byte maps), not counter readings; the corner gather (up to 12 more bytes of prev per pixel, from the caches) is not in them',
               figures_of_the_first_triple={g: {k: round(first[g][k], 4) for k in ('mae_warp', 'mae_static', 'ratio', 'gain_db', 'flagged_share')}
                                            for g in ('all', 'visible', 'masked')},
               per_pair=dict(pairs_per_window=len(some), windows=3, **per_pair, download_and_restatement_over_add_pair=round(ratio, 2),
                             note='wall clock per pair, frames, flow and mask on the device in both ways; add_pair: two launches per pair and one download '
                                  'per video (a fresh evaluator per window); download_and_restatement: 31.5 MB down per pair, then the array form of '
                                  'tests/flow_photo_restate.py on the host (NumPy float32 / float64 and math.fsum)'),
               run_vps_synthetic=tool,
               not_measured=['real footage (none is available): with random weights the synthetic flow is meaningless, so the tool figures prove plumbing, not '
                             'plausibility, and the default thr = 16 is equally unvalidated',
                             'a profiler trace (rocprofv3: event times include the launches)', 'hardware counters for the bytes moved, the cache hit rate of the gather among them',
                             'FlowNet2\'s own padded layout (8-byte loads) and the scalar-load layouts', 'masks and frames off a dword boundary (the byte paths)',
                             'tools/run_config3.py with the new flags (it needs the dataset or a clip)'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1); f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
