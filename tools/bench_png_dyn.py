#!/usr/bin/env python
"""Fixed against dynamic Huffman blocks in the device PNG writer (`vps_png_deflate_h` / `vps_png_deflate_bpp_h`, csrc/png_ops.hip)
-> profiles/png_dynamic_pipeline.json.

Inputs: the synthetic flow field of tools/bench_kitti_flow.py at 375 x 1242 and 1024 x 2048 coded as KITTI 16-bit RGB (6 bytes per pixel),
the flow-colour image of the 1024 x 2048 field of tools/bench_output_pipeline.py (RGB), and its 1024 x 2048 panoptic map (RGB, pan_2ch).
Time: the filter + encode + scan + gather chain, by device events, 5 warm-up calls, the median of 30 with min - max, the two coders
alternating call by call in one process; every call takes the next entry of a pool of distinct device buffers (inputs, outputs,
workspaces) larger than twice the 256 MB Infinity Cache.
Size: the stream of each coder against the fixed stream, zlib's Z_RLE strategy (level 6: the same tokens, zlib's own blocks) and zlib
level 6 over the same filtered bytes.
Writer: `FlowWriter(fmt='kitti')` files/s at 4 worker threads with each coder, the median of 3 windows.
Parent: the fixed chain's times beside the committed profiles (kitti_flow_pipeline.json encode_deflate - which times the flow coding
kernel as well, so that leg is repeated here with it - and png_output_pipeline.json pan_2ch), inside / outside their recorded spread."""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
POOL_BYTES = 600 << 20


def zrle(S):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(S) + c.flush())


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4), 'calls': len(ms)}


def timed_pair(torch, call, warmup=5, n=30):
    """call(i, huffman): the two coders alternate; events round each call"""
    for i in range(warmup):
        call(2 * i, 'fixed'); call(2 * i + 1, 'dynamic')
    torch.cuda.synchronize()
    ev = {h: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for h in ('fixed', 'dynamic')}
    for k in range(n):
        for j, h in enumerate(('fixed', 'dynamic')):
            a, b = ev[h][k]
            a.record()
            call(2 * (warmup + k) + j, h)
            b.record()
    torch.cuda.synchronize()
    return {h: stats([a.elapsed_time(b) for a, b in ev[h]]) for h in ev}


def bench_image(name, imgs_host, bpp, torch, dev, pre=None):
    """imgs_host: up to four dense uint8 [H][rowbytes] images; pre(k, img): an optional kernel enqueued in front of the chain"""
    from vps_amd import kittiflow
    H, rowbytes = imgs_host[0].shape
    cap, wsb = kittiflow.png_encode_bound_bpp(H, rowbytes, bpp)
    per_item = H * rowbytes + cap + wsb
    pool = max(8, -(-POOL_BYTES // per_item))
    imgs = [torch.from_numpy(imgs_host[i % len(imgs_host)]).to(dev) for i in range(pool)]
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(pool)]
    wss = [torch.empty(wsb, dtype=torch.uint8, device=dev) for _ in range(pool)]
    size = torch.zeros(1, dtype=torch.int64, device=dev)

    def call(i, h):
        k = i % pool
        if pre is not None:
            pre(k, imgs[k])
        kittiflow.png_deflate_bpp(imgs[k], bpp, outs[k], wss[k], size, huffman=h)
    rep = {'input': name, 'H': H, 'rowbytes': rowbytes, 'bpp': bpp, 'pool_entries': pool, 'pool_mb': round(pool * per_item / 2 ** 20, 1)}
    rep['time'] = timed_pair(torch, call)
    streams = {}
    for h in ('fixed', 'dynamic'):
        kittiflow.png_deflate_bpp(imgs[0], bpp, outs[0], wss[0], size, huffman=h)
        streams[h] = outs[0][:int(size.item())].cpu().numpy().tobytes()
    S = zlib.decompress(streams['fixed'])
    assert zlib.decompress(streams['dynamic']) == S
    nf, nd, nr, n6 = len(streams['fixed']), len(streams['dynamic']), zrle(S), len(zlib.compress(S, 6))
    rep['size'] = dict(raw_bytes=len(S), fixed_bytes=nf, dynamic_bytes=nd, zrle_bytes=nr, zlib6_bytes=n6, segments=-(-len(S) // 8192),
                       dynamic_over_fixed=round(nd / nf, 4), dynamic_over_zrle=round(nd / nr, 4), dynamic_over_zlib6=round(nd / n6, 4),
                       fixed_over_zlib6=round(nf / n6, 4), inside_the_cap_zrle_plus_274_per_segment=bool(nd <= nr + -(-len(S) // 8192) * 274))
    f, d = rep['time']['fixed']['median_ms'], rep['time']['dynamic']['median_ms']
    rep['dynamic_costs_ms'] = round(d - f, 4)
    # bytes saved per extra microsecond of the chain; None where the dynamic chain is not slower or saves nothing
    rep['bytes_saved_per_extra_us'] = round((nf - nd) / ((d - f) * 1e3), 1) if d > f and nf > nd else None
    del imgs, outs, wss
    torch.cuda.empty_cache()
    return rep


def spread(ours, theirs):
    lo, hi = theirs['min_ms'], theirs['max_ms']
    return dict(here=ours, committed=dict(median_ms=theirs['median_ms'], min_ms=lo, max_ms=hi),
                verdict='inside the recorded spread' if lo <= ours['median_ms'] <= hi else 'OUTSIDE the recorded spread')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_dynamic_pipeline.json'))
    ap.add_argument('--files', type=int, default=32)
    args = ap.parse_args(argv)
    import torch
    import bench_kitti_flow as BK
    import bench_output_pipeline as BO
    from vps_amd import flowvis, hip, kittiflow
    dev = torch.device('cuda:0')
    rep = {'tool': 'tools/bench_png_dyn.py', 'device': torch.cuda.get_device_name(0), 'build': hip.build_info(),
           'protocol': 'device events round each call, 5 warm-up calls, median of 30 with min - max, fixed and dynamic alternating call by call; '
                       'inputs, outputs and workspaces cycle through a pool of %d MB or more (Infinity Cache: 256 MB)' % (POOL_BYTES >> 20),
           'not_measured': 'real KITTI files (sparse ground truth) and real predicted flows; a profiler trace of the dynamic kernel (occupancy, '
                           'LDS conflicts of the histogram); the writers of --device-png / error maps end to end; more than one stream at a time',
           'inputs': []}
    parent = {}
    kitti = json.load(open(os.path.join(ROOT, 'profiles', 'kitti_flow_pipeline.json')))
    for H, W in ((375, 1242), (1024, 2048)):
        fields = [BK.synth_flow(H, W, s) for s in range(4)]
        raws = [BK.np_encode(f, np.ones((H, W), bool)) for f, _ in fields]
        r = bench_image('kitti flow %dx%d' % (H, W), raws, 6, torch, dev)
        rep['inputs'].append(r)
        # the parent's leg: the flow coding kernel + the fixed chain, as tools/bench_kitti_flow.py times it
        src = [torch.from_numpy(fields[i % 4][0]).to(dev) for i in range(r['pool_entries'])]
        r2 = bench_image('kitti flow %dx%d with vps_kitti_flow_encode in front' % (H, W), raws, 6, torch, dev,
                         pre=lambda k, img: kittiflow.kitti_flow_encode(src[k], None, img))
        del src
        old = [s for s in kitti['sizes'] if (s['H'], s['W']) == (H, W)][0]['encode_deflate']
        parent['kitti_flow_%dx%d_encode_deflate' % (H, W)] = spread(r2['time']['fixed'], old)
        rep['inputs'].append(r2)
    H, W = 1024, 2048
    flows = [torch.from_numpy(BO.flow_field(H, W, s)).to(dev) for s in range(4)]
    colour = [flowvis.flow_colour(f).cpu().numpy().reshape(H, 3 * W) for f in flows]
    rep['inputs'].append(bench_image('flow colour RGB %dx%d' % (H, W), colour, 3, torch, dev))
    pans = [BO.label_map(H, W, s).reshape(H, 3 * W) for s in range(4)]
    r = bench_image('panoptic map (pan_2ch) %dx%d' % (H, W), pans, 3, torch, dev)
    rep['inputs'].append(r)
    old = json.load(open(os.path.join(ROOT, 'profiles', 'png_output_pipeline.json')))['pan_2ch']
    lo = old['device_ms_min']
    parent['png_output_pan_2ch'] = dict(here=r['time']['fixed'], committed=dict(median_ms=old['device_ms_median_of_30'], min_ms=lo),
                                        note='the committed profile has no maximum and did not cycle a pool: median against median only',
                                        ratio_of_medians=round(r['time']['fixed']['median_ms'] / old['device_ms_median_of_30'], 3))
    rep['fixed_chain_against_the_committed_profiles'] = parent
    # writer rate
    H, W = 375, 1242
    fl = [torch.from_numpy(BK.synth_flow(H, W, s)[0]).to(dev) for s in range(4)]
    rates = {}
    with tempfile.TemporaryDirectory() as d:
        for window in range(3):
            for h in ('fixed', 'dynamic'):
                w = flowvis.FlowWriter(dev, workers=4, slots=8, fmt='kitti', huffman=h)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.files):
                    w.submit(fl[i % 4], os.path.join(d, '%s_%03d.png' % (h, i)))
                w.close()
                rates.setdefault(h, []).append((args.files / (time.perf_counter() - t0), w.bytes_written / args.files))
    rep['flow_writer_kitti_375x1242_4_threads'] = {
        h: dict(files_per_s_median=round(sorted(r[0] for r in rates[h])[1], 1), min=round(min(r[0] for r in rates[h]), 1),
                max=round(max(r[0] for r in rates[h]), 1), files=args.files, file_bytes=int(rates[h][0][1])) for h in rates}
    with open(args.out, 'w') as f:
        json.dump(rep, f, indent=1)
        f.write('\n')
    print(json.dumps(rep, indent=1))


if __name__ == '__main__':
    main()
