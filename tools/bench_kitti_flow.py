"""Timings of the KITTI flow path (vps_amd/kittiflow.py) -> profiles/kitti_flow_pipeline.json.

    python tools/bench_kitti_flow.py [--out profiles/kitti_flow_pipeline.json] [--sizes 375x1242 1024x2048]

Per size, by device events, after a warm-up, the median of 30 calls with min - max; every call takes the next entry of a pool of distinct
device buffers (inputs AND outputs) that is larger than twice the 256 MB Infinity Cache, so no call finds its data cached:
    reconstruct_adaptive   vps_kitti_flow_reconstruct (both launches) on a file filtered like libpng does it: per row the type with the
                           smallest sum of |int8(residual)| among all five
    reconstruct_paeth      the same on an all-Paeth file: ONE group, the serial worst case
    encode_deflate         vps_kitti_flow_encode + vps_png_deflate_bpp (five launches)
and by a host clock around work that ends in a synchronise, files/s:
    read                   read_kitti_flow of files on disk (inflate on the host, un-filter and decode on the device), `--threads` threads
    write                  FlowWriter(fmt='kitti'), its default worker threads
    baseline_read / baseline_write   zlib + the NumPy restatement of the coding on as many threads. The baseline is WEAK: NumPy holds the
                           interpreter lock between its calls, and it reads only files of None / Sub / Up rows (the ones this writer
                           makes), since Average and Paeth rows do not vectorise along a row; adaptive files have no baseline here.
and the file size against zlib level 6 over the same filtered bytes.

What bounds the un-filter: a group of rows is a dependency chain of W/4 + rows - 1 steps (one barrier each), one workgroup per group, so
its time is set by the longest group and the step latency, not by bytes over bandwidth; the report gives the steps of the longest chain
and the time per step beside the bytes. The deflate has no match search, so a dense predicted flow comes out near raw size: the ratio
is recorded, not tuned. The field is synthetic (smooth motion + noise, 1/64 steps, ~80 % valid pixels); real KITTI files - sparse
ground truth, about a fifth of the pixels labelled - were not available and are NOT measured."""
import argparse
import json
import os
import sys
import tempfile
import threading
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL_BYTES = 600 << 20
F = np.float32


# ---------------------------------------------------------------------------------------------- the NumPy side (inputs and baseline)
def synth_flow(H, W, seed):
    rg = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    u = 30 * np.sin(x / W * 3 + seed) + 0.02 * y + rg.standard_normal((H, W)).astype(F) * 0.3
    v = 8 * np.cos(y / H * 2 + seed) + rg.standard_normal((H, W)).astype(F) * 0.3
    return np.stack([u, v], axis=-1).astype(F), (rg.random((H, W)) < 0.8)


def np_encode(flow, valid):
    """the write rule -> raw uint8 [H, 6 W]"""
    q = np.maximum(np.minimum(flow * F(64) + F(32768), F(65535)), F(0)).astype(np.uint16)
    H, W = valid.shape
    rgb = np.concatenate([q, valid[..., None].astype(np.uint16)], axis=-1)
    return np.stack([(rgb >> 8).astype(np.uint8), (rgb & 255).astype(np.uint8)], axis=-1).reshape(H, 6 * W)


def np_filter(raw, mode):
    """raw -> filtered scanlines. mode 'adaptive': per row the smallest sum of |int8(residual)| among the five types (libpng's
    heuristic); 'paeth': type 4 everywhere; 'nsu': among None / Sub / Up (this repository's writer)"""
    H, n = raw.shape
    v = raw.astype(np.int16)
    a = np.zeros_like(v); a[:, 6:] = v[:, :-6]
    b = np.zeros_like(v); b[1:] = v[:-1]
    c = np.zeros_like(v); c[1:, 6:] = v[:-1, :-6]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = np.stack([v, v - a, v - b, v - ((a + b) >> 1), v - paeth]) & 255
    if mode == 'paeth':
        ft = np.full(H, 4)
    else:
        use = cands if mode == 'adaptive' else cands[:3]
        ft = np.argmin(np.where(use < 128, use, 256 - use).sum(axis=2), axis=0)
    out = np.empty((H, 1 + n), np.uint8)
    out[:, 0] = ft
    out[:, 1:] = cands[ft, np.arange(H)]
    return out, ft


def png16_file(scan_bytes, H, W):
    import struct

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 16, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(scan_bytes, 6)) + chunk(b'IEND', b'')


def np_read(data):
    """baseline reader: zlib + NumPy, files of None / Sub / Up rows only -> (flow, valid)"""
    import struct
    W, H = struct.unpack('>II', data[16:24])
    pos, idat = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        if tag == b'IDAT':
            idat.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    scan = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8).reshape(H, 1 + 6 * W)
    raw = np.empty((H, 6 * W), np.uint8)
    for y in range(H):
        ft, line = scan[y, 0], scan[y, 1:]
        if ft == 0:
            raw[y] = line
        elif ft == 1:
            raw[y] = np.cumsum(line.reshape(W, 6), axis=0, dtype=np.uint8).reshape(-1)
        elif ft == 2:
            raw[y] = line + (raw[y - 1] if y else 0)
        else:
            raise ValueError('the NumPy baseline reads None / Sub / Up rows only')
    s = raw.reshape(H, W, 3, 2).astype(np.int32)
    rgb = s[..., 0] * 256 + s[..., 1]
    valid = rgb[..., 2] > 0
    return np.where(valid[..., None], (rgb[..., :2] - 32768).astype(F) / F(64), F(0)), valid


def np_write(flow, valid):
    raw = np_encode(flow, valid)
    return png16_file(np_filter(raw, 'nsu')[0].tobytes(), *valid.shape)


def threaded_rate(fn, items, threads):
    """files/s of fn over items on `threads` plain threads"""
    it, lock = iter(items), threading.Lock()

    def work():
        while True:
            with lock:
                x = next(it, None)
            if x is None:
                return
            fn(x)
    ts = [threading.Thread(target=work) for _ in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return len(items) / (time.perf_counter() - t0)


# ---------------------------------------------------------------------------------------------- the device side
def stats(ms):
    ms = sorted(ms)
    return {'median_ms': round(ms[len(ms) // 2], 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4), 'calls': len(ms)}


def timed(torch, calls, warmup=5, n=30):
    """calls(i): enqueue call number i (i picks the pool entry). Events round each call."""
    for i in range(warmup):
        calls(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for k, (a, b) in enumerate(ev):
        a.record()
        calls(warmup + k)
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def longest_chain(ft, W, band):
    """steps of the longest group: per band of `band` rows chunks + rows - 1"""
    starts = [y for y in range(len(ft)) if y == 0 or ft[y] < 2] + [len(ft)]
    chunks, best = (W + 3) // 4, 0
    for s, e in zip(starts, starts[1:]):
        rows, steps = e - s, 0
        while rows > 0:
            steps += chunks + min(rows, band) - 1
            rows -= band
        best = max(best, steps)
    return best, len(starts) - 1


def bench_size(H, W, args, torch, dev):
    import ctypes
    from vps_amd import hip, kittiflow
    from vps_amd.flowvis import FlowWriter
    lib = hip.load()
    band = hip.png_block_rows()
    rep = {'H': H, 'W': W, 'scan_bytes': H * (1 + 6 * W), 'flow_bytes': 8 * H * W}
    fields = [synth_flow(H, W, s) for s in range(4)]
    raws = [np_encode(f, v) for f, v in fields]
    need = ctypes.c_int64()
    hip.check(lib.vps_kitti_flow_reconstruct_ws(H, W, ctypes.byref(need)), 'ws')
    per_item = rep['scan_bytes'] + rep['flow_bytes'] + H * W + need.value
    pool = max(8, -(-POOL_BYTES // per_item))
    rep['pool_entries'], rep['pool_mb'] = pool, round(pool * per_item / 2 ** 20, 1)
    flows = [torch.empty(H, W, 2, dtype=torch.float32, device=dev) for _ in range(pool)]
    masks = [torch.empty(H, W, dtype=torch.uint8, device=dev) for _ in range(pool)]
    wss = [torch.empty(need.value, dtype=torch.uint8, device=dev) for _ in range(pool)]
    for mode in ('adaptive', 'paeth'):
        filt = [np_filter(r, mode) for r in raws]
        scans = [torch.from_numpy(filt[i % 4][0].reshape(-1).copy()).to(dev) for i in range(pool)]

        def call(i):
            k = i % pool
            hip.check(lib.vps_kitti_flow_reconstruct(hip.ptr(scans[k]), H, W, None, hip.ptr(flows[k]), flows[k].numel() * 4, hip.ptr(masks[k]),
                                                     hip.ptr(wss[k]), need.value, hip.stream_ptr()), 'vps_kitti_flow_reconstruct')
        r = timed(torch, call)
        steps, groups = longest_chain(filt[0][1], W, band)
        r.update(longest_chain_steps=steps, groups=groups, us_per_step_of_the_longest_chain=round(1e3 * r['median_ms'] / steps, 3),
                 gb_per_s_scan_plus_outputs=round((rep['scan_bytes'] + rep['flow_bytes'] + H * W) / r['median_ms'] / 1e6, 1),
                 filter_type_histogram=np.bincount(filt[0][1], minlength=5).tolist())
        # the result is the field
        want = np.where(fields[0][1][..., None], np_read_raw(raws[0]), F(0))
        call(0)
        torch.cuda.synchronize()
        assert np.array_equal(flows[0].cpu().numpy(), want) and np.array_equal(masks[0].cpu().numpy(), fields[0][1].astype(np.uint8))
        rep['reconstruct_' + mode] = r
        del scans
    # encode + deflate
    cap, wsb = kittiflow.png_encode_bound_bpp(H, 6 * W, 6)
    per_item = rep['flow_bytes'] + 6 * H * W + cap + wsb
    pool_e = max(8, -(-POOL_BYTES // per_item))
    del flows, masks, wss
    src = [torch.from_numpy(fields[i % 4][0]).to(dev) for i in range(pool_e)]
    imgs = [torch.empty(H, 6 * W, dtype=torch.uint8, device=dev) for _ in range(pool_e)]
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(pool_e)]
    dws = [torch.empty(wsb, dtype=torch.uint8, device=dev) for _ in range(pool_e)]
    size = torch.zeros(1, dtype=torch.int64, device=dev)

    def enc(i):
        k = i % pool_e
        kittiflow.kitti_flow_encode(src[k], None, imgs[k])
        kittiflow.png_deflate_bpp(imgs[k], 6, outs[k], dws[k], size)
    r = timed(torch, enc)
    enc(0)
    n = int(size.item())
    stream = outs[0][:n].cpu().numpy().tobytes()
    S = zlib.decompress(stream)
    r.update(pool_entries=pool_e, stream_bytes=n, raw_bytes=len(S), ratio_to_raw=round(n / len(S), 4), zlib6_bytes=len(zlib.compress(S, 6)),
             ratio_to_zlib6=round(n / len(zlib.compress(S, 6)), 3))
    rep['encode_deflate'] = r
    del src, imgs, outs, dws
    # files/s
    nfiles, threads = args.files, args.threads
    with tempfile.TemporaryDirectory() as d:
        own = [np_write(*fields[i % 4]) for i in range(4)]
        names = []
        for i in range(nfiles):
            names.append(os.path.join(d, 'in_%03d.png' % i))
            with open(names[-1], 'wb') as f:
                f.write(own[i % 4])
        blobs = [own[i % 4] for i in range(nfiles)]
        kittiflow.read_kitti_flow(names[0], device=dev)
        torch.cuda.synchronize()

        def rd(nm):
            kittiflow.read_kitti_flow(nm, device=dev)
        rates = []
        for _ in range(3):
            rate_t0 = time.perf_counter()
            threaded_rate(rd, names, threads)
            torch.cuda.synchronize()
            rates.append(nfiles / (time.perf_counter() - rate_t0))
        rep['read'] = {'files_per_s_median': round(sorted(rates)[1], 1), 'min': round(min(rates), 1), 'max': round(max(rates), 1), 'threads': threads,
                       'files': nfiles, 'file_bytes': len(own[0]), 'rows': 'None / Sub / Up (the files of this writer)'}
        rates = [threaded_rate(np_read, blobs[:max(threads, 4)], threads) for _ in range(3)]
        rep['baseline_read'] = {'files_per_s_median': round(sorted(rates)[1], 2), 'min': round(min(rates), 2), 'max': round(max(rates), 2), 'threads': threads,
                                'files': max(threads, 4), 'note': 'zlib + NumPy, weak: interpreter lock, one Python step per row'}
        dflows = [torch.from_numpy(fields[i % 4][0]).to(dev) for i in range(4)]
        rates = []
        for rnd in range(4):
            w = FlowWriter(dev, fmt='kitti')
            t0 = time.perf_counter()
            for i in range(nfiles):
                w.submit(dflows[i % 4], os.path.join(d, 'out_%d_%03d.png' % (rnd, i)))
            w.close()
            torch.cuda.synchronize()
            if rnd:
                rates.append(nfiles / (time.perf_counter() - t0))
        rep['write'] = {'files_per_s_median': round(sorted(rates)[1], 1), 'min': round(min(rates), 1), 'max': round(max(rates), 1), 'files': nfiles,
                        'file_bytes': os.path.getsize(os.path.join(d, 'out_1_000.png'))}
        items = [fields[i % 4] for i in range(max(threads, 4))]
        rates = [threaded_rate(lambda fv: np_write(*fv), items, threads) for _ in range(3)]
        rep['baseline_write'] = {'files_per_s_median': round(sorted(rates)[1], 2), 'min': round(min(rates), 2), 'max': round(max(rates), 2),
                                 'threads': threads, 'files': len(items), 'file_bytes': len(own[0]), 'note': 'NumPy coding and filter + zlib level 6'}
    return rep


def np_read_raw(raw):
    H, W = raw.shape[0], raw.shape[1] // 6
    s = raw.reshape(H, W, 3, 2).astype(np.int32)
    rgb = s[..., 0] * 256 + s[..., 1]
    return (rgb[..., :2] - 32768).astype(F) / F(64)


def main(argv=None):
    ap = argparse.ArgumentParser(description='timings of the KITTI flow path')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kitti_flow_pipeline.json'))
    ap.add_argument('--sizes', nargs='+', default=['375x1242', '1024x2048'])
    ap.add_argument('--files', type=int, default=32, help='files per window of the files/s figures')
    ap.add_argument('--threads', type=int, default=4, help='reader threads, and threads of the NumPy baselines')
    ap.add_argument('--device', default='cuda')
    args = ap.parse_args(argv)
    import torch
    from vps_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit('this benchmark measures the device path: no GPU, no numbers')
    dev = torch.device(args.device)
    rep = {'tool': 'tools/bench_kitti_flow.py', 'csrc_sha16': hip.csrc_sha16(), 'device': torch.cuda.get_device_name(dev),
           'protocol': 'device events round each call, 5 warm-up calls, median of 30 with min - max; inputs and outputs cycle through a pool of '
                       '%d MB or more (Infinity Cache: 256 MB); files/s by a host clock round work that ends in a synchronise, median of 3 windows' % (POOL_BYTES >> 20),
           'not_measured': ['real KITTI files (none available; the ground truth there is sparse, about a fifth of the pixels)',
                            'a NumPy baseline for files with Average / Paeth rows', 'kernel times by a profiler trace', 'several processes sharing the device'],
           'sizes': []}
    for s in args.sizes:
        H, W = (int(v) for v in s.lower().split('x'))
        rep['sizes'].append(bench_size(H, W, args, torch, dev))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rep, f, indent=1)
        f.write('\n')
    print(json.dumps(rep))
    return rep


if __name__ == '__main__':
    main()
