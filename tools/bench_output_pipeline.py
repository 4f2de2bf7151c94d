"""The output side of the clip pipeline, measured: what does writing the two result maps of EVERY frame cost?

    python tools/bench_output_pipeline.py [--frames 30] [--height 1024 --width 2048] [--out profiles/png_output_pipeline.json]

Two map kinds at Cityscapes-VPS size, both synthetic (eight stuff bands with wavy borders, 45 ellipses with distinct object ids):
`pan_2ch` = (pan_seg, pan_ins, pan_obj) as `PanopticUnifier` returns it, `pan_pred` = the same segments painted with 24-bit colours as
`vps_segment_paint` does. Measured:
  device_ms      `vps_png_deflate` (filter + encode + scan + gather) per map, median of 30, timed with events
  fraction       of 8 TB/s for its algorithmic bytes: two reads of the image (filter choice, encode) + the stream written
  file sizes     the device encoder's file against PIL's (`Image.fromarray(map).save`) for both kinds
  frames/s       at two maps per frame: `DevicePngWriter` (2 workers) fed device tensors, `AsyncPngWriter` at 1, 2 and 4 workers fed
                 the host copies it needs (its 2 x 6 MB download per frame included), on the same host
Prints one JSON line and writes it to --out, stamped with `hip.csrc_sha16()`. Needs the GPU.

`--leg overlay` measures the overlay JPEGs instead (and writes profiles/overlay_output_pipeline.json): a synthetic photographic frame
(BGR) and the painted map of above, one overlay per frame at quality 90, 4:2:0.
  device_ms      `vps_overlay_render` and `vps_jpeg_encode_coef`, each the median of 30, timed with events, with their algorithmic bytes
                 over 8 TB/s (render: two inputs read, one image written; encode: the image read, the coefficients written)
  host_ms        `vps_jpeg_write` on one thread for one frame (Huffman coding + container), and the device-to-host copy it waits for
  file sizes     the device path's file and PIL's `save(format='JPEG', quality=90, subsampling=2)` of the same pixels (equal scans)
  frames/s       `DeviceJpegWriter` against "download frame and colour map + NumPy blend + PIL save" on a thread pool, both with the same
                 thread count (1, 2, 4), on the same host
Neither side had been measured before; the report states which one wins.

`--leg overlay_entropy` measures the Huffman coding of those overlays on the device (`entropy='device'`) and adds the key
`device_entropy` to profiles/overlay_output_pipeline.json; the other keys stay as they are.
  device_ms      `vps_jpeg_encode_scan` (5 launches), the median of 30 with the slowest and fastest, timed with events, with its algorithmic bytes
  host_ms        one frame on one thread: copy of the scan + `vps_jpeg_wrap` against copy of the coefficients + `vps_jpeg_write`
  bytes          downloaded per frame in both modes
  frames/s       `DeviceJpegWriter(entropy='device')` against `entropy='host'` - the writer as it was before the option existed - at 1, 2
                 and 4 workers in the same process, the windows of the two modes alternating; the median of --repeats windows of --frames
                 frames with the slowest and fastest

`--leg flow` measures the optical-flow output (and writes profiles/flow_output_pipeline.json): a synthetic flow field (smooth motion
plus noise) in FlowNet2's layout (NHWC, pixel stride 4), one file per frame.
  device_ms      `vps_flow_max_radius` and `vps_flow_colour`, each the median of 30, timed with events, with their algorithmic bytes over
                 8 TB/s (the whole strided map read - the 16-byte pixels share cache lines with their padding; colour: + the image written)
  frames/s       `FlowWriter` at 1, 2 and 4 workers for 'jpg' and 'flo' against the host way on as many threads: download the two flow
                 channels (16.8 MB), the NumPy restatement of the colour coding (tests/flow_vis_restate.py) + PIL save for 'jpg', header
                 + `tofile` for 'flo'; each figure is the median of --repeats windows of --frames frames, with the slowest and fastest

`--leg tubes` measures the track tubes (and writes profiles/tubes_output_pipeline.json): the `pan_2ch` maps of above (45 instances), the
COCO encoding of every instance of every frame.
  device_ms      one `vps_rle_runs` call (two sweeps and the scan), the median of 30, timed with events; the maps are 6 MB each and
                 stay in the caches between calls, so the figure is a cache-resident one; the run count and the bytes downloaded
  host_ms        `vps_rle_strings` on one thread for one frame's run list, the median of 30
  frames/s       `TubeCollector` (things by class) at 1, 2 and 4 coding threads against the host way on as many threads: download
                 `pan_2ch` (6.3 MB), `pan == key` per instance, the NumPy restatement of rleEncode + rleToString (tests/rle_restate.py;
                 pycocotools where it is installed); each figure is the median of --repeats windows of --frames frames"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def label_map(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    wave = (H / 40.0) * np.sin(xx / (W / 13.0) + 0.7 + seed) + (H / 90.0) * np.sin(xx / (W / 47.0))
    seg = np.clip(((yy + wave) * 8.0 / H).astype(np.int64), 0, 7).astype(np.uint8)
    ins = np.zeros((H, W), np.uint8)
    obj = seg.copy()
    for i in range(45):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        ry, rx = int(rng.integers(H // 40, H // 6)), int(rng.integers(W // 60, W // 8))
        y0, y1, x0, x1 = max(0, cy - ry), min(H, cy + ry + 1), max(0, cx - rx), min(W, cx + rx + 1)
        m = ((yy[y0:y1, x0:x1] - cy) / ry) ** 2 + ((xx[y0:y1, x0:x1] - cx) / rx) ** 2 <= 1.0
        seg[y0:y1, x0:x1][m] = 11 + i % 8
        ins[y0:y1, x0:x1][m] = i + 1
        obj[y0:y1, x0:x1][m] = 100 + i
    return np.ascontiguousarray(np.stack([seg, ins, obj], -1))


def painted(two, seed):
    """a colour per (pan_seg, pan_obj) segment, like TrackConverter's lookup table"""
    lut = np.random.default_rng(seed).integers(0, 256, (65536, 3)).astype(np.uint8)
    return np.ascontiguousarray(lut[two[..., 0].astype(np.int64) * 256 + two[..., 2]])


def pil_size(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'PNG')
    return len(b.getvalue())


def numpy_overlay(frame_bgr, colour_rgb, alpha):
    """the host path's blend: what `vps_overlay_render` computes, in NumPy (uint16 arithmetic)"""
    f = frame_bgr[..., ::-1].astype(np.uint16)
    c = colour_rgb.astype(np.uint16)
    out = ((f * (256 - alpha) + c * alpha + 128) >> 8).astype(np.uint8)
    void = ~colour_rgb.any(-1)
    out[void] = frame_bgr[..., ::-1][void]
    edge = np.zeros(void.shape, dtype=bool)
    edge[:, :-1] |= (colour_rgb[:, :-1] != colour_rgb[:, 1:]).any(-1)
    edge[:-1, :] |= (colour_rgb[:-1, :] != colour_rgb[1:, :]).any(-1)
    out[edge] = 255
    return out


def overlay_leg(args):
    import torch
    from PIL import Image
    from vps_amd import hip, synth
    from vps_amd import postprocess as pp
    assert torch.cuda.is_available(), 'the device encoder needs the MI355X'
    dev = torch.device('cuda:0')
    H, W, Q, A = args.height, args.width, 90, 128
    colours = [painted(label_map(H, W, s), s) for s in range(4)]
    frames = [synth.synth_frame(H, W, seed=s, shift=(2 * s, s), noise=2.0).astype(np.uint8) for s in range(4)]       # BGR
    d_col = [torch.from_numpy(a).to(dev) for a in colours]
    d_fr = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in frames]
    rep = dict(mode='overlay_output', size=[H, W], frames=args.frames, quality=Q, subsampling='4:2:0', alpha=A, host_cpus=os.cpu_count(),
               csrc_sha16=hip.csrc_sha16())

    def timed(fn):
        for _ in range(3):
            fn(0)
        torch.cuda.synchronize()
        ms = []
        for i in range(30):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            fn(i)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    _, coef_bytes, _ = pp.jpeg_encode_bound(H, W)
    coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
    rgbs = [pp.render_overlay(d_fr[i], d_col[i], A) for i in range(4)]
    med, mn = timed(lambda i: pp.render_overlay(d_fr[i % 4], d_col[i % 4], A))
    alg = 3 * H * W * 3
    rep['render'] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(mn, 4), algorithmic_MB=round(alg / 1e6, 2),
                         fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4))
    med, mn = timed(lambda i: pp.jpeg_encode_coef(rgbs[i % 4], Q, '4:2:0', coef))
    alg = H * W * 3 + coef_bytes
    rep['encode_coef'] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(mn, 4), algorithmic_MB=round(alg / 1e6, 2),
                              fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4), coefficient_MB=round(coef_bytes / 1e6, 2))
    # host side of one frame, one thread
    pinned = torch.empty(coef_bytes // 2, dtype=torch.int16).pin_memory()
    pp.jpeg_encode_coef(rgbs[1], Q, '4:2:0', coef)
    torch.cuda.synchronize()
    cp, wr = [], []
    buf = np.empty(pp.jpeg_encode_bound(H, W)[2], dtype=np.uint8)
    for _ in range(10):
        t0 = time.perf_counter()
        pinned.copy_(coef, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        data = pp.jpeg_write(pinned, H, W, Q, '4:2:0', buf)
        t2 = time.perf_counter()
        cp.append(1e3 * (t1 - t0)); wr.append(1e3 * (t2 - t1))
    b = io.BytesIO()
    host_rgb = rgbs[1].cpu().numpy()
    Image.fromarray(host_rgb).save(b, format='JPEG', quality=Q, subsampling=2, optimize=False)
    ref = b.getvalue()
    assert data[data.index(b'\xff\xda'):] == ref[ref.index(b'\xff\xda'):], 'the scan differs from PIL\'s'
    assert np.array_equal(host_rgb, numpy_overlay(frames[1], colours[1], A)), 'the host blend is not the device blend'
    rep['host_one_frame'] = dict(copy_ms_median_of_10=round(float(np.median(cp)), 3), jpeg_write_ms_median_of_10=round(float(np.median(wr)), 3))
    rep['file'] = dict(device_file_bytes=len(data), pil_file_bytes=len(ref), scan_equal_to_pil=True, raw_over_file=round(H * W * 3 / len(data), 1))

    def run_device(workers):
        w = pp.DeviceJpegWriter(dev, workers=workers, slots=8, quality=Q)
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(args.frames):
                w.submit(pp.render_overlay(d_fr[f % 4], d_col[f % 4], A), os.path.join(tmp, '%04d.jpg' % f))
            t_submit = time.perf_counter() - t0
            w.close()
            dt = time.perf_counter() - t0
        assert w.device_encoded == args.frames
        return dict(frames_per_s=round(args.frames / dt, 1), submit_s=round(t_submit, 4), total_s=round(dt, 4), MB_written=round(w.bytes_written / 1e6, 2))

    def run_host(workers):
        from concurrent.futures import ThreadPoolExecutor

        def job(fr, col, name):
            Image.fromarray(numpy_overlay(fr, col, A)).save(name, format='JPEG', quality=Q, subsampling=2, optimize=False)
            return os.path.getsize(name)
        with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(workers) as pool:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            futs = []
            for f in range(args.frames):
                fr, col = d_fr[f % 4].cpu().numpy(), d_col[f % 4].cpu().numpy()      # the download the host path needs
                futs.append(pool.submit(job, fr, col, os.path.join(tmp, '%04d.jpg' % f)))
            t_submit = time.perf_counter() - t0
            nbytes = sum(x.result() for x in futs)
            dt = time.perf_counter() - t0
        return dict(frames_per_s=round(args.frames / dt, 1), submit_s=round(t_submit, 4), total_s=round(dt, 4), MB_written=round(nbytes / 1e6, 2))

    run_device(2)                                                    # warm-up: ring slots, pinned staging, copy streams
    run_host(2)
    rep['device_writer'] = {str(n): run_device(n) for n in (1, 2, 4)}
    rep['host_numpy_pil'] = {str(n): run_host(n) for n in (1, 2, 4)}
    rep['verdict'] = {str(n): ('device path %s: %.1f vs %.1f frames/s' % ('wins' if rep['device_writer'][str(n)]['frames_per_s'] > rep['host_numpy_pil'][str(n)]['frames_per_s'] else 'LOSES',
                                                                        rep['device_writer'][str(n)]['frames_per_s'], rep['host_numpy_pil'][str(n)]['frames_per_s'])) for n in (1, 2, 4)}
    rep['not_measured'] = 'a clip of the detector with --overlay against the same clip without it'
    return rep


def overlay_entropy_leg(args):
    """`--leg overlay_entropy`: the Huffman coding of the overlay JPEGs on the device (`vps_jpeg_encode_scan`) against the host coder"""
    import torch
    from vps_amd import hip, synth
    from vps_amd import postprocess as pp
    assert torch.cuda.is_available(), 'the device encoder needs the MI355X'
    dev = torch.device('cuda:0')
    H, W, Q, A = args.height, args.width, 90, 128
    colours = [painted(label_map(H, W, s), s) for s in range(4)]
    frames = [synth.synth_frame(H, W, seed=s, shift=(2 * s, s), noise=2.0).astype(np.uint8) for s in range(4)]       # BGR
    rgbs = [pp.render_overlay(torch.from_numpy(np.ascontiguousarray(f)).to(dev), torch.from_numpy(c).to(dev), A) for f, c in zip(frames, colours)]
    rep = dict(size=[H, W], frames_per_window=args.frames, windows=args.repeats, quality=Q, subsampling='4:2:0', host_cpus=os.cpu_count(),
               csrc_sha16=hip.csrc_sha16())
    _, coef_bytes, _ = pp.jpeg_encode_bound(H, W)
    wsb, scan_cap = pp.jpeg_scan_bound(H, W)
    coefs = [pp.jpeg_encode_coef(r, Q, '4:2:0').clone() for r in rgbs]
    out = torch.empty(coef_bytes // 4, dtype=torch.uint8, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    result = torch.empty(2, dtype=torch.int64, device=dev)
    for i in range(3):
        pp.jpeg_encode_scan(coefs[i % 4], H, W, '4:2:0', out, ws, result)
    torch.cuda.synchronize()
    ms = []
    for i in range(30):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        pp.jpeg_encode_scan(coefs[i % 4], H, W, '4:2:0', out, ws, result)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    pp.jpeg_encode_scan(coefs[1], H, W, '4:2:0', out, ws, result)
    n, status = (int(v) for v in result.cpu())
    assert status == pp.JPEG_SCAN_OK, status
    # bytes the algorithm needs: the coefficients read twice (size, pack), the unstuffed stream written once and read twice (count,
    # stuff), the scan written, a 32-bit size per block written and read
    alg = 2 * coef_bytes + 4 * n + 2 * 4 * (coef_bytes // 128)
    med = float(np.median(ms))
    rep['encode_scan'] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(min(ms), 4), device_ms_max=round(max(ms), 4), launches=5,
                              algorithmic_MB=round(alg / 1e6, 2), fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4), scan_bytes=n,
                              workspace_MB=round(wsb / 1e6, 2), timed='events around the five launches, enqueue included')
    # host side of one frame, one thread: copy of the scan + the container, against copy of the coefficients + vps_jpeg_write
    pin_scan = torch.empty(out.numel(), dtype=torch.uint8).pin_memory()
    pin_coef = torch.empty(coef_bytes // 2, dtype=torch.int16).pin_memory()
    buf = np.empty(pp.jpeg_encode_bound(H, W)[2], dtype=np.uint8)
    t = dict(scan_copy=[], wrap=[], coef_copy=[], jpeg_write=[])
    for _ in range(10):
        t0 = time.perf_counter()
        pin_scan[:n].copy_(out[:n], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        data = pp.jpeg_wrap(pin_scan[:n], H, W, Q, '4:2:0', buf)
        t2 = time.perf_counter()
        pin_coef.copy_(coefs[1], non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ref = pp.jpeg_write(pin_coef, H, W, Q, '4:2:0', buf)
        t4 = time.perf_counter()
        for k, v in zip(('scan_copy', 'wrap', 'coef_copy', 'jpeg_write'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[k].append(1e3 * v)
    assert data == ref, 'the device scan differs from the host coder\'s'
    rep['host_one_frame_ms_median_of_10'] = {k: round(float(np.median(v)), 3) for k, v in t.items()}
    rep['bytes_downloaded_per_frame'] = dict(device_entropy=n + 16, host_entropy=coef_bytes, file_bytes=len(data))

    def window(workers, entropy):
        w = pp.DeviceJpegWriter(dev, workers=workers, slots=8, quality=Q, entropy=entropy)
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(args.frames):
                w.submit(rgbs[f % 4], os.path.join(tmp, '%04d.jpg' % f))
            w.close()
            dt = time.perf_counter() - t0
        assert w.device_encoded == args.frames and w.fallback_encoded == 0
        return args.frames / dt, w.bytes_downloaded / args.frames

    rates = {(n_, e): [] for n_ in (1, 2, 4) for e in ('host', 'device')}
    for n_, e in rates:                                              # warm-up: ring slots, pinned staging, copy streams
        window(n_, e)
    for _ in range(args.repeats):                                    # the two modes alternate, so a busy host hits both
        for n_, e in rates:
            rates[(n_, e)].append(window(n_, e)[0])
    rep['writer_frames_per_s'] = {
        str(n_): {e: dict(median=round(float(np.median(rates[(n_, e)])), 1), min=round(min(rates[(n_, e)]), 1), max=round(max(rates[(n_, e)]), 1))
                  for e in ('host', 'device')} for n_ in (1, 2, 4)}
    rep['verdict'] = {str(n_): "entropy='device' %s: %.1f vs %.1f frames/s" % (
        'wins' if np.median(rates[(n_, 'device')]) > np.median(rates[(n_, 'host')]) else 'LOSES',
        np.median(rates[(n_, 'device')]), np.median(rates[(n_, 'host')])) for n_ in (1, 2, 4)}
    rep['comparison'] = "entropy='host' is the parent commit's DeviceJpegWriter, unchanged; same process, same box, windows alternating"
    rep['not_measured'] = ('kernel times from a profiler trace (the event figure includes the enqueue of five launches); a detector clip with '
                           '--overlay --jpeg-entropy device against the same clip without it; 4:4:4; other qualities')
    return rep


def flow_field(H, W, seed):
    """float32 [H,W,2]: a pan plus a zoom about a moving centre plus noise - a few pixels of motion, like consecutive video frames"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cx, cy = W * (0.4 + 0.05 * seed), H * 0.5
    u = 2.0 + 0.004 * (xx - cx) + 1.5 * np.sin(yy / (H / 5.0) + seed) + rng.normal(0, 0.2, (H, W))
    v = -0.5 + 0.004 * (yy - cy) + 1.0 * np.cos(xx / (W / 7.0)) + rng.normal(0, 0.2, (H, W))
    return np.ascontiguousarray(np.stack([u, v], -1).astype(np.float32))


def flow_leg(args):
    import torch
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import flow_vis_restate as F
    from vps_amd import flowvis, hip, nhwc
    assert torch.cuda.is_available(), 'the flow colour kernels need the MI355X'
    dev = torch.device('cuda:0')
    H, W, Q, LD = args.height, args.width, 90, 4
    fields = [flow_field(H, W, s) for s in range(4)]
    maps = [nhwc.FMap(torch.from_numpy(F.strided(f, LD, 0, 0.0)).to(dev)[None].contiguous(), 2, 0) for f in fields]
    rep = dict(mode='flow_output', size=[H, W], frames=args.frames, flow_pixel_stride=LD, quality=Q, host_cpus=os.cpu_count(), csrc_sha16=hip.csrc_sha16())

    def timed(fn):
        for _ in range(3):
            fn(0)
        torch.cuda.synchronize()
        ms = []
        for i in range(30):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            fn(i)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    rad = torch.empty(1, dtype=torch.float64, device=dev)
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    lib = hip.load()
    med, mn = timed(lambda i: flowvis.flow_max_radius(maps[i % 4], rad))
    alg = H * W * LD * 4
    rep['max_radius'] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(mn, 4), algorithmic_MB=round(alg / 1e6, 2),
                             fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4), note='includes the 8-byte memset the call enqueues')
    flowvis.flow_max_radius(maps[1], rad)
    med, mn = timed(lambda i: hip.check(lib.vps_flow_colour(maps[i % 4].ptr(), LD, 0, H, W, hip.ptr(rad), hip.ptr(rgb), hip.stream_ptr()), 'vps_flow_colour'))
    alg = H * W * LD * 4 + H * W * 3
    rep['colour'] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(mn, 4), algorithmic_MB=round(alg / 1e6, 2),
                         fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4))
    got = flowvis.flow_colour(maps[1]).cpu().numpy()
    assert np.array_equal(got, F.colour(fields[1])), 'the device image is not the restatement\'s'
    rep['image_equal_to_numpy_restatement'] = True

    def run_device(fmt, workers):
        w = flowvis.FlowWriter(dev, workers=workers, slots=8, fmt=fmt, quality=Q)
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(args.frames):
                w.submit(maps[f % 4], os.path.join(tmp, '%04d.%s' % (f, fmt)))
            t_submit = time.perf_counter() - t0
            w.close()
            dt = time.perf_counter() - t0
        assert w.written == args.frames
        return dict(frames_per_s=round(args.frames / dt, 1), submit_s=round(t_submit, 4), total_s=round(dt, 4), MB_written=round(w.bytes_written / 1e6, 2))

    def run_host(fmt, workers):
        from concurrent.futures import ThreadPoolExecutor

        def job(flow, name):
            if fmt == 'flo':
                with open(name, 'wb') as fh:
                    fh.write(flowvis._flo_header(H, W))
                    flow.tofile(fh)
            else:
                Image.fromarray(F.colour(flow)).save(name, format='JPEG', quality=Q, subsampling=2, optimize=False)
            return os.path.getsize(name)
        with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(workers) as pool:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            futs = []
            for f in range(args.frames):
                m = maps[f % 4]                                      # the download the host path needs: the two flow channels, 16.8 MB
                flow = m.t[0, :, :, m.coff:m.coff + 2].contiguous().cpu().numpy()
                futs.append(pool.submit(job, flow, os.path.join(tmp, '%04d.%s' % (f, fmt))))
            t_submit = time.perf_counter() - t0
            nbytes = sum(x.result() for x in futs)
            dt = time.perf_counter() - t0
        return dict(frames_per_s=round(args.frames / dt, 1), submit_s=round(t_submit, 4), total_s=round(dt, 4), MB_written=round(nbytes / 1e6, 2))

    def repeated(fn, fmt, workers):
        """`args.repeats` windows of `args.frames` frames: the median window, with the spread of the rate over the windows"""
        runs = sorted((fn(fmt, workers) for _ in range(args.repeats)), key=lambda r: r['frames_per_s'])
        return dict(runs[len(runs) // 2], frames_per_s_min=runs[0]['frames_per_s'], frames_per_s_max=runs[-1]['frames_per_s'], windows=len(runs))

    rep['repeats'] = args.repeats
    for fmt in ('jpg', 'flo'):
        run_device(fmt, 2)                                           # warm-up: ring slots, pinned staging, copy streams
        rep['device_writer_' + fmt] = {str(n): repeated(run_device, fmt, n) for n in (1, 2, 4)}
        rep['host_numpy_' + fmt] = {str(n): repeated(run_host, fmt, n) for n in (1, 2, 4)}
        rep['verdict_' + fmt] = {str(n): ('device path %s: %.1f vs %.1f frames/s' % (
            'wins' if rep['device_writer_' + fmt][str(n)]['frames_per_s'] > rep['host_numpy_' + fmt][str(n)]['frames_per_s'] else 'LOSES',
            rep['device_writer_' + fmt][str(n)]['frames_per_s'], rep['host_numpy_' + fmt][str(n)]['frames_per_s'])) for n in (1, 2, 4)}
    rep['not_measured'] = "the 'png' format; a clip of the detector with keep_flow and --flow against the same clip without them"
    return rep


def tubes_leg(args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import rle_restate as R
    from vps_amd import hip, tubes
    assert torch.cuda.is_available(), 'vps_rle_runs needs the MI355X'
    dev = torch.device('cuda:0')
    H, W, LAST_STUFF = args.height, args.width, 10
    twos = [label_map(H, W, s) for s in range(4)]
    maps = [torch.from_numpy(t).to(dev) for t in twos]
    try:
        import pycocotools.mask as cm
    except ImportError:
        cm = None
    rep = dict(mode='tubes_output', size=[H, W], frames=args.frames, repeats=args.repeats, host_cpus=os.cpu_count(), csrc_sha16=hip.csrc_sha16(),
               host_encoder='pycocotools' if cm is not None else 'NumPy restatement (tests/rle_restate.py)')
    lib = hip.load()
    cap = H * W // 8
    rs = torch.empty(cap, dtype=torch.int32, device=dev)
    rk = torch.empty(cap, dtype=torch.int16, device=dev)
    nr = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(tubes.rle_runs_ws(H, W), dtype=torch.uint8, device=dev)

    def launch(i):
        hip.check(lib.vps_rle_runs(hip.ptr(maps[i % 4]), H, W, 2, hip.ptr(rs), hip.ptr(rk), cap, hip.ptr(nr), hip.ptr(ws), ws.numel(), hip.stream_ptr()),
                  'vps_rle_runs')
    for i in range(3):
        launch(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(30):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        launch(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    launch(1)
    n = int(nr.item())
    alg = 2 * (H * W * 2) + 2 * ws.numel() + n * 6                   # two sweeps over two channels, the cells written and scanned, the list
    rep['rle_runs'] = dict(device_ms_median_of_30=round(float(np.median(ms)), 4), device_ms_min=round(float(min(ms)), 4), launches=3, runs=n,
                           downloaded_bytes=n * 6, map_bytes=H * W * 3, algorithmic_MB=round(alg / 1e6, 2),
                           inputs='cache-resident: four 6.3 MB maps cycled', timed_with='events around the three launches of one call')
    start, key = tubes.runs_to_host(rs[:n], rk[:n])
    want_start, want_key = R.runs_of(R.key_map(twos[1], 2))
    assert np.array_equal(start, want_start) and np.array_equal(key, want_key), 'the run list is not the restatement\'s'
    keys = tubes.default_keys(key)
    keys = keys[(keys >> 8) > LAST_STUFF]
    hs = []
    for _ in range(33):
        t0 = time.perf_counter()
        strings = tubes.rle_strings(start, key, H * W, keys)
        hs.append((time.perf_counter() - t0) * 1e3)
    km = R.key_map(twos[1], 2)
    assert all(s == R.encode(km == k)['counts'].encode('ascii') for k, s in zip(keys[:5], strings)), 'the strings are not the restatement\'s'
    rep['rle_strings'] = dict(host_ms_median_of_30=round(float(np.median(hs[3:])), 4), host_ms_min=round(float(min(hs[3:])), 4), threads=1, keys=int(keys.size),
                              string_bytes=int(sum(len(s) for s in strings)))
    rep['equal_to_numpy_restatement'] = True

    def run_device(workers):
        col = tubes.TubeCollector(things_only=True, id_last_stuff=LAST_STUFF, workers=workers, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(args.frames):
            col.add(0, '%04d.png' % f, maps[f % 4])
        t_add = time.perf_counter() - t0
        res = col.result()
        dt = time.perf_counter() - t0
        col.close()
        return dict(frames_per_s=round(args.frames / dt, 1), add_s=round(t_add, 4), total_s=round(dt, 4), tracks=len(res['videos'][0]['tracks']))

    def host_frame(two):
        km = two[..., 0].astype(np.int32) * 256 + two[..., 2]
        out = {}
        for k in np.unique(km):
            if (k >> 8) == 255 or (k >> 8) <= LAST_STUFF:
                continue
            mask = km == k
            if cm is not None:
                out[int(k)] = cm.encode(np.asfortranarray(mask.astype(np.uint8)))
            else:
                out[int(k)] = R.encode(mask)
        return len(out)

    def run_host(workers):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(workers) as pool:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            futs = [pool.submit(host_frame, maps[f % 4].cpu().numpy()) for f in range(args.frames)]     # the 6.3 MB download the host way needs
            t_add = time.perf_counter() - t0
            ntr = [x.result() for x in futs]
            dt = time.perf_counter() - t0
        return dict(frames_per_s=round(args.frames / dt, 1), add_s=round(t_add, 4), total_s=round(dt, 4), masks_per_frame=ntr[0])

    def repeated(fn, workers):
        runs = sorted((fn(workers) for _ in range(args.repeats)), key=lambda r: r['frames_per_s'])
        return dict(runs[len(runs) // 2], frames_per_s_min=runs[0]['frames_per_s'], frames_per_s_max=runs[-1]['frames_per_s'], windows=len(runs))

    run_device(2)                                                    # warm-up: the statistics table, the allocator's blocks
    rep['tube_collector'] = {str(w): repeated(run_device, w) for w in (1, 2, 4)}
    rep['host_numpy'] = {str(w): repeated(run_host, w) for w in (1, 2, 4)}
    rep['verdict'] = {str(w): ('device path %s: %.1f vs %.1f frames/s' % (
        'wins' if rep['tube_collector'][str(w)]['frames_per_s'] > rep['host_numpy'][str(w)]['frames_per_s'] else 'LOSES',
        rep['tube_collector'][str(w)]['frames_per_s'], rep['host_numpy'][str(w)]['frames_per_s'])) for w in (1, 2, 4)}
    rep['not_measured'] = 'kernel times from a profiler trace; maps that are not cache-resident; a detector clip with --tubes against the same clip without'
    return rep


def y4m_leg(args):
    """`--leg y4m`: the Y4M output path at 420jpeg. `vps_bgr_to_yuv` by events, and `Y4mWriter` to a file on local disk and to a sink that
    discards against `DeviceJpegWriter(entropy='device')` writing files, same process, alternating windows. The 'output' key of --out."""
    import torch
    from bench_input_pipeline import time_kernel
    from vps_amd import hip, synth, y4m
    from vps_amd import postprocess as pp
    assert torch.cuda.is_available(), 'the conversion runs on the device'
    dev = torch.device('cuda:0')
    H, W = args.height, args.width
    frames = [synth.synth_frame(H, W, seed=s, shift=(2 * s, s), noise=2.0).astype(np.uint8) for s in range(4)]       # BGR
    frames = [np.pad(f, ((0, H - f.shape[0]), (0, W - f.shape[1]), (0, 0)), mode='edge') for f in frames]
    imgs = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    nb = y4m.planar_bytes(H, W, '420jpeg')
    rep = dict(mode='y4m-output', size=[H, W], sampling='420jpeg', range='limited', matrix='bt601', frames_per_window=args.frames, windows=args.repeats,
               host_cpus=os.cpu_count(), csrc_sha16=hip.csrc_sha16(), y4m_MB_per_frame=round((nb + 6) / 1e6, 2))
    moved = nb + 3 * H * W
    npool = int(2 * (256 << 20) // moved) + 2
    src = imgs + [imgs[k % 4].clone() for k in range(4, npool)]
    dst = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(npool)]
    res = time_kernel(lambda i: y4m.bgr_to_yuv(src[i], '420jpeg', 'limited', 'bt601', dst[i]), 4)
    rep['vps_bgr_to_yuv_cache_resident'] = dict(res, inputs_cycled=4, working_set_MB=round(4 * moved / 1e6, 1), GBps_at_median=round(moved / res['ms_median'] / 1e6, 1))
    res = time_kernel(lambda i: y4m.bgr_to_yuv(src[i], '420jpeg', 'limited', 'bt601', dst[i]), npool)
    rep['vps_bgr_to_yuv_beyond_cache'] = dict(res, inputs_cycled=npool, working_set_MB=round(npool * moved / 1e6, 1), GBps_at_median=round(moved / res['ms_median'] / 1e6, 1))
    rep['kernel_bytes_moved'] = moved
    del src, dst

    class Discard:
        def write(self, b):
            return len(b)

        def flush(self):
            pass

    def window(kind):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind.startswith('jpeg'):
                w = pp.DeviceJpegWriter(dev, workers=int(kind[4:]), slots=8, quality=90, entropy='device')
                for f in range(args.frames):
                    w.submit(imgs[f % 4], os.path.join(tmp, '%04d.jpg' % f))
                w.close()
                assert w.device_encoded == args.frames
                mb = w.bytes_written / 1e6
            else:
                w = y4m.Y4mWriter(os.path.join(tmp, 'out.y4m') if kind == 'y4m_file' else Discard(), W, H, sampling='420jpeg', device=dev, slots=4)
                for f in range(args.frames):
                    w.submit(imgs[f % 4])
                w.close()
                assert w.frames == args.frames
                mb = w.bytes / 1e6
            dt = time.perf_counter() - t0
        return args.frames / dt, mb

    kinds = ('y4m_file', 'y4m_discard', 'jpeg1', 'jpeg4')
    rates = {k: [] for k in kinds}
    for k in kinds:                                                  # warm-up: ring slots, pinned staging, copy streams
        window(k)
    for _ in range(args.repeats):                                    # the writers alternate, so a busy host hits all of them
        for k in kinds:
            rates[k].append(window(k))
    names = dict(y4m_file='Y4mWriter to a file on local disk', y4m_discard='Y4mWriter to a sink that discards',
                 jpeg1="DeviceJpegWriter(entropy='device', workers=1) to files", jpeg4="DeviceJpegWriter(entropy='device', workers=4) to files")
    rep['writer_frames_per_s'] = {k: dict(what=names[k], median=round(float(np.median([r[0] for r in rates[k]])), 1), min=round(min(r[0] for r in rates[k]), 1),
                                          max=round(max(r[0] for r in rates[k]), 1), MB_written_per_window=round(rates[k][0][1], 1)) for k in kinds}
    rep['writer_note'] = ('the clock runs from the first submit to the end of close(), file creation included; the JPEG frames are the RGB reading of the same '
                          'arrays (the byte order does not change the work); the file goes to the temporary directory of the host, through its page cache')
    rep['not_measured'] = 'a pipe to an encoder or a player; 444 and 420mpeg2; a detector clip with --overlay-video against the same clip without it'
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', default='png', choices=['png', 'overlay', 'overlay_entropy', 'flow', 'tubes', 'y4m'])
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3, help='--leg flow / tubes / overlay_entropy: windows of --frames frames per writer figure (median and spread are reported)')
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--out', default=None, help='default: profiles/<png|overlay|flow|tubes>_output_pipeline.json by --leg')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', {'png': 'png_output_pipeline.json', 'overlay': 'overlay_output_pipeline.json',
                                                   'overlay_entropy': 'overlay_output_pipeline.json', 'flow': 'flow_output_pipeline.json',
                                                   'tubes': 'tubes_output_pipeline.json'}[args.leg])
    if args.leg == 'y4m':                                            # the 'output' key of profiles/y4m_pipeline.json; 'input' is bench_input_pipeline.py --y4m
        from bench_input_pipeline import merge_y4m_profile
        rep = y4m_leg(args)
        merge_y4m_profile(args.out or os.path.join(ROOT, 'profiles', 'y4m_pipeline.json'), 'output', rep)
        print(json.dumps(rep))
        return
    if args.leg == 'overlay_entropy':                                # a new key in the overlay report; the other keys stay as they are
        rep = overlay_entropy_leg(args)
        print(json.dumps(rep))
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old['device_entropy'] = rep
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(old) + '\n')
        return
    if args.leg in ('overlay', 'flow', 'tubes'):
        line = json.dumps({'overlay': overlay_leg, 'flow': flow_leg, 'tubes': tubes_leg}[args.leg](args))
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(line + '\n')
        return
    import torch
    from vps_amd import hip
    from vps_amd import postprocess as pp
    assert torch.cuda.is_available(), 'the device encoder needs the MI355X'
    dev = torch.device('cuda:0')
    H, W = args.height, args.width
    twos = [label_map(H, W, s) for s in range(4)]                    # a few distinct frames, cycled
    preds = [painted(t, s) for s, t in enumerate(twos)]
    d_twos = [torch.from_numpy(a).to(dev) for a in twos]
    d_preds = [torch.from_numpy(a).to(dev) for a in preds]
    rep = dict(mode='png_output', size=[H, W], frames=args.frames, host_cpus=os.cpu_count(), csrc_sha16=hip.csrc_sha16())

    # ---- the kernels alone ----
    cap, wsb = pp.png_encode_bound(H, W, 3)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    size = torch.empty(1, dtype=torch.int64, device=dev)
    for kind, maps, hosts in (('pan_2ch', d_twos, twos), ('pan_pred', d_preds, preds)):
        for _ in range(3):
            pp.png_deflate(maps[0], out, ws, size)
        torch.cuda.synchronize()
        ms = []
        for i in range(30):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            pp.png_deflate(maps[i % len(maps)], out, ws, size)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        n = int(size.item())
        data = pp.png_container(out[:n].cpu().numpy().tobytes(), H, W, 3)
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), hosts[29 % len(maps)])
        med = float(np.median(ms))
        alg = 2 * H * W * 3 + n
        rep[kind] = dict(device_ms_median_of_30=round(med, 4), device_ms_min=round(min(ms), 4), algorithmic_MB=round(alg / 1e6, 2),
                         fraction_of_8TBps=round(alg / (med * 1e-3) / 8e12, 4), device_file_bytes=len(data), pil_file_bytes=pil_size(hosts[29 % len(maps)]),
                         raw_over_device_file=round(H * W * 3 / len(data), 1))
        rep[kind]['device_over_pil_size'] = round(rep[kind]['device_file_bytes'] / rep[kind]['pil_file_bytes'], 2)

    # ---- the writers: every frame writes its two maps ----
    def run(writer, device_inputs):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(args.frames):
                a, b = d_twos[f % 4], d_preds[f % 4]
                if not device_inputs:                                # what inference_panoptic_video does for a host writer
                    a, b = a.cpu().numpy(), b.cpu().numpy()
                writer.submit(a, os.path.join(tmp, 'pan_2ch', '%04d.png' % f))
                writer.submit(b, os.path.join(tmp, 'pan_pred', '%04d.png' % f))
            t_submit = time.perf_counter() - t0
            writer.close()
            dt = time.perf_counter() - t0
            nbytes = sum(os.path.getsize(os.path.join(tmp, d, x)) for d in ('pan_2ch', 'pan_pred') for x in os.listdir(os.path.join(tmp, d)))
        return dict(frames_per_s=round(args.frames / dt, 1), submit_s=round(t_submit, 4), total_s=round(dt, 4), MB_written=round(nbytes / 1e6, 2))

    run(pp.DevicePngWriter(dev, workers=2), True)                    # warm-up: ring slots, pinned staging, copy streams
    w = pp.DevicePngWriter(dev, workers=2)
    rep['device_writer_2_workers'] = run(w, True)
    assert (w.device_encoded, w.fallback_encoded) == (2 * args.frames, 0)
    rep['pil_writer'] = {str(n): run(pp.AsyncPngWriter(workers=n), False) for n in (1, 2, 4)}
    d, p4 = rep['device_writer_2_workers']['frames_per_s'], rep['pil_writer']['4']['frames_per_s']
    rep['expectation'] = 'device writer at 2 workers out-runs the PIL writer at 4: %s (%.1f vs %.1f frames/s)' % ('holds' if d > p4 else 'REFUTED', d, p4)
    rep['not_measured'] = 'a 30-frame clip of the detector written every frame with --device-png against the same clip without output'
    line = json.dumps(rep)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
