"""SURVEY 8(f) row 1, measured end to end (VERDICT r2 "Missing" #6 / next-round #10): can the input side feed the detector?

    python tools/bench_input_pipeline.py [--frames 48] [--workers 1 2 4 8 16]

Writes `--frames` synthetic 1024x2048 8-bit PNG frames (Cityscapes-VPS size) to a temporary directory, then times
  decode   `vps_amd.pipeline.imread` (mmcv.imread semantics; PIL or cv2) with N host worker threads, frames/s
  upload   the decoded uint8 HWC frame -> device (6 MB, pinned and pageable)
  prep     `DeviceImagePrep.prep` (Normalize + Pad + ImageToTensor as one kernel)
and the three chained with a prefetching thread pool (decode of frame t+k overlaps upload + prep of frame t), which is what a
data loader in front of `tools/test_vpq.py` would do. The detector runs at ~42 frames/s on one MI355X: the question is how many
host threads the decode needs to keep up. Prints one JSON line. The GPU part is skipped without a GPU.

    python tools/bench_input_pipeline.py --node 8 --threads 6 [--seconds 8]

    python tools/bench_input_pipeline.py --format jpeg [--height 1080 --width 1920] [--workers 1 2 4 8] [--out FILE]

JPEG mode (the VIPER frames, 1080x1920 by default): the same run times both decode legs at each worker count - `native`, what a
`ClipFeeder` worker does for a .jpg (`vps_jpeg_decode_coef` into a reused staging buffer; the pixels are rebuilt on the device), and
`imread`, the route such a file took before (PIL: full decode + RGB->BGR copy). With a GPU it adds `vps_jpeg_reconstruct` timed by
events (median of 30 launches) beside its 12.5 MB of algorithmic traffic at 8 TB/s, and a `ClipFeeder` drained by an otherwise idle
consumer. The gain of the native path is host CPU time and pinned pixel semantics; the device stage is microseconds off the model's
critical path.

    python tools/bench_input_pipeline.py --png-device [--frames 16] [--workers 1 2 4 8 16] [--out FILE]

PNG-DEVICE mode (`ClipFeeder(png='device')`: the worker only inflates, the device un-filters): on the same PIL-written 1024x2048 RGB
frames it times, per worker count and alternating in one run, the two host legs of a feeder worker - `decode` (`vps_png_decode_bgr8`:
inflate + un-filter + BGR copy into a reused staging buffer) and `inflate` (`vps_png_inflate` alone) - and reports their single-thread
ms per frame (the difference is what the host stops paying), the filter-type histogram and the longest row group of the files, with a
GPU `vps_png_reconstruct` by events (median of 30 launches on an idle device), and a `ClipFeeder` drained by an otherwise idle consumer
with png='host' and png='device' at equal thread counts (`--feeder-frames` frames timed in steady state). `--clip` adds the PNG-fed
detector clip of `bench.py --full` (its `from_png` extra) with png='host' against png='device', alternating. `--parent-lib FILE`: a shared library built from another commit's
csrc/png_host.cpp, whose `vps_png_decode_bgr8` is timed beside this tree's.

NODE mode (round 6): what the host of an 8-GPU node has to deliver - `--node` decoder PROCESSES (one per rank, as
`bench.py --gpus 8` starts them), each with the thread budget of a rank's `ClipFeeder` (`--threads`, default 6) and pinned to its own
block of cores (os.sched_setaffinity: cores [r * C/8, (r+1) * C/8) - a rank's decode threads stay on the cores next to its GPU and
never compete with another rank's), all decoding 1024x2048 PNG frames with the library's native decoder (`vps_png_decode_bgr8`,
what ClipFeeder uses) for `--seconds`. Reports per-rank and aggregate frames/s; the node needs 8 x (frames/s of one GPU).
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rank_decode(rank, nranks, threads, files, seconds, q):
    # one rank's input side: `threads` decoder threads on this rank's own block of cores
    ncpu = os.cpu_count() or 1
    per = max(ncpu // nranks, 1)
    cores = list(range(rank * per, min((rank + 1) * per, ncpu)))
    pinned = False
    try:
        os.sched_setaffinity(0, cores)
        pinned = True
    except (AttributeError, OSError):
        pass
    import ctypes
    from vps_amd import hip
    lib = hip.load_host()
    # the files sit in the page cache; decode is what is measured - into per-thread staging buffers allocated once, like ClipFeeder's
    # pinned ring slots (a fresh 6 MB numpy array per frame is an mmap + page faults per decode: the process' threads then queue on the mm lock)
    datas = [bytearray(open(f, 'rb').read()) for f in files]
    cbufs = [(ctypes.c_char * len(d)).from_buffer(d) for d in datas]
    H, W, C = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.vps_png_info(cbufs[0], len(datas[0]), ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)) == 0
    stages = [np.empty(H.value * W.value * 3, dtype=np.uint8) for _ in range(threads)]
    n = [0] * threads
    stop = time.perf_counter() + seconds

    def work(i):
        k = i
        out = stages[i].ctypes.data_as(ctypes.c_void_p)
        while time.perf_counter() < stop:
            j = k % len(datas)
            hip.check(lib.vps_png_decode_bgr8(cbufs[j], len(datas[j]), out, stages[i].nbytes), 'vps_png_decode_bgr8')
            n[i] += 1
            k += threads
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    q.put((rank, sum(n) / (time.perf_counter() - t0), len(cores), pinned))


def node_mode(args):
    import multiprocessing as mp
    from PIL import Image
    from vps_amd import synth
    H, W = args.height, args.width
    tmp = tempfile.mkdtemp(prefix='vps_input_')
    files = []
    for t in range(8):
        fr = synth.synth_frame(H, W, seed=t % 4, shift=(2 * (t % 8), t % 8), noise=2.0).astype(np.uint8)
        fn = os.path.join(tmp, 'f%04d_leftImg8bit.png' % t)
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, compress_level=6)
        files.append(fn)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_decode, args=(r, args.node, args.threads, files, args.seconds, q)) for r in range(args.node)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=args.seconds * 4 + 120) for _ in procs)
    for p in procs:
        p.join()
    for f in files:
        os.remove(f)
    os.rmdir(tmp)
    per_rank = [round(r[1], 1) for r in res]
    out = dict(mode='node', ranks=args.node, threads_per_rank=args.threads, host_cpus=os.cpu_count(), cores_per_rank=res[0][2], pinned=all(r[3] for r in res),
               size=[H, W], png_MB_per_frame=round(sum(os.path.getsize(f) for f in files if os.path.exists(f)) / 1e6 / 8, 2) if False else None,
               decode_frames_per_s_per_rank=per_rank, aggregate_frames_per_s=round(sum(per_rank), 1), slowest_rank_frames_per_s=min(per_rank),
               needed_per_rank=args.need, headroom_of_the_slowest_rank=round(min(per_rank) / args.need, 2), seconds=args.seconds,
               decoder='vps_png_decode_bgr8 (libvpship host code, zlib inflate + unfilter + BGR), the decoder of vps_amd.pipeline.ClipFeeder')
    out.pop('png_MB_per_frame')
    print(json.dumps(out))


def jpeg_mode(args):
    import ctypes
    import threading
    import warnings
    import torch
    from PIL import Image
    from vps_amd import hip, synth
    from vps_amd.pipeline import JPEG_QT_BYTES, ClipFeeder, DeviceImagePrep, imread, jpeg_info, jpeg_reconstruct
    H, W = args.height, args.width
    tmp = tempfile.mkdtemp(prefix='vps_input_')
    files = []
    for t in range(args.frames):
        fr = synth.synth_frame(H, W, seed=t % 4, shift=(2 * (t % 8), t % 8), noise=2.0).astype(np.uint8)
        fn = os.path.join(tmp, 'f%04d.jpg' % t)
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, quality=90, subsampling=2)
        files.append(fn)
    lib = hip.load_host()
    ji = jpeg_info(bytearray(open(files[0], 'rb').read()))
    assert ji is not None
    out = dict(mode='jpeg', frames=args.frames, size=[H, W], jpeg_MB_per_frame=round(sum(os.path.getsize(f) for f in files) / 1e6 / len(files), 3),
               coef_MB_per_frame=round(ji.coef_bytes / 1e6, 2), host_cpus=os.cpu_count(), native_frames_per_s={}, imread_frames_per_s={},
               legs='native = file read + vps_jpeg_decode_coef into a reused staging buffer (a ClipFeeder worker); imread = file read + PIL decode '
                    '+ BGR copy (the route of a .jpg before the native path)')
    local = threading.local()

    def native(fn):
        if not hasattr(local, 'stage'):
            local.stage = np.empty(ji.coef_bytes + JPEG_QT_BYTES, dtype=np.uint8)
        data = bytearray(open(fn, 'rb').read())
        cbuf = (ctypes.c_char * len(data)).from_buffer(data)
        hip.check(lib.vps_jpeg_decode_coef(cbuf, len(data), local.stage.ctypes.data_as(ctypes.c_void_p), ji.coef_bytes), 'vps_jpeg_decode_coef')

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for nw in args.workers:
            for name, fn in (('native_frames_per_s', native), ('imread_frames_per_s', imread)):
                with ThreadPoolExecutor(nw) as ex:
                    list(ex.map(fn, files[:nw]))                   # warm-up
                    t0 = time.perf_counter()
                    list(ex.map(fn, files))
                    out[name][str(nw)] = round(len(files) / (time.perf_counter() - t0), 1)
        if torch.cuda.is_available():
            dev = torch.device('cuda:0')
            data = bytearray(open(files[0], 'rb').read())
            host = torch.empty(ji.coef_bytes + JPEG_QT_BYTES, dtype=torch.uint8).pin_memory()
            hip.check(lib.vps_jpeg_decode_coef((ctypes.c_char * len(data)).from_buffer(data), len(data), ctypes.c_void_p(host.data_ptr()), ji.coef_bytes),
                      'vps_jpeg_decode_coef')
            host[ji.coef_bytes:].copy_(torch.from_numpy(ji.qt.view(np.uint8).reshape(-1)))
            buf = host.to(dev)
            ws = torch.empty(ji.coef_bytes // 2, dtype=torch.uint8, device=dev)
            for _ in range(5):
                jpeg_reconstruct(buf, ji, ws)
            torch.cuda.synchronize()
            ms = []
            for _ in range(30):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); jpeg_reconstruct(buf, ji, ws); e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            traffic = ji.coef_bytes + H * W * 3
            out['reconstruct_ms_median_of_30'] = round(med, 4)
            out['reconstruct_algorithmic_MB'] = round(traffic / 1e6, 2)
            out['reconstruct_fraction_of_8TBps'] = round(traffic / 8e12 / (med * 1e-3), 4)
            prep = DeviceImagePrep(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32,
                                   img_scale=(max(H, W), min(H, W)), device=dev)
            out['feeder_frames_per_s'] = {}
            for nw in args.workers:
                fd = ClipFeeder(files, prep, workers=nw)
                fd(0); torch.cuda.synchronize()                    # ring allocation + first decode outside the timing
                t0 = time.perf_counter()
                for t in range(1, len(files)):
                    fd(t)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                fd.close()
                assert fd.native_jpeg == len(files) and fd.fallback_decodes == 0
                out['feeder_frames_per_s'][str(nw)] = dict(frames_per_s=round((len(files) - 1) / dt, 1),
                                                           wait_for_decode_s=round(fd.stats['wait_for_decode_s'], 4),
                                                           upload_prep_s=round(fd.stats['upload_prep_s'], 4))
            out['feeder_note'] = 'consumer = fd(t) in a loop on an otherwise idle main thread (no detector beside it)'
    for f in files:
        os.remove(f)
    os.rmdir(tmp)
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


def detector_clip(args, files, dev):
    """the PNG-fed clip of `bench.py --full` (its `from_png` extra: ClipShardRunner.run(ClipFeeder(...)) over 32 frames of 8 PIL-written files,
    --png-workers decode threads, the pool given 0.2 s to fill its window) with png='host' - the parent commit's path, byte for byte - against
    png='device', alternating in one process; the README states a box-to-box spread of +-1.5 % for the clip rate"""
    import torch
    import vps_amd
    from vps_amd import nhwc, synth
    from vps_amd.clip_shard import ClipShardRunner, DetectorBackend
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[args.prec]
    H, W = args.height, args.width
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    model = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synth.load_synth(model, 0)
    runner = ClipShardRunner(DetectorBackend(model, H, W, prefetch=True), 0, 1, None, dev)

    def reset():
        model._cache = None; model._handoff = None; model._pf = None
        model.reset_tracker()
    prep = DeviceImagePrep(**cfg.img_norm_cfg, size_divisor=32, img_scale=(max(H, W), min(H, W)), device=dev)
    names, nfr = files[:8], 32
    rates = {'host': [], 'device': []}
    vid = 20
    for mode in ('host', 'device'):                                          # warm-up of both paths
        reset()
        runner.run(ClipFeeder([names[t % 8] for t in range(8)], prep, workers=args.png_workers, png=mode), 8, video_id=vid); vid += 1
    for rnd in range(args.clip_rounds):
        for mode in ('host', 'device'):
            reset()
            feeder = ClipFeeder([names[t % 8] for t in range(nfr)], prep, workers=args.png_workers, png=mode).start()
            time.sleep(0.2)
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            runner.run(feeder, nfr, video_id=vid); vid += 1
            torch.cuda.synchronize()
            rates[mode].append(round(nfr / (time.perf_counter() - c0), 3))
            feeder.close()
            assert feeder.fallback_decodes == 0 and feeder.native_png_device == (nfr if mode == 'device' else 0)
    reset()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    ratio = med['device'] / med['host']
    return dict(frames=nfr, decode_threads=args.png_workers, prec=args.prec, rounds_alternating=args.clip_rounds, frames_per_s=rates,
                median_frames_per_s={k: round(v, 3) for k, v in med.items()}, device_over_host=round(ratio, 4),
                yardstick="png=host is the parent commit's path (same decoder code, same bytes); stated box-to-box spread of the clip rate: +-1.5 %",
                finding=('png=device is within the +-1.5 % spread of png=host' if abs(ratio - 1) <= 0.015 else
                         'png=device is %.1f %% %s than png=host, beyond the +-1.5 %% spread: the reconstruct kernel %s' % (
                             100 * abs(ratio - 1), 'slower' if ratio < 1 else 'faster',
                             "disturbs the frame (it runs in order on the consumer's stream)" if ratio < 1 else 'does not hold the frame back')))


def png_device_mode(args):
    import ctypes
    import threading
    import torch
    from PIL import Image
    from vps_amd import hip, synth
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep, png_inflate, png_reconstruct
    H, W = args.height, args.width
    tmp = tempfile.mkdtemp(prefix='vps_input_')
    files = []
    for t in range(args.frames):
        fr = synth.synth_frame(H, W, seed=t % 4, shift=(2 * (t % 8), t % 8), noise=2.0).astype(np.uint8)
        fn = os.path.join(tmp, 'f%04d_leftImg8bit.png' % t)
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, compress_level=6)
        files.append(fn)
    lib = hip.load_host()
    datas = [bytearray(open(f, 'rb').read()) for f in files]                 # the files sit in memory: the decoders are what is timed
    cbufs = [(ctypes.c_char * len(d)).from_buffer(d) for d in datas]
    scan0, pi = png_inflate(datas[0])
    hist, longest = [0] * 5, 0
    for d in datas[:8]:
        types = png_inflate(d)[0].reshape(pi.H, 1 + pi.W * pi.C)[:, 0]
        for k in range(5):
            hist[k] += int((types == k).sum())
        starts = np.flatnonzero((types < 2) | (np.arange(pi.H) == 0))
        longest = max(longest, int(np.diff(np.append(starts, pi.H)).max()))
    out = dict(mode='png-device', frames=args.frames, size=[H, W], channels=pi.C, png_MB_per_frame=round(sum(len(d) for d in datas) / 1e6 / len(datas), 2),
               scan_MB_per_frame=round(pi.scan_bytes / 1e6, 2), host_cpus=os.cpu_count(),
               filter_type_rows_of_8_files=dict(zip(('none', 'sub', 'up', 'average', 'paeth'), hist)), longest_row_group_of_8_files=longest,
               legs='decode = vps_png_decode_bgr8 (inflate + un-filter + BGR copy), inflate = vps_png_inflate; both from memory into a reused '
                    'per-thread staging buffer, as a ClipFeeder worker calls them')
    legs = [('decode', lib.vps_png_decode_bgr8, H * W * 3), ('inflate', lib.vps_png_inflate, pi.scan_bytes)]
    if args.parent_lib:
        par = ctypes.CDLL(args.parent_lib)
        par.vps_png_decode_bgr8.restype = ctypes.c_int
        par.vps_png_decode_bgr8.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
        legs.insert(0, ('parent_decode', par.vps_png_decode_bgr8, H * W * 3))
    local = threading.local()

    def leg(fn, nbytes):
        def work(i):
            if getattr(local, 'n', 0) < nbytes:
                local.stage, local.n = np.empty(nbytes, dtype=np.uint8), nbytes
            hip.check(fn(cbufs[i], len(datas[i]), local.stage.ctypes.data_as(ctypes.c_void_p), nbytes), 'png host leg')
        return work
    idx = list(range(len(datas)))
    for name, _, _ in legs:
        out[name + '_frames_per_s'] = {}
    for nw in args.workers:
        for rnd in range(2):                                                  # alternating; the second round is kept
            for name, fn, nbytes in legs:
                with ThreadPoolExecutor(nw) as ex:
                    list(ex.map(leg(fn, nbytes), idx[:nw]))                   # warm-up: the threads' buffers
                    t0 = time.perf_counter()
                    list(ex.map(leg(fn, nbytes), idx))
                    out[name + '_frames_per_s'][str(nw)] = round(len(idx) / (time.perf_counter() - t0), 1)
    ms = {}
    for rnd in range(3):                                                      # one thread, alternating, best of 3 passes over the files
        for name, fn, nbytes in legs:
            w = leg(fn, nbytes)
            t0 = time.perf_counter()
            for i in idx:
                w(i)
            ms[name] = min(ms.get(name, 1e9), 1e3 * (time.perf_counter() - t0) / len(idx))
    out['one_thread_ms_per_frame'] = {k: round(v, 3) for k, v in ms.items()}
    out['one_thread_unfilter_and_bgr_ms_per_frame'] = round(ms['decode'] - ms['inflate'], 3)
    out['one_thread_unfilter_share_of_decode'] = round((ms['decode'] - ms['inflate']) / ms['decode'], 3)
    if torch.cuda.is_available():
        dev = torch.device('cuda:0')
        scan = torch.from_numpy(scan0).to(dev)
        need = ctypes.c_int64()
        hip.check(hip.load().vps_png_reconstruct_ws(pi.H, pi.W, pi.C, ctypes.byref(need)), 'vps_png_reconstruct_ws')
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        for _ in range(5):
            png_reconstruct(scan, pi.H, pi.W, pi.C, ws)
        torch.cuda.synchronize()
        t = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); png_reconstruct(scan, pi.H, pi.W, pi.C, ws); e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        out['reconstruct_ms_median_of_30'] = round(float(np.median(t)), 4)
        out['reconstruct_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
        out['reconstruct_block_rows'] = hip.png_block_rows()
        prep = DeviceImagePrep(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32,
                               img_scale=(max(H, W), min(H, W)), device=dev)
        out['feeder_frames_per_s'] = {}
        for nw in args.workers:
            # steady state only: the read-ahead window is 2 x workers frames, so the clock starts after the first window + 1 frames have
            # been consumed (the pool refills behind the consumer from then on) and stops `timed` frames later, with a full window of
            # the clip still ahead - the window is as far ahead at the stop as at the start, and no frame decoded before the start counts
            warm, timed = 2 * nw + 1, args.feeder_frames
            clip = [files[k % len(files)] for k in range(warm + timed + 2 * nw + 2)]
            res = {}
            for rnd in range(2):                                              # alternating; the second round is kept
                for mode in ('host', 'device'):
                    fd = ClipFeeder(clip, prep, workers=nw, png=mode)
                    for k in range(warm):
                        fd(k)
                    torch.cuda.synchronize()
                    w0, u0 = fd.stats['wait_for_decode_s'], fd.stats['upload_prep_s']
                    t0 = time.perf_counter()
                    for k in range(warm, warm + timed):
                        fd(k)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    n_dev = fd.native_png_device
                    fd.close()
                    assert fd.fallback_decodes == 0 and fd.out_of_window == 0 and n_dev == (warm + timed if mode == 'device' else 0)
                    res[mode] = dict(frames_per_s=round(timed / dt, 1), wait_for_decode_s=round(fd.stats['wait_for_decode_s'] - w0, 4),
                                     upload_prep_s=round(fd.stats['upload_prep_s'] - u0, 4))
            out['feeder_frames_per_s'][str(nw)] = res
        out['feeder_timed_frames'] = args.feeder_frames
        out['feeder_note'] = ('consumer = fd(t) in a loop on an otherwise idle main thread (no detector beside it); steady state: the clock starts after '
                              '2 x workers + 1 frames and stops with a full read-ahead window still to come')
        if args.clip:
            out['detector_clip'] = detector_clip(args, files, dev)
    for f in files:
        os.remove(f)
    os.rmdir(tmp)
    line = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


def merge_y4m_profile(path, key, rep):
    """profiles/y4m_pipeline.json has one key per tool ('input': this file's --y4m, 'output': bench_output_pipeline.py --leg y4m)"""
    old = json.load(open(path)) if os.path.exists(path) else {}
    old = old if set(old) <= {'input', 'output'} else {}
    old[key] = rep
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(old, f, indent=1)
        f.write('\n')


def time_kernel(fn, pool, batch=20, reps=30):
    """device ms per call: `reps` samples, each `batch` back-to-back launches between two events divided by `batch` (one launch alone
    is at the scale of the launch itself) -> median, min, max. `pool`: how many different inputs / outputs the calls cycle through."""
    import torch
    for i in range(batch):
        fn(i % pool)
    torch.cuda.synchronize()
    ms, k = [], 0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn(k % pool)
            k += 1
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    return dict(ms_median=round(float(np.median(ms)), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5), samples=reps, launches_per_sample=batch)


def y4m_mode(args):
    """--y4m: the Y4M input path at 420jpeg. `vps_yuv_to_bgr` by events, and the feeder drained by an idle consumer from a .y4m file
    against the same frames as PNG files with png='host', same process, alternating windows. Writes the 'input' key of --out."""
    import torch
    from PIL import Image
    from vps_amd import hip, synth, y4m
    from vps_amd.pipeline import ClipFeeder, DeviceImagePrep
    assert torch.cuda.is_available(), 'the conversion runs on the device'
    dev = torch.device('cuda:0')
    H, W = args.height, args.width
    workers = [w for w in args.workers if w <= 4] or [1, 2, 4]
    tmp = tempfile.mkdtemp(prefix='vps_input_')
    frames = [np.ascontiguousarray(synth.synth_frame(H, W, seed=t % 4, shift=(2 * (t % 8), t % 8), noise=2.0).astype(np.uint8)) for t in range(args.frames)]
    frames = [np.pad(f, ((0, H - f.shape[0]), (0, W - f.shape[1]), (0, 0)), mode='edge') for f in frames]
    files = []
    for t, fr in enumerate(frames):
        fn = os.path.join(tmp, 'f%04d_leftImg8bit.png' % t)
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, compress_level=6)
        files.append(fn)
    nmax = max(workers)
    total = 2 * nmax + 1 + args.feeder_frames + 2 * nmax + 2
    path = os.path.join(tmp, 'clip.y4m')
    wr = y4m.Y4mWriter(path, W, H, sampling='420jpeg', device=dev)
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    for k in range(total):                                                    # the same frames, in the order the PNG clip cycles them
        wr.submit(dframes[k % len(dframes)])
    wr.close()
    reader = y4m.Y4mReader(path)
    info = reader.info
    out = dict(mode='y4m-input', size=[H, W], sampling='420jpeg', range='limited', matrix='bt601', host_cpus=os.cpu_count(), csrc_sha16=hip.csrc_sha16(),
               y4m_MB_per_frame=round(info.frame_bytes / 1e6, 2), png_MB_per_frame=round(sum(os.path.getsize(f) for f in files) / 1e6 / len(files), 2),
               bgr_MB_per_frame=round(3 * H * W / 1e6, 2), clip_frames=len(reader),
               files='written just before they are read: both the .y4m file and the PNG files come from the page cache, not from the disk')
    # ---- the kernel: a few inputs that stay in the 256 MiB Infinity Cache, and a pool of inputs + outputs beyond it ----------------------------
    rs = np.random.RandomState(0)
    moved = info.frame_bytes + 3 * H * W
    npool = int(2 * (256 << 20) // moved) + 2
    src = [torch.from_numpy(rs.randint(0, 256, info.frame_bytes, dtype=np.uint8)).to(dev) for _ in range(4)]
    src += [src[k % 4].clone() for k in range(4, npool)]
    dst = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(npool)]
    res = time_kernel(lambda i: y4m.yuv_to_bgr(src[i], info, 'bt601', dst[i]), 4)
    out['vps_yuv_to_bgr_cache_resident'] = dict(res, inputs_cycled=4, working_set_MB=round(4 * moved / 1e6, 1), GBps_at_median=round(moved / res['ms_median'] / 1e6, 1))
    res = time_kernel(lambda i: y4m.yuv_to_bgr(src[i], info, 'bt601', dst[i]), npool)
    out['vps_yuv_to_bgr_beyond_cache'] = dict(res, inputs_cycled=npool, working_set_MB=round(npool * moved / 1e6, 1), GBps_at_median=round(moved / res['ms_median'] / 1e6, 1))
    out['kernel_bytes_moved'] = moved
    del src, dst
    # ---- the feeder ------------------------------------------------------------------------------------------------------------------------------
    prep = DeviceImagePrep(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32,
                           img_scale=(max(H, W), min(H, W)), device=dev)

    def window(mode, nw):
        # steady state, as in --png-device: the clock starts after the first read-ahead window + 1 frames and stops with a full window to come
        warm, timed = 2 * nw + 1, args.feeder_frames
        clip = [files[k % len(files)] for k in range(warm + timed + 2 * nw + 2)]
        fd = ClipFeeder(clip if mode == 'png' else reader, prep, workers=nw, png='host')
        for k in range(warm):
            fd(k)
        torch.cuda.synchronize()
        w0, u0 = fd.stats['wait_for_decode_s'], fd.stats['upload_prep_s']
        t0 = time.perf_counter()
        for k in range(warm, warm + timed):
            fd(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        fd.close()
        assert fd.fallback_decodes == 0 and fd.out_of_window == 0 and fd.native_y4m == (warm + timed if mode == 'y4m' else 0)
        return timed / dt, fd.stats['wait_for_decode_s'] - w0, fd.stats['upload_prep_s'] - u0

    runs = {(nw, m): [] for nw in workers for m in ('png', 'y4m')}
    for key in runs:                                                          # warm-up: pinned rings, the library's buffers
        window(key[1], key[0])
    for _ in range(args.repeats):                                             # the two sources alternate, so a busy host hits both
        for key in runs:
            runs[key].append(window(key[1], key[0]))
    out['feeder_frames_per_s'] = {
        str(nw): {m: dict(median=round(float(np.median([r[0] for r in runs[(nw, m)]])), 1), min=round(min(r[0] for r in runs[(nw, m)]), 1),
                          max=round(max(r[0] for r in runs[(nw, m)]), 1),
                          wait_for_decode_s_median=round(float(np.median([r[1] for r in runs[(nw, m)]])), 4),
                          upload_prep_s_median=round(float(np.median([r[2] for r in runs[(nw, m)]])), 4)) for m in ('png', 'y4m')} for nw in workers}
    out['feeder_timed_frames'], out['feeder_windows'] = args.feeder_frames, args.repeats
    out['feeder_note'] = ('consumer = fd(t) in a loop on an otherwise idle main thread (no detector beside it); steady state: the clock starts after '
                          '2 x workers + 1 frames and stops with a full read-ahead window still to come; png = ClipFeeder(png=host) on the same frames')
    y1 = out['feeder_frames_per_s'][str(min(workers))]['y4m']['median']
    p4 = out['feeder_frames_per_s'][str(max(workers))]['png']['median']
    out['expectation'] = 'one Y4M worker (%.1f frames/s) %s the %d-worker PNG rate (%.1f frames/s)' % (
        y1, 'exceeds' if y1 > p4 else 'does NOT exceed', max(workers), p4)
    out['not_measured'] = 'a detector clip fed from Y4M against the same clip from PNG; a .y4m file read from a cold disk; other samplings'
    reader.close()
    for f in files + [path]:
        os.remove(f)
    os.rmdir(tmp)
    if args.out:
        merge_y4m_profile(args.out, 'input', out)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=48)
    ap.add_argument('--workers', type=int, nargs='+', default=[1, 2, 4, 8, 16])
    ap.add_argument('--format', choices=['png', 'jpeg'], default='png', help='jpeg: native entropy decode against the PIL route, 1080x1920 frames')
    ap.add_argument('--height', type=int, default=None, help='default 1024 (png, Cityscapes-VPS) / 1080 (jpeg, VIPER)')
    ap.add_argument('--width', type=int, default=None, help='default 2048 (png) / 1920 (jpeg)')
    ap.add_argument('--out', default=None, help='jpeg / png-device mode: also write the JSON line to this file')
    ap.add_argument('--png-device', action='store_true', help="png: the host legs and the feeder with png='host' against png='device' (inflate on the "
                    "worker, un-filter on the device), and vps_png_reconstruct by events")
    ap.add_argument('--feeder-frames', type=int, default=96, help='png-device mode: frames timed per feeder run, in steady state')
    ap.add_argument('--clip', action='store_true', help="png-device mode: also the PNG-fed detector clip of bench.py --full (32 frames) with png='host' against png='device'")
    ap.add_argument('--clip-rounds', type=int, default=3)
    ap.add_argument('--png-workers', type=int, default=6, help='--clip: decode threads, as bench.py --png-workers')
    ap.add_argument('--prec', default='f16x3', choices=['f32', 'bf16x6', 'f16x3'], help='--clip: arithmetic of the detector, as bench.py --prec')
    ap.add_argument('--parent-lib', default=None, help='png-device mode: a library with another build of vps_png_decode_bgr8, timed beside this one')
    ap.add_argument('--y4m', action='store_true', help="the Y4M input path: vps_yuv_to_bgr by events, the feeder from a .y4m file against the same frames as "
                    "PNG files (png='host') at the --workers up to 4, alternating windows; --out defaults to profiles/y4m_pipeline.json (key 'input')")
    ap.add_argument('--repeats', type=int, default=3, help='--y4m: windows per feeder figure (median and spread are reported)')
    ap.add_argument('--node', type=int, default=0, help='node mode: this many rank processes decode concurrently')
    ap.add_argument('--threads', type=int, default=6, help='node mode: decode threads per rank (ClipFeeder workers)')
    ap.add_argument('--seconds', type=float, default=8.0)
    ap.add_argument('--need', type=float, default=56.0, help='node mode: frames/s one GPU consumes')
    args = ap.parse_args()
    if args.height is None:
        args.height = 1080 if args.format == 'jpeg' else 1024
    if args.width is None:
        args.width = 1920 if args.format == 'jpeg' else 2048
    if args.y4m:
        args.out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'y4m_pipeline.json')
        return y4m_mode(args)
    if args.format == 'jpeg':
        return jpeg_mode(args)
    if args.node:
        return node_mode(args)
    if args.png_device:
        return png_device_mode(args)
    import torch
    from PIL import Image
    from vps_amd import synth
    from vps_amd.pipeline import imread
    H, W = args.height, args.width
    tmp = tempfile.mkdtemp(prefix='vps_input_')
    files = []
    for t in range(args.frames):
        # low-pass noise + per-frame translation and noise: compresses like a camera frame rather than like a flat image
        fr = synth.synth_frame(H, W, seed=t % 4, shift=(2 * (t % 8), t % 8), noise=2.0).astype(np.uint8)
        fn = os.path.join(tmp, 'f%04d_leftImg8bit.png' % t)
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(fn, compress_level=6)
        files.append(fn)
    mb = sum(os.path.getsize(f) for f in files) / 1e6 / len(files)
    out = dict(frames=args.frames, size=[H, W], png_MB_per_frame=round(mb, 2), host_cpus=os.cpu_count(), decode_frames_per_s={})
    for nw in args.workers:
        with ThreadPoolExecutor(nw) as ex:
            list(ex.map(imread, files[:nw]))                       # warm-up
            t0 = time.perf_counter()
            list(ex.map(imread, files))
            out['decode_frames_per_s'][str(nw)] = round(len(files) / (time.perf_counter() - t0), 1)
    if torch.cuda.is_available():
        from vps_amd.pipeline import DeviceImagePrep
        dev = torch.device('cuda:0')
        prep = DeviceImagePrep(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True, size_divisor=32, device=dev)
        img = imread(files[0])
        pinned = torch.from_numpy(img).pin_memory()
        for name, src in (('pageable', torch.from_numpy(img)), ('pinned', pinned)):
            for _ in range(3):
                src.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                src.to(dev, non_blocking=True)
            torch.cuda.synchronize()
            out['upload_ms_' + name] = round(1e3 * (time.perf_counter() - t0) / 20, 3)
        d = pinned.to(dev)
        for _ in range(3):
            prep.prep(d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            prep.prep(d)
        torch.cuda.synchronize()
        out['prep_ms'] = round(1e3 * (time.perf_counter() - t0) / 50, 4)
        out['chained_frames_per_s'] = {}
        for nw in args.workers:
            with ThreadPoolExecutor(nw) as ex:
                t0 = time.perf_counter()
                futs = [ex.submit(imread, f) for f in files]       # the pool runs ahead of the consumer
                for f in futs:
                    prep.prep(torch.from_numpy(f.result()).to(dev, non_blocking=True))
                torch.cuda.synchronize()
                out['chained_frames_per_s'][str(nw)] = round(len(files) / (time.perf_counter() - t0), 1)
    for f in files:
        os.remove(f)
    os.rmdir(tmp)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
