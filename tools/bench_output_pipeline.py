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
Prints one JSON line and writes it to --out, stamped with `hip.csrc_sha16()`. Needs the GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=30)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_output_pipeline.json'))
    args = ap.parse_args()
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
