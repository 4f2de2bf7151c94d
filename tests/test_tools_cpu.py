"""CPU checks of the measurement tools that post-process GPU-side output (so a broken parser is found here, not on the GPU box)."""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trace_gaps_on_a_synthetic_kernel_trace(tmp_path):
    """three frames of two overlapping 'streams': busy = union of the intervals, work = their sum, the gap classes add up to idle"""
    rows, t = [], 1000
    for fr in range(6):
        for k in range(10):
            rows.append((t, t + 90_000, 'conv'))                 # main stream: 90 us kernels, 10 us apart
            rows.append((t + 20_000, t + 60_000, 'side'))        # side stream: fully inside the main kernel
            t += 100_000
        rows.append((t, t + 50_000, 'void (anonymous namespace)::panoptic_combine_kernel(float const*)'))
        t += 50_000
    d = tmp_path / 'trace' / 'box'
    d.mkdir(parents=True)
    with open(d / '1_kernel_trace.csv', 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['Kind', 'Start_Timestamp', 'End_Timestamp', 'Kernel_Name'])
        for a, b, n in rows:
            w.writerow(['KERNEL_DISPATCH', a, b, n])
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'trace_gaps.py'), str(tmp_path / 'trace')], capture_output=True, text=True, check=True)
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r['frames'] == 5 and abs(r['period_ms'] - 1.05) < 1e-6
    assert abs(r['busy_ms'] - 0.95) < 1e-6 and abs(r['idle_ms'] - 0.10) < 1e-6          # 10 gaps of 10 us
    assert abs(r['work_ms'] - (0.95 + 0.40)) < 1e-6 and r['launches_per_frame'] == 21
    assert r['idle_gaps']['10-50us'] == [10, 0.1] and r['idle_gaps']['<2us'][0] == 0


def test_bench_dump_outputs_writes_exact_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one DIR/<name>.npy per array of the frame's output dict, uint8 maps as float32 and int64 vectors as
    float64 (values exact), non-array entries skipped; past the 64 MB budget an array is replaced by a fixed seeded sample + indices"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(0)
    out = {'fcn_outputs': torch.from_numpy(rng.integers(0, 19, (1, 64, 128), dtype=np.uint8)),
           'panoptic_cls_inds': torch.arange(7), 'panoptic_cls_prob': torch.rand(7),
           'panoptic_det_obj_ids': np.arange(7) * 2 ** 40, 't': 3}
    bench.dump_outputs(out, str(tmp_path / 'a'))
    assert sorted(os.listdir(tmp_path / 'a')) == ['fcn_outputs.npy', 'panoptic_cls_inds.npy', 'panoptic_cls_prob.npy', 'panoptic_det_obj_ids.npy']
    got = {k: np.load(tmp_path / 'a' / (k + '.npy')) for k in out if k != 't'}
    assert got['fcn_outputs'].dtype == np.float32 and np.array_equal(got['fcn_outputs'], out['fcn_outputs'].numpy())
    assert got['panoptic_det_obj_ids'].dtype == np.float64 and np.array_equal(got['panoptic_det_obj_ids'], out['panoptic_det_obj_ids'])
    assert got['panoptic_cls_prob'].dtype == np.float32 and got['panoptic_cls_inds'].dtype == np.float64
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 16 << 10)
    for d in ('b', 'c'):
        bench.dump_outputs(out, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / 'b'))
    assert 'fcn_outputs.sample.npy' in names and 'fcn_outputs.npy' not in names and 'panoptic_cls_inds.npy' in names
    assert sum(os.path.getsize(tmp_path / 'b' / n) for n in names) <= (16 << 10) + 128 * len(names)      # + the .npy headers
    s, i = np.load(tmp_path / 'b' / 'fcn_outputs.sample.npy'), np.load(tmp_path / 'b' / 'fcn_outputs.sample_index.npy').astype(np.int64)
    assert np.array_equal(s, out['fcn_outputs'].numpy().reshape(-1)[i].astype(np.float32))
    assert np.array_equal(i, np.load(tmp_path / 'c' / 'fcn_outputs.sample_index.npy').astype(np.int64))         # the same sample every run
