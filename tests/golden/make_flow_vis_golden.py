"""Writes tests/golden/flow_vis_cases.npz by running the REAL reference functions `vis_flow` and `writeFlow`
(/root/reference/mmdet/datasets/pipelines/flow_utils.py, loaded by file path with an empty `cv2` module: it imports cv2 and never
uses it) in the build container. Run from the repo root:

    python tests/golden/make_flow_vis_golden.py

Per case: `flow/<case>` the float32 field [H,W,2]; `rgb64/<case>` = vis_flow(flow.astype(float64)), the product semantics;
`rgb32/<case>` = vis_flow(flow.copy()), the reference's own call on the float32 array, whose last level depends on NumPy's scalar
promotion and its float32 arctan2 - recorded with `numpy_version` and only bounded by the tests; `flo/<case>` the bytes of the file
writeFlow writes. The script asserts that the two images differ by at most one level in at most 1e-3 of the pixels.
The GPU box has no /root/reference: tests read the committed .npz only."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

# (u, v) of the first pixels of the first row of every case at least 9 wide: zero flow, the four axes, v = -0, the diagonal, and the
# two forms of unknown flow (u > 1e9, v > 1e9)
SPECIAL = [(0, 0), (2.5, 0), (-2.5, 0), (0, 1.5), (0, -1.5), (2.5, -0.0), (1.25, 1.25), (1e10, 1), (1, 2e9)]


def load_flow_utils():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    spec = importlib.util.spec_from_file_location('ref_flow_utils', os.path.join(REF, 'mmdet', 'datasets', 'pipelines', 'flow_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth_field(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rng = np.random.default_rng(0)
    u = 3 * np.sin(x / 17) + 0.02 * (y - 40) + rng.normal(0, 0.3, (H, W))
    v = -2 * np.cos(y / 11) + 0.01 * (x - 90) + rng.normal(0, 0.3, (H, W))
    return np.stack([u, v], -1).astype(np.float32)


def cases():
    rng = np.random.default_rng(1)
    out = {'1x1_zero': np.zeros((1, 1, 2), np.float32),
           '3x5': rng.normal(0, 2, (3, 5, 2)).astype(np.float32),
           '67x131': rng.normal(0, 3, (67, 131, 2)).astype(np.float32),
           '96x160_smooth': smooth_field(96, 160)}
    for f in out.values():
        if f.shape[1] >= len(SPECIAL):
            f[0, :len(SPECIAL)] = np.asarray(SPECIAL, dtype=np.float32)
    return out


def main():
    fu = load_flow_utils()
    out = {'numpy_version': np.array(np.__version__)}
    for name, flow in cases().items():
        rgb64 = fu.vis_flow(flow.astype(np.float64))                 # (vis_flow edits its argument in place: always a copy)
        rgb32 = fu.vis_flow(flow.copy())
        assert rgb64.dtype == np.uint8 and rgb64.shape == flow.shape[:2] + (3,)
        d = np.abs(rgb64.astype(np.int32) - rgb32.astype(np.int32))
        frac = float((d.max(-1) > 0).mean())
        assert d.max() <= 1 and frac <= 1e-3, (name, int(d.max()), frac)
        with tempfile.TemporaryDirectory() as tmp:
            fn = os.path.join(tmp, 'x.flo')
            fu.writeFlow(fn, flow.copy())
            flo = open(fn, 'rb').read()
            assert np.array_equal(fu.readFlow(fn), flow)
        out['flow/' + name] = flow
        out['rgb64/' + name] = rgb64
        out['rgb32/' + name] = rgb32
        out['flo/' + name] = np.frombuffer(flo, dtype=np.uint8)
        print('%-14s float32 vs float64 call: max level difference %d on %.2e of the pixels' % (name, int(d.max()), frac))
    path = os.path.join(HERE, 'flow_vis_cases.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, NumPy %s, %d bytes' % (path, len(cases()), np.__version__, os.path.getsize(path)))


if __name__ == '__main__':
    main()
