"""GPU: `vps_boundary_band` through the C ABI against the per-segment erosion of tests/boundary_restate.py, byte for byte, on maps that
put segment edges where the window formulation can be off by one (stripes of width 2d, 2d+1, 2d+2; edges on and beside every tile seam
and at distance d-1, d, d+1 from the image border); the device evaluators of vps_amd/boundary.py against the per-pixel restatement;
one run of tools/run_vps_synthetic.py --boundary."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_restate as R
import stq_cases as K
from vps_amd import boundary, hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = np.array([0, 1, 2, 255, 256, 300, 65535, 65536, 70000, 0x123456, 0xFFFFFE, 0x800000], dtype=np.int64)      # all three bytes in use


def tile():
    t = (ctypes.c_int32 * 2)()
    assert hip.load().vps_boundary_tile(t) == 0
    return int(t[0]), int(t[1])


def band(dev, pan, d, slack=0, shift=0):
    """the C call on a host map; `slack` extra workspace bytes, `shift` puts the map at that byte offset of a larger buffer"""
    lib = hip.load()
    H, W = pan.shape[:2]
    buf = torch.zeros(pan.size + 8, dtype=torch.uint8, device=dev)
    src = buf[shift:shift + pan.size]
    src.copy_(torch.from_numpy(np.ascontiguousarray(pan).reshape(-1)))
    n = ctypes.c_int64(0)
    assert lib.vps_boundary_band_ws(H, W, d, ctypes.byref(n)) == 0 and n.value == 4 * H * W
    ws = torch.full((n.value + slack,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((H * W * 3 + 16,), 0x5A, dtype=torch.uint8, device=dev)
    hip.check(lib.vps_boundary_band(hip.ptr(src), H, W, d, hip.ptr(out), hip.ptr(ws), ws.numel(), hip.stream_ptr()), 'vps_boundary_band')
    host = out.cpu().numpy()
    assert (host[H * W * 3:] == 0x5A).all(), 'bytes behind the output were written'
    return host[:H * W * 3].reshape(H, W, 3)


def rectangles(seed, H, W, n=14):
    rng = np.random.default_rng(seed)
    m = IDS[rng.integers(0, len(IDS), size=(1, 1))].repeat(H, 0).repeat(W, 1)
    for _ in range(n):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, max(2, H))), int(rng.integers(1, max(2, W)))
        m[y0:y0 + h, x0:x0 + w] = IDS[int(rng.integers(0, len(IDS)))]
    m[: max(1, H // 7), : max(1, W // 5)] = 0                                    # a void region whatever the seed paints
    return m


def stripes(n, d, seam, ids=(7, 70000, 0xFFFFFE, 0)):
    """a 1-D id sequence of length n whose runs end at: distance d-1, d, d+1 from either end, every multiple of `seam` and one position
    either side of it, and otherwise after 2d, 2d+1, 2d+2 positions in turn; neighbouring runs always differ"""
    cuts = {d - 1, d, d + 1, n - d - 1, n - d, n - d + 1}
    for s in range(seam, n, seam):
        cuts |= {s - 1, s, s + 1}
    x, k = 0, 0
    while x < n:
        x += 2 * d + k % 3
        cuts.add(x); k += 1
    cuts = sorted(c for c in cuts if 0 < c < n)
    out = np.zeros(n, dtype=np.int64)
    for i, (a, b) in enumerate(zip([0] + cuts, cuts + [n])):
        out[a:b] = ids[i % len(ids)]
    return out


def plain_stripes(n, d):
    """runs of width exactly 2d, 2d+1 and 2d+2 in turn, from position 0: the off-by-one of the window"""
    out, x, k = np.zeros(n, dtype=np.int64), 0, 0
    while x < n:
        w = 2 * d + k % 3
        out[x:x + w] = (5, 0x10203, 0xFFFFFE)[k % 3]
        x += w; k += 1
    return out


def cases():
    TR, TC = tile()
    big = (2 * TR + 5, 2 * TC + 37)
    out = []
    for H, W in ((1, 200), (200, 1), (37, 53), (64, 64)):
        half = (min(H, W) + 1) // 2
        for d in (1, 2, 3, 7, max(half, 8)):                                     # the last one: 2d+1 exceeds the smaller side, everything is band
            out.append(('rect %dx%d d%d' % (H, W, d), rectangles(H * 1000 + W + d, H, W), d))
    for d in (1, 2, 3, 7):
        out.append(('vstripes 37x53 d%d' % d, np.tile(plain_stripes(53, d)[None, :], (37, 1)), d))
        out.append(('hstripes 64x64 d%d' % d, np.tile(plain_stripes(64, d)[:, None], (1, 64)), d))
        out.append(('vstripes 1x200 d%d' % d, plain_stripes(200, d)[None, :], d))
        out.append(('hstripes 200x1 d%d' % d, plain_stripes(200, d)[:, None], d))
    yy, xx = np.mgrid[0:37, 0:53]
    out.append(('checkerboard d1', np.where((yy + xx) % 2 == 0, 9, 0x40000), 1))
    out.append(('checkerboard d2', np.where((yy + xx) % 2 == 0, 9, 0x40000), 2))
    out.append(('uniform d3', np.full((64, 64), 0xFFFFFE, dtype=np.int64), 3))
    out.append(('uniform d31', np.full((64, 64), 513, dtype=np.int64), 31))        # a 2 x 2 interior is left
    out.append(('uniform d32', np.full((64, 64), 513, dtype=np.int64), 32))        # nothing is
    out.append(('void', np.zeros((37, 53), dtype=np.int64), 2))
    for d in (1, 2, 3, 7):                                                          # two tiles by two tiles and a remainder
        out.append(('seam vstripes d%d' % d, np.tile(stripes(big[1], d, TC)[None, :], (big[0], 1)), d))
        out.append(('seam hstripes d%d' % d, np.tile(stripes(big[0], d, TR)[:, None], (1, big[1])), d))
    cross = np.where(np.tile(stripes(big[0], 3, TR)[:, None], (1, big[1])) == 7, 7, np.tile(stripes(big[1], 3, TC)[None, :], (big[0], 1)))
    out.append(('seam crossed d3', cross, 3))
    out.append(('seam rect d3', rectangles(5, *big), 3))
    out.append(('seam rect d7', rectangles(6, *big, n=20), 7))
    out.append(('seam rect d40', rectangles(7, *big, n=6), 40))                     # 2d+1 = 81 > 69 rows: all band, halo wider than a tile of rows
    return out


CASES = cases() if os.path.exists(hip.LIB_PATH) else []
_REF = {}


def reference(i):
    """computed once per case and never changed"""
    if i not in _REF:
        name, ids, d = CASES[i]
        _REF[i] = R.band_map(R.pan_of(ids), d)
        _REF[i].setflags(write=False)
    return _REF[i]


@pytest.mark.parametrize('i', range(len(CASES)), ids=[c[0] for c in CASES])
def test_band_equals_the_per_segment_erosion(dev, i):
    name, ids, d = CASES[i]
    want = reference(i)
    got = band(dev, R.pan_of(ids), d)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(-1))[:8])
    if 'uniform d32' in name or name.endswith('d40') or name == 'void':
        assert np.array_equal(got, R.pan_of(ids))                                   # all band (or all void): the map itself


def test_same_bytes_for_any_workspace_size_and_map_alignment(dev):
    for i in (12, len(CASES) - 3):                                                  # rect 37x53 d3, seam rect d3
        name, ids, d = CASES[i]
        want = reference(i)
        for slack, shift in ((0, 0), (4096, 0), (0, 1), (12, 2), (0, 3)):
            assert np.array_equal(band(dev, R.pan_of(ids), d, slack, shift), want), (name, slack, shift)


def test_python_entry_point(dev):
    name, ids, d = CASES[12]
    pan = R.pan_of(ids)
    assert np.array_equal(boundary.boundary_band(pan, d, device=dev).cpu().numpy(), reference(12))
    t = torch.from_numpy(pan).to(dev)
    out = boundary.boundary_band(t, ratio=0.05)                                     # 0.05 * sqrt(37^2 + 53^2) = 3.2 -> d = 3
    assert out.is_cuda and out.shape == t.shape and np.array_equal(out.cpu().numpy(), reference(12))


# ---------------------------------------------------------------------------------------------- the evaluators
def _with_areas(frames):
    """stq_cases frames as the PQ / VPQ evaluators take them: ground-truth areas from the map, predicted entries only for painted ids"""
    out = []
    for gt_ann, pred_ann, gt_pan, pred_pan in frames:
        g, p = R.ids_of(gt_pan), R.ids_of(pred_pan)
        gt = [dict(s, area=int((g == s['id']).sum())) for s in gt_ann['segments_info']]
        pred = [dict(s, area=int((p == s['id']).sum()), iscrowd=0) for s in pred_ann['segments_info'] if (p == s['id']).any()]
        out.append(({'segments_info': gt}, {'segments_info': pred}, gt_pan, pred_pan, {}))
    return out


def _videos():
    vids = [(_with_areas(v), {c: dict(e, id=c) for c, e in K.CATS5.items()}) for v in K.two_videos(64, 128)]
    vids += [(_with_areas(K.random_video(seed, nframes=3, H=64, W=128)), {c: dict(e, id=c) for c, e in K.CATS5.items()}) for seed in (1, 2)]
    return vids


def _same(stat, want, cats):
    n = 0
    for c in cats:
        got = stat[c]
        assert (got.tp, got.fp, got.fn) == (want[c]['tp'], want[c]['fp'], want[c]['fn']), c
        assert got.iou == want[c]['iou'] and got.biou == want[c]['biou'], c           # the same float64 operations in the same order
        n += got.tp
    return n


def test_device_evaluators_equal_the_per_pixel_restatement(dev):
    assert boundary.dilation(64, 128) == 3
    matched = 0
    for clip, cats in _videos():
        stat = boundary.pq_compute_single_core([f[0] for f in clip], [f[1] for f in clip], [f[2] for f in clip], [f[3] for f in clip],
                                               [f[4] for f in clip], cats, device=dev)
        matched += _same(stat, R.boundary_pq(clip), cats)
        cache = {}
        for nf in (1, 2):
            matched += _same(boundary.vpq_compute_single_core(clip, cats, nframes=nf, device=dev, _cache=cache), R.boundary_vpq(clip, nf), cats)
    assert matched > 10
    # the boundary measure is the stricter one on these clips: some pair that mask PQ matches is lost
    clip, cats = _videos()[1]
    plain = R.mask_pq(clip); strict = R.boundary_pq(clip)
    assert sum(v['tp'] for v in strict.cat.values()) <= sum(v['tp'] for v in plain.cat.values())


def test_run_vps_synthetic_boundary_scores_itself_100(dev, tmp_path):
    out = str(tmp_path / 'run')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_vps_synthetic.py'), '--videos', '1', '--frames', '25', '--height', '128', '--width', '256',
                        '--out', out, '--boundary'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    rep = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])
    pred = os.path.join(out, 'pred')
    assert all(os.path.exists(os.path.join(pred, 'bvpq-%d.txt' % k)) for k in (0, 5, 10, 15))
    fin = open(os.path.join(pred, 'bvpq-final.txt')).read().splitlines()
    assert fin[0] == 'bvpq_all:100.0000' and rep['bvpq']['bvpq'] == 100.0 and rep['vpq'] == 100.0
    assert all(v == 100.0 for v in rep['bvpq']['biou_per_window'].values())
