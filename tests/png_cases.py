"""Inputs shared by tests/test_png_out.py (CPU) and tests/test_png_out_gpu.py: the smallest images that reach each way the PNG encoder
can go wrong, built with fixed seeds. `cases()` -> {name: uint8 array [H,W] or [H,W,3]}; `restated(name)` -> the restatement's file
bytes, computed once per process."""
import functools

import numpy as np

import png_restate as R

SEG = R.SEG


def label_map(H, W, seed=0, n_things=45):
    """PanopticUnifier-style (pan_seg, pan_ins, pan_obj) map: eight stuff bands with wavy borders and ellipses with distinct object ids"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    wave = (H / 40.0) * np.sin(xx / (W / 13.0) + 0.7) + (H / 90.0) * np.sin(xx / (W / 47.0))
    seg = np.clip(((yy + wave) * 8.0 / H).astype(np.int64), 0, 7).astype(np.uint8)
    ins = np.zeros((H, W), np.uint8)
    obj = seg.copy()
    for i in range(n_things):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        ry, rx = int(rng.integers(max(2, H // 40), max(3, H // 6))), int(rng.integers(max(2, W // 60), max(3, W // 8)))
        y0, y1, x0, x1 = max(0, cy - ry), min(H, cy + ry + 1), max(0, cx - rx), min(W, cx + rx + 1)
        m = ((yy[y0:y1, x0:x1] - cy) / ry) ** 2 + ((xx[y0:y1, x0:x1] - cx) / rx) ** 2 <= 1.0
        seg[y0:y1, x0:x1][m] = 11 + i % 8
        ins[y0:y1, x0:x1][m] = i + 1
        obj[y0:y1, x0:x1][m] = 100 + i                    # distinct object ids
    return np.ascontiguousarray(np.stack([seg, ins, obj], -1))


def _run_row(lengths):
    """one grey row: a run of zeros of each length, separated by single bytes that alternate between two non-zero values (so that the
    separators never merge into a run). A first pixel of 90 keeps the filter byte (0 for a single row) out of the first run"""
    parts, k = [np.array([90], np.uint8)], 0
    for n in lengths:
        parts.append(np.zeros(n, np.uint8))
        parts.append(np.array([60 + (k & 1)], np.uint8)); k += 1
    return np.concatenate(parts)[None, :]


def _alignment_cases():
    """eight one-segment images whose bits before the stored block (3 header + tokens + 7 end-of-block) end on each bit alignment"""
    out = {}
    for w in range(1, 64):
        img = (200 + 3 * np.arange(w, dtype=np.int64) % 50).astype(np.uint8)[None, :]
        S = R.filter_rows(img)[0]
        assert len(S) <= SEG
        a = (3 + R.segment_token_bits(S) + 7) % 8
        out.setdefault(a, img)
        if len(out) == 8:
            break
    assert sorted(out) == list(range(8))
    return {'align%d' % a: img for a, img in out.items()}


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20)
    c = {}
    c['1x1x1'] = np.array([[77]], np.uint8)
    c['1x1x3'] = np.array([[[1, 200, 143]]], np.uint8)
    c['1x7x3'] = rng.integers(0, 256, (1, 7, 3)).astype(np.uint8)
    c['5x1x3'] = rng.integers(0, 256, (5, 1, 3)).astype(np.uint8)
    # a run of R zeros = one literal + R-1 more: R-1 in 0..6 (rem 0, 1, 2, 3...), 258..262 and 516..520 (the 258 cap, once and twice)
    c['runs'] = _run_row([1 + r for r in list(range(0, 7)) + list(range(258, 263)) + list(range(516, 521))])
    c['lit144'] = np.array([[0, 143, 144, 255, 145, 142, 1, 143, 143, 144, 144, 144, 144, 7]], np.uint8)
    c['const'] = np.full((3, SEG + 5), 9, np.uint8)                     # runs cross row and segment boundaries (rows of SEG + 6 bytes)
    c['twos'] = np.stack([np.zeros(40, np.uint8), np.full(40, 2, np.uint8)])    # a row of 2s below a row of zeros (Sub wins it: 2 against 80)
    top = rng.integers(0, 256, 40).astype(np.uint8)
    c['up2'] = np.stack([top, top + np.uint8(2)])                               # row 1: Up; filter byte 2 + residuals 2 = one run of 41
    c.update(_alignment_cases())
    c['noise'] = rng.integers(0, 256, (64, 96, 3)).astype(np.uint8)
    c['ff_rgb'] = np.full((64, 96, 3), 255, np.uint8)
    c['ff_grey'] = np.full((600, 600), 255, np.uint8)
    c['labels'] = label_map(128, 256, seed=1, n_things=12)
    c['full'] = label_map(1088, 1920, seed=2, n_things=45)
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    return R.png_file(cases()[name])
