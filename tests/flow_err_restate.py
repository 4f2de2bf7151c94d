"""Plain per-pixel restatement of the optical-flow accuracy measures (the contract in the docstring of vps_amd/floweval.py and in
include/vps_hip.h), sharing no code with vps_amd/floweval.py or the kernel, twice: `flow_error_loop` is one Python loop over the pixels with
`math.sqrt` on Python floats, `flow_error` the same on whole np.float64 arrays (what the larger tests can afford); in both every
operation is a float64 operation of its own in the stated order, the sums are taken with `math.fsum` (exactly rounded, so they do not
depend on any order), and tests/test_flow_eval.py holds the two against each other. The rules themselves (KITTI's outlier rule and error
colours, Sintel's speed bins, Middlebury's unknown-flow convention) are restated from memory of those kits; what pins them are the
hand-derived answers of tests/test_flow_eval.py.

    flow_error(pred, gt, mask, occ_pred)       -> {'counts' int64 [25], 'sums' float64 [8], 'abs' float64 [8] (the sums of |terms|, for the
                                                  summation bound), 'n' (pixels), 'rgb' uint8 [H,W,3]}
    flow_error_loop(pred, gt, mask, occ_pred)  -> the same, pixel by pixel
    figures(counts, sums)                      -> the result figures from the tables
"""
import math

import numpy as np

UNKNOWN = 1e9
ROWS = ((0.1875, (49, 54, 149)), (0.375, (69, 117, 180)), (0.75, (116, 173, 209)), (1.5, (171, 217, 233)), (3.0, (224, 243, 248)),
        (6.0, (254, 224, 144)), (12.0, (253, 174, 97)), (24.0, (244, 109, 67)), (48.0, (215, 48, 39)), (math.inf, (165, 0, 38)))
BLACK, MAGENTA = (0, 0, 0), (255, 0, 255)


def _inputs(pred, gt, mask, occ_pred):
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.dtype == gt.dtype == np.float32 and pred.shape == gt.shape and pred.ndim == 3 and pred.shape[2] == 2
    H, W = pred.shape[:2]
    mask = np.ones((H, W), dtype=np.uint8) if mask is None else np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.shape == (H, W)
    assert occ_pred is None or (np.asarray(occ_pred).dtype == np.uint8 and np.asarray(occ_pred).shape == (H, W))
    return pred, gt, mask, (None if occ_pred is None else np.asarray(occ_pred)), H, W


def flow_error_loop(pred, gt, mask=None, occ_pred=None):
    pred, gt, mask, occ_pred, H, W = _inputs(pred, gt, mask, occ_pred)
    counts = [0] * 25
    terms = [[] for _ in range(8)]
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            u, v, ug, vg = float(pred[y, x, 0]), float(pred[y, x, 1]), float(gt[y, x, 0]), float(gt[y, x, 1])
            m = int(mask[y, x])
            unknown = math.isnan(ug) or math.isnan(vg) or abs(ug) > UNKNOWN or abs(vg) > UNKNOWN
            if m not in (1, 2) or unknown:
                counts[24] += 1
                rgb[y, x] = BLACK
                continue
            g = 12 * (m - 1)
            if occ_pred is not None and int(occ_pred[y, x]) <= 2:
                counts[g + 9 + int(occ_pred[y, x])] += 1
            if any(math.isnan(c) or math.isinf(c) or abs(c) > UNKNOWN for c in (u, v)):
                counts[g + 1] += 1
                rgb[y, x] = MAGENTA
                continue
            du, dv = u - ug, v - vg
            epe = math.sqrt(du * du + dv * dv)
            mag = math.sqrt(ug * ug + vg * vg)
            counts[g] += 1
            counts[g + 2] += epe > 3.0 and epe > 0.05 * mag
            counts[g + 3] += epe > 1.0
            counts[g + 4] += epe > 3.0
            counts[g + 5] += epe > 5.0
            b = 0 if mag < 10.0 else (1 if mag < 40.0 else 2)
            counts[g + 6 + b] += 1
            terms[4 * (m - 1)].append(epe)
            terms[4 * (m - 1) + 1 + b].append(epe)
            n_err = epe / 3.0 if mag == 0.0 else min(epe / 3.0, epe / (0.05 * mag))
            rgb[y, x] = next(c for hi, c in ROWS if n_err < hi)
    return {'counts': np.array(counts, dtype=np.int64), 'sums': np.array([math.fsum(t) for t in terms]),
            'abs': np.array([math.fsum(abs(e) for e in t) for t in terms]), 'n': H * W, 'rgb': rgb}


def flow_error(pred, gt, mask=None, occ_pred=None):
    pred, gt, mask, occ_pred, H, W = _inputs(pred, gt, mask, occ_pred)
    D = np.float64
    with np.errstate(all='ignore'):
        u, v, ug, vg = pred[..., 0].astype(D), pred[..., 1].astype(D), gt[..., 0].astype(D), gt[..., 1].astype(D)
        unknown = np.isnan(ug) | np.isnan(vg) | (np.abs(ug) > UNKNOWN) | (np.abs(vg) > UNKNOWN)
        valid = ((mask == 1) | (mask == 2)) & ~unknown
        bad = valid & (np.isnan(u) | np.isnan(v) | np.isinf(u) | np.isinf(v) | (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN))
        good = valid & ~bad
        du, dv = u - ug, v - vg
        epe = np.sqrt(du * du + dv * dv)
        mag = np.sqrt(ug * ug + vg * vg)
        rel = D(0.05) * mag
        outlier = (epe > 3.0) & (epe > rel)
        third = epe / D(3.0)
        n_err = np.where(mag == 0.0, third, np.minimum(third, epe / rel))
    assert all(a.dtype == np.float64 for a in (epe, mag, rel, n_err))
    bins = np.where(mag < 10.0, 0, np.where(mag < 40.0, 1, 2))
    counts = np.zeros(25, dtype=np.int64)
    sums, sabs = np.zeros(8), np.zeros(8)
    counts[24] = int((~valid).sum())
    for g in range(2):
        sel = good & (mask == g + 1)
        allg = valid & (mask == g + 1)
        c = counts[12 * g:12 * g + 12]
        c[0], c[1], c[2] = sel.sum(), (bad & (mask == g + 1)).sum(), (sel & outlier).sum()
        c[3], c[4], c[5] = (sel & (epe > 1.0)).sum(), (sel & (epe > 3.0)).sum(), (sel & (epe > 5.0)).sum()
        for b in range(3):
            c[6 + b] = (sel & (bins == b)).sum()
            if occ_pred is not None:
                c[9 + b] = (allg & (occ_pred == b)).sum()
        for k, s in enumerate([sel] + [sel & (bins == b) for b in range(3)]):
            sums[4 * g + k] = math.fsum(epe[s].tolist())
            sabs[4 * g + k] = math.fsum(np.abs(epe[s]).tolist())
    rgb = np.zeros((H, W, 3), dtype=np.uint8)
    row = np.zeros((H, W), dtype=np.int64)
    for hi, _ in ROWS[:-1]:
        row += ~(n_err < hi)                                    # the first row with n_err < hi
    rgb[good] = np.array([c for _, c in ROWS], dtype=np.uint8)[row[good]]
    rgb[bad] = MAGENTA
    return {'counts': counts, 'sums': sums, 'abs': sabs, 'n': H * W, 'rgb': rgb}


def _div(a, b):
    return a / b if b else 0.0


def figures(counts, sums, with_occ=False):
    """the figures of vps_amd/floweval.py's docstring, restated: EPE all / noc / occ, Fl-all and Fl-noc in percent, the speed bins over both
    groups, the shares within 1 / 3 / 5 px of the valid pixels that are not bad, the bad share of the valid and the invalid share of all
    pixels; with_occ: precision, recall, F1 of 'occ_pred code != 0' against mask value 2 over the valid pixels, and both shares"""
    c = np.asarray(counts, dtype=np.int64).reshape(25)
    s = np.asarray(sums, dtype=np.float64).reshape(8)
    noc, occ = c[:12], c[12:24]
    n = int(noc[0] + occ[0])
    valid = n + int(noc[1] + occ[1])
    out = {'epe_all': _div(s[0] + s[4], n), 'epe_noc': _div(s[0], int(noc[0])), 'epe_occ': _div(s[4], int(occ[0])),
           'fl_all': 100.0 * _div(int(noc[2] + occ[2]), n), 'fl_noc': 100.0 * _div(int(noc[2]), int(noc[0])),
           's0_10': _div(s[1] + s[5], int(noc[6] + occ[6])), 's10_40': _div(s[2] + s[6], int(noc[7] + occ[7])),
           's40plus': _div(s[3] + s[7], int(noc[8] + occ[8])),
           'acc_1px': _div(n - int(noc[3] + occ[3]), n), 'acc_3px': _div(n - int(noc[4] + occ[4]), n), 'acc_5px': _div(n - int(noc[5] + occ[5]), n),
           'bad_share': _div(valid - n, valid), 'invalid_share': _div(int(c[24]), valid + int(c[24])), 'n': n, 'bad': valid - n, 'invalid': int(c[24])}
    if with_occ:
        tp, fp, fn = int(occ[10] + occ[11]), int(noc[10] + noc[11]), int(occ[9])
        p, r = _div(tp, tp + fp), _div(tp, tp + fn)
        out.update(occ_precision=p, occ_recall=r, occ_f1=_div(2 * p * r, p + r), occ_pred_share=_div(tp + fp, valid),
                   occ_true_share=_div(int(occ[0] + occ[1]), valid))
    return out
