"""Optical-flow accuracy against ground truth: end-point error (EPE), outlier rate (Fl), speed bins, accuracy shares, the quality of a
predicted occlusion mask and a colour-coded error image, with the per-pixel pass on the device (`vps_flow_error`,
csrc/flow_err_ops.hip).

The reference has no flow evaluation. The rules below - KITTI 2015's outlier rule and error colours, Sintel's speed bins and its
`invalid` / `occlusions` masks, Middlebury's unknown-flow convention - are RESTATED FROM MEMORY of those benchmark kits; no copy of any of
them is available where this was written. The colour table in particular is this module's definition, not a checked copy of the
devkit's. They are pinned only by hand-derived answers (tests/test_flow_eval.py) and by an independent per-pixel restatement
(tests/flow_err_restate.py), not by a run of an original.

One pair: `pred` and `gt`, fp32 [H][W][2], channel 0 = x, 1 = y, of equal size. `mask`, uint8 [H][W]: 1 = valid and not occluded (group
noc), 2 = valid and occluded in the ground truth (group occ), 0 and >= 3 = invalid; no mask: every pixel is noc. `occ_pred`, uint8
[H][W]: the codes of `tc.flow_occlusion` (0 visible, 1 occluded, 2 not in view). Per pixel, fp64 from the fp32 values, every operation
rounded on its own:
    invalid    the mask says so, or a gt component is NaN or |.| > 1e9 (Middlebury's unknown flow): counted as invalid, nothing else; black
    bad        valid, but a pred component is NaN, +-inf or |.| > 1e9: counted as bad (and in its occ_pred cell); no sum; (255, 0, 255)
    otherwise  du = u - ug, dv = v - vg, epe = sqrt(du*du + dv*dv), mag = sqrt(ug*ug + vg*vg)
               outlier (KITTI) iff epe > 3.0 and epe > 0.05 * mag, both strict, a product and no division
               speed bin (Sintel) by mag: < 10, 10 <= mag < 40, >= 40
               colour: n_err = min(epe / 3.0, epe / (0.05 * mag)), epe / 3.0 when mag == 0; the first row of `ERROR_COLOURS` with n_err < hi
Tables (`COUNT_CELLS` int64, `SUM_CELLS` float64): counts[g * 12 + k] for g = 0 (noc), 1 (occ): k = 0 n (valid and not bad), 1 bad,
2 outliers, 3 / 4 / 5 epe > 1 / 3 / 5, 6 / 7 / 8 n per speed bin, 9 / 10 / 11 valid pixels (bad ones too) whose occ_pred code is 0 / 1 / 2
(a code >= 3 is counted in none); counts[24] invalid pixels. sums[g * 4 + k]: k = 0 the sum of epe over the group's n, 1 / 2 / 3 over
its speed bins. Figures (`flow_from_tables`), n = n_noc + n_occ, every quotient 0 when its denominator is 0:
    epe_all = (S_noc + S_occ) / n, epe_noc = S_noc / n_noc, epe_occ = S_occ / n_occ
    fl_all = 100 * outliers / n, fl_noc = 100 * outliers_noc / n_noc (percent)
    s0_10, s10_40, s40plus = the sum of epe in the bin / the n of the bin, over both groups (Sintel)
    acc_1px, acc_3px, acc_5px = (n - #(epe > t)) / n: the share within t pixels (<=) of the valid pixels with a usable prediction
    bad_share = bad / (n + bad), invalid_share = invalid / all pixels
With `occ_pred`, over the valid pixels (n + bad), "predicted occluded" = code 1 or 2 (not visible in the other frame), "truly occluded" =
mask value 2:
    occ_precision = TP / (TP + FP), occ_recall = TP / (TP + FN), occ_f1 = 2 P R / (P + R),
    occ_pred_share = (TP + FP) / valid, occ_true_share = occ pixels / valid
KITTI's 16-bit PNG ground truth is read by vps_amd/kittiflow.py. Out of scope: angular error, and running FlowNet2 on frames whose
size is no multiple of 64 (a 436 x 1024 Sintel frame needs padding that `FlowNet2.run` does not do for general sizes).

`flow_from_tables`, `FlowEvalStats` and `flow_text` are NumPy / Python only. The counting (`flow_error`, `FlowEvaluator`) is
`vps_flow_error`: no CPU path, the HIP library must load and a device must be present; host arrays are uploaded, device flows (`FMap`,
[H,W,2], [1,2,H,W]: `pano_results['flow']`, `flow_between`) are used where they lie. The sums are reproducible byte for byte: no
floating-point atomics (include/vps_hip.h)."""
import numpy as np
import torch

from . import flowvis, hip, pairtables

COUNT_CELLS, SUM_CELLS = 25, 8
ERROR_COLOURS = ((0.1875, (49, 54, 149)), (0.375, (69, 117, 180)), (0.75, (116, 173, 209)), (1.5, (171, 217, 233)), (3.0, (224, 243, 248)),
                 (6.0, (254, 224, 144)), (12.0, (253, 174, 97)), (24.0, (244, 109, 67)), (48.0, (215, 48, 39)), (float('inf'), (165, 0, 38)))
INVALID_COLOUR, BAD_COLOUR = (0, 0, 0), (255, 0, 255)
FIGURES = ('epe_all', 'epe_noc', 'epe_occ', 'fl_all', 'fl_noc', 's0_10', 's10_40', 's40plus', 'acc_1px', 'acc_3px', 'acc_5px', 'bad_share',
           'invalid_share')
OCC_FIGURES = ('occ_precision', 'occ_recall', 'occ_f1', 'occ_pred_share', 'occ_true_share')


def _q(a, b):
    return float(a) / float(b) if b else 0.0


def flow_from_tables(counts, sums, with_occ=False):
    """One pair's or one set's tables -> the figures of the module docstring as plain Python numbers, plus 'n', 'n_noc', 'n_occ', 'bad',
    'invalid', 'outliers'. with_occ: also `OCC_FIGURES` (the tables were counted with an occ_pred)."""
    c = np.asarray(counts, dtype=np.int64).reshape(COUNT_CELLS)
    s = np.asarray(sums, dtype=np.float64).reshape(SUM_CELLS)
    g = c[:24].reshape(2, 12)
    tot = g.sum(0)
    n, bad, invalid = int(tot[0]), int(tot[1]), int(c[24])
    out = {'epe_all': _q(s[0] + s[4], n), 'epe_noc': _q(s[0], g[0, 0]), 'epe_occ': _q(s[4], g[1, 0]),
           'fl_all': 100.0 * _q(tot[2], n), 'fl_noc': 100.0 * _q(g[0, 2], g[0, 0]),
           's0_10': _q(s[1] + s[5], tot[6]), 's10_40': _q(s[2] + s[6], tot[7]), 's40plus': _q(s[3] + s[7], tot[8]),
           'acc_1px': _q(n - tot[3], n), 'acc_3px': _q(n - tot[4], n), 'acc_5px': _q(n - tot[5], n),
           'bad_share': _q(bad, n + bad), 'invalid_share': _q(invalid, n + bad + invalid),
           'n': n, 'n_noc': int(g[0, 0]), 'n_occ': int(g[1, 0]), 'bad': bad, 'invalid': invalid, 'outliers': int(tot[2])}
    if with_occ:
        tp, fp, fn = int(g[1, 10] + g[1, 11]), int(g[0, 10] + g[0, 11]), int(g[1, 9])
        p, r = _q(tp, tp + fp), _q(tp, tp + fn)
        out.update(occ_precision=p, occ_recall=r, occ_f1=_q(2 * p * r, p + r), occ_pred_share=_q(tp + fp, n + bad),
                   occ_true_share=_q(int(g[1, 0] + g[1, 1]), n + bad))
    return out


class FlowEvalStats:
    """Host side of the evaluation: collects downloaded tables and turns them into the result. No device."""

    def __init__(self):
        self.counts = np.zeros(COUNT_CELLS, dtype=np.int64)
        self.sums = np.zeros(SUM_CELLS, dtype=np.float64)
        self.pairs = []                                  # (name, counts, sums) of every pair that came with its own row
        self.with_occ = False
        self.npairs = 0

    def add_tables(self, counts, sums, npairs=1, names=None, with_occ=False):
        """counts int64 [25] and sums float64 [8] of `npairs` pairs together, or [npairs][25] and [npairs][8]: one row per pair"""
        counts, sums = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
        self.with_occ = self.with_occ or bool(with_occ)
        if counts.ndim == 2:
            assert counts.shape == (npairs, COUNT_CELLS) and sums.shape == (npairs, SUM_CELLS), (counts.shape, sums.shape)
            for i in range(npairs):
                self.pairs.append((str(names[i]) if names is not None else str(self.npairs + i), counts[i].copy(), sums[i].copy()))
            # the set's sums are the sums of the rows in order: a fixed order, so the total is reproducible too
            for i in range(npairs):
                self.counts += counts[i]
                self.sums += sums[i]
        else:
            self.counts += counts.reshape(COUNT_CELLS)
            self.sums += sums.reshape(SUM_CELLS)
        self.npairs += npairs

    def result(self):
        """the figures of the set (`flow_from_tables`) with 'pairs' (their number), 'counts' and 'sums' (the tables as lists) and
        'per_pair': [{'pair', + the figures}] for the pairs counted with per-pair rows: plain Python numbers, lists and strings, so
        that it survives JSON unchanged"""
        res = flow_from_tables(self.counts, self.sums, self.with_occ)
        res.update(pairs=self.npairs, counts=[int(v) for v in self.counts], sums=[float(v) for v in self.sums],
                   per_pair=[dict(flow_from_tables(c, s, self.with_occ), pair=name) for name, c, s in self.pairs])
        return res


def flow_text(result):
    """the text of flow-eval.txt: one row per pair (if the result has them) and the total row - EPE all / noc / occ, Fl-all and Fl-noc in
    percent, the three speed bins, the shares within 1 / 3 / 5 px, the bad and invalid shares x100. A result with the occlusion figures:
    three more columns, precision, recall and F1 x100"""
    occ = 'occ_f1' in result
    width = 112 + (24 if occ else 0)
    head = '{:16s}| {:>7s} {:>7s} {:>7s} {:>6s} {:>6s} {:>7s} {:>7s} {:>7s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s}'.format(
        'PAIR', 'EPE', 'EPE-noc', 'EPE-occ', 'Fl-all', 'Fl-noc', 's0-10', 's10-40', 's40+', '<=1px', '<=3px', '<=5px', 'BAD', 'INVAL')
    if occ:
        head += ' {:>7s} {:>7s} {:>7s}'.format('OCC-P', 'OCC-R', 'OCC-F1')

    def row(name, r):
        t = '{:16s}| {:7.3f} {:7.3f} {:7.3f} {:6.2f} {:6.2f} {:7.3f} {:7.3f} {:7.3f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f}'.format(
            name[:16], r['epe_all'], r['epe_noc'], r['epe_occ'], r['fl_all'], r['fl_noc'], r['s0_10'], r['s10_40'], r['s40plus'],
            100 * r['acc_1px'], 100 * r['acc_3px'], 100 * r['acc_5px'], 100 * r['bad_share'], 100 * r['invalid_share'])
        if occ:
            t += ' {:7.2f} {:7.2f} {:7.2f}'.format(100 * r['occ_precision'], 100 * r['occ_recall'], 100 * r['occ_f1'])
        return t
    out = ['=' * width, head, '-' * width]
    out += [row(str(r['pair']), r) for r in result.get('per_pair', [])]
    out += ['-' * width, row('All (%d)' % result['pairs'], result)]
    return '\n'.join(out) + '\n'


# ---------------------------------------------------------------------------------------------- the device side
def _device_flow(f, device):
    """what `flowvis._flow_view` takes, or a host array / tensor [H,W,2] or [1,2,H,W], which is uploaded -> the view"""
    if isinstance(f, np.ndarray) or (torch.is_tensor(f) and not f.is_cuda):
        f = torch.from_numpy(flowvis._host_hw2(f).astype(np.float32)).to(device)
    return flowvis._flow_view(f)


def _accumulate(pred, gt, mask, occ_pred, counts, sums, err_rgb, device):
    """one `vps_flow_error` on the current stream into the caller's device tables; returns the error image or None"""
    lib = hip.load()
    pt, pld, pco, H, W = _device_flow(pred, device)
    gtt, gld, gco, gH, gW = _device_flow(gt, device)
    if (gH, gW) != (H, W):
        raise ValueError('pred and gt must have equal H, W: pred %s, gt %s' % ((H, W), (gH, gW)))
    mask = pairtables.byte_map(mask, H, W, device, 'mask', 'flows')
    occ_pred = pairtables.byte_map(occ_pred, H, W, device, 'occ_pred', 'flows')
    if err_rgb is True:
        err_rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
    elif err_rgb is False:
        err_rgb = None
    pairtables.out_map(err_rgb, (H, W, 3), 'err_rgb is True, or a contiguous device uint8 [H,W,3] tensor')
    nbytes = int(lib.vps_flow_error_ws_bytes(H, W))
    hip.check(min(nbytes, 0), 'vps_flow_error_ws_bytes')
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)   # (stream-ordered: the allocator hands the block on only behind its last use)
    hip.check(lib.vps_flow_error(hip.ptr(pt), pld, pco, hip.ptr(gtt), gld, gco, hip.ptr(mask), hip.ptr(occ_pred), H, W, hip.ptr(counts), hip.ptr(sums),
                                 hip.ptr(err_rgb), hip.ptr(ws), nbytes, hip.stream_ptr()), 'vps_flow_error')
    return err_rgb


def _device(device):
    return pairtables.device_or_raise(device, 'the flow accuracy is counted on the device (vps_flow_error); there is no CPU path and no device is present')


def flow_error(pred, gt, mask=None, occ_pred=None, err_rgb=False, device=None):
    """One pair -> (counts device int64 [25], sums device float64 [8], the error image device uint8 [H,W,3] or None) on the current
    stream; nothing is downloaded or synchronised. pred, gt: `FMap`, device fp32 [H,W,2] or [1,2,H,W] (used where they lie) or host
    arrays of those shapes (uploaded). err_rgb: True, or a caller-owned contiguous device uint8 [H,W,3] tensor."""
    if device is None:
        device = next((t.device for t in (getattr(pred, 't', pred), getattr(gt, 't', gt)) if torch.is_tensor(t) and t.is_cuda), 'cuda')
    device = _device(device)
    counts = torch.zeros(COUNT_CELLS, dtype=torch.int64, device=device)
    sums = torch.zeros(SUM_CELLS, dtype=torch.float64, device=device)
    return counts, sums, _accumulate(pred, gt, mask, occ_pred, counts, sums, err_rgb, device)


class FlowEvaluator(FlowEvalStats):
    """The device side. `add_pair` counts one pair into tables that stay on the device (`vps_flow_error`, no synchronisation between
    pairs); `result()` is the ONE download. per_pair=True: every pair gets its own row of the tables (in blocks of 16 rows, still one
    download), the set's tables are the sum of the rows and `result()['per_pair']` has the figures of every pair."""

    def __init__(self, device='cuda', per_pair=False):
        super().__init__()
        self.device = _device(device)
        self.per_pair = bool(per_pair)
        self.lib = hip.load()
        self._tables = pairtables.PairTables(self.device, self.per_pair, [((COUNT_CELLS,), torch.int64), ((SUM_CELLS,), torch.float64)])
        self._names = []

    def add_pair(self, pred, gt, mask=None, occ_pred=None, err_rgb=None, name=None):
        """count one pair; err_rgb: None, True or a contiguous device uint8 [H,W,3] tensor that receives the error image (returned).
        Every pair of a set comes with an occ_pred or none does. Nothing is downloaded."""
        if self._tables.n and (occ_pred is not None) != self.with_occ:
            raise ValueError('a set is counted with a predicted occlusion mask for every pair or for none')
        counts, sums = self._tables.row()
        img = _accumulate(pred, gt, mask, occ_pred, counts, sums, False if err_rgb is None else err_rgb, self.device)
        self.with_occ = occ_pred is not None
        self._names.append(str(self._tables.n) if name is None else str(name))
        self._tables.n += 1
        return img

    def result(self):
        """the one download (and synchronisation) of what `add_pair` has counted since the last call, then `FlowEvalStats.result`"""
        if self._tables.n:
            n, (counts, sums) = self._tables.download()
            names, self._names = self._names, []
            self.add_tables(counts, sums, n, names if self.per_pair else None, self.with_occ)
        return super().result()


def write_outputs(result, out_dir):
    """flow-eval.txt and flow-eval.json in `out_dir`"""
    pairtables.write_result(result, out_dir, 'flow-eval', flow_text(result))
