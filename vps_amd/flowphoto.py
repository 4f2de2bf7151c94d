"""Flow quality without ground truth: the photometric warp error of a flow between the two frames it was computed from, beside the
"static" error of not warping at all, with the per-pixel pass on the device (`vps_flow_photo`,
csrc/flow_photo_ops.hip).

The reference has nothing of the kind. This is the warp / interpolation error that the Middlebury flow benchmark (Baker et al., "A
database and evaluation methodology for optical flow", IJCV 2011) reports beside the end-point error, RESTATED FROM MEMORY; no copy of
the benchmark's kit is available where this was written. It is pinned only by hand-derived answers (tests/test_flow_photo.py) and by an
independent per-pixel restatement (tests/flow_photo_restate.py), not by a run of an original. `PHOTO_THR`, the default of the flag
threshold, is a parameter default with NO real footage behind it: nobody has looked at what it flags on a real clip.

One pair: `cur` and `prev`, uint8 [H][W][3] frames (BGR as the detector holds them; the figures do not depend on the channel order), and
`flow`, fp32 [H][W][2] of the same H, W, on the grid of cur and pointing into prev (the direction of `pano_results['flow']`, see
vps_amd/tc.py): warped(p) = prev(p + flow(p)). `mask`, uint8 [H][W]: the codes of `tc.flow_occlusion`; 0 puts a pixel into group 0
("visible"), any other byte into group 1; no mask: every pixel is in group 0. Frames of another size than the flow's are refused:
H, W is the decoded frame at the native 1024 x 2048 in the tools, resized or padded inputs are out of scope. Per pixel p = (x, y) of
cur, in this order, every operation rounded on its own:
    1. in view, fp32   u, v = flow(p); sx = float(x) + u, sy = float(y) + v; in view iff floorf(sx + 0.5f) and floorf(sy + 0.5f) lie in
                       [0, W-1] and [0, H-1], compared as floats (the rule of vps_amd/tc.py: NaN, +-inf, 1e30 fall out).
                       Not in view: counts[20] += 1, mask_out = 2, residual = 0, nothing else
    2. group           g = 0 when there is no mask or mask[p] == 0, otherwise 1
    3. sample, fp32    corners and weights as `tc.flow_occlusion` forms them: x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1, both clamped to
                       [0, W-1] after conversion to int; the same for y. Per channel c, the corner bytes converted to float:
                       top = b00 + wx*(b01 - b00), bot = b10 + wx*(b11 - b10), s_c = top + wy*(bot - top)
    4. errors, fp64    dw_c = double(s_c) - double(cur_c); aw = (|dw_0| + |dw_1|) + |dw_2|; qw = (dw_0*dw_0 + dw_1*dw_1) + dw_2*dw_2;
                       e = aw / 3.0. The static twin from prev(p) itself, exact integers: as = sum |prev_c(p) - cur_c(p)| and
                       qs = sum (prev_c(p) - cur_c(p))^2
    5. flagged         iff e > double(thr), strictly
    6. tables          counts[g * 10 + k] (`COUNT_CELLS` int64): k = 0 n, 1 flagged, 2 the sum of as, 3 the sum of qs, 4 / 5 / 6 / 7 pixels
                       with e > 4 / 8 / 16 / 32, 8 pixels with aw < double(as) (the flow helps), 9 pixels with aw > double(as);
                       sums[g * 2] += aw, sums[g * 2 + 1] += qw (`SUM_CELLS` float64). Cells 0 of both groups and cell 20 together grow
                       by H W per pair
    7. mask_out[p]     mask[p] when that is non-zero, else 3 when flagged, else 0
    8. residual[p]     min(255, (int)floor(e + 0.5))
Figures (`photo_from_tables`), per group ('visible', 'masked') and overall ('all'), every quotient 0 when its denominator is 0:
    mae_warp = sum aw / (3 n), rms_warp = sqrt(sum qw / (3 n)), psnr_warp = 10 log10(255^2 / (sum qw / (3 n))), inf at zero error
    mae_static, rms_static, psnr_static: the same from the sums of as and qs
    ratio = mae_warp / mae_static (below 1: warping with the flow explains the frame better than not warping)
    gain_db = psnr_warp - psnr_static (0 when either is inf)
    above_4, above_8, above_16, above_32: the shares of n with e above the level; helped, hurt: the shares with aw < as and aw > as
    flagged_share = flagged / n; overall also outside_share = outside / (n + outside)
What it is for: a figure for the flow on a clip that has no ground truth (rows 3e - 3g of DESIGN.md 6 all rest on the flow and none
can rate it there); a check of `tc.flow_occlusion`, whose occluded pixels should show a clearly higher residual than its visible ones;
and a third mask state for the temporal consistency (`TcEvaluator(photometric=)`): in view, not occluded, yet photometrically wrong -
the flow that is wrong but self-consistent in both directions. Limits: brightness changes, specular surfaces and sensor noise are
charged to the flow; a flow can match the colours of the wrong place (flat regions cost nothing whatever the flow says).

`photo_from_tables`, `PhotoStats`, `photo_text` are NumPy / Python only. The counting (`flow_photometric`, `PhotoEvaluator`) is
`vps_flow_photo`: no CPU path, the HIP library must load and a device must be present; host arrays are uploaded, device tensors are
used where they lie. The sums are reproducible byte for byte: no floating-point atomics (include/vps_hip.h).

The ternary census residual (`vps_flow_census`, csrc/flow_census_ops.hip) is the illumination-robust twin of the
above, opt-in: the hard ternary census (Stein, "Efficient computation of optical flow using the census transform", 2004) as UnFlow
(Meister et al., AAAI 2018) uses it, RESTATED FROM MEMORY; UnFlow's soft, differentiable form is not built. It compares the ordering of
each pixel against its 7 x 7 neighbourhood, not the intensities: an additive brightness change cancels exactly, a moderate gain change
too. `CENSUS_EPS` and `CENSUS_THR` are parameter defaults with NO real footage behind them. Inputs as above. The rule:
    1. grey            g = 299 R + 587 G + 114 B of a BGR pixel, an integer in 0 .. 255 000, held as fp32 (exact)
    2. warped grey     Wg(p): the in-view rule of step 1 above and the corners and weights of step 3 above, verbatim; the bilinear sample
                       of the four corners' greys in fp32 in that order (top, bot, then s), every operation rounded on its own. A pixel
                       that is not in view has no Wg
    3. window          the neighbours q = p + (dx, dy), dx, dy in -3 .. 3, not both zero: 48
    4. code            for an image A: code_A(p, q) = +1 if A(q) - A(p) > eps, -1 if it is < -eps, else 0: one fp32 subtraction and two
                       comparisons; eps is fp32 in units of g (`CENSUS_EPS` = 2000.0: two grey levels)
    5. warped count    a neighbour counts when q lies in the image and Wg(q) exists: n_w(p) of them, d_w(p) of those with
                       code_cur != code_Wg
    6. static count    prev unwarped in the place of Wg: n_s counts every neighbour in the image, d_s as in 5
    7. scored          p is in view and n_w(p) >= 1
    8. flagged         a scored pixel with 100 d_w > thr n_w, thr an integer percent in 0 .. 100 (`CENSUS_THR` = 25), strictly, in integers
    9. helped / hurt   d_w n_s < d_s n_w / d_w n_s > d_s n_w
   10. table           int64 [2][13] (`CENSUS_CELLS`), row g as in step 2 above (also for the pixels that are not scored): 0 scored pixels,
                       1 / 2 the sums of d_w / n_w, 3 / 4 the sums of d_s / n_s over scored pixels, 5 / 6 / 7 scored pixels with
                       100 d_w > 10 / 25 / 50 n_w, 8 helped, 9 hurt, 10 flagged, 11 not in view, 12 in view with n_w = 0. Cells 0, 11
                       and 12 of both rows together grow by H W per pair. Integer adds only: twice without zeroing is exactly double
   11. mask_out[p]     2 when p is not in view, else mask[p] when that is non-zero, else 3 when flagged, else 0
   12. residual[p]     (255 d_w + n_w / 2) / n_w in integer division; 0 for a pixel that is not scored
Figures (`census_from_tables`), per group and overall, every quotient 0 when its denominator is 0: ce_warp = sum d_w / sum n_w,
ce_static = sum d_s / sum n_s, ratio = ce_warp / ce_static, gain = ce_static - ce_warp, above_10 / above_25 / above_50, helped, hurt,
flagged_share (shares of the scored pixels), outside (cell 11), alone (cell 12), outside_share = outside / (n + outside + alone).
`census_from_tables`, `CensusStats`, `census_text` are NumPy / Python only; `flow_census` and `CensusEvaluator` are `vps_flow_census`:
no CPU path."""
import math

import numpy as np
import torch

from . import hip, pairtables
from .tc import _flow_layout

COUNT_CELLS, SUM_CELLS = 21, 4
PHOTO_THR = 16.0                                         # grey levels; a parameter default with no real footage behind it
LEVELS = (4, 8, 16, 32)
GROUPS = ('visible', 'masked')
CENSUS_CELLS = 13
CENSUS_EPS = 2000.0                                      # units of g (two grey levels); a parameter default with no real footage behind it
CENSUS_THR = 25                                          # percent of the counted neighbours; a parameter default with no real footage behind it
CENSUS_LEVELS = (10, 25, 50)
CENSUS_FIGURES = ('ce_warp', 'ce_static', 'ratio', 'gain', 'above_10', 'above_25', 'above_50', 'helped', 'hurt', 'flagged_share', 'outside_share')
FIGURES = ('mae_warp', 'rms_warp', 'psnr_warp', 'mae_static', 'rms_static', 'psnr_static', 'ratio', 'gain_db', 'above_4', 'above_8', 'above_16',
           'above_32', 'helped', 'hurt', 'flagged_share')


def _q(a, b):
    return float(a) / float(b) if b else 0.0


def _psnr(mse):
    return 10.0 * math.log10(255.0 * 255.0 / mse) if mse > 0 else float('inf')


def _figures(c, s):
    """one group's ten cells and two sums -> its figures"""
    n = int(c[0])
    mse_w, mse_s = _q(s[1], 3 * n), _q(c[3], 3 * n)
    out = {'n': n, 'flagged': int(c[1]), 'mae_warp': _q(s[0], 3 * n), 'rms_warp': math.sqrt(mse_w), 'psnr_warp': _psnr(mse_w),
           'mae_static': _q(c[2], 3 * n), 'rms_static': math.sqrt(mse_s), 'psnr_static': _psnr(mse_s)}
    out['ratio'] = _q(out['mae_warp'], out['mae_static'])
    out['gain_db'] = out['psnr_warp'] - out['psnr_static'] if math.isfinite(out['psnr_warp']) and math.isfinite(out['psnr_static']) else 0.0
    for i, lv in enumerate(LEVELS):
        out['above_%d' % lv] = _q(c[4 + i], n)
    out.update(helped=_q(c[8], n), hurt=_q(c[9], n), flagged_share=_q(c[1], n))
    return out


def photo_from_tables(counts, sums):
    """One pair's or one set's tables -> {'all': figures, 'visible': figures of group 0, 'masked': figures of group 1, 'outside',
    'outside_share'} as plain Python numbers; 'all' is the two groups' cells and sums added (group 0 first)."""
    c = np.asarray(counts, dtype=np.int64).reshape(COUNT_CELLS)
    s = np.asarray(sums, dtype=np.float64).reshape(SUM_CELLS)
    g, gs = c[:20].reshape(2, 10), s.reshape(2, 2)
    outside = int(c[20])
    out = {'all': _figures(g[0] + g[1], gs[0] + gs[1]), 'visible': _figures(g[0], gs[0]), 'masked': _figures(g[1], gs[1]), 'outside': outside}
    out['outside_share'] = _q(outside, out['all']['n'] + outside)
    return out


class PhotoStats:
    """Host side of the evaluation: collects the downloaded tables of every video and turns them into the result. No device."""

    def __init__(self, thr=PHOTO_THR):
        if not float(thr) >= 0:
            raise ValueError('thr is not negative, got %r' % (thr,))
        self.thr = float(thr)
        self.counts = np.zeros(COUNT_CELLS, dtype=np.int64)
        self.sums = np.zeros(SUM_CELLS, dtype=np.float64)
        self.videos = []
        self.npairs = 0

    def add_tables(self, video_id, counts, sums, npairs=1):
        """one video's tables: counts int64 [21] and sums float64 [4] of `npairs` pairs together, or [npairs][21] and [npairs][4], one
        row per pair (the video's tables are then the sums of the rows in order: a fixed order, so the total is reproducible too)"""
        counts, sums = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
        pairs = None
        if counts.ndim == 2:
            assert counts.shape == (npairs, COUNT_CELLS) and sums.shape == (npairs, SUM_CELLS), (counts.shape, sums.shape)
            pairs = [dict(photo_from_tables(counts[i], sums[i]), pair=i + 1) for i in range(npairs)]
            vc, vs = np.zeros(COUNT_CELLS, dtype=np.int64), np.zeros(SUM_CELLS, dtype=np.float64)
            for i in range(npairs):
                vc += counts[i]
                vs += sums[i]
        else:
            vc, vs = counts.reshape(COUNT_CELLS).copy(), sums.reshape(SUM_CELLS).copy()
        self.counts += vc
        self.sums += vs
        self.npairs += npairs
        st = dict(photo_from_tables(vc, vs), video=len(self.videos) if video_id is None else video_id, pairs=npairs, counts=vc, sums=vs, per_pair=pairs)
        self.videos.append(st)
        return st

    def result(self):
        """`photo_from_tables` of the set with 'thr', 'pairs', 'counts' and 'sums' (the tables as lists), 'per_video': [{'video', 'pairs',
        'all', 'visible', 'masked', 'outside', 'outside_share'}] and 'per_pair': [{'video', 'pair', ...}] for the videos counted with
        per-pair rows: plain Python numbers, lists and strings (a PSNR of inf is the float inf, which `json` writes as Infinity)"""
        res = photo_from_tables(self.counts, self.sums)
        keep = ('all', 'visible', 'masked', 'outside', 'outside_share')
        res.update(thr=self.thr, pairs=self.npairs, counts=[int(v) for v in self.counts], sums=[float(v) for v in self.sums],
                   per_video=[dict({k: st[k] for k in keep}, video=st['video'], pairs=st['pairs']) for st in self.videos],
                   per_pair=[dict({k: p[k] for k in keep}, video=st['video'], pair=p['pair']) for st in self.videos for p in (st['per_pair'] or [])])
        return res


def photo_text(result):
    """the text of flow-photo.txt: per video and for the set one row per group (all, visible, masked) - the number of pixels, MAE and PSNR
    warped and static, their ratio and gain, the shares x100 above 4 / 8 / 16 / 32 grey levels, helped, hurt and flagged - and the share of
    pixels not in view"""
    width = 122
    head = '{:16s}| {:8s} {:>11s} {:>7s} {:>7s} {:>6s} {:>7s} {:>7s} {:>7s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s}'.format(
        'VIDEO', 'GROUP', 'N', 'MAE-w', 'MAE-s', 'RATIO', 'PSNR-w', 'PSNR-s', 'GAIN', '>4', '>8', '>16', '>32', 'HELP', 'HURT', 'FLAG')

    def rows(name, r):
        out = []
        for grp in ('all',) + GROUPS:
            f = r[grp]
            out.append('{:16s}| {:8s} {:11d} {:7.3f} {:7.3f} {:6.3f} {:7.2f} {:7.2f} {:7.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f}'.format(
                name[:16], grp, f['n'], f['mae_warp'], f['mae_static'], f['ratio'], f['psnr_warp'], f['psnr_static'], f['gain_db'], 100 * f['above_4'],
                100 * f['above_8'], 100 * f['above_16'], 100 * f['above_32'], 100 * f['helped'], 100 * f['hurt'], 100 * f['flagged_share']))
        return out
    out = ['=' * width, head, '-' * width]
    for r in result.get('per_video', []):
        out += rows(str(r['video']), r)
    out += ['-' * width] + rows('All (%d)' % result['pairs'], result)
    out.append('thr {:g}  outside {:d} ({:.2f} %)'.format(result['thr'], result['outside'], 100 * result['outside_share']))
    return '\n'.join(out) + '\n'


def _residual_lut():
    """256 x RGB: 0 -> 0,0,0 (the overlay keeps the frame), then black -> red -> yellow -> white with the residual, saturated at 64"""
    lut = np.zeros((256, 3), dtype=np.uint8)
    for r in range(1, 256):
        t = min(r, 64) / 64.0
        lut[r] = (min(255, int(round(765 * t))), min(255, max(0, int(round(765 * t - 255)))), min(255, max(0, int(round(765 * t - 510)))))
        lut[r, 0] = max(lut[r, 0], 1)
    return lut


RESIDUAL_PALETTE = _residual_lut()


def residual_colour(residual):
    """the residual image uint8 [H,W] (device) painted through the 256-entry `RESIDUAL_PALETTE`: RGB uint8 [H,W,3] for `render_overlay`,
    where 0,0,0 (no residual) keeps the frame"""
    lut = torch.from_numpy(RESIDUAL_PALETTE).to(residual.device)
    return lut[residual.to(torch.int64)]


# ---------------------------------------------------------------------------------------------- the device side
def _device(device):
    return pairtables.device_or_raise(device, 'the photometric error is counted on the device (vps_flow_photo); there is no CPU path and no device is present')


def _pair_inputs(cur, prev, flow, mask, mask_out, residual, device):
    """the checks both kernels share -> (flow, ld, H, W, cur, prev, mask) on the device"""
    flow, ld = _flow_layout(flow, device)
    H, W = int(flow.shape[0]), int(flow.shape[1])
    cur, prev = pairtables.frame(cur, H, W, device, 'cur'), pairtables.frame(prev, H, W, device, 'prev')
    mask = pairtables.byte_map(mask, H, W, device, 'mask', 'flow')            # (a device mask is used where it lies: it may be mask_out)
    for t, what in ((mask_out, 'mask_out'), (residual, 'residual')):
        pairtables.out_map(t, (H, W), '%s is a contiguous device uint8 [%d,%d] tensor' % (what, H, W))
    return flow, ld, H, W, cur, prev, mask


def _accumulate(lib, cur, prev, flow, mask, thr, counts, sums, mask_out, residual, device):
    flow, ld, H, W, cur, prev, mask = _pair_inputs(cur, prev, flow, mask, mask_out, residual, device)
    if not float(thr) >= 0:
        raise ValueError('thr is not negative, got %r' % (thr,))
    nbytes = int(lib.vps_flow_photo_ws_bytes(H, W))
    hip.check(min(nbytes, 0), 'vps_flow_photo_ws_bytes')
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)           # (stream-ordered: the allocator hands the block on only behind its last use)
    hip.check(lib.vps_flow_photo(hip.ptr(cur), hip.ptr(prev), H, W, hip.ptr(flow), ld, 0, hip.ptr(mask), float(thr), hip.ptr(counts), hip.ptr(sums),
                                 hip.ptr(mask_out), hip.ptr(residual), hip.ptr(ws), nbytes, hip.stream_ptr()), 'vps_flow_photo')


def flow_photometric(cur, prev, flow, mask=None, thr=PHOTO_THR, counts=None, sums=None, mask_out=None, residual=None):
    """One pair through `vps_flow_photo` on the current stream; nothing is downloaded or synchronised. cur, prev: uint8 [H,W,3] frames
    (device tensors are used where they lie, host arrays are uploaded); flow: a device fp32 [H,W,2] tensor on the grid of cur pointing
    into prev (a view of a wider NHWC map is read where it lies). mask: None or uint8 [H,W] (`tc.flow_occlusion`'s codes). counts,
    sums: None (fresh zeroed tables) or contiguous device int64 [21] / float64 [4] tensors the call ADDS to. mask_out, residual: None or
    contiguous device uint8 [H,W] tensors; mask_out may be `mask` itself. -> (counts, sums)."""
    if not (torch.is_tensor(flow) and flow.is_cuda):
        raise hip.VpsHipError('flow_photometric runs on the device (vps_flow_photo); there is no CPU path')
    dev = flow.device
    if counts is None:
        counts = torch.zeros(COUNT_CELLS, dtype=torch.int64, device=dev)
    elif not (torch.is_tensor(counts) and counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == COUNT_CELLS):
        raise ValueError('counts is a contiguous device int64 [%d] tensor' % COUNT_CELLS)
    if sums is None:
        sums = torch.zeros(SUM_CELLS, dtype=torch.float64, device=dev)
    elif not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == SUM_CELLS):
        raise ValueError('sums is a contiguous device float64 [%d] tensor' % SUM_CELLS)
    _accumulate(hip.load(), cur, prev, flow, mask, thr, counts, sums, mask_out, residual, dev)
    return counts, sums


class _VideoPairs:
    """What `PhotoEvaluator` and `CensusEvaluator` share, in front of their Stats class: pairs are counted into `pairtables.PairTables`
    (`_count_pair` is the one kernel call), a video is one download."""

    def _open(self, device, per_pair, specs):
        self.device = _device(device)
        self.per_pair = bool(per_pair)
        self.lib = hip.load()
        self._tables = pairtables.PairTables(self.device, self.per_pair, specs)

    _n = property(lambda self: self._tables.n)           # the pairs of the open video

    def add_pair(self, prev_frame, cur_frame, flow, mask=None, residual=None):
        """count one pair into the open video (opened by the first pair). mask: None or uint8 [H,W], `tc.flow_occlusion`'s codes;
        residual: None or a contiguous device uint8 [H,W] tensor that receives the residual image. Nothing is downloaded."""
        self._count_pair(cur_frame, prev_frame, flow, mask, residual, *self._tables.row())
        self._tables.n += 1

    def end_video(self, video_id=None):
        """the one download (and synchronisation) of the open video; returns its entry"""
        assert self._tables.n, 'no video is open'
        n, tables = self._tables.download()
        return self.add_tables(video_id, *tables, n)

    def add_video(self, frames, flows, video_id=None, masks=None, residuals=None):
        """frames: the frames of one video in order, uint8 [H,W,3]; flows: one per frame, flows[t] the flow of frame t to frame t-1
        (flows[0] is not used and may be None); masks, residuals: None or one entry (or None) per frame. Returns the video's entry."""
        assert not self._tables.n, 'a video opened by add_pair is not ended'
        if len(flows) != len(frames) or any(x is not None and len(x) != len(frames) for x in (masks, residuals)):
            raise ValueError('one flow (mask, residual) per frame, the first is not used: %d frames, %d flows' % (len(frames), len(flows)))
        if len(frames) < 2:
            return self.add_tables(video_id, *self._tables.zeros(), 0)
        for t in range(1, len(frames)):                  # no synchronisation between pairs
            self.add_pair(frames[t - 1], frames[t], flows[t], mask=None if masks is None else masks[t], residual=None if residuals is None else residuals[t])
        return self.end_video(video_id)

    def result(self):
        assert not self._tables.n, 'a video opened by add_pair is not ended'
        return super().result()


class PhotoEvaluator(_VideoPairs, PhotoStats):
    """The device side. `add_pair` counts one pair into tables that stay on the device (`vps_flow_photo`, no synchronisation between
    pairs); `end_video` is the ONE download of a video. per_pair=True: every pair gets its own row of the tables (in blocks of 16 rows,
    still one download), the video's tables are the sum of the rows and `result()['per_pair']` has the figures of every pair."""

    def __init__(self, device='cuda', thr=PHOTO_THR, per_pair=False):
        PhotoStats.__init__(self, thr)
        self._open(device, per_pair, [((COUNT_CELLS,), torch.int64), ((SUM_CELLS,), torch.float64)])

    def _count_pair(self, cur, prev, flow, mask, residual, counts, sums):
        _accumulate(self.lib, cur, prev, flow, mask, self.thr, counts, sums, None, residual, self.device)


def score_videos(evaluator, frames, flows, names, nframes_per_video, back_flows=None, map_dir=None, alpha=128, quality=90, entropy='host'):
    """What `--flow-photo` of the tools does with a run's decoded frames (BGR uint8 [H,W,3], videos one after the other,
    `nframes_per_video` each) and the flows kept for them (`flows[i]` = `pano_results['flow']` of frame i): every video through
    `add_pair`, one download per video. back_flows (`--tc-occlusion`): `back_flows[i]` = `flow_between(ref_img, img)` of frame i; the
    mask of `tc.flow_occlusion` then splits every pair into its visible and its masked group. Neither list is changed (the temporal
    consistency counts the same flows afterwards). map_dir (`--flow-photo-map`): the residual image of every pair, painted with
    `RESIDUAL_PALETTE`, blended over `frames[i]` by `render_overlay` and written as map_dir/<name>.jpg by a `DeviceJpegWriter`.
    Returns the written file names."""
    from . import tc
    from .postprocess import DeviceJpegWriter, overlay_name, render_overlay, video_name_of
    assert len(frames) == len(flows) == len(names) and (back_flows is None or len(back_flows) == len(frames))
    writer = DeviceJpegWriter(evaluator.device, quality=quality, entropy=entropy) if map_dir is not None else None
    out = []
    try:
        for v0 in range(0, len(frames), nframes_per_video):
            n = len(frames[v0:v0 + nframes_per_video])
            for j in range(1, n):
                i = v0 + j
                flow, _ = _flow_layout(flows[i], evaluator.device)
                mask = None if back_flows is None else tc.flow_occlusion(flow, _flow_layout(back_flows[i], evaluator.device)[0])
                res = torch.empty(flow.shape[:2], dtype=torch.uint8, device=evaluator.device) if writer is not None else None
                evaluator.add_pair(frames[i - 1], frames[i], flow, mask=mask, residual=res)
                if writer is not None:
                    out.append(overlay_name(map_dir, names[i]))
                    writer.submit(render_overlay(frames[i], residual_colour(res), alpha), out[-1])
            if n > 1:
                evaluator.end_video(video_name_of(names[v0:v0 + nframes_per_video], v0 // nframes_per_video))
    finally:
        if writer is not None:
            writer.close()
    return out


def write_outputs(result, out_dir):
    """flow-photo.txt and flow-photo.json in `out_dir`"""
    pairtables.write_result(result, out_dir, 'flow-photo', photo_text(result))


# ---------------------------------------------------------------------------------------------- the ternary census residual (row 3i)
def _census_figures(c):
    """one row of the table (or the sum of both) -> its figures"""
    n = int(c[0])
    out = {'n': n, 'ce_warp': _q(c[1], c[2]), 'ce_static': _q(c[3], c[4])}
    out['ratio'] = _q(out['ce_warp'], out['ce_static'])
    out['gain'] = out['ce_static'] - out['ce_warp']
    for i, lv in enumerate(CENSUS_LEVELS):
        out['above_%d' % lv] = _q(c[5 + i], n)
    out.update(helped=_q(c[8], n), hurt=_q(c[9], n), flagged=int(c[10]), flagged_share=_q(c[10], n), outside=int(c[11]), alone=int(c[12]))
    out['outside_share'] = _q(out['outside'], n + out['outside'] + out['alone'])
    return out


def census_from_tables(table):
    """One pair's or one set's int64 [2][13] table -> {'all': figures, 'visible': figures of row 0, 'masked': figures of row 1} as plain
    Python numbers; 'all' is the two rows added."""
    t = np.asarray(table, dtype=np.int64).reshape(2, CENSUS_CELLS)
    return {'all': _census_figures(t[0] + t[1]), 'visible': _census_figures(t[0]), 'masked': _census_figures(t[1])}


def _census_args(thr, eps):
    if not (isinstance(thr, (int, np.integer)) and not isinstance(thr, bool) and 0 <= int(thr) <= 100):
        raise ValueError('thr is an integer percent in 0 .. 100, got %r' % (thr,))
    if not (math.isfinite(float(eps)) and float(eps) >= 0):
        raise ValueError('eps is finite and not negative, got %r' % (eps,))
    return int(thr), float(eps)


class CensusStats:
    """Host side of the census evaluation: collects the downloaded tables of every video and turns them into the result. No device."""

    def __init__(self, thr=CENSUS_THR, eps=CENSUS_EPS):
        self.thr, self.eps = _census_args(thr, eps)
        self.table = np.zeros((2, CENSUS_CELLS), dtype=np.int64)
        self.videos = []
        self.npairs = 0

    def add_tables(self, video_id, table, npairs=1):
        """one video's table: int64 [2][13] of `npairs` pairs together, or [npairs][2][13], one per pair"""
        table = np.asarray(table, dtype=np.int64)
        pairs = None
        if table.ndim == 3:
            assert table.shape == (npairs, 2, CENSUS_CELLS), table.shape
            pairs = [dict(census_from_tables(table[i]), pair=i + 1) for i in range(npairs)]
            vt = table.sum(0)
        else:
            vt = table.reshape(2, CENSUS_CELLS).copy()
        self.table += vt
        self.npairs += npairs
        st = dict(census_from_tables(vt), video=len(self.videos) if video_id is None else video_id, pairs=npairs, table=vt, per_pair=pairs)
        self.videos.append(st)
        return st

    def result(self):
        """`census_from_tables` of the set with 'thr', 'eps', 'pairs', 'table' (as lists), 'per_video' and 'per_pair' (for the videos
        counted with per-pair rows): plain Python numbers, lists and strings"""
        res = census_from_tables(self.table)
        keep = ('all', 'visible', 'masked')
        res.update(thr=self.thr, eps=self.eps, pairs=self.npairs, table=[[int(v) for v in row] for row in self.table],
                   per_video=[dict({k: st[k] for k in keep}, video=st['video'], pairs=st['pairs']) for st in self.videos],
                   per_pair=[dict({k: p[k] for k in keep}, video=st['video'], pair=p['pair']) for st in self.videos for p in (st['per_pair'] or [])])
        return res


def census_text(result):
    """the text of flow-census.txt: per video and for the set one row per group (all, visible, masked) - the scored pixels, the census
    error warped and static, their ratio and gain, the shares x100 above 10 / 25 / 50 percent, helped, hurt and flagged, and the pixels
    not in view and in view without a counted neighbour"""
    width = 124
    head = '{:16s}| {:8s} {:>11s} {:>7s} {:>7s} {:>6s} {:>7s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s} {:>6s} {:>10s} {:>8s}'.format(
        'VIDEO', 'GROUP', 'N', 'CE-w', 'CE-s', 'RATIO', 'GAIN', '>10', '>25', '>50', 'HELP', 'HURT', 'FLAG', 'OUTSIDE', 'ALONE')

    def rows(name, r):
        out = []
        for grp in ('all',) + GROUPS:
            f = r[grp]
            out.append('{:16s}| {:8s} {:11d} {:7.4f} {:7.4f} {:6.3f} {:7.4f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:6.2f} {:10d} {:8d}'.format(
                name[:16], grp, f['n'], f['ce_warp'], f['ce_static'], f['ratio'], f['gain'], 100 * f['above_10'], 100 * f['above_25'],
                100 * f['above_50'], 100 * f['helped'], 100 * f['hurt'], 100 * f['flagged_share'], f['outside'], f['alone']))
        return out
    out = ['=' * width, head, '-' * width]
    for r in result.get('per_video', []):
        out += rows(str(r['video']), r)
    out += ['-' * width] + rows('All (%d)' % result['pairs'], result)
    out.append('thr {:d} %  eps {:g}  outside {:.2f} %'.format(result['thr'], result['eps'], 100 * result['all']['outside_share']))
    return '\n'.join(out) + '\n'


def _census_accumulate(lib, cur, prev, flow, mask, thr, eps, table, mask_out, residual, device):
    thr, eps = _census_args(thr, eps)
    flow, ld, H, W, cur, prev, mask = _pair_inputs(cur, prev, flow, mask, mask_out, residual, device)
    nbytes = int(lib.vps_flow_census_ws_bytes(H, W))
    hip.check(min(nbytes, 0), 'vps_flow_census_ws_bytes')
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)            # (stream-ordered: the allocator hands the block on only behind its last use)
    hip.check(lib.vps_flow_census(hip.ptr(cur), hip.ptr(prev), H, W, hip.ptr(flow), ld, 0, hip.ptr(mask), thr, eps, hip.ptr(table), hip.ptr(mask_out),
                                  hip.ptr(residual), hip.ptr(ws), nbytes, hip.stream_ptr()), 'vps_flow_census')


def flow_census(cur, prev, flow, mask=None, thr=CENSUS_THR, eps=CENSUS_EPS, table=None, mask_out=None, residual=None):
    """One pair through `vps_flow_census` on the current stream; nothing is downloaded or synchronised. The arguments of
    `flow_photometric`; thr: an integer percent in 0 .. 100, eps in units of g. table: None (a fresh zeroed table) or a contiguous device
    int64 [2,13] tensor the call ADDS to. mask_out may be `mask` itself. -> table."""
    if not (torch.is_tensor(flow) and flow.is_cuda):
        raise hip.VpsHipError('flow_census runs on the device (vps_flow_census); there is no CPU path')
    dev = flow.device
    if table is None:
        table = torch.zeros((2, CENSUS_CELLS), dtype=torch.int64, device=dev)
    elif not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int64 and table.is_contiguous() and table.numel() == 2 * CENSUS_CELLS):
        raise ValueError('table is a contiguous device int64 [2,%d] tensor' % CENSUS_CELLS)
    _census_accumulate(hip.load(), cur, prev, flow, mask, thr, eps, table, mask_out, residual, dev)
    return table


class CensusEvaluator(_VideoPairs, CensusStats):
    """The device side. `add_pair` counts one pair into a table that stays on the device (`vps_flow_census`, no synchronisation between
    pairs); `end_video` is the ONE download of a video. per_pair=True: every pair gets its own table (in blocks of 16, still one
    download), the video's table is their sum and `result()['per_pair']` has the figures of every pair."""

    def __init__(self, device='cuda', thr=CENSUS_THR, eps=CENSUS_EPS, per_pair=False):
        CensusStats.__init__(self, thr, eps)
        self._open(device, per_pair, [((2, CENSUS_CELLS), torch.int64)])

    def _count_pair(self, cur, prev, flow, mask, residual, table):
        _census_accumulate(self.lib, cur, prev, flow, mask, self.thr, self.eps, table, None, residual, self.device)


def write_census_outputs(result, out_dir):
    """flow-census.txt and flow-census.json in `out_dir`"""
    pairtables.write_result(result, out_dir, 'flow-census', census_text(result))
