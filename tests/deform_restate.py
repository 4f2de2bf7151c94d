"""Float64 restatement of the DCNv1 forward (mmdet/ops/dcn/src/deform_conv_cuda_kernel.cu:83-113,189-241), on the CPU, without any
project code: what tests/test_deform_conv_gpu.py compares the deformable kernels with.

  * the sampling position is formed as the kernels and the reference form it: ONE fp32 addition of the (integer) tap position and
    the fp32 offset. Everything after it is float64: floor, the four bilinear weights, the validity of the sample and of each
    corner, the blend and the contraction with the weights;
  * a sample that fails  -1 < h < H  &&  -1 < w < W  contributes exactly 0 whatever its offset is (NaN and +-inf fail the test):
    it is SELECTED away, never multiplied by zero;
  * a corner outside the image contributes 0.

Layouts are the reference's: x [N, C, H, W], offset [N, 2 * kh * kw, Ho, Wo] with (dh, dw) of tap t in channels 2 t, 2 t + 1,
weight [O, C, kh, kw]."""
import collections

import torch

Deform64 = collections.namedtuple('Deform64', 'out den cols32 valid')


def positions(offset, H, W, kh, kw, stride, padding):
    """-> h_im, w_im: fp32 [N, kh * kw, Ho, Wo], one fp32 addition each"""
    N, _, Ho, Wo = offset.shape
    assert offset.dtype == torch.float32 and offset.shape[1] == 2 * kh * kw
    ky = torch.arange(kh).repeat_interleave(kw).view(1, -1, 1, 1)
    kx = torch.arange(kw).repeat(kh).view(1, -1, 1, 1)
    by = (torch.arange(Ho).view(1, 1, Ho, 1) * stride - padding + ky).to(torch.float32)
    bx = (torch.arange(Wo).view(1, 1, 1, Wo) * stride - padding + kx).to(torch.float32)
    return by + offset[:, 0::2], bx + offset[:, 1::2]


def columns(x, offset, kh, kw, stride, padding):
    """-> col, colabs: float64 [N, tap, C, Ho, Wo] = sum over the corners of bw_c x_c resp. bw_c |x_c|; valid: bool [N, tap, Ho, Wo]"""
    N, C, H, W = x.shape
    h32, w32 = positions(offset, H, W, kh, kw, stride, padding)
    valid = (h32 > -1) & (w32 > -1) & (h32 < H) & (w32 < W)
    zero = torch.zeros((), dtype=torch.float64)
    h = torch.where(valid, h32.double(), zero)
    w = torch.where(valid, w32.double(), zero)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    hh, hw = 1.0 - lh, 1.0 - lw
    hl, wl = hl.long(), wl.long()
    hu, wu = hl + 1, wl + 1
    x64 = x.double()
    xa = x64.abs()
    T, Ho, Wo = h.shape[1:]
    col = torch.zeros(N, T, C, Ho, Wo, dtype=torch.float64)
    colabs = torch.zeros_like(col)
    for yy, xx, bw in ((hl, wl, hh * hw), (hl, wu, hh * lw), (hu, wl, lh * hw), (hu, wu, lh * lw)):
        ok = valid & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(N, 1, -1).expand(N, C, -1)
        bw = torch.where(ok, bw, zero).unsqueeze(2)                                        # [N, T, 1, Ho, Wo]
        for src, dst in ((x64, col), (xa, colabs)):
            v = src.reshape(N, C, H * W).gather(2, idx).view(N, C, T, Ho, Wo).permute(0, 2, 1, 3, 4)
            dst += torch.where(ok.unsqueeze(2), bw * v, zero)
    return col, colabs, valid


def deform_conv_f64(x, offset, weight, stride, padding):
    """-> Deform64: out float64 [N, O, Ho, Wo]; den = sum_k |w_k| * sum_corners bw_c |x_c|, the magnitude every error is measured
    against; cols32: the column matrix rounded to fp32 [N, tap, C, Ho, Wo] (for `accumulation_allowance`); valid [N, tap, Ho, Wo]"""
    assert x.dtype == torch.float32 and weight.dtype == torch.float32
    O, C, kh, kw = weight.shape
    col, colabs, valid = columns(x, offset, kh, kw, stride, padding)
    N, T, _, Ho, Wo = col.shape
    w64 = weight.double().permute(0, 2, 3, 1).reshape(O, T * C)
    out = torch.matmul(w64, col.view(N, T * C, Ho * Wo)).view(N, O, Ho, Wo)
    den = torch.matmul(w64.abs(), colabs.view(N, T * C, Ho * Wo)).view(N, O, Ho, Wo)
    return Deform64(out, den, col.float(), valid)


def accumulation_allowance(ref, weight):
    """err / den of a float32 CPU matmul of the restatement's fp32 columns against the float64 result: what fp32 accumulation costs on
    the reference's side, in the measure of the tests (taken over the elements with den > 0)"""
    O, C, kh, kw = weight.shape
    w32 = weight.permute(0, 2, 3, 1).reshape(O, kh * kw * C).contiguous()
    N, T, _, Ho, Wo = ref.cols32.shape
    got = torch.stack([(w32 @ ref.cols32[n].reshape(T * C, Ho * Wo)).view(O, Ho, Wo) for n in range(N)], 0)
    pos = ref.den > 0
    return float(((got.double() - ref.out).abs()[pos] / ref.den[pos]).max())


def brute_force(x, offset, weight, stride, padding):
    """the same, one sample at a time in Python floats (float64): for small maps only -> out [N, O, Ho, Wo]"""
    import math
    import numpy as np
    N, C, H, W = x.shape
    O, _, kh, kw = weight.shape
    _, _, Ho, Wo = offset.shape
    xn, wn = x.double().numpy(), weight.double().numpy()
    off = offset.numpy()
    out = np.zeros((N, O, Ho, Wo))
    for n in range(N):
        for oy in range(Ho):
            for ox in range(Wo):
                acc = np.zeros(O)
                for i in range(kh):
                    for j in range(kw):
                        t = i * kw + j
                        h = float(np.float32(oy * stride - padding + i) + off[n, 2 * t, oy, ox])
                        w = float(np.float32(ox * stride - padding + j) + off[n, 2 * t + 1, oy, ox])
                        if not (h > -1 and w > -1 and h < H and w < W):
                            continue
                        h0, w0 = math.floor(h), math.floor(w)
                        lh, lw = h - h0, w - w0
                        val = np.zeros(C)
                        for yy, xx, bw in ((h0, w0, (1 - lh) * (1 - lw)), (h0, w0 + 1, (1 - lh) * lw), (h0 + 1, w0, lh * (1 - lw)), (h0 + 1, w0 + 1, lh * lw)):
                            if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                                val += bw * xn[n, :, yy, xx]
                        acc += wn[:, :, i, j] @ val
                out[n, :, oy, ox] = acc
    return torch.from_numpy(out)
