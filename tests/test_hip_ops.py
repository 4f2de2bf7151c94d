"""GPU parity tests of the individual libvpship kernels (called through the C-ABI) against the CPU oracle
(`oracle/`, the restatement of the reference operators) or, for the dense fp32 contraction, plain PyTorch-CPU fp32.

Tolerances: the conv kernel is exact-fp32 MFMA (an fmaf chain) — it differs from the CPU only by summation
order: |err| <= 2e-5 * (1 + |ref|) scaled by sqrt(K)-ish magnitudes is ample; gather kernels 1e-5 abs.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O
from oracle import fusetrack as OF
from vps_amd import hip, nhwc

pytestmark = pytest.mark.gpu


def _cmp(got, ref, rtol=2e-5, atol=2e-5, what=''):
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    assert not bad.any(), '%s: %d/%d bad, max abs err %.3e (ref max %.3e)' % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(ref.abs().max()))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ conv family
CONV_CASES = [
    # cin, cout, k, stride, pad, H, W, act, bn, res
    (3, 64, 7, 2, 3, 64, 96, 'relu', True, False),      # ResNet stem / FlowNet conv1-like
    (64, 64, 1, 1, 0, 32, 48, 'relu', True, False),
    (64, 256, 1, 1, 0, 32, 48, 'relu', True, True),     # bottleneck conv3 + residual
    (64, 64, 3, 1, 1, 33, 47, 'relu', True, False),     # ragged M
    (128, 128, 3, 2, 1, 32, 48, 'relu', True, False),
    (256, 512, 1, 2, 0, 16, 24, 'none', True, False),   # downsample
    (6, 64, 3, 1, 1, 40, 56, 'leaky', False, False),    # FlowNetSD conv0 (cin pad 8)
    (11, 64, 3, 1, 1, 40, 56, 'leaky', False, False),   # Fusion conv0 (cin pad 12)
    (12, 64, 7, 2, 3, 64, 64, 'leaky', False, False),   # FlowNetS conv1
    (64, 128, 5, 2, 2, 32, 32, 'leaky', False, False),
    (194, 2, 3, 1, 1, 16, 24, 'none', False, False),    # predict_flow2 (cin not multiple of 4, cout 2)
    (256, 18, 3, 1, 1, 16, 24, 'none', False, False),   # DCN offset conv
    (512, 19, 1, 1, 0, 16, 24, 'none', False, False),   # conv_pred
    (339, 64, 3, 1, 1, 16, 24, 'leaky', False, False),  # LiteFlowNet estimator input
    (1024, 1024, 3, 1, 1, 4, 8, 'leaky', False, False), # conv6_1: deep, tiny M -> split-K
    (512, 512, 3, 2, 1, 16, 16, 'leaky', False, False), # split-K, stride 2
    (256, 36, 1, 1, 0, 7, 9, 'none', False, False),     # tile_n 64, tiny M
    # narrow outputs (exact-fp32 vector kernels in every mode): sliding-window 3x3 kernel with 1..5 channel slots per lane
    (16, 2, 3, 1, 1, 40, 56, 'none', False, False),     # 4 lanes per pixel
    (386, 2, 3, 1, 1, 16, 24, 'none', False, False),    # predict_flow3: two channel slots per lane
    (1026, 2, 3, 1, 1, 8, 13, 'none', False, False),    # predict_flow5: five slots, 76 KB of weights in LDS, ragged run
    (64, 3, 3, 1, 1, 16, 24, 'leaky', False, False),    # cout 3
    # narrow 1x1 / strided layers: the batched vector kernel (eight loads per lane in flight, 8 | 16 | 1 lanes per pixel, several rounds per wavefront)
    (256, 3, 1, 1, 0, 64, 99, 'none', False, False),    # RPN objectness
    (1024, 4, 1, 1, 0, 9, 13, 'relu', True, True),      # 32 slots over 16 lanes... four batches per pixel, BN + residual epilogue
    (6, 2, 3, 2, 1, 41, 57, 'leaky', False, False),     # stride 2, 2 lanes per pixel, ragged
    (2, 2, 5, 1, 2, 40, 56, 'none', False, False),      # one lane per pixel, 25 taps: four batches, the last one partly masked
    # whole 8x16 output patches, stride 1, 3x3, chunk-major k: the halo-staged kernel in the split-bf16 modes
    (64, 64, 3, 1, 1, 16, 32, 'relu', True, True),      # tile_n 64, residual
    (82, 16, 3, 1, 1, 24, 48, 'leaky', False, False),   # fusion conv (cin pad 84 -> 3 chunks, tile_n 32)
    (256, 256, 3, 1, 1, 8, 16, 'relu', True, False),    # tile_n 128, a single patch
    (194, 130, 3, 1, 1, 16, 16, 'none', False, False),  # ragged channel chunk, cout not a multiple of 32
    # enough 256-row tiles to fill the chip, 128-column tile: the 8-wave halo kernel (weights through LDS) in f16x3 / bf16x3
    (64, 128, 3, 1, 1, 256, 512, 'relu', True, True),   # 8x32 patches, residual + BN epilogue
    (82, 256, 3, 1, 1, 250, 500, 'leaky', False, False),  # overhanging patches (250 % 8, 500 % 32), ragged channel chunk, 2 column tiles
    # stride-2 layers with >= 256 tiles of 8x32 outputs (FlowNet conv2 / conv3, ResNet stage entries): the phase-split 8-wave halo
    # kernel in f16x3 / bf16x3 (the uniform-lead kernel with VPS_S2_HALO=0 in the environment)
    (64, 128, 5, 2, 2, 512, 512, 'leaky', False, False),
    (128, 256, 3, 2, 1, 500, 516, 'relu', True, True),   # overhanging patches, two column tiles, residual + BN epilogue
    (64, 64, 3, 2, 1, 500, 1030, 'leaky', False, False), # the 64-column variant of the phase-split kernel (FlowNetSD / Fusion conv1), overhanging patches
    # narrow outputs at sizes where a workgroup walks several runs (grid-stride loop, folding reduction over 64 / 16 / 4 lanes)
    (194, 2, 3, 1, 1, 64, 131, 'none', False, False),
    (64, 2, 3, 1, 1, 40, 57, 'leaky', False, False),
    (16, 2, 3, 1, 1, 130, 258, 'none', False, False),
    # 5..16 output channels on >= 256 patches of 8x32: the 16x16x32 kernel in f16x3 (overhanging patches, ragged channel chunk;
    # 10 channels: scalar stores and the channel guard; residual + BN epilogue)
    (82, 16, 3, 1, 1, 130, 520, 'leaky', False, False),
    (64, 10, 3, 1, 1, 136, 520, 'relu', True, True),
    # 64 output channels on a map with >= 256 patches of 8x32 (where a 64-column 8-wave instance was tried and dropped): overhanging patches, residual
    (96, 64, 3, 1, 1, 130, 520, 'relu', True, True),
    # thin-input layers on >= 512 patches: the thin-input kernel (csrc/conv_thin.hip) in f16x3 - all four instances, overhanging patches,
    # BN + residual epilogue on one of them (the ResNet stem has BN + ReLU)
    (6, 64, 3, 1, 1, 250, 530, 'leaky', False, False),
    (11, 64, 3, 1, 1, 256, 512, 'leaky', True, False),
    (3, 64, 7, 2, 3, 500, 1050, 'relu', True, False),
    (12, 64, 7, 2, 3, 250, 1100, 'leaky', False, False),
]


PRECS = [(hip.PREC_F32, 2e-5), (hip.PREC_BF16X3, 4e-4), (hip.PREC_BF16X6, 2e-5), (hip.PREC_F16X3, 2e-5)]


@pytest.mark.parametrize('prec,tol', PRECS, ids=['f32', 'bf16x3', 'bf16x6', 'f16x3'])
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'ci%d_co%d_k%d_s%d' % c[:4])
def test_conv2d_matches_torch_cpu(dev, case, prec, tol):
    cin, cout, k, stride, pad, H, W, act, bn, res = case
    x = _rand(1, cin, H, W, seed=1)
    w = _rand(cout, cin, k, k, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    b = None if bn else _rand(cout, seed=3, scale=0.1)
    ref = F.conv2d(x, w, b, stride=stride, padding=pad)
    bnd = None
    if bn:
        bnd = dict(weight=torch.rand(cout) + 0.5, bias=_rand(cout, seed=4, scale=0.1),
                   running_mean=_rand(cout, seed=5, scale=0.1), running_var=torch.rand(cout) + 0.5, eps=1e-5)
        ref = F.batch_norm(ref, bnd['running_mean'], bnd['running_var'], bnd['weight'], bnd['bias'], False, 0., 1e-5)
    r = None
    if res:
        r = _rand(*ref.shape, seed=6)
        ref = ref + r
    a = {'none': hip.ACT_NONE, 'relu': hip.ACT_RELU, 'leaky': hip.ACT_LEAKY}[act]
    ref = {'none': lambda t: t, 'relu': F.relu, 'leaky': lambda t: F.leaky_relu(t, 0.1)}[act](ref)
    pc = nhwc.PackedConv(w, b, bnd, stride=stride, padding=pad, act=a, slope=0.1, device=dev, prec=prec)
    ws = nhwc.Workspace(dev)
    xm = nhwc.from_nchw(x.to(dev))
    rm = nhwc.from_nchw(r.to(dev)) if res else None
    out = pc(xm, ws=ws, name='out', res=rm)
    torch.cuda.synchronize()
    _cmp(out.to_nchw(), ref, rtol=tol, atol=tol * max(1.0, float(ref.abs().max()) / 4), what='conv %s prec %d' % (case, prec))


def test_conv_writes_into_concat_window_and_reads_padded_window(dev):
    """producer writes channels [128,192) of a 194(+2 pad)-wide concat buffer; a consumer reads all 194."""
    H, W = 12, 20
    ws = nhwc.Workspace(dev)
    cat = ws.fmap('cat', 1, H, W, 194, ld=196)
    a = _rand(1, 128, H, W, seed=1); b_in = _rand(1, 32, H, W, seed=2); c = _rand(1, 2, H, W, seed=3)
    w = _rand(64, 32, 3, 3, seed=4, scale=0.1)
    pc = nhwc.PackedConv(w, None, None, 1, 1, device=dev)
    # fill windows 0..128 and 192..194 through the transpose kernel
    lib = hip.load()
    for t, off in ((a, 0), (c, 192)):
        td = t.to(dev).contiguous()
        hip.check(lib.vps_nchw_to_nhwc(hip.ptr(td), cat.ptr(), cat.ld, off, 1, t.shape[1], H, W, t.shape[1], hip.stream_ptr()), 't')
    pc(nhwc.from_nchw(b_in.to(dev)), out=cat.window(128, 64))
    full = torch.cat([a, F.conv2d(b_in, w, padding=1), c], 1)
    _cmp(cat.to_nchw(), full, what='concat buffer')
    w2 = _rand(2, 194, 3, 3, seed=5, scale=0.05)
    p2 = nhwc.PackedConv(w2, _rand(2, seed=6), None, 1, 1, device=dev)
    out = p2(cat, ws=ws, name='flow')
    _cmp(out.to_nchw(), F.conv2d(full, w2, p2.shift.cpu(), padding=1), what='predict_flow on concat')


@pytest.mark.parametrize('prec,tol', PRECS, ids=['f32', 'bf16x3', 'bf16x6', 'f16x3'])
@pytest.mark.parametrize('cin,cout,k,pad,H,W', [(1024, 512, 4, 1, 4, 8), (386, 64, 4, 1, 16, 24), (2, 2, 4, 1, 8, 12),
                                                (256, 256, 2, 0, 14, 14), (162, 16, 4, 1, 20, 28),
                                                # whole 8x16 patches per parity class: halo-staged kernel
                                                (386, 64, 4, 1, 16, 32), (162, 16, 4, 1, 8, 48), (128, 160, 4, 1, 24, 16),
                                                # 4 parity classes x 128 tiles of 8x32: the 8-wave halo kernel on a transposed conv
                                                (96, 128, 4, 1, 128, 256),
                                                # 16 output channels, 4 classes x 153 patches of 8x32: the 16x16x32 kernel (f16x3)
                                                (162, 16, 4, 1, 130, 260),
                                                # 64 output channels, 4 classes x 72 patches of 8x32 (4-wave halo kernel, ragged width)
                                                (96, 64, 4, 1, 64, 260),
                                                # the 2-channel up-flow layer on a map with several rounds per wavefront (batched narrow kernel, 4 classes in LDS)
                                                (2, 2, 4, 1, 130, 258), (34, 3, 4, 1, 20, 31)])
def test_conv_transpose_matches_torch_cpu(dev, cin, cout, k, pad, H, W, prec, tol):
    x = _rand(2 if k == 2 else 1, cin, H, W, seed=1)
    w = _rand(cin, cout, k, k, seed=2, scale=(1.0 / (cin * k)) ** 0.5)
    b = _rand(cout, seed=3, scale=0.1)
    ref = F.leaky_relu(F.conv_transpose2d(x, w, b, stride=2, padding=pad), 0.1)
    pc = nhwc.PackedConv(w, b, None, stride=2, padding=pad, act=hip.ACT_LEAKY, transposed=True, device=dev, prec=prec)
    out = pc(nhwc.from_nchw(x.to(dev)), ws=nhwc.Workspace(dev), name='o')
    _cmp(out.to_nchw(), ref, rtol=tol, atol=tol * max(1.0, float(ref.abs().max()) / 4), what='deconv')


@pytest.mark.parametrize('prec,tol', PRECS[1:], ids=['bf16x3', 'bf16x6', 'f16x3'])
def test_halo_conv_batch_and_concat_window(dev, prec, tol):
    """halo-staged kernel with N=2 images, reading a channel window of a wider buffer and writing into a concat window"""
    N, H, W = 2, 16, 32
    x = _rand(N, 96, H, W, seed=1); w = _rand(48, 96, 3, 3, seed=2, scale=0.05); b = _rand(48, seed=3, scale=0.1)
    ws = nhwc.Workspace(dev)
    src = ws.fmap('src', N, H, W, 128)                       # input lives in channels [32, 128) of a 128-wide buffer
    xd = x.to(dev)                                           # kept alive until the synchronize below
    hip.check(hip.load().vps_nchw_to_nhwc(hip.ptr(xd), src.ptr(), src.ld, 32, N, 96, H, W, 96, hip.stream_ptr()), 't')
    dst = ws.fmap('dst', N, H, W, 80)
    pc = nhwc.PackedConv(w, b, None, 1, 1, act=hip.ACT_LEAKY, slope=0.1, device=dev, prec=prec)
    pc(src.window(32, 96), out=dst.window(16, 48))
    torch.cuda.synchronize()
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.1)
    _cmp(dst.to_nchw()[:, 16:64], ref, rtol=tol, atol=tol * max(1.0, float(ref.abs().max()) / 4), what='halo conv window')
    full = dst.to_nchw()
    assert float(full[:, :16].abs().max()) == 0.0 and float(full[:, 64:].abs().max()) == 0.0


def test_fpn_topdown_residual_upsample(dev):
    """lateral conv + nearest x2 upsample-add fused through res_shift=1 (necks/fpn.py:108-111)"""
    x = _rand(1, 64, 16, 24, seed=1); top = _rand(1, 32, 8, 12, seed=2)
    w = _rand(32, 64, 1, 1, seed=3, scale=0.1); b = _rand(32, seed=4)
    ref = F.conv2d(x, w, b) + F.interpolate(top, scale_factor=2, mode='nearest')
    pc = nhwc.PackedConv(w, b, None, 1, 0, device=dev)
    out = pc(nhwc.from_nchw(x.to(dev)), ws=nhwc.Workspace(dev), name='o', res=nhwc.from_nchw(top.to(dev)), res_shift=1)
    _cmp(out.to_nchw(), ref, what='fpn lateral')


def test_linear_as_conv_with_nhwc_flatten(dev):
    R, C, S = 37, 16, 49
    feats_nchw = _rand(R, C, 7, 7, seed=1)
    w = _rand(24, C * S, seed=2, scale=0.05); b = _rand(24, seed=3)
    ref = F.relu(F.linear(feats_nchw.view(R, -1), w, b))
    pl = nhwc.pack_linear(w, b, act=hip.ACT_RELU, device=dev, chw=(C, S))
    nh = feats_nchw.permute(0, 2, 3, 1).contiguous().view(1, 1, R, S * C).to(dev)
    out = pl(nhwc.FMap(nh), ws=nhwc.Workspace(dev), name='fc')
    _cmp(out.t.view(R, 24), ref, what='linear')


@pytest.mark.parametrize('prec,tol', PRECS, ids=['f32', 'bf16x3', 'bf16x6', 'f16x3'])
@pytest.mark.parametrize('cin,cout,H,W', [(256, 256, 12, 20), (256, 128, 9, 13), (128, 128, 16, 16)])
def test_deform_conv_matches_oracle(dev, cin, cout, H, W, prec, tol):
    x = _rand(1, cin, H, W, seed=1)
    off = _rand(1, 18, H, W, seed=2, scale=1.5)
    w = _rand(cout, cin, 3, 3, seed=3, scale=(2.0 / (cin * 9)) ** 0.5)
    ref = O.deform_conv(x, off, w, 1, 1)
    pc = nhwc.PackedConv(w, None, None, 1, 1, device=dev, deform=True, prec=prec)
    out = pc(nhwc.from_nchw(x.to(dev)), ws=nhwc.Workspace(dev), name='o', offset=nhwc.from_nchw(off.to(dev)))
    _cmp(out.to_nchw(), ref, rtol=tol, atol=tol * max(1.0, float(ref.abs().max()) / 4), what='deform conv')


def test_deform_conv_256_column_tile_equals_the_128_column_tile(dev, monkeypatch):
    monkeypatch.setattr(nhwc, 'DCN256', [True])
    """Deformable layers with 256 output channels on maps of >= 256 pixel tiles run as ONE 128 x 256 block per pixel tile
    (vps_conv_desc.tile_n 256: the bilinear loader works once per pixel tile instead of twice). Every output element is the same
    chain of MFMA accumulations in either tiling -> bitwise equal to the 128-column launch, the GroupNorm sums of the epilogue too;
    against the oracle (dcn/functions/deform_conv.py:10-80 semantics) on a ragged map."""
    H, W = 181, 187                                    # 33847 pixels = 265 tiles of 128, the last one ragged
    x = _rand(1, 256, H, W, seed=1)
    off = _rand(1, 18, H, W, seed=2, scale=1.5)
    w = _rand(256, 256, 3, 3, seed=3, scale=(2.0 / (256 * 9)) ** 0.5)
    pc = nhwc.PackedConv(w, None, None, 1, 1, device=dev, deform=True, prec=hip.PREC_F16X3)
    xs, offs = nhwc.from_nchw(x.to(dev)), nhwc.from_nchw(off.to(dev))
    got = []
    for wide in (False, True):
        nhwc.DCN256[0] = wide
        ws = nhwc.Workspace(dev)
        slot = ws.get('gn', (nhwc.GN_REP, 64), dtype=torch.float64); slot.zero_()
        trace = []
        monkeypatch.setattr(nhwc, 'CONV_TRACE', trace)
        o = pc(xs, ws=ws, name='o', offset=offs, gn=(slot, 32))
        monkeypatch.setattr(nhwc, 'CONV_TRACE', None)
        assert pc.gn_fused and ('tile%d ' % (256 if wide else 128)) in trace[0][3], trace[0][3]
        got.append((o.t.clone(), slot.sum(dim=0).clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    ref = O.deform_conv(x, off, w, 1, 1)
    _cmp(nhwc.FMap(got[1][0], 256, 0).to_nchw(), ref, rtol=2e-5, atol=2e-5 * max(1.0, float(ref.abs().max()) / 4), what='deform conv, 256-column tile')


@pytest.mark.parametrize('prec', [hip.PREC_F16X3, hip.PREC_BF16X6], ids=['f16x3', 'bf16x6'])
@pytest.mark.parametrize('cin,cout,H,W', [(256, 256, 128, 160), (256, 128, 157, 211)])
def test_deform_conv_epilogue_takes_the_groupnorm_sums(dev, cin, cout, H, W, prec):
    """vps_conv_desc.gn_stats: the deformable conv's epilogue adds sum / sum of squares of each GroupNorm group of its output
    (groups of 8 resp. 4 channels) -> equal to the sums of the stored tensor, and GroupNorm+ReLU finished by vps_groupnorm_apply
    equals the two-pass vps_groupnorm_relu and torch (upsnetFPN.py:39-52). Split-K launches leave the slot alone."""
    x = _rand(1, cin, H, W, seed=1)
    off = _rand(1, 18, H, W, seed=2, scale=1.5)
    w = _rand(cout, cin, 3, 3, seed=3, scale=(2.0 / (cin * 9)) ** 0.5)
    g = torch.rand(cout) + 0.5; b = _rand(cout, seed=4, scale=0.2)
    ws = nhwc.Workspace(dev)
    pc = nhwc.PackedConv(w, None, None, 1, 1, device=dev, deform=True, prec=prec)
    xs, offs = nhwc.from_nchw(x.to(dev)), nhwc.from_nchw(off.to(dev))
    slot = ws.get('gn', (nhwc.GN_REP, 64), dtype=torch.float64); slot.zero_()
    raw = pc(xs, ws=ws, name='raw', offset=offs, gn=(slot, 32))
    assert pc.gn_fused
    o = raw.to_nchw().double().view(32, cout // 32, -1)
    sums = torch.stack([o.sum(dim=(1, 2)), (o * o).sum(dim=(1, 2))], dim=1).reshape(-1).cpu()
    got = slot.sum(dim=0).cpu()
    # lanes add their <= 8 values in fp32 before everything goes to double: errors relative to sum|v| resp. sum v^2
    scale = torch.stack([o.abs().sum(dim=(1, 2)), (o * o).sum(dim=(1, 2))], dim=1).reshape(-1).cpu()
    assert float(((got - sums).abs() / scale).max()) < 1e-6, (got[:6], sums[:6])
    gd, bd = g.to(dev), b.to(dev)
    fused = nhwc.groupnorm_relu(raw, ws.fmap('f', 1, H, W, cout), 32, gd, bd, 1e-5, slot, stats_ready=True).to_nchw()
    two = nhwc.groupnorm_relu(raw, ws.fmap('t', 1, H, W, cout), 32, gd, bd, 1e-5, ws.get('st2', (64,), dtype=torch.float64)).to_nchw()
    _cmp(fused, two, rtol=1e-6, atol=1e-6, what='fused vs two-pass groupnorm')
    _cmp(fused, F.relu(F.group_norm(raw.to_nchw().cpu(), 32, g, b, 1e-5)), rtol=1e-5, atol=1e-5, what='fused groupnorm vs torch')
    # a launch that is split over K keeps the two-pass route
    small = nhwc.from_nchw(x[:, :, :8, :16].contiguous().to(dev))
    slot.zero_()
    pc(small, ws=ws, name='raws', offset=nhwc.from_nchw(off[:, :, :8, :16].contiguous().to(dev)), gn=(slot, 32))
    assert not pc.gn_fused and float(slot.abs().max()) == 0.0


def test_f16x3_reports_operands_beyond_the_fp16_range(dev):
    """VPS_PREC_F16X3: activations above 65504 overflow fp16 -> the launch ORs bit 0 into vps_conv_desc.status and
    nhwc.check_f16_range raises; in range, wide dynamic range (1e-4 .. 3e4) and per-channel weight scales stay fp32-grade"""
    x = _rand(1, 64, 16, 32, seed=1) * torch.logspace(-4, 3.9, 64).view(1, 64, 1, 1)      # |x| up to ~3e4
    w = _rand(96, 64, 3, 3, seed=2, scale=0.05) * torch.logspace(-3, 2, 96).view(96, 1, 1, 1)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    den = F.conv2d(x.double().abs(), w.double().abs(), padding=1)
    pc = nhwc.PackedConv(w, None, None, 1, 1, device=dev, prec=hip.PREC_F16X3)
    nhwc.check_f16_range(dev)
    out = pc(nhwc.from_nchw(x.to(dev)), ws=nhwc.Workspace(dev), name='o').to_nchw().cpu().double()
    nhwc.check_f16_range(dev)                                   # in range: no report
    rel = float(((out - ref).abs() / den).max())
    f32 = float(((F.conv2d(x, w, padding=1).double() - ref).abs() / den).max())
    print('f16x3 error / sum|x||w| = %.2e (plain fp32 CPU conv: %.2e)' % (rel, f32))
    assert rel < 4e-7
    xb = x.clone(); xb[0, 5, 3, 7] = 7.0e4
    pc(nhwc.from_nchw(xb.to(dev)), ws=nhwc.Workspace(dev), name='o')
    with pytest.raises(hip.VpsHipError):
        nhwc.check_f16_range(dev)
    nhwc.check_f16_range(dev)                                   # the report clears the word


# ------------------------------------------------------------------------------------------------ flow ops
@pytest.mark.parametrize('H,W,mag', [(32, 48, 3.0), (17, 23, 40.0)])
def test_resample2d_nchw_api(dev, H, W, mag):
    img = _rand(2, 3, H, W, seed=1); flow = _rand(2, 2, H, W, seed=2, scale=mag)
    ref = O.resample2d(img, flow)
    a, f = img.to(dev), flow.to(dev)
    out = torch.empty_like(a)
    hip.check(hip.load().vps_resample2d(hip.tensor4_nchw(a), hip.tensor4_nchw(f), hip.tensor4_nchw(out), 2, 3, H, W,
                                        hip.stream_ptr()), 'resample2d')
    _cmp(out, ref, rtol=1e-6, atol=1e-6, what='resample2d')


def test_channelnorm(dev):
    x = _rand(2, 3, 20, 28, seed=1)
    a = x.to(dev); out = torch.empty(2, 1, 20, 28, device=dev)
    hip.check(hip.load().vps_channelnorm(hip.tensor4_nchw(a), hip.tensor4_nchw(out), 2, 3, 20, 28, hip.stream_ptr()), 'cn')
    _cmp(out, O.channelnorm(x), rtol=1e-6, atol=1e-7, what='channelnorm')


@pytest.mark.parametrize('C,H,W,md,s2', [(256, 12, 20, 20, 2), (256, 16, 24, 4, 1), (64, 9, 11, 4, 1), (256, 10, 16, 20, 2),
                                          (128, 7, 24, 20, 2), (256, 6, 8, 4, 1),
                                          # stride 1 on the half-wavefront kernel (corr_half.hip): one / two float4 per lane, a channel count
                                          # that leaves lanes idle, enough groups for several rounds per wavefront
                                          (128, 9, 12, 4, 1), (200, 10, 16, 4, 1), (256, 70, 132, 4, 1)])
def test_correlation_matches_oracle(dev, C, H, W, md, s2):
    a = _rand(1, C, H, W, seed=1); b = _rand(1, C, H, W, seed=2)
    ref = F.leaky_relu(O.correlation(a, b, md, 1, md, 1, s2), 0.1)
    D = (2 * (md // s2) + 1) ** 2
    ws = nhwc.Workspace(dev)
    out = ws.fmap('corr', 1, H, W, D)
    nhwc.correlation(nhwc.from_nchw(a.to(dev)), nhwc.from_nchw(b.to(dev)), out, md, s2, hip.ACT_LEAKY, 0.1)
    _cmp(out.to_nchw(), ref, rtol=1e-5, atol=1e-5, what='correlation')


@pytest.mark.parametrize('H,W', [(32, 48), (64, 36)])
def test_flow_stage_full_pixel_kernels(dev, H, W):
    """vps_flow_stage_full (whole 12-float pixels, FlowNetS input and FlowNetFusion input) == the channel-wise vps_flow_stage +
    vps_axpb route (same formulas, contracted differently by the compiler, then amplified by the image gradient in the warp: 2e-5), and == the torch / oracle composition of flownet2.py:142-187 (upsample, Resample2d, ChannelNorm)"""
    lib = hip.load()
    sp = hip.stream_ptr
    D = 20.0
    img = _rand(1, 6, H, W, seed=1, scale=1.0)
    fa = _rand(1, 2, H // 4, W // 4, seed=2, scale=0.2)
    fb = _rand(1, 2, H // 4, W // 4, seed=3, scale=60.0)
    ws = nhwc.Workspace(dev)
    x6 = ws.fmap('x6', 1, H, W, 6, ld=8); x6.t[..., :6] = img.permute(0, 2, 3, 1).to(dev)
    la, lb = nhwc.from_nchw(fa.to(dev)), nhwc.from_nchw(fb.to(dev))

    def stage(flow_lo, out, *a):
        hip.check(lib.vps_flow_stage(x6.ptr(), x6.ld, flow_lo.ptr(), flow_lo.ld, flow_lo.coff, H, W, a[0], a[1], a[2], out.ptr(), out.ld,
                                     a[3], a[4], a[5], a[6], a[7], a[8], sp()), 'stage')

    # FlowNetS input
    old = ws.fmap('old', 1, H, W, 12); new = ws.fmap('new', 1, H, W, 12)
    hip.check(lib.vps_axpb(x6.ptr(), x6.ld, 0, old.ptr(), old.ld, 0, x6.npix, 6, 1.0, 0.0, sp()), 'axpb')
    stage(la, old, 0, D, 0, 9, D, 6, 11, -1, -1)
    hip.check(lib.vps_flow_stage_full(x6.ptr(), 8, la.ptr(), la.ld, la.coff, la.ptr(), la.ld, la.coff, H, W, 0, D, new.ptr(), 12, sp()), 'full')
    _cmp(new.t, old.t.cpu(), rtol=2e-5, atol=2e-5, what='whole-pixel vs channel-wise stage')     # same formulas; the compiler contracts them differently
    up = F.interpolate(fa * D, scale_factor=4, mode='bilinear', align_corners=False)
    warped = O.resample2d(img[:, 3:], up)
    ref = torch.cat([img, warped, up / D, O.channelnorm(img[:, :3] - warped)], dim=1)
    _cmp(new.to_nchw(), ref, rtol=1e-5, atol=1e-5, what='FlowNetS input')
    # FlowNetFusion input
    old3 = ws.fmap('old3', 1, H, W, 11); new3 = ws.fmap('new3', 1, H, W, 11)
    stage(la, old3, 1, D, 0, 5, 0.0, -1, 10, 8, 0)
    stage(lb, old3, 1, D, 1, 3, 0.0, -1, 9, 7, -1)
    hip.check(lib.vps_flow_stage_full(x6.ptr(), 8, la.ptr(), la.ld, la.coff, lb.ptr(), lb.ld, lb.coff, H, W, 1, D, new3.ptr(), 12, sp()), 'full')
    _cmp(new3.t[..., :11], old3.t[..., :11].cpu(), rtol=2e-5, atol=2e-5, what='whole-pixel vs channel-wise fusion stage')
    assert float(new3.t[..., 11].abs().max()) == 0.0
    f2 = F.interpolate(fa * D, scale_factor=4, mode='nearest'); fd = F.interpolate(fb / D, scale_factor=4, mode='nearest')
    ref3 = torch.cat([img[:, :3], fd, f2, O.channelnorm(fd), O.channelnorm(f2), O.channelnorm(img[:, :3] - O.resample2d(img[:, 3:], fd)),
                      O.channelnorm(img[:, :3] - O.resample2d(img[:, 3:], f2))], dim=1)
    _cmp(new3.to_nchw(), ref3, rtol=1e-5, atol=1e-5, what='FlowNetFusion input')


def test_flow_warp_matches_grid_sample(dev):
    x = _rand(1, 64, 24, 40, seed=1); flow = _rand(1, 2, 24, 40, seed=2, scale=4.0)
    ref = OF.warping_layer(x, flow)
    ws = nhwc.Workspace(dev)
    out = nhwc.flow_warp(nhwc.from_nchw(x.to(dev)), nhwc.from_nchw(flow.to(dev)), ws.fmap('w', 1, 24, 40, 64))
    _cmp(out.to_nchw(), ref, rtol=1e-4, atol=1e-4, what='flow warp')


# ------------------------------------------------------------------------------------------------ nn ops
@pytest.mark.parametrize('mode,Hi,Wi,Ho,Wo', [('bilinear', 8, 12, 32, 48), ('nearest', 8, 12, 32, 48), ('bilinear', 32, 48, 8, 12),
                                               ('bilinear', 6, 10, 12, 20), ('nearest', 16, 24, 8, 12)])
def test_resize(dev, mode, Hi, Wi, Ho, Wo):
    x = _rand(1, 19, Hi, Wi, seed=1)
    ref = F.interpolate(x, size=(Ho, Wo), mode=mode, **({'align_corners': False} if mode == 'bilinear' else {})) * 0.25
    ws = nhwc.Workspace(dev)
    out = nhwc.resize(nhwc.from_nchw(x.to(dev)), ws.fmap('r', 1, Ho, Wo, 19), mode, 0.25)
    _cmp(out.to_nchw(), ref, rtol=1e-6, atol=1e-6, what='resize')


@pytest.mark.parametrize('mode', ['max', 'avg'])
def test_pool3x3s2(dev, mode):
    x = _rand(1, 64, 18, 26, seed=1)
    ref = F.max_pool2d(x, 3, 2, 1) if mode == 'max' else F.avg_pool2d(x, 3, 2, 1)
    ws = nhwc.Workspace(dev)
    out = nhwc.pool3x3s2(nhwc.from_nchw(x.to(dev)), ws.fmap('p', 1, 9, 13, 64), mode)
    _cmp(out.to_nchw(), ref, rtol=1e-6, atol=1e-6, what='pool')


def test_bfp_gather_scatter(dev):
    lv = [_rand(1, 32, 32 >> i, 64 >> i, seed=i) for i in range(5)]
    ref = OF.bfp_gather(lv)
    ws = nhwc.Workspace(dev)
    maps = [nhwc.from_nchw(t.to(dev)) for t in lv]
    out = nhwc.bfp_gather(maps, ws.fmap('g', 1, 32, 64, 32))
    _cmp(out.to_nchw(), ref, rtol=1e-6, atol=1e-6, what='gather')
    for i in range(5):
        r = F.adaptive_max_pool2d(ref, lv[i].shape[2:]) + lv[i]
        o = nhwc.bfp_scatter(out, maps[i], ws.fmap('s%d' % i, 1, 32 >> i, 64 >> i, 32))
        _cmp(o.to_nchw(), r, rtol=1e-6, atol=1e-6, what='scatter %d' % i)


def _ab_env(var, fn):
    """fn() under var=0 and var=1 (the kernel-family switches of round 6 are read per call) -> {'0': tensor, '1': tensor}"""
    outs, old = {}, os.environ.get(var)
    try:
        for mode in ('0', '1'):
            os.environ[var] = mode
            outs[mode] = fn()
    finally:
        if old is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = old
    return outs


@pytest.mark.parametrize('cin,cout,stride,H,W,res', [(64, 256, 1, 256, 512, 1), (64, 64, 1, 256, 512, 0), (128, 512, 1, 128, 256, 1), (256, 256, 1, 256, 512, 2),
                                                      (256, 512, 2, 256, 512, 0), (512, 256, 1, 250, 500, 0), (256, 128, 1, 255, 509, 1)])
def test_persistent_pointwise_kernel_is_bitwise_the_uniform_lead_kernel(dev, cin, cout, stride, H, W, res):
    """conv_pw_kernel (round 6: persistent blocks, loads across tile boundaries, counted stores) against conv_mfma_bf16q_kernel (VPS_PW=0):
    bitwise - two / four / eight / sixteen k-steps, 128- and 64-column tiles, stride 2, residual at the same size (res 1) and upsampled
    x2 (res 2: the FPN lateral), pixel counts that are no multiple of the tile (masked rows) - and against a fp64 GEMM"""
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    pc = nhwc.PackedConv(w, b, None, stride=stride, padding=0, act=hip.ACT_RELU, device=dev, prec=hip.PREC_F16X3)
    x = nhwc.FMap(torch.randn(1, H, W, cin, generator=g).to(dev), cin, 0)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rs = 1 if res == 2 else 0
    r = None
    if res:
        assert Ho % (1 << rs) == 0 and Wo % (1 << rs) == 0
        r = nhwc.FMap(torch.randn(1, Ho >> rs, Wo >> rs, cout, generator=g).to(dev), cout, 0)

    def run():
        pc.forget_launches()
        out = nhwc.FMap(torch.full((1, Ho, Wo, cout), 7.0, device=dev), cout, 0)
        pc(x, out=out, ws=nhwc.Workspace(dev), res=r, res_shift=rs)
        torch.cuda.synchronize()
        return out.t.clone()
    outs = _ab_env('VPS_PW', run)
    assert torch.equal(outs['0'], outs['1'])
    ref = x.t[:, ::stride, ::stride].reshape(-1, cin).double() @ w.view(cout, cin).t().double().to(dev) + b.double().to(dev)
    if r is not None:
        rr = r.t.repeat_interleave(2, 1).repeat_interleave(2, 2) if rs else r.t
        ref = ref + rr.reshape(-1, cout).double()
    ref = ref.clamp_min(0).float().view(1, Ho, Wo, cout)
    _cmp(outs['1'], ref, rtol=2e-5, atol=2e-5 * max(1.0, float(ref.abs().max()) / 4), what='pointwise conv')


@pytest.mark.parametrize('cin,cout,H,W,res', [(256, 256, 128, 256, False), (128, 128, 256, 512, False), (473, 256, 128, 256, False), (256, 256, 250, 500, True),
                                              (96, 128, 256, 512, False)])
def test_pipelined_8_wave_halo_kernel_is_bitwise_conv_mfma_h8(dev, cin, cout, H, W, res):
    """conv_mfma_h8p_kernel (round 6: weights three taps ahead through a ring of three LDS slots with the third plane derived at staging,
    activation rows half a chunk ahead, fragments one slab ahead across the barrier) against conv_mfma_h8_kernel (VPS_H8P=0): bitwise -
    3 .. 15 chunks, a channel count off the 32-grid (473: the last chunk is partly padding), ragged 8 x 32 patches, residual - and against
    F.conv2d in fp64 on a crop"""
    g = torch.Generator().manual_seed(cin + H)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    pc = nhwc.PackedConv(w, b, None, stride=1, padding=1, act=hip.ACT_LEAKY, device=dev, prec=hip.PREC_F16X3)
    cp = (cin + 3) // 4 * 4
    xt = torch.zeros(1, H, W, cp, device=dev)
    xt[..., :cin] = torch.randn(1, H, W, cin, generator=g).to(dev)
    x = nhwc.FMap(xt, cin, 0)
    r = nhwc.FMap(torch.randn(1, H, W, cout, generator=g).to(dev), cout, 0) if res else None

    def run():
        pc.forget_launches()
        out = nhwc.FMap(torch.full((1, H, W, cout), 7.0, device=dev), cout, 0)
        pc(x, out=out, ws=nhwc.Workspace(dev), res=r)
        torch.cuda.synchronize()
        return out.t.clone()
    outs = _ab_env('VPS_H8P', run)
    assert torch.equal(outs['0'], outs['1'])
    ch, cw = 40, 72
    ref = F.conv2d(xt[0, :ch + 1, :cw + 1, :cin].permute(2, 0, 1)[None].double(), w.double().to(dev), b.double().to(dev), padding=1)[0, :, :ch, :cw].permute(1, 2, 0)
    if r is not None:
        ref = ref + r.t[0, :ch, :cw].double()
    ref = F.leaky_relu(ref, 0.1).float()
    _cmp(outs['1'][0, :ch, :cw], ref, rtol=2e-5, atol=2e-5 * max(1.0, float(ref.abs().max()) / 4), what='3x3 conv, pipelined halo kernel')


@pytest.mark.parametrize('cin,cout,H,W', [(162, 16, 128, 256), (82, 12, 120, 250), (64, 8, 128, 256)])
def test_transposed_16_column_layer_with_the_four_classes_in_one_block_is_bitwise_the_class_launches(dev, cin, cout, H, W):
    """conv_mfma_n16t_kernel (round 6: a stride-2 transposed 4x4 layer with <= 16 output channels - FlowNetFusion deconv0 - stages its
    input patch once for all four parity classes) against the four class launches of conv_mfma_n16_kernel (VPS_N16T=0) - bitwise - and
    against F.conv_transpose2d; ragged patches, channel counts that are no multiple of 32 / 4 included"""
    w = _rand(cin, cout, 4, 4, seed=3, scale=(2.0 / (cin * 4)) ** 0.5)
    b = _rand(cout, seed=4, scale=0.1)
    x = _rand(1, cin, H, W, seed=5)
    ref = F.leaky_relu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1), 0.1).float()
    pc = nhwc.PackedConv(w, b, None, stride=2, padding=1, act=hip.ACT_LEAKY, transposed=True, device=dev, prec=hip.PREC_F16X3)
    xin = nhwc.from_nchw(x.to(dev))
    outs = {}
    old = os.environ.get('VPS_N16T')
    try:
        for mode in ('0', '1'):
            os.environ['VPS_N16T'] = mode
            pc.forget_launches()
            o = pc(xin, ws=nhwc.Workspace(dev), name='o')
            torch.cuda.synchronize()
            outs[mode] = o.t.clone()
            _cmp(o.to_nchw(), ref, rtol=2e-5, atol=2e-5 * max(1.0, float(ref.abs().max()) / 4), what='transposed 16-column layer, VPS_N16T=' + mode)
    finally:
        if old is None:
            os.environ.pop('VPS_N16T', None)
        else:
            os.environ['VPS_N16T'] = old
    assert torch.equal(outs['0'], outs['1'])


@pytest.mark.parametrize('cin,cout,k,tr,H,W', [(162, 32, 3, False, 128, 256), (100, 20, 3, False, 120, 250), (128, 32, 4, True, 128, 256), (64, 24, 3, False, 128, 256)])
def test_17_to_32_column_layers_on_the_two_column_block_kernel(dev, cin, cout, k, tr, H, W):
    """conv_mfma_n32_kernel (round 6: FlowNetFusion's 162->32 3x3 @512x1024 and 128->32 transposed layers - the 16-column structure with two
    column blocks per wave) against torch in fp64, and against the 32-column halo kernel it replaces (VPS_N32=0) at the fp32-grade tolerance
    (the two accumulate in different orders); ragged patches and channel counts off the 32 / 16 grid included"""
    w = _rand(*((cin, cout, k, k) if tr else (cout, cin, k, k)), seed=3, scale=(2.0 / (cin * (4 if tr else 9))) ** 0.5)
    b = _rand(cout, seed=4, scale=0.1)
    x = _rand(1, cin, H, W, seed=5)
    if tr:
        ref = F.leaky_relu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1), 0.1).float()
    else:
        ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.1).float()
    pc = nhwc.PackedConv(w, b, None, stride=2 if tr else 1, padding=1, act=hip.ACT_LEAKY, transposed=tr, device=dev, prec=hip.PREC_F16X3)
    xin = nhwc.from_nchw(x.to(dev))
    outs = {}
    old = os.environ.get('VPS_N32')
    try:
        for mode in ('0', '1'):
            os.environ['VPS_N32'] = mode
            pc.forget_launches()
            o = pc(xin, ws=nhwc.Workspace(dev), name='o')
            torch.cuda.synchronize()
            outs[mode] = o.to_nchw().cpu()
            _cmp(outs[mode], ref, rtol=2e-5, atol=2e-5 * max(1.0, float(ref.abs().max()) / 4), what='17..32-column layer, VPS_N32=' + mode)
    finally:
        if old is None:
            os.environ.pop('VPS_N32', None)
        else:
            os.environ['VPS_N32'] = old
    assert float((outs['0'] - outs['1']).abs().max()) <= 4e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize('C,H,W,L', [(256, 64, 128, 5), (32, 16, 48, 5), (64, 24, 40, 4), (32, 8, 12, 3), (96, 2, 6, 2)])
def test_bfp_scatter_all_levels_in_one_pass_is_bitwise_the_level_launches(dev, C, H, W, L):
    """vps_bfp_scatter_all (round 6: one pass over the refined map, 2 x 2 maxima level by level through LDS) against vps_bfp_scatter per
    level (bfp_tcea.py:139-147) - bitwise, values with ties, negative zeros and one -inf included; shapes it does not take are handed back"""
    g = torch.Generator().manual_seed(C + H)
    bsf = (torch.randn(1, H, W, C, generator=g) * 4).round() / 4                                # quarter steps: ties between window members
    bsf[0, 0, 0, :4] = -0.0; bsf[0, 0, 1, :4] = 0.0; bsf[0, 1, 1, 5] = float('-inf')
    x = nhwc.FMap(bsf.to(dev).contiguous())
    lv = [nhwc.FMap(torch.randn(1, H >> l, W >> l, C, generator=g).to(dev)) for l in range(L)]
    ws = nhwc.Workspace(dev)
    one = [ws.fmap('a%d' % l, 1, H >> l, W >> l, C) for l in range(L)]
    sep = [nhwc.bfp_scatter(x, lv[l], ws.fmap('b%d' % l, 1, H >> l, W >> l, C)) for l in range(L)]
    assert nhwc.bfp_scatter_all(x, lv, one) is one
    torch.cuda.synchronize()
    for l in range(L):
        assert torch.equal(one[l].t, sep[l].t), l
    # not the kernel's shapes: odd cell count / channel count that is no multiple of 32 -> None, nothing launched
    assert nhwc.bfp_scatter_all(nhwc.FMap(torch.zeros(1, 24, 40, 64, device=dev)), [nhwc.FMap(torch.zeros(1, 24 >> l, 40 >> l, 64, device=dev)) for l in range(5)],
                                [nhwc.FMap(torch.zeros(1, 24 >> l, 40 >> l, 64, device=dev)) for l in range(5)]) is None


@pytest.mark.parametrize('C,H,W,coff', [(256, 16, 24, 0), (256, 9, 7, 64), (64, 5, 33, 4)])
def test_tcea_temporal_and_modulate(dev, C, H, W, coff):
    """utils/tcea_modules.py:56-66 (per-frame correlation with the centre embedding -> sigmoid -> scale the frame) and :76-77
    (fea * sigmoid(att) * 2 + att_add) as the two kernels of necks._TCEAFusion, kernel level. The frames come in as channel
    windows of wider buffers, as the neck passes them (bsf is a window of the LiteFlowNet input buffer)."""
    emb = _rand(1, 2 * C, H, W, seed=1, scale=0.2)
    emb_ref = _rand(1, C, H, W, seed=2, scale=0.2)
    f0, f1 = _rand(1, C, H, W, seed=3), _rand(1, C, H, W, seed=4)
    cor = [torch.sigmoid((emb[:, i * C:(i + 1) * C] * emb_ref).sum(1, keepdim=True)) for i in range(2)]
    ref = torch.cat([f0 * cor[0], f1 * cor[1]], 1)
    ws = nhwc.Workspace(dev)
    wide = ws.fmap('wide', 1, H, W, C + coff + 12)
    wide.window(coff, C).t[..., coff:coff + C] = nhwc.from_nchw(f0.to(dev)).t
    out = nhwc.tcea_temporal(nhwc.from_nchw(emb.to(dev)), nhwc.from_nchw(emb_ref.to(dev)), wide.window(coff, C),
                             nhwc.from_nchw(f1.to(dev)), ws.fmap('al', 1, H, W, 2 * C))
    _cmp(out.to_nchw(), ref, rtol=1e-5, atol=1e-6, what='tcea temporal')
    # the sigmoid saturates cleanly (|logit| up to ~C * 25): no NaN, exact 0 / 1 limits like torch
    big = nhwc.tcea_temporal(nhwc.from_nchw((emb * 50).to(dev)), nhwc.from_nchw((emb_ref * 50).to(dev)), wide.window(coff, C),
                             nhwc.from_nchw(f1.to(dev)), ws.fmap('al2', 1, H, W, 2 * C))
    cor = [torch.sigmoid((emb[:, i * C:(i + 1) * C] * 50 * (emb_ref * 50)).sum(1, keepdim=True)) for i in range(2)]
    _cmp(big.to_nchw(), torch.cat([f0 * cor[0], f1 * cor[1]], 1), rtol=2e-3, atol=1e-6, what='tcea temporal saturated')   # a logit of magnitude ~1e3 carries ~1e-4 of summation-order noise
    fea, att, add = _rand(1, C, H, W, seed=5), _rand(1, C, H, W, seed=6, scale=3.0), _rand(1, C, H, W, seed=7)
    o = nhwc.tcea_modulate(nhwc.from_nchw(fea.to(dev)), nhwc.from_nchw(att.to(dev)), nhwc.from_nchw(add.to(dev)), ws.fmap('mod', 1, H, W, C))
    _cmp(o.to_nchw(), fea * torch.sigmoid(att) * 2 + add, rtol=1e-6, atol=1e-6, what='tcea modulate')


@pytest.mark.parametrize('C', [256, 128])
def test_groupnorm_relu(dev, C):
    x = _rand(1, C, 20, 28, seed=1, scale=2.0) + 0.5
    g = torch.rand(C) + 0.5; b = _rand(C, seed=2, scale=0.2)
    ref = F.relu(F.group_norm(x, 32, g, b, 1e-5))
    ws = nhwc.Workspace(dev)
    stats = ws.get('st', (64,), dtype=torch.float64)
    gd, bd = g.to(dev), b.to(dev)
    out = nhwc.groupnorm_relu(nhwc.from_nchw(x.to(dev)), ws.fmap('o', 1, 20, 28, C), 32, gd, bd, 1e-5, stats)
    _cmp(out.to_nchw(), ref, rtol=1e-5, atol=1e-5, what='groupnorm')
    # into a channel window of a wider buffer (float4 path: offset multiple of 4; scalar path: odd leading dimension)
    for ld, coff in ((C + 32, 16), (C + 7, 3)):
        wide = ws.fmap('w%d' % ld, 1, 20, 28, ld)
        nhwc.groupnorm_relu(nhwc.from_nchw(x.to(dev)), wide.window(coff, C), 32, gd, bd, 1e-5, stats)
        full = wide.to_nchw()
        _cmp(full[:, coff:coff + C], ref, rtol=1e-5, atol=1e-5, what='groupnorm window ld %d' % ld)
        assert float(full[:, :coff].abs().max()) == 0.0 and float(full[:, coff + C:].abs().max()) == 0.0


@pytest.mark.parametrize('C,Hi,Wi,mode', [(64, 33, 47, 0), (3, 32, 48, 1), (8, 16, 24, 1), (6, 17, 9, 0)])
def test_pool3x3s2_vector_and_scalar_paths(dev, C, Hi, Wi, mode):
    x = _rand(2, C, Hi, Wi, seed=3)
    ref = F.max_pool2d(x, 3, 2, 1) if mode == 0 else F.avg_pool2d(x, 3, 2, 1, count_include_pad=True)
    ws = nhwc.Workspace(dev)
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    out = nhwc.pool3x3s2(nhwc.from_nchw(x.to(dev)), ws.fmap('p', 2, Ho, Wo, C), mode='max' if mode == 0 else 'avg')
    _cmp(out.to_nchw(), ref, rtol=1e-6, atol=1e-6, what='pool')


@pytest.mark.parametrize('C,mode', [(128, 'bilinear'), (2, 'bilinear'), (19, 'bilinear'), (32, 'nearest'), (3, 'nearest')])
def test_resize_vector_and_scalar_paths(dev, C, mode):
    x = _rand(1, C, 12, 20, seed=4)
    ref = F.interpolate(x, size=(48, 80), mode=mode, align_corners=False) if mode == 'bilinear' else F.interpolate(x, size=(48, 80), mode=mode)
    ws = nhwc.Workspace(dev)
    out = nhwc.resize(nhwc.from_nchw(x.to(dev)), ws.fmap('r', 1, 48, 80, C), mode)
    _cmp(out.to_nchw(), ref, rtol=1e-6, atol=1e-6, what='resize')


# ------------------------------------------------------------------------------------------------ detection ops
def _rand_rois(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    cx = torch.rand(n, generator=g) * W; cy = torch.rand(n, generator=g) * H
    s = torch.exp(torch.rand(n, generator=g) * math_log(16, 512))
    ar = torch.exp((torch.rand(n, generator=g) - 0.5))
    w = s * ar; h = s / ar
    b = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    b[:, 0::2] = b[:, 0::2].clamp(0, W - 1); b[:, 1::2] = b[:, 1::2].clamp(0, H - 1)
    return torch.cat([torch.zeros(n, 1), b], 1)


def math_log(lo, hi):
    import math
    return math.log(hi / lo)


@pytest.mark.parametrize('P', [7, 14])
def test_roi_align_multilevel(dev, P):
    H, W = 256, 512
    feats = [_rand(1, 32, H // s, W // s, seed=s) for s in (4, 8, 16, 32)]
    rois = _rand_rois(200, H, W, seed=3)
    ref = OF.roi_extract(feats, rois, P)
    maps = [nhwc.from_nchw(f.to(dev)) for f in feats]
    out = nhwc.roi_align(maps, [4, 8, 16, 32], rois.to(dev), P)
    _cmp(out.permute(0, 3, 1, 2), ref, rtol=5e-5, atol=5e-5, what='roi align')


def test_nms_batched_matches_oracle(dev):
    lib = hip.load()
    nb, nmax = 3, 700
    counts = [700, 333, 64]
    boxes = torch.zeros(nb, nmax, 5)
    keeps_ref = []
    for i, n in enumerate(counts):
        r = _rand_rois(n, 300, 500, seed=10 + i)[:, 1:]
        sc = torch.rand(n, generator=torch.Generator().manual_seed(20 + i))
        sc, order = torch.sort(sc, descending=True)
        d = torch.cat([r[order], sc[:, None]], 1)
        boxes[i, :n] = d
        keeps_ref.append(O._greedy_nms_sorted(d[:, :4].numpy(), 0.5))
    bd = boxes.to(dev)
    cd = torch.tensor(counts, dtype=torch.int32, device=dev)
    cb = (nmax + 63) // 64
    mask = torch.empty(nb * nmax * cb, dtype=torch.int64, device=dev)
    keep = torch.full((nb, nmax), -1, dtype=torch.int32, device=dev)
    nkeep = torch.zeros(nb, dtype=torch.int32, device=dev)
    hip.check(lib.vps_nms_batched(hip.ptr(bd), nb, nmax, hip.ptr(cd), 0.5, hip.ptr(mask), hip.ptr(keep), hip.ptr(nkeep),
                                  hip.stream_ptr()), 'nms')
    nk = nkeep.cpu().numpy(); kp = keep.cpu().numpy()
    for i in range(nb):
        assert nk[i] == len(keeps_ref[i])
        assert np.array_equal(kp[i, :nk[i]], keeps_ref[i])


def test_delta2bbox_overlaps_softmax(dev):
    lib = hip.load()
    n = 500
    anchors = _rand_rois(n, 256, 512, seed=1)[:, 1:]
    deltas = _rand(n, 4, seed=2, scale=0.5); scores = torch.rand(n)
    ref = torch.cat([OF.delta2bbox(anchors, deltas, (0, 0, 0, 0), (1, 1, 1, 1), (256, 512)), scores[:, None]], 1)
    out = torch.empty(n, 5, device=dev)
    ad, dd, sd_ = anchors.to(dev), deltas.to(dev), scores.to(dev)   # keep the device tensors alive across the launch
    hip.check(lib.vps_delta2bbox(hip.ptr(ad), hip.ptr(dd), hip.ptr(sd_), hip.ptr(out), n,
                                 1., 1., 1., 1., 256., 512., hip.stream_ptr()), 'd2b')
    _cmp(out, ref, rtol=1e-5, atol=1e-4, what='delta2bbox')
    a = _rand_rois(40, 256, 512, seed=3)[:, 1:]; b = _rand_rois(70, 256, 512, seed=4)[:, 1:]
    o = torch.empty(40, 70, device=dev)
    a_d, b_d = a.to(dev), b.to(dev)
    hip.check(lib.vps_bbox_overlaps(hip.ptr(a_d), 4, 40, hip.ptr(b_d), 4, 70, hip.ptr(o), hip.stream_ptr()), 'iou')
    _cmp(o, OF.bbox_overlaps(a, b), rtol=1e-6, atol=1e-7, what='iou')
    x = _rand(300, 9, seed=5, scale=3.0)
    for mode, fn in ((0, F.softmax), (1, F.log_softmax)):
        o = torch.empty(300, 9, device=dev)
        xd = x.to(dev)
        hip.check(lib.vps_row_softmax(hip.ptr(xd), hip.ptr(o), 300, 9, mode, hip.stream_ptr()), 'sm')
        _cmp(o, fn(x, dim=1), rtol=1e-5, atol=1e-6, what='softmax')


@pytest.mark.parametrize('quant', [0.0, 0.5, 1e9], ids=['continuous', 'ties', 'constant'])
def test_rpn_select_matches_topk_gather_decode(dev, quant):
    """vps_rpn_select (one launch: sigmoid, top nms_pre per level, gathers, delta2bbox) against the chain it replaces
    (rpn_head.py:62-91): torch sigmoid / stable descending sort on the device + gen anchors + vps_delta2bbox. Levels: one
    below nms_pre (kept whole), one above the 8192-key sort buffer (radix select), one in between; logits quantised to force
    exactly tied scores (ascending position among equals, also across the threshold) and a constant map (every score tied)."""
    from ctypes import c_float, c_int32, c_void_p
    from vps_amd import heads as HD
    lib = hip.load()
    A, nms_pre = 3, 1000
    shapes = [(96, 160), (40, 72), (16, 18)]
    strides = [4., 8., 16.]
    nlv = len(shapes)
    base = torch.stack([HD.gen_base_anchors(int(s), (8,), (0.5, 1.0, 2.0)) for s in strides]).to(dev).contiguous()      # [nlv, A = 3, 4]
    assert base.shape == (nlv, A, 4)
    cls_t, reg_t = [], []
    for li, (H, W) in enumerate(shapes):
        c = _rand(H, W, 4, seed=10 + li, scale=2.0)
        if quant >= 1e9:
            c = torch.zeros_like(c) + 0.25
        elif quant > 0:
            c = torch.round(c / quant) * quant
        cls_t.append(c.to(dev).contiguous()); reg_t.append(_rand(H, W, 12, seed=20 + li, scale=0.3).to(dev).contiguous())
    boxes = torch.full((nlv, nms_pre, 5), -1.0, device=dev)
    cp = (c_void_p * nlv)(*[c.data_ptr() for c in cls_t]); cl = (c_int32 * nlv)(*[4] * nlv)
    rp = (c_void_p * nlv)(*[r.data_ptr() for r in reg_t]); rl = (c_int32 * nlv)(*[12] * nlv)
    Hs = (c_int32 * nlv)(*[h for h, _ in shapes]); Ws = (c_int32 * nlv)(*[w for _, w in shapes])
    st = (c_float * nlv)(*strides); stds = (c_float * 4)(1., 1., 1., 1.)
    keys = torch.empty(sum(h * w * A for h, w in shapes), dtype=torch.int32, device=dev)
    hist = torch.zeros(nlv * 4096, dtype=torch.int32, device=dev)
    for _ in range(2):          # twice: the launch must leave its histogram scratch zero
        hip.check(lib.vps_rpn_select(cp, cl, rp, rl, Hs, Ws, st, nlv, A, hip.ptr(base), nms_pre, stds, 384., 640., hip.ptr(keys), hip.ptr(hist),
                                     hip.ptr(boxes), hip.stream_ptr()), 'vps_rpn_select')
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0
    for li, (H, W) in enumerate(shapes):
        scores = cls_t[li][..., :A].reshape(-1).sigmoid()
        deltas = reg_t[li][..., :4 * A].reshape(-1, 4)
        sx = torch.arange(0, W, dtype=torch.float32) * strides[li]; sy = torch.arange(0, H, dtype=torch.float32) * strides[li]
        xx = sx.repeat(H); yy = sy.view(-1, 1).repeat(1, W).view(-1)
        anchors = (base[li].cpu()[None] + torch.stack([xx, yy, xx, yy], -1)[:, None, :]).view(-1, 4).to(dev)
        sc, order = torch.sort(scores, descending=True, stable=True)
        n = min(scores.numel(), nms_pre)
        order = order[:n]
        d_, a_, s_ = deltas[order].contiguous(), anchors[order].contiguous(), sc[:n].contiguous()
        ref = torch.zeros(nms_pre, 5, device=dev)
        hip.check(lib.vps_delta2bbox(hip.ptr(a_), hip.ptr(d_), hip.ptr(s_), hip.ptr(ref), n, 1., 1., 1., 1., 384., 640., hip.stream_ptr()), 'd2b')
        torch.cuda.synchronize()
        got = boxes[li].cpu(); ref = ref.cpu()
        assert torch.equal(got[:, 4], ref[:, 4]), 'level %d: scores / selection differ (first at %s)' % (li, torch.nonzero(got[:, 4] != ref[:, 4])[:3].flatten().tolist())
        assert torch.equal(got, ref), 'level %d: decoded boxes differ, max %.3e' % (li, float((got - ref).abs().max()))


# ------------------------------------------------------------------------------------------------ reference-named operator API
def test_reference_named_operator_wrappers(dev):
    """vps_amd/operators.py: the reference's operator classes (NCHW signatures) backed by the C-ABI"""
    from vps_amd import operators as P
    img = _rand(1, 3, 24, 32, seed=1); flow = _rand(1, 2, 24, 32, seed=2, scale=2.0)
    _cmp(P.Resample2d()(img.to(dev), flow.to(dev)), O.resample2d(img, flow), 1e-6, 1e-6, 'Resample2d')
    _cmp(P.ChannelNorm()(img.to(dev)), O.channelnorm(img), 1e-6, 1e-7, 'ChannelNorm')
    a = _rand(1, 64, 10, 12, seed=3); b = _rand(1, 64, 10, 12, seed=4)
    _cmp(P.Correlation(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1)(a.to(dev), b.to(dev)),
         O.correlation(a, b, 4, 1, 4, 1, 1), 1e-5, 1e-5, 'Correlation')
    f = _rand(1, 16, 32, 48, seed=5); rois = _rand_rois(30, 128, 192, seed=6)
    _cmp(P.RoIAlign(7, 1 / 4.0, 2)(f.to(dev), rois.to(dev)), O.roi_align(f, rois, 7, 0.25, 2), 5e-5, 5e-5, 'RoIAlign')
    x = _rand(1, 32, 10, 14, seed=7); off = _rand(1, 18, 10, 14, seed=8)
    dc = P.DeformConv(32, 64, 3, padding=1)
    _cmp(dc(x.to(dev), off.to(dev)), O.deform_conv(x, off, dc.weight.detach(), 1, 1), 2e-5, 2e-5, 'DeformConv')
    d = torch.cat([_rand_rois(200, 100, 150, seed=9)[:, 1:], torch.rand(200, 1)], 1)
    kept, inds = P.nms(d.to(dev), 0.5)
    assert torch.equal(inds.cpu(), O.nms_mmdet(d, 0.5)[1])
    assert P.gpu_nms_wrapper(0.5, 0)(d.numpy()) == O.nms_upsnet(d.numpy(), 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize('box', [(10, 20, 70, 56), (-15, -9, 120, 90), (300, 100, 1323, 333), (5, 5, 5, 5), (1900, 900, 2100, 1100), (40, 40, 67, 67)])
def test_mask_removal_device_resize_equals_torch_bilinear(dev, box):
    """the cv2.resize(INTER_LINEAR) of mask_removal.py:66-70 as the MaskRemoval kernels evaluate it per pixel (csrc/pan_ops.hip:
    resized_logit) against an INDEPENDENT implementation of the same sampling rule - F.interpolate(bilinear, align_corners=False) -
    (VERDICT r4 next #5a): the count of positive pixels inside the clipped box, the overlap count against an occupancy plane, and the
    committed occupancy agree except at pixels whose logit is within the fp32 coordinate rounding of zero"""
    import torch.nn.functional as F
    lib = hip.load()
    H, W, S = 1024, 2048, 28
    g = torch.Generator().manual_seed(box[0] * 31 + box[3])
    m28 = (torch.randn(S, S, generator=g) * 3).to(dev)
    x1, y1, x2, y2 = box
    w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    ref = F.interpolate(m28[None, None].cpu(), size=(h, w), mode='bilinear', align_corners=False)[0, 0]
    cx0, cx1, cy0, cy1 = max(x1, 0), min(x2 + 1, W), max(y1, 0), min(y2 + 1, H)
    crop = ref[cy0 - y1:cy1 - y1, cx0 - x1:cx1 - x1]
    unsure = int((crop.abs() <= 7e-6 * float(m28.abs().max())).sum())
    occ = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    occ[::2] = 1                                                                       # every other row is occupied
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    hip.check(lib.vps_mask_count(hip.ptr(m28), S, x1, y1, x2, y2, H, W, hip.ptr(occ), hip.ptr(counts), hip.stream_ptr()), 'vps_mask_count')
    pos = crop > 0
    want_ms = int(pos.sum())
    want_ov = int((pos & (occ[cy0:cy1, cx0:cx1].cpu() >= 1)).sum())
    ms, ov = [int(v) for v in counts.cpu()]
    assert abs(ms - want_ms) <= unsure and abs(ov - want_ov) <= unsure, (ms, want_ms, ov, want_ov, unsure)
    # commit with a threshold that keeps the box: the occupancy plane gains exactly the positive pixels
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    occ.zero_()
    hip.check(lib.vps_mask_commit(hip.ptr(m28), S, x1, y1, x2, y2, H, W, hip.ptr(occ), hip.ptr(counts), 2.0, hip.ptr(flag), hip.stream_ptr()), 'vps_mask_commit')
    torch.cuda.synchronize()
    if want_ms > unsure:
        assert int(flag.item()) == 1
        got = occ[cy0:cy1, cx0:cx1].cpu() >= 1
        assert int((got != pos).sum()) <= unsure
        assert int(occ.sum().item()) == int(got.sum())                                 # nothing outside the clipped box


@pytest.mark.gpu
@pytest.mark.parametrize('n,seed', [(1, 0), (12, 1), (60, 2), (100, 3), (100, 4), (100, 5)])
def test_mask_removal_one_launch_equals_the_level_launches(dev, n, seed):
    """vps_mask_removal_hist (round 6 default: per-pixel box patterns, one wavefront per class, no chain) and vps_mask_removal_dep (one
    workgroup per box, waits on the boxes it depends on; round 5) against the per-level launches (vps_mask_level) and the
    one-workgroup-per-class walk (vps_mask_removal): identical kept lists and instance tables on crowded lists (up to 100 boxes of 2..8
    classes, long same-class overlap chains, boxes overhanging every edge, 1-pixel boxes; 100 boxes of ONE class: the two-pass walk of ranks 0..63 | 64..99)"""
    import ctypes
    from vps_amd import panoptic_ops as P
    H, W, S = 1024, 2048, 28
    rg = np.random.default_rng(seed)
    ncls = 1 if seed == 5 else 2 if seed % 2 else 8
    cx = rg.uniform(0, W, n); cy = rg.uniform(0, H, n)
    bw = np.exp(rg.uniform(np.log(2), np.log(900), n)); bh = np.exp(rg.uniform(np.log(2), np.log(600), n))
    rows = np.zeros((n, 8), dtype=np.float32)
    rows[:, 1] = cx - bw / 2; rows[:, 2] = cy - bh / 2; rows[:, 3] = cx + bw / 2; rows[:, 4] = cy + bh / 2
    rows[:, 1:5] += rg.uniform(-40, 40, (n, 4)).astype(np.float32) * (rg.random((n, 1)) < 0.2)        # some overhang the image
    if n > 3:
        rows[3, 3], rows[3, 4] = rows[3, 1], rows[3, 2]                                                # a 1-pixel box
    rows[:, 5] = np.sort(rg.uniform(0.6, 1.0, n))[::-1]
    rows[:, 6] = rg.integers(1, ncls + 1, n)
    rows[:, 7] = np.arange(n)
    rows_d = torch.from_numpy(rows).to(dev)
    masks = (torch.from_numpy(rg.standard_normal((n, S, S)).astype(np.float32)) * 2 + 0.6).to(dev)
    cm = {c: 10 + c for c in range(1, ncls + 1)}
    res = {}
    old = P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH
    old_pairs = P.HIST_MAX_PAIRS
    P.HIST_MAX_PAIRS = 10 ** 9           # every list through the pattern kernels here (the detector keeps lists with > 200 intersecting pairs on `dep`)
    try:
        for mode in ('hist', 'dep', 'level', 'single'):
            P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH = mode, mode == 'single'
            ws = nhwc.Workspace(dev)
            out = P.MaskRemoval(0.3)(rows, rows_d, masks, (H, W), ws, cm)
            torch.cuda.synchronize()
            kinfo = out['kinfo'].cpu().numpy()
            assert kinfo[2] == 0, (mode, kinfo)
            k = int(kinfo[0])
            res[mode] = (k, out['keep'][:k].cpu().numpy().copy(), bytes(out['inst'].cpu().numpy()[:k * ctypes.sizeof(hip.PanInst)]),
                         ws.bufs['mr.occ'].ne(0).cpu().numpy().copy(), 'mr.hist' in ws.bufs)
    finally:
        P.MASK_REMOVAL_MODE, P.MASK_REMOVAL_SINGLE_LAUNCH = old
        P.HIST_MAX_PAIRS = old_pairs
    for mode in ('level', 'single'):
        assert res['dep'][0] == res[mode][0], (mode, res['dep'][0], res[mode][0])
        assert np.array_equal(res['dep'][1], res[mode][1]) and res['dep'][2] == res[mode][2], mode
        assert np.array_equal(res['dep'][3], res[mode][3]), mode                   # the occupancy planes (as "occupied or not")
    assert res['hist'][0] == res['level'][0] and np.array_equal(res['hist'][1], res['level'][1]) and res['hist'][2] == res['level'][2]
    assert res['hist'][4], 'the pattern kernels ran (<= 127 boxes per class)'
    assert 1 <= res['dep'][0] <= n


@pytest.mark.gpu
def test_mask_removal_patterns_table_full_status_and_bounds(dev):
    """vps_mask_removal_hist: a full pattern table raises status bit 2 (forced: VPS_MR_HIST_CAP=1 on a list with several distinct overlap
    patterns) - the bit the detector recovers from; the undisturbed call on the same list keeps box 0 only (every later box overlaps it
    entirely); argument bounds (scratch too small, more than 32 classes)"""
    import ctypes
    lib = hip.load()
    H, W, n, S = 256, 512, 24, 28
    boxes = torch.tensor([[10 + i, 10 + i, 200 + i, 200 + i] for i in range(n)], dtype=torch.int32, device=dev)
    cls0 = torch.zeros(n, dtype=torch.int32, device=dev)
    midx = torch.arange(n, dtype=torch.int32, device=dev)
    rank = torch.arange(n, dtype=torch.int32, device=dev)
    scratch = torch.zeros(n + 2 + 2 * 4096, dtype=torch.int32, device=dev)
    flags = torch.full((n,), 7, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lg = torch.ones(n, S, S, device=dev)
    call = lambda ncls=1, nbytes=None, mr=n - 1: lib.vps_mask_removal_hist(hip.ptr(lg), S, hip.ptr(boxes), hip.ptr(cls0), hip.ptr(midx), hip.ptr(rank), mr, n, ncls, H, W,
                                                                  hip.ptr(scratch), scratch.numel() * 4 if nbytes is None else nbytes, ctypes.c_double(0.3),
                                                                  hip.ptr(flags), hip.ptr(status), hip.stream_ptr())
    assert call(33) == -1001 and call(1, 64) == -1002 and call(1, None, 127) == -1003
    assert call() == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(flags[0].item()) == 1 and int(flags[1:].sum().item()) == 0
    assert int(scratch[0].item()) == 191 * 191                                       # mask_sum of box 0: its whole clipped rectangle
    old = os.environ.get('VPS_MR_HIST_CAP')
    os.environ['VPS_MR_HIST_CAP'] = '1'
    try:
        assert call() == 0
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop('VPS_MR_HIST_CAP', None)
        else:
            os.environ['VPS_MR_HIST_CAP'] = old
    assert int(status.item()) & 4


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['plain', 'pad200', 'pad800'])
def test_flow_prep_pad_in_isolation(dev, case):
    """SURVEY 8(a) row a1 (VERDICT r5 missing #5): vps_flow_prep_pad - `denormalize` of both frames (utils/flow_utils.py:5-10), the zero
    pad of the two special sizes (panoptic_fusetrack.py:125-128: 800x1600 -> 832x1664, 200x400 -> 256x448) and FlowNet2's input
    normalisation (flownet2.py:135-139) fused - against (a) the tensor the REAL reference hands to flownetc (tests/golden/flow_prep.npz,
    captured by a hook: make_flow_prep_golden.py) and (b) the oracle's restatement on the whole tensor. Tolerance 1e-5 of a value range
    of +-0.5: the kernel takes the mean in fp64, the reference in fp32 (its own mean is ~4e-6 off, see the golden's channel sums)."""
    import sys
    from oracle.flownet2 import flow_input
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from make_flow_prep_golden import sample_index
    from vps_amd import synth
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flow_prep.npz'))
    H, W, Hp, Wp = [int(v) for v in g[case + '.shape']]
    fr = synth.synth_clip(H, W, 2, int(g['seed'][0]))
    mean_l, std_l = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    img, ref = fr[1].to(dev).contiguous(), fr[0].to(dev).contiguous()
    mean, std = torch.tensor(mean_l, device=dev), torch.tensor(std_l, device=dev)
    out = torch.full((Hp, Wp, 8), 7.0, device=dev)
    nblk = 512
    partial = torch.zeros(3 * nblk, dtype=torch.float64, device=dev)
    rgb_mean = torch.zeros(4, device=dev)
    hip.check(hip.load().vps_flow_prep_pad(hip.ptr(img), hip.ptr(ref), hip.ptr(mean), hip.ptr(std), hip.ptr(out), 8, H, W, Hp, Wp,
                                           hip.ptr(partial), nblk, hip.ptr(rgb_mean), hip.stream_ptr()), 'vps_flow_prep_pad')
    torch.cuda.synchronize()
    got = out[..., :6].permute(2, 0, 1).cpu().numpy()
    ri, ci = sample_index(H, Hp), sample_index(W, Wp)
    assert np.abs(got[:, ri][:, :, ci] - g[case + '.sample']).max() < 1e-5                    # (a) the real reference
    want = flow_input(fr[1], fr[0], mean_l, std_l)[0].numpy()
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-5                         # (b) every element, pad region included
    # the mean the kernel reports = the fp64 mean of the denormalised, padded pair
    den = torch.stack([fr[1][0].double() * torch.tensor(std_l).double().view(3, 1, 1) + torch.tensor(mean_l).double().view(3, 1, 1),
                       fr[0][0].double() * torch.tensor(std_l).double().view(3, 1, 1) + torch.tensor(mean_l).double().view(3, 1, 1)], 1)
    m64 = den.sum(dim=(1, 2, 3)) / (2.0 * Hp * Wp)
    assert np.abs(rgb_mean[:3].cpu().numpy() - m64.numpy()).max() < 1e-4


@pytest.mark.gpu
def test_mask_removal_one_launch_bounds_and_expiry_status(dev):
    """vps_mask_removal_dep refuses S > 32 (its LDS logit array is 32 x 32: ADVICE r5) and reports an expired dependency wait in
    status bit 2 (forced: VPS_MR_SPIN_LIMIT=0 on a list whose boxes all overlap) - the bit the detector recovers from"""
    import ctypes
    lib = hip.load()
    H, W, n = 256, 512, 24
    boxes = torch.tensor([[10 + i, 10 + i, 200 + i, 200 + i] for i in range(n)], dtype=torch.int32, device=dev)
    cls0 = torch.zeros(n, dtype=torch.int32, device=dev)
    midx = torch.arange(n, dtype=torch.int32, device=dev)
    occ = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev); done = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda S, lg: lib.vps_mask_removal_dep(hip.ptr(lg), S, hip.ptr(boxes), hip.ptr(cls0), hip.ptr(midx), n, 1, H, W, hip.ptr(occ),
                                                  ctypes.c_double(0.3), hip.ptr(flags), hip.ptr(done), hip.ptr(status), hip.stream_ptr())
    assert call(33, torch.ones(n, 33, 33, device=dev)) == -1003
    lg = torch.ones(n, 28, 28, device=dev)
    assert call(28, lg) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(flags[0].item()) == 1 and int(flags[1:].sum().item()) == 0      # box 0 kept, the rest overlap it
    old = os.environ.get('VPS_MR_SPIN_LIMIT')
    os.environ['VPS_MR_SPIN_LIMIT'] = '0'
    try:
        assert call(28, lg) == 0
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop('VPS_MR_SPIN_LIMIT', None)
        else:
            os.environ['VPS_MR_SPIN_LIMIT'] = old
    assert int(status.item()) & 4


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,md,s2,act', [(128, 256, 20, 2, hip.ACT_LEAKY), (256, 512, 4, 1, hip.ACT_NONE), (6, 128, 20, 2, hip.ACT_NONE),
                                           (5, 64, 4, 1, hip.ACT_LEAKY), (3, 192, 4, 1, hip.ACT_NONE)])
def test_correlation_split_fp16_on_mfma_equals_the_exact_kernels(dev, H, W, md, s2, act):
    """vps_correlation_f16 (csrc/corr_mfma.hip: banded Gram matrices on the matrix cores, fp16 pairs with a scaled residual, round 5)
    against the exact fp32 kernels at the two BASELINE shapes (441 channels @128x256, 81 channels @256x512) and on ragged ones (first /
    last rows and columns see out-of-image displacements; 3 segments per row; both column parities): fp32-grade - within 2e-6 of the
    largest output, the tolerance the exact kernels themselves are held to against the reference's own kernel
    (tests/test_ref_native_gpu.py)"""
    C = 256
    g = torch.Generator().manual_seed(H * 7 + W)
    # feature-like operands: mixed magnitudes per channel, some large values, exact zeros (ReLU-like)
    scale = torch.exp(torch.randn(C, generator=g) * 1.5)
    a = (torch.randn(1, H, W, C, generator=g) * scale).clamp_min(-0.3 * scale.max())
    b = (torch.randn(1, H, W, C, generator=g) * scale)
    b[..., ::7] = 0
    x1, x2 = nhwc.FMap(a.to(dev).contiguous()), nhwc.FMap(b.to(dev).contiguous())
    D = 2 * (md // s2) + 1
    ld = (D * D + 3) // 4 * 4 + 4
    o_exact = nhwc.FMap(torch.zeros(1, H, W, ld, device=dev), D * D, 4)
    o_f16 = nhwc.FMap(torch.full((1, H, W, ld), 7.0, device=dev), D * D, 4)
    nhwc.correlation(x1, x2, o_exact, md, s2, act, 0.1)
    st = nhwc.f16_status(dev); st.zero_()
    old = nhwc.CORR_F16[0]
    nhwc.CORR_F16[0] = True
    try:
        nhwc.correlation(x1, x2, o_f16, md, s2, act, 0.1, prec=hip.PREC_F16X3)
    finally:
        nhwc.CORR_F16[0] = old
    torch.cuda.synchronize()
    assert int(st[nhwc.F16_CORR_SLOT].item()) == 0
    e, f = o_exact.t[..., 4:4 + D * D].cpu(), o_f16.t[..., 4:4 + D * D].cpu()
    err = float((e - f).abs().max() / e.abs().max())
    print('correlation f16-split vs exact %dx%d md %d s2 %d: max err %.2e of max |out| %.3g' % (H, W, md, s2, err, float(e.abs().max())))
    assert err < 2e-6, err
    assert torch.equal(o_f16.t[..., :4].cpu(), torch.full((1, H, W, 4), 7.0)) and torch.equal(o_f16.t[..., 4 + D * D:].cpu(), torch.full((1, H, W, ld - 4 - D * D), 7.0))
    # out-of-image displacements are exact zeros like the exact kernels'
    assert torch.equal(e == 0, f == 0) or float(((e == 0) != (f == 0)).float().mean()) < 1e-4


@pytest.mark.gpu
def test_correlation_split_fp16_reports_the_fp16_range(dev):
    """an operand beyond 65504 raises the correlations' status slot; nhwc.f16_fallback then switches them to the exact kernels for good"""
    H, W, C = 4, 128, 256                  # the FlowNetC configuration (stride-2 displacements, radius 10): the shape that runs on MFMA
    a = torch.randn(1, H, W, C); b = torch.randn(1, H, W, C)
    b[0, 2, 17, 5] = 1.0e5
    x1, x2 = nhwc.FMap(a.to(dev)), nhwc.FMap(b.to(dev))
    out = nhwc.FMap(torch.zeros(1, H, W, 444, device=dev), 441, 0)
    st = nhwc.f16_status(dev); st.zero_()
    old = nhwc.CORR_F16[0]
    nhwc.CORR_F16[0] = True
    try:
        nhwc.correlation(x1, x2, out, 20, 2, prec=hip.PREC_F16X3)
        torch.cuda.synchronize()
        assert int(st[nhwc.F16_CORR_SLOT].item()) == 1
        assert nhwc.f16_fallback(dev) == 1 and nhwc.CORR_F16[0] is False and int(st.amax().item()) == 0
        ref = nhwc.FMap(torch.zeros(1, H, W, 444, device=dev), 441, 0)
        nhwc.correlation(x1, x2, ref, 20, 2)
        nhwc.correlation(x1, x2, out, 20, 2, prec=hip.PREC_F16X3)          # now the exact kernel
        assert torch.equal(out.t, ref.t)
    finally:
        nhwc.CORR_F16[0] = old
        nhwc.F16_FALLBACKS[0] = 0


# ------------------------------------------------------------------------------------------------ detection ops: edges
def _edge_rois(Hi, Wi, B, seed):
    """RoIs wholly and partly outside the image, a one-pixel RoI, scales exactly on the level edges (112, 224, 448), random ones"""
    fixed = [[-300, -300, -200, -200], [Wi + 50, Hi + 50, Wi + 150, Hi + 100], [-20, -10, 40, 30], [Wi - 30, Hi - 20, Wi + 40, Hi + 35],
             [-50, 5, Wi + 60, 20], [17, 9, 17, 9], [10, 10, 121, 121], [5, 5, 228, 228], [0, 0, 447, 447], [3, 2, 113, 114], [0.4, 0.6, 6.2, 5.1]]
    r = torch.cat([torch.tensor(fixed, dtype=torch.float32), _rand_rois(20, Hi, Wi, seed)[:, 1:]], 0)
    b = (torch.arange(r.shape[0]) % B).float()
    return torch.cat([b[:, None], r], 1)


@pytest.mark.parametrize('nlevels,C,B,win,Hi,Wi', [(4, 4, 2, True, 256, 512), (4, 32, 2, False, 256, 512), (2, 8, 1, True, 8, 64), (1, 4, 2, False, 64, 96)],
                         ids=['4lv_c4_b2_window', '4lv_c32_b2', '2lv_h1_window', '1lv_b2'])
def test_roi_align_edges(dev, nlevels, C, B, win, Hi, Wi):
    """vps_roi_align against the oracle's per-level roi_align: sample points outside the map (the zero branch), on the last row /
    column (the clamp), batch index > 0, level maps that are channel windows of wider buffers (ld = C + 8, offset 4), 1 / 2 / 4
    levels, C = 4, a level map with H = 1 (8 x 64 image at stride 8), and R = 0"""
    from ctypes import c_float, c_int, c_void_p
    lib = hip.load()
    strides = [4, 8, 16, 32][:nlevels]
    ld, off = (C + 8, 4) if win else (C, 0)
    bufs = [_rand(B, Hi // s, Wi // s, ld, seed=s).to(dev).contiguous() for s in strides]
    feats = [b[..., off:off + C].permute(0, 3, 1, 2).contiguous().cpu() for b in bufs]
    if nlevels == 2:
        assert feats[1].shape[2] == 1
    rois = _edge_rois(Hi, Wi, B, seed=3)
    R_, P = rois.shape[0], 7
    ref = OF.roi_extract(feats, rois, P)
    if nlevels == 4:
        assert OF.map_roi_levels(rois, 4)[6:9].tolist() == [1, 2, 3]
        assert float(ref[0].abs().max()) == 0.0 and float(ref[1].abs().max()) == 0.0          # wholly outside: zeros
    ptrs = (c_void_p * nlevels)(*[b.data_ptr() + 4 * off for b in bufs]); lds = (c_int * nlevels)(*[ld] * nlevels)
    Hs = (c_int * nlevels)(*[Hi // s for s in strides]); Ws = (c_int * nlevels)(*[Wi // s for s in strides])
    sc = (c_float * nlevels)(*[1.0 / s for s in strides])
    rd = rois.to(dev)
    out = torch.full((R_ + 1, P, P, C), -7.0, device=dev)
    hip.check(lib.vps_roi_align(ptrs, lds, Hs, Ws, sc, nlevels, 56.0, hip.ptr(rd), 0, C, P, 2, hip.ptr(out), hip.stream_ptr()), 'R = 0')
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    hip.check(lib.vps_roi_align(ptrs, lds, Hs, Ws, sc, nlevels, 56.0, hip.ptr(rd), R_, C, P, 2, hip.ptr(out), hip.stream_ptr()), 'vps_roi_align')
    torch.cuda.synchronize()
    assert bool((out[R_] == -7.0).all())
    _cmp(out[:R_].permute(0, 3, 1, 2), ref, rtol=5e-5, atol=5e-5, what='roi align edges')


def _run_nms(dev, boxes, counts, thr):
    nb, nmax = boxes.shape[:2]
    bd = boxes.to(dev); cd = torch.tensor(counts, dtype=torch.int32, device=dev)
    cb = (nmax + 63) // 64
    mask = torch.empty(nb * nmax * cb, dtype=torch.int64, device=dev)
    keep = torch.full((nb, nmax), -7, dtype=torch.int32, device=dev)
    nkeep = torch.full((nb,), -7, dtype=torch.int32, device=dev)
    hip.check(hip.load().vps_nms_batched(hip.ptr(bd), nb, nmax, hip.ptr(cd), thr, hip.ptr(mask), hip.ptr(keep), hip.ptr(nkeep), hip.stream_ptr()), 'nms')
    torch.cuda.synchronize()
    return keep.cpu().numpy(), nkeep.cpu().numpy()


@pytest.mark.parametrize('thr', [0.3, 0.7])
def test_nms_batched_counts_around_the_block_size_and_duplicates(dev, thr):
    """one call with 0, 1, 63, 64, 65 and 129 boxes (empty list, one box, around the 64-box block), duplicate boxes included;
    the rows of `keep` past the kept count stay untouched"""
    counts = [0, 1, 63, 64, 65, 129]
    nmax = 129
    boxes = torch.zeros(len(counts), nmax, 5)
    refs = []
    for i, n in enumerate(counts):
        r = _rand_rois(max(n, 1), 120, 200, seed=40 + i)[:n, 1:]
        if n > 4:
            r[n // 2] = r[0]; r[n - 1] = r[n - 2]; r[3] = r[2]                      # duplicates: IoU exactly 1
        sc = torch.sort(torch.rand(n, generator=torch.Generator().manual_seed(50 + i)), descending=True)[0]
        boxes[i, :n] = torch.cat([r, sc[:, None]], 1)
        refs.append(O._greedy_nms_sorted(r.numpy(), thr))
    kp, nk = _run_nms(dev, boxes, counts, thr)
    for i, n in enumerate(counts):
        assert nk[i] == len(refs[i]) and np.array_equal(kp[i, :nk[i]], refs[i]), i
        assert (kp[i, nk[i]:] == -7).all()
        if n > 4:
            assert n // 2 not in refs[i] and len(refs[i]) < n


def test_nms_iou_exactly_at_the_threshold_is_kept(dev):
    """integer boxes: 10 x 10 against its 10 x 5 half, IoU = 50 / 100 exactly = thr: strict '>', not suppressed; its duplicate is"""
    d = torch.tensor([[[0, 0, 9, 9, .9], [0, 0, 9, 4, .8], [0, 0, 9, 9, .7], [20, 20, 29, 29, .6], [20, 25, 29, 29, .5]]], dtype=torch.float32)
    assert O._greedy_nms_sorted(d[0, :, :4].numpy(), 0.5).tolist() == [0, 1, 3, 4]
    kp, nk = _run_nms(dev, d, [5], 0.5)
    assert nk[0] == 4 and kp[0, :4].tolist() == [0, 1, 3, 4]


def test_nms_kept_boxes_of_block_0_suppress_column_blocks_past_32(dev):
    """2200 boxes (35 column blocks) in dense overlapping chains: 64 columns of boxes 40 px apart, block b sits 0 / 3 / 6 / 9 px off
    its column (IoU with the block-0 box 1 / 0.82 / 0.68 / 0.55 at thr 0.7: chains of kept and suppressed boxes), blocks 33 and 34
    sit exactly ON the block-0 boxes - suppressed by a box kept in block 0 and by no other kept box: the second lap of the reduce
    kernel's propagate loop (32 column blocks per lap)"""
    n, thr = 2200, 0.7
    i = np.arange(n)
    b, lane = i // 64, i % 64
    pat = np.where(lane % 2 == 0, np.array([0, 3, 6, 9])[b % 4], np.array([0, 6, 3, 9])[b % 4]).astype(np.float32)
    pat[b >= 33] = 0
    x1 = lane * 40.0 + pat
    boxes = np.stack([x1, 0 * pat, x1 + 30, 0 * pat + 30, 1.0 - i / 4000.0], 1).astype(np.float32)
    ref = O._greedy_nms_sorted(boxes[:, :4], thr)
    assert ref.max() < 33 * 64 and len(ref) == 128 and set(range(64)) <= set(ref.tolist())
    # only block-0 boxes stand against blocks 33 / 34: every other kept box is 6 px off its column (IoU 0.68 < thr)
    assert (pat[ref[ref >= 64]] == 6).all()
    kp, nk = _run_nms(dev, torch.from_numpy(boxes)[None], [n], thr)
    assert nk[0] == len(ref) and np.array_equal(kp[0, :nk[0]], ref)


@pytest.mark.parametrize('n', [1, 257])
def test_delta2bbox_stds_ratio_clip_and_clamps(dev, n):
    """target stds other than 1, dw / dh beyond the wh_ratio_clip in both signs, boxes clamped on each of the four sides"""
    H, W = 256., 512.
    stds = (0.1, 0.1, 0.2, 0.2)
    anchors = _rand_rois(max(n, 8), 256, 512, seed=7)[:, 1:]
    deltas = _rand(max(n, 8), 4, seed=8, scale=4.0)
    deltas[0] = torch.tensor([0.5, -0.5, 25.0, -25.0])                              # 0.2 * 25 = 5 > log(1000 / 16) = 4.135
    deltas[1, 2:] = torch.tensor([-30.0, 30.0])
    anchors[:6] = torch.tensor([100., 100., 199., 179.]); deltas[2:6, 2:] = 0.5
    deltas[2, 0] = -60.0; deltas[3, 0] = 60.0; deltas[4, 1] = -60.0; deltas[5, 1] = 60.0      # centres shifted six sizes: off each side
    anchors, deltas = anchors[:n].contiguous(), deltas[:n].contiguous()
    scores = torch.rand(n, generator=torch.Generator().manual_seed(9))
    ref = torch.cat([OF.delta2bbox(anchors, deltas, (0, 0, 0, 0), stds, (256, 512)), scores[:, None]], 1)
    if n > 8:
        assert float(ref[2, 2]) == 0.0 and float(ref[3, 0]) == W - 1 and float(ref[4, 3]) == 0.0 and float(ref[5, 1]) == H - 1
    ad, dd, sd_ = anchors.to(dev), deltas.to(dev), scores.to(dev)
    out = torch.full((n + 1, 5), -7.0, device=dev)
    hip.check(hip.load().vps_delta2bbox(hip.ptr(ad), hip.ptr(dd), hip.ptr(sd_), hip.ptr(out), n, *stds, H, W, hip.stream_ptr()), 'd2b')
    torch.cuda.synchronize()
    assert bool((out[n] == -7.0).all())
    _cmp(out[:n], ref, rtol=1e-5, atol=1e-4, what='delta2bbox stds')


def test_bbox_overlaps_strided_rows_disjoint_and_identical(dev):
    """lda = 5 (detections with their score column), ldb = 4, as the tracker calls it; disjoint pairs give exactly 0, identical 1"""
    m, n = 7, 41
    a = torch.cat([_rand_rois(m, 256, 512, seed=11)[:, 1:], torch.full((m, 1), 1e6)], 1).contiguous()
    b = _rand_rois(n, 256, 512, seed=12)[:, 1:].contiguous()
    b[0] = a[0, :4]; b[5] = a[6, :4]
    b[1] = torch.tensor([2000., 2000., 2100., 2050.]); b[2] = torch.tensor([-500., 10., -400., 60.])
    ad, bd = a.to(dev), b.to(dev)
    o = torch.full((m + 1, n), -7.0, device=dev)
    hip.check(hip.load().vps_bbox_overlaps(hip.ptr(ad), 5, m, hip.ptr(bd), 4, n, hip.ptr(o), hip.stream_ptr()), 'iou')
    torch.cuda.synchronize()
    o = o.cpu()
    assert bool((o[m] == -7.0).all())
    assert float(o[0, 0]) == 1.0 and float(o[6, 5]) == 1.0 and bool((o[:m, 1] == 0).all()) and bool((o[:m, 2] == 0).all())
    _cmp(o[:m], OF.bbox_overlaps(a[:, :4], b), rtol=1e-6, atol=1e-7, what='iou lda 5')
