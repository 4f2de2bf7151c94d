"""The deformable 3x3 kernels (vps_amd/csrc/conv_mfma.hip: conv_mfma_f32_kernel<..., true>, the DEFORM instances of
conv_mfma_bf16p_kernel and its 256-column instance) against the float64 restatement of tests/deform_restate.py, on every route a
deformable launch can take (tests/deform_cases.py:ROUTES), with two images, channel windows and the sampling edges.

Every case asserts its route: the kernel name comes from the host planner for the descriptor that was launched, tile_n, ksplit and
whether tile_counter is set from that descriptor (pc._launches). PackedConv produces split-K launches of both kinds: with the
default switches the partial sums go to a separate reduce kernel (tile_counter NULL: f32_split_reduce, p_split3_reduce_f16x3, the two
stride-2 cases), with nhwc.SPLITK_LAST_BLOCK the last block of a tile sums them (the p_split* cases).

Three tests per route:
  1. integer operands, windows everywhere (in_coff 8 of a buffer 20 channels wider than cin_pad, off_ld 20, the output at channel 8
     of a pre-filled concat buffer): BITWISE equal to the float64 result (why that can be asked: tests/deform_cases.py), the rest of
     the concat buffer untouched;
  2. the edge offset field with random float operands, contiguous: max |got - ref| / den <= bound, den = sum |w| sum bw |x|, and an
     element whose den is 0 is exactly 0.
         bound = B_split + B_sample + B_acc
     B_split: the design bound of the operand split, BOUND[prec] of tests/test_split_arith.py (0 in f32);
     B_sample = 8 * 2^-24: three fp32 roundings in a bilinear weight (1 - l, 1 - l, the product; l itself is exact), then four
       products and three additions in the blend, each relative to sum bw |x|;
     B_acc: fp32 accumulation. Taken from the REFERENCE's side, never from the kernel: err / den of a float32 CPU matmul of the
       restatement's fp32 columns against the float64 result, times 4 (the matrix pipe adds in another order than the CPU).
     Both figures are printed per case;
  3. the GroupNorm sums of the epilogue (the unsplit split-operand routes, one image) equal the sums of the stored tensor under the
     edge field; with two images the launch does not take them (conv_geometry) and the slot stays zero."""
import functools

import pytest
import torch

import conv_planner
import deform_cases as DC
import deform_restate as DR
from test_split_arith import BOUND
from vps_amd import hip, nhwc

pytestmark = pytest.mark.gpu

PREC = dict(f32=hip.PREC_F32, bf16x3=hip.PREC_BF16X3, bf16x6=hip.PREC_BF16X6, f16x3=hip.PREC_F16X3)
B_SAMPLE = 8 * 2.0 ** -24
IDS = dict(ids=lambda r: '%s_n%d' % (r[0], r[3]))


@pytest.fixture(scope='module')
def planned_kernel(tmp_path_factory):
    """descriptor -> name of the kernel vpsi_conv_plan gives it (tests/conv_planner.py)"""
    return conv_planner.planned_kernel(tmp_path_factory.mktemp('plan'))


@functools.lru_cache(maxsize=None)
def _reference(route, kind):
    """the float64 result of a case, once; asserts what the case promises (tests/deform_cases.py)"""
    name, cin, cout, N, H, W, stride = route[:7]
    x, w, off, cls = DC.operands(route, kind)
    ref = DR.deform_conv_f64(x, off, w, stride, 1)
    h, ww = DR.positions(off, H, W, 3, 3, stride, 1)
    DC.check_field(off, cls, h, ww, ref.valid, H, W, DC.INT_SHARES if kind == 'int' else DC.EDGE_SHARES)
    assert bool(torch.isfinite(ref.out).all())
    assert int((ref.den > 0).sum()) >= 0.9 * ref.den.numel()
    return ref


def _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed, gn=None, fused=False):
    """one launch of the route's layer -> (output window [N, Ho, Wo, cout] on the host, whole output buffer on the host, PackedConv)"""
    name, cin, cout, N, H, W, stride, prec, switches, (kernel, tile_n, ksplit, counter) = route
    for k, v in switches:
        monkeypatch.setattr(nhwc, k, [v] if k == 'DCN256' else v)
    # packed on the host (the power-of-two channel scaling of f16x3 is exact there), then moved
    pc = nhwc.PackedConv(w, None, None, stride, 1, device=torch.device('cpu'), deform=True, prec=PREC[prec])
    for a in ('w', 'w_split', 'scale'):
        if getattr(pc, a) is not None:
            setattr(pc, a, getattr(pc, a).to(dev))
    assert pc.prec == (hip.PREC_F32 if kernel == 'f32' else PREC[prec]) and pc.shift is None and pc.w_thin is None
    Ho, Wo = pc.out_hw(H, W)
    assert (N, 18, Ho, Wo) == tuple(off.shape)
    in_coff, in_ld, off_ld, out_coff, out_ld = (8, pc.cin_pad + 20, 20, 8, cout + 24) if windowed else (0, pc.cin_pad, 18, 0, cout)
    xb = torch.full((N, H, W, in_ld), 777.0)
    xb[..., in_coff:in_coff + pc.cin_pad] = 0.0
    xb[..., in_coff:in_coff + cin] = x.permute(0, 2, 3, 1)
    ob = torch.full((N, Ho, Wo, off_ld), 555.0)
    ob[..., :18] = off.permute(0, 2, 3, 1)
    outb = torch.full((N, Ho, Wo, out_ld), 7.0)
    xd, od, outd = xb.to(dev), ob.to(dev), outb.to(dev)
    pc(nhwc.FMap(xd, cin, in_coff), out=nhwc.FMap(outd, cout, out_coff), offset=nhwc.FMap(od, 18, 0), gn=gn)
    torch.cuda.synchronize()
    launch, = pc._launches.values()
    d = launch.desc
    assert planned_kernel(d) == kernel
    assert (d.tile_n, d.ksplit, bool(d.tile_counter)) == (tile_n, ksplit, counter)
    assert (d.N, d.in_coff, d.in_ld, d.off_ld, d.out_coff, d.out_ld, d.stride) == (N, in_coff, in_ld, off_ld, out_coff, out_ld, stride)
    assert bool(d.gn_stats) == fused and pc.gn_fused == fused
    if pc.prec == hip.PREC_F16X3:
        assert int(nhwc.f16_status(dev)[pc.f16_slot]) == 0           # no status word: nothing staged left the fp16 range
    assert torch.equal(xd.cpu(), xb) and torch.equal(od.cpu().view(torch.int32), ob.view(torch.int32))      # (bit patterns: NaN offsets)
    whole = outd.cpu()
    return whole[..., out_coff:out_coff + cout], whole, pc


@pytest.mark.parametrize('route', DC.ROUTES, **IDS)
def test_integer_operands_in_channel_windows_are_bitwise_the_float64_result(dev, monkeypatch, planned_kernel, route):
    x, w, off, cls = DC.operands(route, 'int')
    ref = _reference(route, 'int')
    assert torch.equal(ref.out.float().double(), ref.out)                       # fp32 numbers: no fp32 addition can have rounded
    got, whole, pc = _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed=True)
    cout = route[2]
    assert torch.equal(whole[..., :8], torch.full_like(whole[..., :8], 7.0))
    assert torch.equal(whole[..., 8 + cout:], torch.full_like(whole[..., 8 + cout:], 7.0))
    want = ref.out.permute(0, 2, 3, 1)
    diff = got.double() != want
    print('%s: %d of %d outputs differ, max |diff| %.3e' % (route[0], int(diff.sum()), diff.numel(), float((got.double() - want).abs().max())))
    assert not bool(diff.any())


@pytest.mark.parametrize('route', DC.ROUTES, **IDS)
def test_edge_offset_field_stays_within_the_bound_of_its_arithmetic(dev, monkeypatch, planned_kernel, route):
    x, w, off, cls = DC.operands(route, 'edge')
    ref = _reference(route, 'edge')
    got, whole, pc = _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed=False)
    b_acc = 4 * DR.accumulation_allowance(ref, w)
    bound = (0.0 if pc.prec == hip.PREC_F32 else BOUND[pc.prec]) + B_SAMPLE + b_acc
    got = got.double()
    assert bool(torch.isfinite(got).all())
    want, den = ref.out.permute(0, 2, 3, 1), ref.den.permute(0, 2, 3, 1)
    pos = den > 0
    rel = float(((got - want).abs()[pos] / den[pos]).max())
    print('%s: max |got - ref| / den = %.3e, bound %.3e (B_acc %.3e)' % (route[0], rel, bound, b_acc))
    assert rel <= bound
    assert not bool((got[~pos] != 0).any())


@pytest.mark.parametrize('route', DC.GN_ROUTES, **IDS)
def test_epilogue_groupnorm_sums_equal_the_sums_of_the_stored_tensor(dev, monkeypatch, planned_kernel, route):
    """the relative measure of test_deform_conv_epilogue_takes_the_groupnorm_sums (tests/test_hip_ops.py): lanes add their <= 8
    values in fp32 before everything goes to double - errors relative to sum |v| resp. sum v^2, below 1e-6"""
    cout, G = route[2], 32
    x, w, off, cls = DC.operands(route, 'edge')
    slot = torch.zeros(nhwc.GN_REP, 2 * G, dtype=torch.float64, device=dev)
    got, whole, pc = _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed=False, gn=(slot, G), fused=True)
    o = got.double().reshape(-1, G, cout // G)
    sums = torch.stack([o.sum(dim=(0, 2)), (o * o).sum(dim=(0, 2))], dim=1).reshape(-1)
    scale = torch.stack([o.abs().sum(dim=(0, 2)), (o * o).sum(dim=(0, 2))], dim=1).reshape(-1)
    rel = float(((slot.sum(dim=0).cpu() - sums).abs() / scale).max())
    print('%s: GroupNorm sums, max relative error %.3e' % (route[0], rel))
    assert rel < 1e-6


@pytest.mark.parametrize('route', [r for r in DC.ROUTES if r[0] in [g[0] for g in DC.GN_ROUTES]], **IDS)
def test_two_images_leave_the_groupnorm_slot_alone(dev, monkeypatch, planned_kernel, route):
    """the slot has no image dimension: conv_geometry declines the sums for N = 2 (vpsi_conv_check would refuse them, VPS_EARG 15:
    tests/test_deform_restate.py), the caller sees gn_fused False and runs the statistics pass itself"""
    x, w, off, cls = DC.operands(route, 'edge')
    slot = torch.zeros(nhwc.GN_REP, 64, dtype=torch.float64, device=dev)
    got, whole, pc = _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed=False, gn=(slot, 32), fused=False)
    assert float(slot.abs().max()) == 0.0
    plain, _, _ = _run(dev, monkeypatch, planned_kernel, route, x, w, off, windowed=False)
    assert torch.equal(got, plain)
