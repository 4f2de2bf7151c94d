"""CPU checks of what tests/test_deform_conv_gpu.py stands on: the float64 restatement of the deformable convolution
(tests/deform_restate.py) against the oracle and against a per-sample loop, the edge offset field and the integer operands
(tests/deform_cases.py), the launch geometry of every route of the table, and the refusal of GroupNorm sums for more than one image
(conv_geometry and vpsi_conv_check)."""
import pytest
import torch

import conv_planner
import deform_cases as DC
import deform_restate as DR
from oracle import ops as O
from vps_amd import hip, nhwc

PREC = dict(f32=hip.PREC_F32, bf16x3=hip.PREC_BF16X3, bf16x6=hip.PREC_BF16X6, f16x3=hip.PREC_F16X3)
SMALL = [r for r in DC.ROUTES + DC.GN_ROUTES if r[4] * r[5] <= 1024]      # the references of the large maps are left to the GPU test


@pytest.mark.parametrize('stride', [1, 2])
def test_restatement_equals_the_oracle_on_finite_random_offsets(stride):
    g = torch.Generator().manual_seed(5 + stride)
    x, w = DC.float_operands(8, 12, 2, 11, 14, g)
    Ho, Wo = DC.out_hw(11, 14, stride)
    off = torch.randn(2, 18, Ho, Wo, generator=g) * 1.5
    ref = DR.deform_conv_f64(x, off, w, stride, 1)
    # the oracle on float64 operands: its positions and bilinear weights stay fp32, its blend and contraction become float64
    got = O.deform_conv(x.double(), off, w.double(), stride, 1)
    assert got.dtype == torch.float64 and got.shape == ref.out.shape
    rel = float(((got - ref.out).abs() / ref.den).max())
    print('oracle vs restatement, stride %d: max |diff| / den = %.3e' % (stride, rel))
    assert rel <= 1e-6


@pytest.mark.parametrize('stride', [1, 2])
def test_restatement_equals_a_per_sample_loop_under_the_edge_field(stride):
    N, H, W = 2, 5, 6
    g = torch.Generator().manual_seed(17 + stride)
    x, w = DC.float_operands(3, 4, N, H, W, g)
    off, cls = DC.offset_field(N, H, W, stride, 1, g)
    ref = DR.deform_conv_f64(x, off, w, stride, 1)
    h, ww = DR.positions(off, H, W, 3, 3, stride, 1)
    if stride == 1:
        DC.check_field(off, cls, h, ww, ref.valid, H, W)
    assert bool(torch.isfinite(ref.out).all())
    brute = DR.brute_force(x, off, w, stride, 1)
    assert float(((brute - ref.out).abs() / ref.den.clamp_min(1e-300)).max()) <= 1e-13
    assert torch.equal(brute[ref.den == 0], torch.zeros_like(brute[ref.den == 0]))
    # the oracle selects an invalid sample away as the reference does (deform_conv_cuda_kernel.cu:225-237): NaN and infinite
    # offsets leave no trace
    got = O.deform_conv(x.double(), off, w.double(), stride, 1)
    assert bool(torch.isfinite(got).all())
    assert float(((got - ref.out).abs() / ref.den.clamp_min(1e-300))[ref.den > 0].max()) <= 1e-6


@pytest.mark.parametrize('route', DC.ROUTES + DC.GN_ROUTES, ids=lambda r: '%s_n%d' % (r[0], r[3]))
def test_offset_fields_of_every_case_hold_their_class_shares(route):
    name, cin, cout, N, H, W, stride = route[:7]
    for kind, shares in (('edge', DC.EDGE_SHARES), ('int', DC.INT_SHARES)):
        x, w, off, cls = DC.operands(route, kind)
        h, ww = DR.positions(off, H, W, 3, 3, stride, 1)
        valid = (h > -1) & (ww > -1) & (h < H) & (ww < W)
        DC.check_field(off, cls, h, ww, valid, H, W, shares)


@pytest.mark.parametrize('route', SMALL, ids=lambda r: '%s_n%d' % (r[0], r[3]))
def test_integer_cases_have_fp32_results_and_enough_nonzero_magnitudes(route):
    stride = route[6]
    for kind in ('int', 'edge'):
        x, w, off, cls = DC.operands(route, kind)
        ref = DR.deform_conv_f64(x, off, w, stride, 1)
        assert bool(torch.isfinite(ref.out).all())
        assert int((ref.den > 0).sum()) >= 0.9 * ref.den.numel()
        if kind == 'int':
            assert torch.equal(ref.out.float().double(), ref.out)
            assert int((ref.out != 0).sum()) >= 0.5 * ref.out.numel()


def _layer(route):
    name, cin, cout, N, H, W, stride, prec = route[:8]
    w = DC.operands(route, 'int')[1]
    return nhwc.PackedConv(w, None, None, stride, 1, device=torch.device('cpu'), deform=True, prec=PREC[prec])


@pytest.mark.parametrize('route', DC.ROUTES + DC.GN_ROUTES, ids=lambda r: '%s_n%d' % (r[0], r[3]))
def test_conv_geometry_gives_every_case_the_tiling_of_its_route(route, monkeypatch):
    name, cin, cout, N, H, W, stride, prec, switches, (kernel, tile_n, ksplit, counter) = route
    for k, v in switches:
        monkeypatch.setattr(nhwc, k, [v] if k == 'DCN256' else v)
    pc = _layer(route)
    assert pc.prec == (hip.PREC_F32 if kernel == 'f32' else PREC[prec])
    assert pc.korder == (0 if name == 'f32_tapmajor_forced' else 1)
    Ho, Wo = pc.out_hw(H, W)
    geo = nhwc.conv_geometry(pc, N, Ho, Wo, cout, 0, False, None)
    assert (geo.tile_n, geo.ksplit) == (tile_n, ksplit)


def test_conv_geometry_declines_groupnorm_sums_for_more_than_one_image():
    pc = _layer(DC.GN_ROUTES[0])
    assert nhwc.conv_geometry(pc, 1, 11, 15, 256, 0, False, 32).gn_cpg == 8
    assert nhwc.conv_geometry(pc, 2, 11, 15, 256, 0, False, 32).gn_cpg == 0
    assert nhwc.conv_geometry(pc, 1, 11, 15, 256, 0, False, None).gn_cpg == 0


def test_conv_check_refuses_groupnorm_sums_for_more_than_one_image(tmp_path):
    """a descriptor that asks for the sums with N = 2 (conv_geometry never builds one): VPS_EARG(15) before anything is launched"""
    check = conv_planner.make_planner(tmp_path)
    pc = _layer(DC.GN_ROUTES[0])
    slot = torch.zeros(nhwc.GN_REP, 64, dtype=torch.float64)
    for N, err in ((1, 0), (2, -1015)):
        x = nhwc.FMap(torch.zeros(N, 11, 15, 32), 32, 0)
        out = nhwc.FMap(torch.zeros(N, 11, 15, 256), 256, 0)
        off = nhwc.FMap(torch.zeros(N, 11, 15, 18), 18, 0)
        geo = nhwc.ConvGeometry(128, 1, 8, 0, 0)
        d = pc._describe(x, out, 11, 15, None, 0, off, None, (slot, 32), geo)
        assert d.gn_stats and d.N == N
        kernel, _, got = check(d)
        assert got == err and kernel == ('bf16p' if err == 0 else 'none'), (N, kernel, got)
