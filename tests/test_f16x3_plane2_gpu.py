"""f16x3: the third weight plane g2 = fp16(2^-11 * g0) is derived in registers by the kernels (csrc/conv_common.h:derive_weight_plane)
instead of being read from the packed tensor. One small layer per kernel family runs through vps_conv2d and is compared, for EXACT
equality, with a float64 evaluation of the same three-product formula h0*g1 + h1*g2 + h0*g0 that takes g2 from the packed tensor.

Why exact equality can be asked for. The kernels accumulate in fp32, the reference in float64; the two agree bit for bit only if no
fp32 addition rounds. The operands are built so that none does, whatever the accumulation order:
  * activations: every K x K window of the input (K = taps per axis of a parity class) holds exactly ONE non-zero value, in a random
    channel: +-(1 + 2^-12) * 2^e. Its split is h0 = +-2^e, h1 = +-2^(e-1), so an output element is the three products of ONE weight;
  * weights: random, low 4 significand bits cleared. For a weight of magnitude 2^f (after the per-channel scaling) g0 has bits
    2^f .. 2^(f-10), g1 = fp16(w' - g0) bits >= 2^(f-19), h1/h0 * g2 = 2^-12 g0 bits >= 2^(f-22): with a carry the sum of the three
    products spans 2^(f+1) .. 2^(f-22), 24 bits - exactly an fp32 significand. fp16 subnormals are multiples of 2^-24 below 2^-14:
    fewer bits still. The epilogue scale is a power of two. The test asserts that the float64 result is fp32-representable.
The weights hold what makes the derived plane differ from a careless one: one output channel scaled by 2^-20 and one by 2^-30 (the
per-channel power-of-two scaling of PackedConv undoes those exactly), and, inside every channel, an eighth of the weights scaled by
2^-14 (g0 * 2^-11 lands in the fp16 subnormals and is rounded there) and an eighth by 2^-26 (it underflows to zero).
Deformable layer: integer offsets in [-2, 2], the same for the nine taps of a pixel (bilinear weights 1, 0, 0, 0: exact sampling)."""
import pytest
import torch

import conv_planner
from vps_amd import hip, nhwc

pytestmark = pytest.mark.gpu

PA, PB = [0, 1, 0], [1, 2, 0]          # Split<VPS_PREC_F16X3>: products h0*g1, h1*g2, h0*g0 in the kernels' order

# name, cin, cout, kernel, stride, H, W, transposed, deformable. Which family a shape reaches: csrc/conv_plan.cpp (halo: stride-1 3x3 /
# 2x2 classes on small maps; h8 / h8p / h8s2: >= 256 tiles of 8 x 32 pixels x 128 columns, >= 3 chunks; n16: >= 256 patches) - KERNEL
# below, asserted through the host planner for the descriptor that was launched. The persistent pointwise kernel (pw) needs two
# rounds of resident blocks, >= 65536 pixels for 128 columns: no map up to 64x128 plans it, the 64x128 case runs q like the small one
# (pw is compared bitwise with q on large maps in tests/test_hip_ops.py).
KERNEL = {'halo_3x3': 'halo', 'halo_2x2_transposed': 'halo', 'q_1x1': 'q', 'q_1x1_64x128': 'q', 'h8p_3x3_128x128': 'h8p',
          'h8_2x2_transposed_64x64': 'h8', 'h8s2_3x3_stride2': 'h8s2', 'deformable': 'bf16p', 'n16_64x128': 'halo', 'n16_256x256': 'n16',
          'split_k': 'halo'}
CASES = [
    ('halo_3x3', 64, 128, 3, 1, 16, 32, False, False),
    ('halo_2x2_transposed', 96, 64, 4, 2, 16, 16, True, False),
    ('q_1x1', 256, 128, 1, 1, 16, 32, False, False),
    ('q_1x1_64x128', 256, 128, 1, 1, 64, 128, False, False),
    ('h8p_3x3_128x128', 96, 512, 3, 1, 128, 128, False, False),
    ('h8_2x2_transposed_64x64', 96, 512, 4, 2, 64, 64, True, False),
    ('h8s2_3x3_stride2', 96, 512, 3, 2, 256, 256, False, False),
    ('deformable', 128, 128, 3, 1, 16, 32, False, True),
    ('n16_64x128', 64, 16, 3, 1, 64, 128, False, False),
    ('n16_256x256', 64, 16, 3, 1, 256, 256, False, False),
    ('split_k', 512, 512, 3, 1, 8, 16, False, False),
]


@pytest.fixture(scope='module')
def planned_kernel(tmp_path_factory):
    """descriptor -> name of the kernel vpsi_conv_plan gives it: the stand-alone planner of tests/test_conv_plan.py (host C++), default
    switches, the limits recorded in tests/conv_plan_cases.json"""
    return conv_planner.planned_kernel(tmp_path_factory.mktemp('plan'))


def _weights(cin, cout, k, transposed, g):
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = torch.randn(shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    u = torch.rand(shape, generator=g)
    w = torch.where(u < 0.125, w * 2.0 ** -14, torch.where(u < 0.25, w * 2.0 ** -26, w))
    och = 1 if transposed else 0
    sc = torch.ones(cout)
    sc[1], sc[cout - 2] = 2.0 ** -20, 2.0 ** -30
    w = w * sc.view([-1 if i == och else 1 for i in range(4)])
    return (w.view(torch.int32) & ~0xF).view(torch.float32)          # low 4 significand bits cleared (see the module docstring)


def _activations(cin, H, W, S, g):
    """[1, H, W, cin]: one non-zero per S x S cell (so per S x S window), random channel, +-(1 + 2^-12) * 2^e, e in -2 .. 2"""
    x = torch.zeros(1, H, W, cin)
    ys, xs = torch.arange(S // 2, H, S), torch.arange(S // 2, W, S)
    yy, xx = torch.meshgrid(ys, xs, indexing='ij')
    n = yy.numel()
    ch = torch.randint(0, cin, (n,), generator=g)
    e = torch.randint(-2, 3, (n,), generator=g)
    sign = torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0
    x[0, yy.reshape(-1), xx.reshape(-1), ch] = sign * torch.ldexp(torch.tensor(1.0 + 2.0 ** -12).expand(n), e)
    return x


def _unpack_planes(pc):
    """w_split -> float64 [plane][class][cout_pad][tap][channels] in natural order (undoes the fragment order and the k order)"""
    ws = pc.w_split
    P, C, OB, KB = ws.shape[:4]
    ws = ws.permute(0, 1, 2, 5, 3, 4, 6).reshape(P, C, OB * 32, KB * 16).double()
    ntap = pc.KH * pc.KW
    if pc.korder == 0:
        return ws[..., :ntap * pc.cin_pad].reshape(P, C, OB * 32, ntap, pc.cin_pad)
    nch = (pc.cin_pad + 31) // 32
    return ws[..., :nch * ntap * 32].reshape(P, C, OB * 32, nch, ntap, 32).permute(0, 1, 2, 4, 3, 5).reshape(P, C, OB * 32, ntap, nch * 32)


def _reference(pc, x, Ho, Wo, off):
    """float64, on the host: sum over the taps and the three products of (activation plane) x (weight plane of the PACKED tensor),
    times the scale. A gathered pixel has one non-zero channel: its products are that channel's weight column, no GEMM needed."""
    planes = _unpack_planes(pc).cpu()
    x = x.cpu()
    off = None if off is None else off.cpu()
    assert planes.shape[0] == 3
    g0, g2 = planes[0], planes[2]
    assert torch.equal(g2, (g0 * 2.0 ** -11).to(torch.float16).double())          # what the host packed: RNE into fp16, subnormals kept
    sub = (g2 != 0) & (g2.abs() < 2.0 ** -14)
    assert int(sub.sum()) > 0 and int(((g2 * 2048.0 != g0) & sub).sum()) > 0       # subnormal g2, some of them rounded
    assert int(((g0 != 0) & (g2 == 0)).sum()) > 0                                  # g2 underflowed to zero
    H, W, C = x.shape[1], x.shape[2], x.shape[3]
    h0 = x.to(torch.float16)
    h1 = ((x - h0.float()) * 2048.0).to(torch.float16)
    assert float(h1.abs().max()) > 0
    assert int((x[0] != 0).sum(-1).max()) == 1
    ch = x[0].abs().argmax(-1)                                                     # [H][W]: the pixel's non-zero channel
    v = [h0.double()[0].gather(-1, ch.unsqueeze(-1))[..., 0], h1.double()[0].gather(-1, ch.unsqueeze(-1))[..., 0]]
    Qh, Qw = (H, W) if pc.transposed else (Ho, Wo)
    qy, qx = torch.meshgrid(torch.arange(Qh), torch.arange(Qw), indexing='ij')
    out = torch.zeros(1, Ho, Wo, pc.cout, dtype=torch.float64)
    for py in range(pc.os):
        for px in range(pc.os):
            cls = py * pc.os + px
            acc = torch.zeros(Qh * Qw, pc.cout, dtype=torch.float64)
            for uy in range(pc.KH):
                for ux in range(pc.KW):
                    tap = uy * pc.KW + ux
                    iy, ix = qy * pc.stride - pc.pad_y[py] + uy, qx * pc.stride - pc.pad_x[px] + ux
                    if off is not None:
                        iy, ix = iy + off[0, :, :, 2 * tap].long(), ix + off[0, :, :, 2 * tap + 1].long()
                    ok = ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).reshape(-1).double()
                    iyc, ixc = iy.clamp(0, H - 1).reshape(-1), ix.clamp(0, W - 1).reshape(-1)
                    c = ch[iyc, ixc]
                    for pa, pb in zip(PA, PB):
                        acc += (v[pa][iyc, ixc] * ok).unsqueeze(1) * planes[pb][cls, :pc.cout, tap, :C].t()[c]
            if pc.scale is not None:
                acc = acc * pc.scale.double().cpu().view(1, -1)
            out[0, py::pc.os, px::pc.os] = acc.view(Qh, Qw, pc.cout)
    return out


@pytest.mark.parametrize('name,cin,cout,k,stride,H,W,transposed,deform', CASES, ids=[c[0] for c in CASES])
def test_f16x3_kernel_equals_the_three_product_formula_with_the_packed_plane2(dev, planned_kernel, name, cin, cout, k, stride, H, W, transposed, deform):
    g = torch.Generator().manual_seed(len(name) * 131 + cin + cout)
    w = _weights(cin, cout, k, transposed, g)
    pc = nhwc.PackedConv(w, None, None, stride=stride, padding=k // 2 if not transposed else 1, transposed=transposed, deform=deform,
                         device=torch.device('cpu'), prec=hip.PREC_F16X3)
    assert pc.prec == hip.PREC_F16X3 and pc.w_split.shape[0] == 3 and pc.w_thin is None
    # packed on the host (the power-of-two channel scaling is exact there: the bit budget above counts on it), then moved
    pc.w_split, pc.scale = pc.w_split.to(dev), pc.scale.to(dev)
    x = _activations(cin, H, W, pc.KH, g).to(dev)
    off = None
    if deform:
        d = torch.randint(-2, 3, (1, H, W, 2), generator=g).float()
        off = d.repeat(1, 1, 1, 9).contiguous().to(dev)                            # (dy, dx) of the pixel for each of its nine taps
    Ho, Wo = pc.out_hw(H, W)
    out = nhwc.FMap(torch.full((1, Ho, Wo, cout), 7.0, device=dev), cout, 0)
    pc(nhwc.FMap(x, cin, 0), out=out, ws=nhwc.Workspace(dev), offset=None if off is None else nhwc.FMap(off, 18, 0))
    torch.cuda.synchronize()
    launch, = pc._launches.values()
    assert planned_kernel(launch.desc) == KERNEL[name]
    assert int(nhwc.f16_status(dev)[pc.f16_slot]) == 0
    ref = _reference(pc, x, Ho, Wo, off)
    nrep = int((ref.float().double() != ref).sum())
    print('%s: %d of %d reference values are not fp32 numbers' % (name, nrep, ref.numel()))
    assert nrep == 0                                                               # no fp32 addition can have rounded
    assert int((ref != 0).sum()) > ref.numel() // (2 * pc.KH * pc.KW)
    got = out.t.double().cpu()
    nbad = int((got != ref).sum())
    print('%s: %d of %d outputs differ, max |diff| %.3e' % (name, nbad, ref.numel(), float((got - ref).abs().max())))
    assert torch.equal(got, ref)
