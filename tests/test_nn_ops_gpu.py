"""Kernel-level tests of the glue kernels of vps_amd/csrc/nn_ops.hip (resize, 3x3/s2 pooling, BFP gather / scatter, GroupNorm, the TCEA
kernels, axpb) and of the non-correlation half of vps_amd/csrc/flow_ops.hip (the layout transposes, resample2d, channelnorm, flow_warp,
flow_prep, the flow_stage family), against tests/nn_restate.py (plain numpy restatements, pinned to torch and the oracle on the CPU by
tests/test_nn_restate.py) on the cases of tests/nn_cases.py.

EVERY kernel is called through the C ABI (hip.load().vps_*): all cases go round the wrappers of vps_amd/nhwc.py (which forbid most of the
windows used here); vps_groupnorm_apply gets a hand-built [nrep][2 G] sums array, vps_tcea_modulate_ld is called directly. Inputs and
outputs move with torch and numpy on the host, NOT with from_nchw / to_nchw (except in the transposes' own tests).

Guards: every output is a window [coff, coff + C) of a buffer with leading dimension ld; the whole buffer, with a guard row of pixels
before and after, is pre-filled with a quiet-NaN sentinel and compared WHOLE - everything outside the window must still hold the sentinel
bit for bit. Inputs sit in buffers of their own leading dimension with 1e30 beside their window and are checked unchanged after the call.

Comparison: kernels that move or select values (nearest resize, max pool, BFP scatter, the transposes, axpb's single fma, the
all-corners-outside zeros of flow_warp) compare BITWISE with the float64 restatement cast to float32. Everything else compares with the
float64 restatement under bound = max(one float32 ulp of the largest |reference|, 4 x max|float32 restatement - float64 restatement|),
derived here from the case's own inputs; tests/test_nn_restate.py asserts on the CPU that it never exceeds what tests/test_hip_ops.py
allows the kernel. Measured figures: tests/tolerances.py (NN_OPS_MEASURED)."""
import ctypes

import numpy as np
import pytest
import torch

import nn_cases as K
from kernel_buf import Buf, written_outside          # shared with tests/test_corr_gpu.py
from vps_amd import hip

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _in(dev, a):
    """upload a wide input map [..., ld] (or a flat array: one row)"""
    a = np.asarray(a)
    ld = a.shape[-1] if a.ndim > 1 else a.size
    return Buf(dev, a, a.size // ld, ld)


def _out(dev, rows, ld):
    return Buf(dev, None, rows, ld)


def _check(c, outs, ins, rc=0, relayout=None):
    """outs: {name: (Buf, coff, C)} - the window of each output (several may share a buffer); compares against the restatement of the
    case, whole buffers. relayout: brings a restated array into the buffer's layout."""
    torch.cuda.synchronize()
    assert rc == 0, 'return code %d' % rc
    for b in ins:
        assert b.unchanged(), 'an input buffer was written'
    inp = K.inputs(c)
    r64 = K.reference(c, inp, F64)
    if c['exact']:
        want = K.expected_bits(c, r64)
        bnd = None
    else:
        bnd = K.bounds(c, K.reference(c, inp, F32), r64)
    if relayout is not None:
        r64 = {k: relayout(v) for k, v in r64.items()}
    for name, (buf, coff, C) in outs.items():
        got = buf.bits()
        nout = written_outside(got, [(coff2, C2) for b2, coff2, C2 in outs.values() if b2 is buf])
        assert nout == 0, '%s: %d elements outside the window written' % (name, nout)
        w = got[1:-1, coff:coff + C]
        if c['exact']:
            e = np.ascontiguousarray(want[name]).view(np.int32).reshape(w.shape)
            assert np.array_equal(w, e), '%s: %d of %d elements differ bitwise, first at %s' % (name, int((w != e).sum()), w.size, np.argwhere(w != e)[:4].tolist())
            continue
        ref = r64[name].reshape(w.shape)
        err = np.abs(w.view(F32).astype(F64) - ref)
        assert not np.isnan(err).any(), '%s: %d NaN (sentinel left or computed)' % (name, int(np.isnan(err).sum()))
        b, dist, floor, cap = bnd[name]
        print('%s %s %s: max err %.3g, float32 vs float64 %.3g, floor %.3g, bound %.3g' % (c['op'], c['id'], name, float(err.max()), dist, floor, b))
        assert float(err.max()) <= b, '%s: max err %.3g > bound %.3g (float32 vs float64 restatement %.3g), at %s' % (
            name, float(err.max()), b, dist, np.unravel_index(int(err.argmax()), err.shape))
    return r64


def _ids(op):
    return dict(argvalues=K.cases(*op.split(',')), ids=K.case_id)


# ------------------------------------------------------------------------------------------------ nn_ops.hip
@pytest.mark.parametrize('c', **_ids('resize'))
def test_resize(dev, c):
    """non-integer ratios both ways, Hi = 1 / Wi = 1 (yp = xp = 0 everywhere), the identity size, N = 2, windows on both sides on the
    float4 path, the scalar path forced by out_ld = 19 with C = 8, C = 3; alpha 1, 0.25, -20 in both modes"""
    x = _in(dev, K.inputs(c)['x'])
    o = _out(dev, c['N'] * c['Ho'] * c['Wo'], c['out_ld'])
    rc = hip.load().vps_resize(x.p(), c['in_ld'], c['in_coff'], c['Hi'], c['Wi'], o.p(), c['out_ld'], c['out_coff'], c['Ho'], c['Wo'], c['N'], c['C'],
                               1 if c['mode'] == 'nearest' else 0, c['alpha'], hip.stream_ptr())
    _check(c, dict(out=(o, c['out_coff'], c['C'])), [x], rc)


@pytest.mark.parametrize('c', **_ids('pool'))
def test_pool3x3s2(dev, c):
    """maps of 1 or 2 rows / columns (most taps are clamped duplicates), N = 2, a float4 window and C = 3; all-negative inputs (a zero
    pad would win the max; the avg divisor stays 9), -inf and -0.0 entries (max: bitwise)"""
    x = _in(dev, K.inputs(c)['x'])
    Ho, Wo = (c['Hi'] - 1) // 2 + 1, (c['Wi'] - 1) // 2 + 1
    o = _out(dev, c['N'] * Ho * Wo, c['out_ld'])
    rc = hip.load().vps_pool3x3s2(x.p(), c['in_ld'], c['in_coff'], c['Hi'], c['Wi'], o.p(), c['out_ld'], c['out_coff'], c['N'], c['C'],
                                  0 if c['mode'] == 'max' else 1, hip.stream_ptr())
    _check(c, dict(out=(o, c['out_coff'], c['C'])), [x], rc)


def _ptrs(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.p() for b in bufs])


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


@pytest.mark.parametrize('c', **_ids('gather'))
def test_bfp_gather(dev, c):
    """1, 2, 3 and 5 levels (absent levels re-read level 0 and are not summed; the divisor is the level count), ratios (1, 3), N = 2,
    level leading dimensions wider than C, an output window"""
    lv = [_in(dev, l) for l in K.inputs(c)['levels']]
    o = _out(dev, c['N'] * c['H0'] * c['W0'], c['out_ld'])
    L = len(lv)
    rc = hip.load().vps_bfp_gather(_ptrs(lv), _ints([c['lvl_ld']] * L), _ints(c['ratios']), L, o.p(), c['out_ld'], c['out_coff'], c['N'], c['H0'], c['W0'],
                                   c['C'], hip.stream_ptr())
    _check(c, dict(out=(o, c['out_coff'], c['C'])), lv, rc)


@pytest.mark.parametrize('c', **_ids('scatter'))
def test_bfp_scatter(dev, c):
    """ratios 1, 2, 3 (the min(dx0 + j, r - 1) duplicate columns), 4, 8; N = 2; quarter-step values with ties, +-0.0 and one -inf,
    bitwise against the restatement; leading dimensions wider than C"""
    inp = K.inputs(c)
    bsf, lvl = _in(dev, inp['bsf']), _in(dev, inp['level'])
    o = _out(dev, lvl.rows, c['ld'])
    rc = hip.load().vps_bfp_scatter(bsf.p(), c['ld'], lvl.p(), c['ld'], o.p(), c['ld'], c['N'], c['H0'], c['W0'], c['C'], c['r'], hip.stream_ptr())
    _check(c, dict(out=(o, 0, c['C'])), [bsf, lvl], rc)


@pytest.mark.parametrize('c', **_ids('scatter_all'))
def test_bfp_scatter_all(dev, c):
    """2, 3 and 5 levels in one pass, N = 2 (the block decode of cy and n), leading dimensions wider than C - against the restatement,
    not against vps_bfp_scatter"""
    inp = K.inputs(c)
    bsf, lv = _in(dev, inp['bsf']), [_in(dev, l) for l in inp['levels']]
    outs = [_out(dev, l.rows, c['ld']) for l in lv]
    lds = _ints([c['ld']] * c['L'])
    rc = hip.load().vps_bfp_scatter_all(bsf.p(), c['ld'], _ptrs(lv), lds, _ptrs(outs), lds, c['L'], c['N'], c['H0'], c['W0'], c['C'], hip.stream_ptr())
    _check(c, {'out%d' % l: (outs[l], 0, c['C']) for l in range(c['L'])}, [bsf] + lv, rc)


@pytest.mark.parametrize('c', **_ids('axpb'))
def test_axpb(dev, c):
    """C = 3 between windows of an 8- and a 12-wide buffer, as copy, scale and scale-and-shift: ONE fused multiply-add (the library is
    built with hipcc's default contraction, see tests/test_nn_restate.py), so bitwise np.float32(np.float64(x) a + b)"""
    x = _in(dev, K.inputs(c)['x'])
    o = _out(dev, c['npix'], c['out_ld'])
    rc = hip.load().vps_axpb(x.p(), c['in_ld'], c['in_coff'], o.p(), c['out_ld'], c['out_coff'], c['npix'], c['C'], c['a'], c['b'], hip.stream_ptr())
    _check(c, dict(out=(o, c['out_coff'], c['C'])), [x], rc)


@pytest.mark.parametrize('c', **_ids('groupnorm'))
def test_groupnorm(dev, c):
    """C from 256 down to 4 on the float4 path (pixels per block up to 256) and 2, 1 on the scalar one, 1 or 2 channels per group (a
    float4 spans several groups) and G = 1, fewer pixels than a block takes and a single pixel, relu off, in_ld > C, output windows on
    both paths; a constant input (the var < 0 -> 0 clamp: the output is relu(beta)); vps_groupnorm_apply with 1 and 3 partial copies
    of the float64 sums (one all zeros, one carrying a negative part).
    The far-mean cases (mean 1000, std 0.01) are ill-conditioned BY DESIGN. They show that the statistics are taken in float64: float32
    sums lose the variance altogether, which moves the output by whole units (and makes the bound derived from the float32 restatement
    useless, though it is derived like every other) - so they are held to K.groupnorm_affine_bound as well: the rounding of the float32
    affine (x - mean) sc + beta and of the float64 sums, from the number formats alone."""
    inp = K.inputs(c)
    x, g, b = _in(dev, inp['x']), _in(dev, inp['gamma']), _in(dev, inp['beta'])
    o = _out(dev, c['npix'], c['out_ld'])
    lib, ins = hip.load(), [x, g, b]
    if c['entry'] == 'apply':
        st = torch.from_numpy(inp['sums'].copy()).to(dev)
        rc = lib.vps_groupnorm_apply(x.p(), c['in_ld'], o.p(), c['out_ld'], c['out_coff'], c['npix'], c['C'], c['G'], g.p(), b.p(), 1e-5, c['relu'],
                                     hip.ptr(st), c['nrep'], hip.stream_ptr())
    else:
        st = torch.full((2 * c['G'] + 2,), 7.0, dtype=torch.float64, device=dev)
        rc = lib.vps_groupnorm_relu(x.p(), c['in_ld'], o.p(), c['out_ld'], c['out_coff'], c['npix'], c['C'], c['G'], g.p(), b.p(), 1e-5, c['relu'],
                                    hip.ptr(st), hip.stream_ptr())
    r64 = _check(c, dict(out=(o, c['out_coff'], c['C'])), ins, rc)
    if c['entry'] == 'apply':
        assert np.array_equal(st.cpu().numpy(), inp['sums']), 'the sums are read only'
    else:
        got, want = st.cpu().numpy(), K.R.group_sums(K.win(inp['x'], 0, c['C']), c['G'])
        assert (got[2 * c['G']:] == 7.0).all() and np.allclose(got[:2 * c['G']], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    if c['ill']:
        err = np.abs(o.bits()[1:-1, c['out_coff']:c['out_coff'] + c['C']].view(F32).astype(F64) - r64['out'])
        ab = K.groupnorm_affine_bound(c, inp)
        print('far mean: max err %.3g, affine bound %.3g' % (float(err.max()), ab))
        assert float(err.max()) <= ab


@pytest.mark.parametrize('c', **_ids('tcea_temporal'))
def test_tcea_temporal(dev, c):
    """C = 4 (one live lane), 64, 256, 512 (two trips of the channel loop); 1, 5 and 67 pixels (not a multiple of the 4 per block);
    emb_ld > 2 C, fea0 a window of a wider buffer, out_ld > 2 C.
    The saturated case (logits of magnitude ~1e3) is ill-conditioned BY DESIGN: it is there to show the sigmoid's limits - exactly 0 and 1
    times the feature, no NaN out of exp's overflow; its bound is derived like every other."""
    inp = K.inputs(c)
    emb, ref, f0, f1 = (_in(dev, inp[k]) for k in ('emb', 'emb_ref', 'fea0', 'fea1'))
    o = _out(dev, c['npix'], c['out_ld'])
    rc = hip.load().vps_tcea_temporal(emb.p(), c['emb_ld'], ref.p(), c['ref_ld'], f0.p(c['f0_coff']), c['f0_ld'], f1.p(), c['f1_ld'], o.p(), c['out_ld'],
                                      c['npix'], c['C'], hip.stream_ptr())
    _check(c, dict(out=(o, 0, 2 * c['C'])), [emb, ref, f0, f1], rc)


@pytest.mark.parametrize('c', **_ids('tcea_modulate'))
def test_tcea_modulate(dev, c):
    """the flat entry with 1 and 1027 elements; vps_tcea_modulate_ld (otherwise reached only when a wrapper sees a window) with four
    different leading dimensions; attention logits of +-100 among the rest"""
    inp = K.inputs(c)
    fea, att, add = (_in(dev, inp[k]) for k in ('fea', 'att', 'add'))
    l = c['lds']
    o = _out(dev, c['npix'], l[3])
    if c['entry'] == 'flat':
        rc = hip.load().vps_tcea_modulate(fea.p(), att.p(), add.p(), o.p(), c['npix'], hip.stream_ptr())
    else:
        rc = hip.load().vps_tcea_modulate_ld(fea.p(), l[0], att.p(), l[1], add.p(), l[2], o.p(), l[3], c['npix'], c['C'], hip.stream_ptr())
    _check(c, dict(out=(o, 0, c['C'])), [fea, att, add], rc)


# ------------------------------------------------------------------------------------------------ flow_ops.hip
@pytest.mark.parametrize('c', **_ids('nchw_to_nhwc,nhwc_to_nchw'))
def test_transposes(dev, c):
    """N > 1 (blockIdx.z), C and H W that are no multiples of the 32 x 32 tile, a single element, Cpad > C (the pad channels are +0.0),
    windows on the NHWC side - bit patterns (NaN payloads, -0.0, denormals) unchanged"""
    N, C, H, W = c['N'], c['C'], c['H'], c['W']
    x = K.inputs(c)['x']
    src = Buf(dev, x.view(F32), 1, x.size) if c['op'] == 'nchw_to_nhwc' else Buf(dev, x.view(F32), N * H * W, c['in_ld'])
    if c['op'] == 'nchw_to_nhwc':
        o = _out(dev, N * H * W, c['out_ld'])
        rc = hip.load().vps_nchw_to_nhwc(src.p(), o.p(), c['out_ld'], c['out_coff'], N, C, H, W, c['Cpad'], hip.stream_ptr())
        _check(c, dict(out=(o, c['out_coff'], c['Cpad'])), [src], rc)
    else:
        o = _out(dev, 1, N * C * H * W)
        rc = hip.load().vps_nhwc_to_nchw(src.p(), c['in_ld'], c['in_coff'], o.p(), N, C, H, W, hip.stream_ptr())
        _check(c, dict(out=(o, 0, N * C * H * W)), [src], rc)


def _t4(dev, a, lay, k, C, out=False):
    """a [B, C, H, W] as a vps_tensor4: lay 'c' = contiguous NCHW, 'h' = a channel window of an NHWC buffer (sc = 1, sw = ld) ->
    (Buf, Tensor4, coff, window width, rows)"""
    B, _, H, W = a.shape
    if lay == 'c':
        b = _out(dev, 1, a.size) if out else Buf(dev, a, 1, a.size)
        return b, hip.Tensor4(b.p(), C * H * W, H * W, W, 1), 0, a.size
    ld, coff = C + 3 + k, 1 + k
    b = _out(dev, B * H * W, ld) if out else _in(dev, K.wide(np.transpose(a, (0, 2, 3, 1)), ld, coff))
    return b, hip.Tensor4(b.p(coff), H * W * ld, 1, W * ld, ld), coff, C


@pytest.mark.parametrize('c', **_ids('resample2d,channelnorm'))
def test_resample2d_and_channelnorm(dev, c):
    """B = 2, C = 1, 3, 5; NCHW strides and NHWC windows (sc = 1, sw = ld) on input, flow and output independently; flows N(0, 3),
    all-integer (alpha = beta = 0), and a field that lands exactly on W - 1, on W - 1 + 0.5, on -0.5, at -7 and at W + 7 (likewise in y)"""
    inp = K.inputs(c)
    B, C, H, W = c['B'], c['C'], c['H'], c['W']
    lay = c['lay']
    img, ti, _, _ = _t4(dev, inp['img'], lay[0], 0, C)
    if c['op'] == 'resample2d':
        fl, tf, _, _ = _t4(dev, inp['flow'], lay[1], 1, 2)
        o, to, coff, width = _t4(dev, np.empty((B, C, H, W), dtype=F32), lay[2], 2, C, out=True)
        rc = hip.load().vps_resample2d(ti, tf, to, B, C, H, W, hip.stream_ptr())
        ins = [img, fl]
    else:
        o, to, coff, width = _t4(dev, np.empty((B, 1, H, W), dtype=F32), lay[1], 2, 1, out=True)
        rc = hip.load().vps_channelnorm(ti, to, B, C, H, W, hip.stream_ptr())
        ins = [img]
    # the restatement is NCHW: bring the expectation into an NHWC buffer's layout
    _check(c, dict(out=(o, coff, width)), ins, rc, relayout=(lambda v: np.transpose(v, (0, 2, 3, 1))) if lay[-1] == 'h' else None)


@pytest.mark.parametrize('c', **_ids('flow_warp'))
def test_flow_warp(dev, c):
    """N = 2, odd H and W (the two branches of linspace meet at n / 2), the smallest map 2 x 2, the flow read from channels [4, 6) of an
    8-wide buffer, input and output windows; flows N(0, 2), zero (NOT the identity: the reference's align_corners mismatch), everything
    beyond the map by more than a pixel (exactly +0.0, bitwise), and samples in (-1, 0) / (W - 1, W): one row or column of corners outside"""
    inp = K.inputs(c)
    x, f = _in(dev, inp['x']), _in(dev, inp['flow'])
    o = _out(dev, c['N'] * c['H'] * c['W'], c['out_ld'])
    rc = hip.load().vps_flow_warp(x.p(), c['in_ld'], c['in_coff'], f.p(), c['flow_ld'], c['flow_coff'], o.p(), c['out_ld'], c['out_coff'], c['N'], c['H'],
                                  c['W'], c['C'], hip.stream_ptr())
    _check(c, dict(out=(o, c['out_coff'], c['C'])), [x, f], rc)


@pytest.mark.parametrize('c', **_ids('flow_stage'))
def test_flow_stage(dev, c):
    """the smallest legal map 4 x 4 (a 1 x 1 low-resolution flow: yp = xp = 0 everywhere), 8 x 12, 20 x 36; bilinear and nearest with
    flo * mul and flo / mul; flow_out_div 0 and 20; each output alone and all together at non-overlapping offsets of a 16-wide buffer;
    x_ld 6 and 8 (img_off with x_ld != 8 among them); the low-resolution flow through flo_coff = 2 of a 4-wide buffer"""
    inp = K.inputs(c)
    x6, flo = _in(dev, inp['x6']), _in(dev, inp['flo'])
    H, W = c['H'], c['W']
    o = _out(dev, H * W, c['out_ld'])
    off = {k: (K.STAGE_OFFSETS[k] if k in c['outs'] else -1) for k in K.STAGE_OFFSETS}
    rc = hip.load().vps_flow_stage(x6.p(), c['x_ld'], flo.p(), c['flo_ld'], c['flo_coff'], H, W, c['up_mode'], c['mul'], c['div_mode'], o.p(), c['out_ld'],
                                   off['flow'], c['flow_out_div'], off['warp'], off['diffnorm'], off['flownorm'], off['img'], hip.stream_ptr())
    _check(c, {k: (o, K.STAGE_OFFSETS[k], K.STAGE_WIDTH[k]) for k in c['outs']}, [x6, flo], rc)


@pytest.mark.parametrize('c', **_ids('flow_stage_full'))
def test_flow_stage_full(dev, c):
    """the FlowNetS and the FlowNetFusion input at 4 x 4 and 8 x 12, against the restatement directly"""
    inp = K.inputs(c)
    x6, fa, fb = _in(dev, inp['x6']), _in(dev, inp['fa']), _in(dev, inp['fb'])
    o = _out(dev, c['H'] * c['W'], 12)
    rc = hip.load().vps_flow_stage_full(x6.p(), 8, fa.p(), c['a_ld'], c['a_coff'], fb.p(), c['b_ld'], c['b_coff'], c['H'], c['W'], c['mode'], c['mul'], o.p(), 12,
                                        hip.stream_ptr())
    _check(c, dict(out=(o, 0, 12)), [x6, fa, fb], rc)


@pytest.mark.parametrize('c', **_ids('flow_prep'))
def test_flow_prep_pad(dev, c):
    """no pad, a pad on both sides, a pad four times the frame; 1, 4 and 64 blocks for 35 / 256 pixels (blocks with empty loops must
    still write a zero partial sum); out_ld 8 and 12 (channels 6 .. out_ld are zeroed); rgb_mean against the float64 mean over the
    padded pair"""
    inp = K.inputs(c)
    img, ref, mean, std = (_in(dev, inp[k]) for k in ('img', 'ref', 'mean3', 'std3'))
    o = _out(dev, c['Hp'] * c['Wp'], c['out_ld'])
    partial = torch.full((3 * c['nblk'] + 2,), 7.0, dtype=torch.float64, device=dev)
    rgb = _out(dev, 1, 3)
    rc = hip.load().vps_flow_prep_pad(img.p(), ref.p(), mean.p(), std.p(), o.p(), c['out_ld'], c['H'], c['W'], c['Hp'], c['Wp'], hip.ptr(partial), c['nblk'],
                                      rgb.p(), hip.stream_ptr())
    _check(c, dict(out=(o, 0, 6), zeros=(o, 6, c['out_ld'] - 6), rgb_mean=(rgb, 0, 3)), [img, ref, mean, std], rc)
    assert (partial[3 * c['nblk']:] == 7.0).all()


# ------------------------------------------------------------------------------------------------ argument refusals
def _refusals():
    """(id, entry point, arguments with 'A' .. 'D' = valid input buffers, 'O' = the sentinel output, None = a null pointer). Only what
    the entry points refuse BEFORE any launch: nothing here could be launched and read out of bounds."""
    i = lambda *v: ('ints', v)
    p = lambda *k: ('ptrs', k)
    s = 'S'                                                                     # the stream
    return [
        ('resize_null_in', 'vps_resize', (None, 8, 0, 4, 4, 'O', 8, 0, 4, 4, 1, 8, 0, 1.0, s)),
        ('resize_null_out', 'vps_resize', ('A', 8, 0, 4, 4, None, 8, 0, 4, 4, 1, 8, 0, 1.0, s)),
        ('resize_Ho0', 'vps_resize', ('A', 8, 0, 4, 4, 'O', 8, 0, 0, 4, 1, 8, 0, 1.0, s)),
        ('pool_null', 'vps_pool3x3s2', (None, 8, 0, 4, 4, 'O', 8, 0, 1, 8, 0, s)),
        ('pool_C0', 'vps_pool3x3s2', ('A', 8, 0, 4, 4, 'O', 8, 0, 1, 0, 0, s)),
        ('gather_L0', 'vps_bfp_gather', (p('A'), i(8), i(1), 0, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('gather_L6', 'vps_bfp_gather', (p('A', 'A', 'A', 'A', 'A', 'A'), i(8, 8, 8, 8, 8, 8), i(1, 1, 1, 1, 1, 1), 6, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('gather_C6', 'vps_bfp_gather', (p('A'), i(8), i(1), 1, 'O', 8, 0, 1, 4, 4, 6, s)),
        ('gather_out_ld', 'vps_bfp_gather', (p('A'), i(8), i(1), 1, 'O', 10, 0, 1, 4, 4, 8, s)),
        ('gather_out_coff', 'vps_bfp_gather', (p('A'), i(8), i(1), 1, 'O', 12, 2, 1, 4, 4, 8, s)),
        ('gather_lvl_ld', 'vps_bfp_gather', (p('A'), i(10), i(1), 1, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('gather_ratio', 'vps_bfp_gather', (p('A', 'B'), i(8, 8), i(1, 3), 2, 'O', 8, 0, 1, 4, 4, 8, s)),          # H0 % ratio != 0
        ('gather_null_level', 'vps_bfp_gather', (p('A', None), i(8, 8), i(1, 2), 2, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('scatter_C6', 'vps_bfp_scatter', ('A', 8, 'B', 8, 'O', 8, 1, 4, 4, 6, 2, s)),
        ('scatter_ld', 'vps_bfp_scatter', ('A', 10, 'B', 8, 'O', 8, 1, 4, 4, 8, 2, s)),
        ('scatter_ratio', 'vps_bfp_scatter', ('A', 8, 'B', 8, 'O', 8, 1, 4, 4, 8, 3, s)),
        ('scatter_null', 'vps_bfp_scatter', ('A', 8, None, 8, 'O', 8, 1, 4, 4, 8, 2, s)),
        ('scatter_all_L1', 'vps_bfp_scatter_all', ('A', 32, p('B', 'C'), i(32, 32), p('O', 'O'), i(32, 32), 1, 1, 4, 4, 32, s)),
        ('scatter_all_L6', 'vps_bfp_scatter_all', ('A', 32, p('B', 'C'), i(32, 32), p('O', 'O'), i(32, 32), 6, 1, 32, 32, 32, s)),
        ('scatter_all_C8', 'vps_bfp_scatter_all', ('A', 8, p('B', 'C'), i(8, 8), p('O', 'O'), i(8, 8), 2, 1, 4, 4, 8, s)),
        ('scatter_all_H', 'vps_bfp_scatter_all', ('A', 32, p('B', 'C'), i(32, 32), p('O', 'O'), i(32, 32), 2, 1, 3, 4, 32, s)),
        ('scatter_all_null_out', 'vps_bfp_scatter_all', ('A', 32, p('B', 'C'), i(32, 32), p('O', None), i(32, 32), 2, 1, 4, 4, 32, s)),
        ('axpb_null', 'vps_axpb', ('A', 8, 0, None, 8, 0, 4, 3, 1.0, 0.0, s)),
        ('axpb_npix0', 'vps_axpb', ('A', 8, 0, 'O', 8, 0, 0, 3, 1.0, 0.0, s)),
        ('gn_C24', 'vps_groupnorm_relu', ('A', 24, 'O', 24, 0, 4, 24, 4, 'B', 'C', 1e-5, 1, 'D', s)),              # 256 % C != 0
        ('gn_G3', 'vps_groupnorm_relu', ('A', 16, 'O', 16, 0, 4, 16, 3, 'B', 'C', 1e-5, 1, 'D', s)),               # C % G != 0
        ('gn_C512', 'vps_groupnorm_relu', ('A', 512, 'O', 512, 0, 1, 512, 32, 'B', 'C', 1e-5, 1, 'D', s)),
        ('gn_null_stats', 'vps_groupnorm_relu', ('A', 16, 'O', 16, 0, 4, 16, 4, 'B', 'C', 1e-5, 1, None, s)),
        ('gn_apply_nrep0', 'vps_groupnorm_apply', ('A', 16, 'O', 16, 0, 4, 16, 4, 'B', 'C', 1e-5, 1, 'D', 0, s)),
        ('gn_apply_G3', 'vps_groupnorm_apply', ('A', 16, 'O', 16, 0, 4, 16, 3, 'B', 'C', 1e-5, 1, 'D', 1, s)),
        ('tcea_C6', 'vps_tcea_temporal', ('A', 16, 'B', 8, 'C', 8, 'D', 8, 'O', 16, 4, 6, s)),
        ('tcea_ld', 'vps_tcea_temporal', ('A', 18, 'B', 8, 'C', 8, 'D', 8, 'O', 16, 4, 8, s)),
        ('tcea_misaligned', 'vps_tcea_temporal', ('A', 16, 'B', 8, ('C', 4), 8, 'D', 8, 'O', 16, 4, 8, s)),         # a pointer 4 bytes off the 16-byte grid
        ('tcea_null', 'vps_tcea_temporal', ('A', 16, 'B', 8, 'C', 8, None, 8, 'O', 16, 4, 8, s)),
        ('modulate_null', 'vps_tcea_modulate', ('A', 'B', None, 'O', 16, s)),
        ('modulate_n0', 'vps_tcea_modulate', ('A', 'B', 'C', 'O', 0, s)),
        ('modulate_ld_C6', 'vps_tcea_modulate_ld', ('A', 8, 'B', 8, 'C', 8, 'O', 8, 4, 6, s)),
        ('modulate_ld_ld', 'vps_tcea_modulate_ld', ('A', 8, 'B', 10, 'C', 8, 'O', 8, 4, 8, s)),
        ('modulate_ld_misaligned', 'vps_tcea_modulate_ld', ('A', 8, 'B', 8, 'C', 8, ('O', 8), 8, 4, 8, s)),
        ('warp_H1', 'vps_flow_warp', ('A', 8, 0, 'B', 2, 0, 'O', 8, 0, 1, 1, 8, 8, s)),
        ('warp_W1', 'vps_flow_warp', ('A', 8, 0, 'B', 2, 0, 'O', 8, 0, 1, 8, 1, 8, s)),
        ('warp_C6', 'vps_flow_warp', ('A', 8, 0, 'B', 2, 0, 'O', 8, 0, 1, 4, 4, 6, s)),
        ('warp_in_coff', 'vps_flow_warp', ('A', 16, 2, 'B', 2, 0, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('warp_out_ld', 'vps_flow_warp', ('A', 8, 0, 'B', 2, 0, 'O', 10, 0, 1, 4, 4, 8, s)),
        ('warp_null_flow', 'vps_flow_warp', ('A', 8, 0, None, 2, 0, 'O', 8, 0, 1, 4, 4, 8, s)),
        ('to_nhwc_Cpad', 'vps_nchw_to_nhwc', ('A', 'O', 8, 0, 1, 8, 4, 4, 7, s)),                                  # Cpad < C
        ('to_nhwc_null', 'vps_nchw_to_nhwc', (None, 'O', 8, 0, 1, 8, 4, 4, 8, s)),
        ('to_nchw_null', 'vps_nhwc_to_nchw', ('A', 8, 0, None, 1, 8, 4, 4, s)),
        ('to_nchw_N0', 'vps_nhwc_to_nchw', ('A', 8, 0, 'O', 0, 8, 4, 4, s)),
        ('prep_nblk0', 'vps_flow_prep_pad', ('A', 'B', 'C', 'C', 'O', 8, 4, 4, 4, 4, 'D', 0, 'E', s)),
        ('prep_nblk2049', 'vps_flow_prep_pad', ('A', 'B', 'C', 'C', 'O', 8, 4, 4, 4, 4, 'D', 2049, 'E', s)),
        ('prep_out_ld', 'vps_flow_prep_pad', ('A', 'B', 'C', 'C', 'O', 5, 4, 4, 4, 4, 'D', 4, 'E', s)),
        ('prep_Hp', 'vps_flow_prep_pad', ('A', 'B', 'C', 'C', 'O', 8, 4, 4, 3, 4, 'D', 4, 'E', s)),
        ('prep_null_partial', 'vps_flow_prep_pad', ('A', 'B', 'C', 'C', 'O', 8, 4, 4, 4, 4, None, 4, 'E', s)),
        ('stage_H6', 'vps_flow_stage', ('A', 8, 'B', 2, 0, 6, 8, 0, 20.0, 0, 'O', 16, 0, 0.0, -1, -1, -1, -1, s)),   # H & 3
        ('stage_W2', 'vps_flow_stage', ('A', 8, 'B', 2, 0, 4, 2, 0, 20.0, 0, 'O', 16, 0, 0.0, -1, -1, -1, -1, s)),
        ('stage_null', 'vps_flow_stage', ('A', 8, None, 2, 0, 4, 4, 0, 20.0, 0, 'O', 16, 0, 0.0, -1, -1, -1, -1, s)),
        ('full_H6', 'vps_flow_stage_full', ('A', 8, 'B', 2, 0, 'C', 2, 0, 6, 8, 0, 20.0, 'O', 12, s)),
        ('full_x_ld', 'vps_flow_stage_full', ('A', 6, 'B', 2, 0, 'C', 2, 0, 4, 4, 0, 20.0, 'O', 12, s)),
        ('full_mul0', 'vps_flow_stage_full', ('A', 8, 'B', 2, 0, 'C', 2, 0, 4, 4, 0, 0.0, 'O', 12, s)),
        ('full_out_ld', 'vps_flow_stage_full', ('A', 8, 'B', 2, 0, 'C', 2, 0, 4, 4, 0, 20.0, 'O', 16, s)),
        ('full_mode2', 'vps_flow_stage_full', ('A', 8, 'B', 2, 0, 'C', 2, 0, 4, 4, 2, 20.0, 'O', 12, s)),
        ('full_mode1_null_b', 'vps_flow_stage_full', ('A', 8, 'B', 2, 0, None, 2, 0, 4, 4, 1, 20.0, 'O', 12, s)),
        ('full_misaligned', 'vps_flow_stage_full', (('A', 4), 8, 'B', 2, 0, 'C', 2, 0, 4, 4, 0, 20.0, 'O', 12, s)),
        ('resample2d_null', 'vps_resample2d', (('t4', None), ('t4', 'B'), ('t4', 'O'), 1, 3, 4, 4, s)),
        ('resample2d_C0', 'vps_resample2d', (('t4', 'A'), ('t4', 'B'), ('t4', 'O'), 1, 0, 4, 4, s)),
        ('channelnorm_null', 'vps_channelnorm', (('t4', 'A'), ('t4', None), 1, 3, 4, 4, s)),
        ('channelnorm_B0', 'vps_channelnorm', (('t4', 'A'), ('t4', 'O'), 0, 3, 4, 4, s)),
    ]


@pytest.mark.parametrize('name,entry,args', _refusals(), ids=[r[0] for r in _refusals()])
def test_argument_refusals(dev, name, entry, args):
    """every entry point hands a shape, leading dimension, offset, count or null pointer it does not take back with a non-zero code
    BEFORE any launch: the sentinel-filled output (and every input) is untouched after a synchronise"""
    bufs = {k: Buf(dev, np.zeros((1024, 4), dtype=F32), 1024, 4) for k in 'ABCDE'}
    bufs['O'] = _out(dev, 1024, 4)
    keep = []

    def conv(a):
        if a == 'S':
            return hip.stream_ptr()
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, str):
            return bufs[a].p()
        kind, v = a
        if kind == 'ints':
            return _ints(v)
        if kind == 'ptrs':
            arr = (ctypes.c_void_p * len(v))(*[None if k is None else bufs[k].p() for k in v])
            keep.append(arr)
            return arr
        if kind == 't4':
            return hip.Tensor4(None if v is None else bufs[v].p(), 48, 16, 4, 1)
        return bufs[kind].p(v // 4)                                            # (buffer, byte offset): a misaligned pointer
    if 'nblk2049' in name or 'nblk0' in name:
        bufs['D'] = Buf(dev, np.zeros((4096, 4), dtype=F32), 4096, 4)
    rc = getattr(hip.load(), entry)(*[conv(a) for a in args])
    torch.cuda.synchronize()
    assert rc != 0, '%s accepted %s' % (entry, name)
    for k, b in bufs.items():
        assert b.unchanged(), '%s: buffer %s written by a refused call' % (name, k)
