"""CPU tests of tests/nn_restate.py, the yardstick of tests/test_nn_ops_gpu.py (no GPU needed).

1. Pinning: the float32 evaluation of every restatement against what the project already trusts (torch on the CPU, the oracle) - exactly
   where values are only moved or selected, to a stated number of float32 ulps of the output magnitude elsewhere (measured figures in
   the comments beside the asserts).
2. For EVERY case the GPU tests run (tests/nn_cases.py): the bound the GPU test will derive stays under the cap (what tests/test_hip_ops.py
   allows the same kernel), and every deliberately wrong variant listed for the case differs from the right restatement by more than ten
   times that bound (exact cases: in at least one element) - on the very inputs the GPU test uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_cases as K
import nn_restate as R
from oracle import flownet2 as OFN
from oracle import fusetrack as OF
from oracle import ops as O

F32, F64 = np.float32, np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _nchw(a):
    return _t(np.transpose(a, (0, 3, 1, 2)))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _ulps(got, want):
    """max|got - want| in float32 ulps of the largest |want|"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return float(np.abs(got - want).max() / np.spacing(F32(np.abs(want).max())))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. pinning
def test_nearest_index_is_torch_float32_cpu_for_every_small_size():
    for Hi in range(1, 20):
        src = torch.arange(Hi, dtype=torch.float32).view(1, 1, Hi, 1)
        for Ho in range(1, 40):
            want = F.interpolate(src, size=(Ho, 1), mode='nearest').view(-1).long().numpy()
            assert np.array_equal(R.nearest_index(Hi, Ho), want), (Hi, Ho)


@pytest.mark.parametrize('c', K.cases('resize'), ids=K.case_id)
def test_resize_is_torch_interpolate(c):
    x = K.win(K.inputs(c)['x'], c['in_coff'], c['C'])
    if c['mode'] == 'nearest':
        want = _nhwc(F.interpolate(_nchw(x), size=(c['Ho'], c['Wo']), mode='nearest')) * F32(c['alpha'])
        assert np.array_equal(_bits(R.resize(x, c['Ho'], c['Wo'], 'nearest', c['alpha'], F32)), _bits(want))
    else:
        want = _nhwc(F.interpolate(_nchw(x), size=(c['Ho'], c['Wo']), mode='bilinear', align_corners=False)) * F32(c['alpha'])
        assert _ulps(R.resize(x, c['Ho'], c['Wo'], 'bilinear', c['alpha'], F32), want) <= 4          # a few ulps; measured <= 2
        assert _ulps(R.resize(x, c['Ho'], c['Wo'], 'bilinear', c['alpha'], F64), want) <= 4          # measured <= 1.08 (float32 index, float64 values)


@pytest.mark.parametrize('c', K.cases('pool'), ids=K.case_id)
def test_pool_is_torch_pool(c):
    x = K.win(K.inputs(c)['x'], c['in_coff'], c['C'])
    got = R.pool3x3s2(x, c['mode'], F32)
    if c['mode'] == 'max':
        assert np.array_equal(_bits(got), _bits(_nhwc(F.max_pool2d(_nchw(x), 3, 2, 1))))
    else:
        assert _ulps(got, _nhwc(F.avg_pool2d(_nchw(x), 3, 2, 1, count_include_pad=True))) <= 2          # measured 0


@pytest.mark.parametrize('c', K.cases('gather'), ids=K.case_id)
def test_gather_is_the_oracle(c):
    lv = [K.win(l, 0, c['C']) for l in K.inputs(c)['levels']]
    assert _ulps(R.bfp_gather(lv, c['ratios'], F32), _nhwc(OF.bfp_gather([_nchw(l) for l in lv]))) <= 1     # measured 0 (same order of additions)


@pytest.mark.parametrize('c', K.cases('scatter', 'scatter_all'), ids=K.case_id)
def test_scatter_pooling_is_adaptive_max_pool(c):
    inp = K.inputs(c)
    bsf = K.win(inp['bsf'], 0, c['C']).copy()
    bsf[bsf == 0] = F32(0.5)                          # the sign of a maximum over {+0.0, -0.0} is no property of either implementation
    for r in ([c['r']] if c['op'] == 'scatter' else [1 << l for l in range(c['L'])]):
        zero = np.zeros((c['N'], c['H0'] // r, c['W0'] // r, c['C']), dtype=F32)
        want = _nhwc(F.adaptive_max_pool2d(_nchw(bsf), (c['H0'] // r, c['W0'] // r)))
        assert np.array_equal(_bits(R.bfp_scatter(bsf, zero, r, F32)), _bits(want))


@pytest.mark.parametrize('c', K.cases('nchw_to_nhwc', 'nhwc_to_nchw'), ids=K.case_id)
def test_transposes_are_permute(c):
    x = K.inputs(c)['x']
    if c['op'] == 'nchw_to_nhwc':
        got = R.nchw_to_nhwc(x, c['Cpad'])
        assert np.array_equal(got[..., :c['C']], _t(x).permute(0, 2, 3, 1).numpy()) and not got[..., c['C']:].any()
    else:
        w = np.ascontiguousarray(K.win(x, c['in_coff'], c['C']))
        assert np.array_equal(R.nhwc_to_nchw(w), _t(w).permute(0, 3, 1, 2).contiguous().numpy())


@pytest.mark.parametrize('c', [c for c in K.cases('groupnorm') if c['entry'] == 'relu' and not c['ill']], ids=K.case_id)
def test_groupnorm_is_torch_group_norm_in_float64(c):
    inp = K.inputs(c)
    x = K.win(inp['x'], 0, c['C'])
    want = F.group_norm(_t(x.T[None].astype(F64)), c['G'], _t(inp['gamma'].astype(F64)), _t(inp['beta'].astype(F64)), 1e-5)
    if c['relu']:
        want = F.relu(want)
    want = want[0].numpy().T
    # eps: the kernel's is the float32 1e-5, torch's the double 1e-5 - 2.5e-13 apart, nothing against a variance of 4 (or eps itself)
    assert _ulps(R.groupnorm(x, c['G'], inp['gamma'], inp['beta'], 1e-5, c['relu'], F64), want) <= 0.01      # measured <= 3e-4 ulp
    if c['data'] == 'constant':
        assert np.abs(R.groupnorm(x, c['G'], inp['gamma'], inp['beta'], 1e-5, c['relu'], F64) -
                      (np.maximum(inp['beta'], 0) if c['relu'] else inp['beta'])).max() == 0


def test_groupnorm_from_split_sums_is_groupnorm():
    for c in [c for c in K.cases('groupnorm') if c['entry'] == 'apply']:
        inp = K.inputs(c)
        x = K.win(inp['x'], 0, c['C'])
        a = R.groupnorm(x, c['G'], inp['gamma'], inp['beta'], 1e-5, c['relu'], F64, sums=inp['sums'])
        b = R.groupnorm(x, c['G'], inp['gamma'], inp['beta'], 1e-5, c['relu'], F64)
        assert inp['sums'].shape == (c['nrep'], 2 * c['G']) and _ulps(a, b) <= 0.01
        if c['nrep'] == 3:
            assert not inp['sums'][1].any() and (inp['sums'][2, 1::2] < 0).all()


@pytest.mark.parametrize('c', K.cases('tcea_temporal', 'tcea_modulate'), ids=K.case_id)
def test_tcea_is_torch(c):
    inp, C = K.inputs(c), c['C']
    if c['op'] == 'tcea_modulate':
        fea, att, add = (_t(K.win(inp[k], 0, C)) for k in ('fea', 'att', 'add'))
        assert _ulps(R.tcea_modulate(fea.numpy(), att.numpy(), add.numpy(), F32), (fea * torch.sigmoid(att) * 2 + add).numpy()) <= 2   # measured <= 0.5
        return
    emb, ref, f0, f1 = (_t(K.win(inp['emb'], 0, 2 * C)).double(), _t(K.win(inp['emb_ref'], 0, C)).double(),
                        _t(K.win(inp['fea0'], c['f0_coff'], C)).double(), _t(K.win(inp['fea1'], 0, C)).double())
    cor = [torch.sigmoid((emb[:, i * C:(i + 1) * C] * ref).sum(1, keepdim=True)) for i in range(2)]
    want = torch.cat([f0 * cor[0], f1 * cor[1]], 1).numpy()
    got = R.tcea_temporal(*(t.numpy() for t in (emb, ref, f0, f1)), F64)
    assert np.isfinite(got).all() and _ulps(got, want) <= 0.01                  # measured <= 3e-7 ulp; the saturated case too: limits 0 and 1, no NaN


@pytest.mark.parametrize('c', K.cases('resample2d', 'channelnorm'), ids=K.case_id)
def test_resample2d_and_channelnorm_are_the_oracle(c):
    inp = K.inputs(c)
    if c['op'] == 'channelnorm':
        assert _ulps(R.channelnorm(inp['img'], F32), O.channelnorm(_t(inp['img'])).numpy()) <= 2                 # measured <= 1
    else:
        # the oracle takes the products in double and rounds each to float32 (as the reference does); the float32 restatement takes them in float32
        assert _ulps(R.resample2d(inp['img'], inp['flow'], F32), O.resample2d(_t(inp['img']), _t(inp['flow'])).numpy()) <= 2     # measured <= 1
        assert _ulps(R.resample2d(inp['img'], inp['flow'], F64), O.resample2d(_t(inp['img']), _t(inp['flow'])).numpy()) <= 2     # measured <= 1.01


@pytest.mark.parametrize('c', K.cases('flow_warp'), ids=K.case_id)
def test_flow_warp_is_the_oracle_warping_layer(c):
    inp = K.inputs(c)
    x, f = K.win(inp['x'], c['in_coff'], c['C']), K.win(inp['flow'], c['flow_coff'], 2)
    want = _nhwc(OF.warping_layer(_nchw(x), _nchw(f)))
    got = R.flow_warp(x, f, F32)
    if c['flows'] == 'outside':
        assert not want.any() and np.array_equal(_bits(R.flow_warp(x, f, F64)), np.zeros(x.shape, dtype=np.int32))      # exactly +0.0
    else:
        # float32 coordinates carry ~ulp(W) of noise, multiplied by the differences of neighbouring N(0, 1) values
        assert np.abs(got - want).max() <= 64 * np.spacing(F32(max(c['H'], c['W'])))          # measured <= 5.9 ulp(W)
    if c['flows'] == 'zero':
        assert np.abs(R.flow_warp(x, f, F64) - x).max() > 0.1                      # the align_corners mismatch: zero flow is not the identity


@pytest.mark.parametrize('c', K.cases('flow_stage_full'), ids=K.case_id)
def test_flow_stage_is_the_torch_oracle_composition(c):
    """the composition written out in test_flow_stage_full_pixel_kernels of tests/test_hip_ops.py (flownet2.py:142-187)"""
    inp = K.inputs(c)
    D = c['mul']
    x6 = K.win(inp['x6'], 0, 6)
    img = _nchw(x6[None])
    fa, fb = _nchw(K.win(inp['fa'], c['a_coff'], 2)[None]), _nchw(K.win(inp['fb'], c['b_coff'], 2)[None])
    if c['mode'] == 0:
        up = F.interpolate(fa * D, scale_factor=4, mode='bilinear', align_corners=False)
        warped = O.resample2d(img[:, 3:], up)
        want = torch.cat([img, warped, up / D, O.channelnorm(img[:, :3] - warped)], dim=1)
    else:
        f2 = F.interpolate(fa * D, scale_factor=4, mode='nearest'); fd = F.interpolate(fb / D, scale_factor=4, mode='nearest')
        want = torch.cat([img[:, :3], fd, f2, O.channelnorm(fd), O.channelnorm(f2), O.channelnorm(img[:, :3] - O.resample2d(img[:, 3:], fd)),
                          O.channelnorm(img[:, :3] - O.resample2d(img[:, 3:], f2)), torch.zeros_like(fd[:, :1])], dim=1)
    got = R.flow_stage_full(x6, K.win(inp['fa'], c['a_coff'], 2), K.win(inp['fb'], c['b_coff'], 2), c['mode'], D, F32)
    assert got.shape == (c['H'], c['W'], 12)
    # a flow of +-4 pixels moves by an ulp (5e-7) between two float32 evaluations, times the image's differences (N(0, 0.25)): 1e-6
    assert np.abs(got - _nhwc(want)[0]).max() <= 2e-6


@pytest.mark.parametrize('c', K.cases('flow_prep'), ids=K.case_id)
def test_flow_prep_is_the_oracle_flow_input(c):
    inp = K.inputs(c)
    out, mean = R.flow_prep(inp['img'], inp['ref'], inp['mean3'], inp['std3'], c['H'], c['W'], F32)       # the oracle pads its two special sizes only
    want = OFN.flow_input(_t(inp['img'])[None], _t(inp['ref'])[None], inp['mean3'].tolist(), inp['std3'].tolist())[0]
    assert _ulps(out, want.permute(1, 2, 0).numpy()) <= 4                           # measured <= 1.5
    # the padded mean: pad pixels add 0 to the sums and count in the divisor
    outp, meanp = R.flow_prep(inp['img'], inp['ref'], inp['mean3'], inp['std3'], c['Hp'], c['Wp'], F64)
    _, m64 = R.flow_prep(inp['img'], inp['ref'], inp['mean3'], inp['std3'], c['H'], c['W'], F64)
    assert np.allclose(meanp, m64 * (c['H'] * c['W']) / (c['Hp'] * c['Wp']), rtol=1e-12)
    assert np.allclose(outp[c['H']:], -np.tile(meanp, 2) / 255, rtol=1e-12) and np.allclose(outp[:, c['W']:], -np.tile(meanp, 2) / 255, rtol=1e-12)


def test_axpb_is_one_fused_multiply_add():
    """vps_amd/csrc/Makefile sets no -ffp-contract: hipcc's default for device code is `fast`, x * a + b becomes ONE v_fma_f32 (one rounding).
    float64 holds the product of two float32 exactly, so float64 arithmetic cast to float32 is that single rounding."""
    mk = open(K.__file__.replace('tests/nn_cases.py', 'vps_amd/csrc/Makefile')).read()
    assert 'ffp-contract' not in mk
    for c in K.cases('axpb'):
        x = K.win(K.inputs(c)['x'], c['in_coff'], c['C'])
        fused = K.expected_bits(c, K.reference(c, K.inputs(c), F64))['out']
        assert np.array_equal(_bits(fused), _bits(R.axpb(x, c['a'], c['b'], F64, fma=True)))
        two = R.axpb(x, c['a'], c['b'], F32)
        assert _ulps(two, fused) <= 1
        if c['b'] == 0:
            assert np.array_equal(_bits(two), _bits(fused))                        # nothing to contract


# ------------------------------------------------------------------------------------------------ 2. every GPU case: bound <= cap, wrong is caught
def test_the_case_table_covers_what_the_issue_lists():
    ids = [(c['op'], c['id']) for c in K.CASES]
    assert len(set(ids)) == len(ids)
    gn = K.cases('groupnorm')
    assert {(c['C'], c['G']) for c in gn if c['npix'] == 37} >= {(256, 32), (64, 32), (32, 32), (16, 4), (8, 8), (4, 1), (4, 4), (2, 1), (1, 1), (128, 1)}
    for C in (64, 2):
        assert {c['npix'] for c in gn if c['C'] == C} >= {1, 3, 37, 560}
    assert {(c['nrep'], c['relu'], c['out_ld'] & 3) for c in gn if c['entry'] == 'apply'} == {(n, r, p) for n in (1, 3) for r in (0, 1) for p in (0, 3)}
    fs = K.cases('flow_stage')
    assert {(c['H'], c['up_mode'], c['div_mode']) for c in fs} == {(h, u, d) for h in (4, 8, 20) for u in (0, 1) for d in (0, 1)}
    assert {c['outs'] for c in fs} >= {('flow',), ('warp',), ('diffnorm',), ('flownorm',), ('img',), tuple(K.STAGE_OFFSETS)}
    assert any(c['outs'] == ('img',) and c['x_ld'] == 6 for c in fs) and any(c['div_mode'] == 1 and c['up_mode'] == 0 for c in fs)
    assert any(c['outs'] == ('flownorm',) for c in fs) and {c['flow_out_div'] for c in fs} == {0.0, 20.0}


@pytest.mark.parametrize('c', K.CASES, ids=lambda c: '%s-%s' % (c['op'], c['id']))
def test_every_gpu_case_has_its_bound_under_the_cap_and_tells_wrong_from_right(c):
    inp = K.inputs(c)
    r64 = K.reference(c, inp, F64)
    assert c['wrong'], 'every case names at least one wrong variant'
    if c['exact']:
        want = K.expected_bits(c, r64)
        for w in c['wrong']:
            bad = K.expected_bits(c, K.reference(c, inp, F64, w))
            assert any(not np.array_equal(bad[k].view(np.int32), want[k].view(np.int32)) for k in want), w
        return
    r32 = K.reference(c, inp, F32)
    bnd = K.bounds(c, r32, r64)
    ill = c.get('ill', False)
    for k, (b, dist, floor, cap) in bnd.items():
        assert np.isfinite(r64[k]).all() and r64[k].dtype == F64 and r32[k].dtype == F32
        # the two cases that are ill-conditioned by design (far-mean GroupNorm, saturated TCEA logits) derive their bound in the same way but
        # cannot meet the cap of the well-conditioned ones: see their comments in tests/test_nn_ops_gpu.py
        assert ill or b <= cap, '%s: bound %.3g (float32 vs float64 %.3g, floor %.3g) above the cap %.3g' % (k, b, dist, floor, cap)
    applied = {k: v[0] for k, v in bnd.items()}
    if c['op'] == 'groupnorm' and ill:
        applied['out'] = min(applied['out'], K.groupnorm_affine_bound(c, inp))
    for w in c['wrong']:
        bad = K.reference(c, inp, F64, w)
        assert any(float(np.abs(bad[k] - r64[k]).max()) > 10 * applied[k] for k in r64), (w, {k: float(np.abs(bad[k] - r64[k]).max()) for k in r64}, applied)
