"""CPU tests of tests/corr_restate.py and tests/corr_cases.py, the yardstick and the case table of tests/test_corr_gpu.py (no GPU needed).

1. Pinning: the float32 restatement is oracle.ops.correlation to within summation order, on the two configurations of the path and on
   off-path ones; its mask is where the oracle's zero padding is read.
2. For EVERY exact case of the table the bound the GPU test will derive stays under what tests/test_hip_ops.py allows the exact kernels;
   the inputs hold no zero and differ per image.
3. The table's intent: expected_route - the dispatch of vps_correlation / vps_correlation_f16 restated in Python - gives every case the
   kernel its row is there for, and every route reachable at the default switch values has the cases the table was written to hold.
   (Which kernel RAN is not observed on the device.)
4. What vps_correlation and vps_correlation_f16 refuse before any launch (the library loads without a GPU)."""
import numpy as np
import pytest
import torch

import corr_cases as K
import corr_restate as R
from oracle import ops as O
from vps_amd import hip

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ 1. pinning
@pytest.mark.parametrize('N,H,W,C,md,s2', [(2, 6, 16, 32, 20, 2), (2, 9, 12, 36, 4, 1), (1, 7, 9, 8, 6, 3), (2, 5, 7, 4, 0, 1), (1, 4, 6, 260, 3, 1)])
def test_the_float32_restatement_is_the_oracle(N, H, W, C, md, s2):
    c = dict(id='pin_%d_%d_%d_%d_%d_%d' % (N, H, W, C, md, s2), N=N, H=H, W=W, C=C)
    inp = K.inputs(c)
    a, b = (torch.from_numpy(np.ascontiguousarray(np.transpose(inp[k], (0, 3, 1, 2)))) for k in ('in1', 'in2'))
    want = O.correlation(a, b, md, 1, md, 1, s2).permute(0, 2, 3, 1).numpy()
    got, outside = R.correlation(inp['in1'], inp['in2'], md, s2, F32)
    assert got.dtype == F32 and got.shape == want.shape
    # the same float32 products in another summation order (torch's sum over a strided axis, / C for * (1 / C)): C ulps of the largest
    # sum of |products| / C would be the worst case; a few ulps of the largest output is what pairwise sums leave (measured <= 1.5)
    assert np.abs(got.astype(F64) - want).max() <= 4 * np.spacing(F32(np.abs(want).max()))
    got64, o64 = R.correlation(inp['in1'], inp['in2'], md, s2, F64)
    assert got64.dtype == F64 and np.array_equal(o64, outside)
    assert np.abs(got64 - want).max() <= 4 * np.spacing(F32(np.abs(want).max()))
    # the mask: exactly where the oracle reads its zero padding - an all-ones in2 correlates to mean(in1) inside and to 0 there
    ones = O.correlation(torch.ones_like(a), torch.ones_like(b), md, 1, md, 1, s2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(outside, ones == 0) and not got[outside].any() and not got64[outside].any()
    assert (got64[~outside] != 0).all()
    lk, _ = R.correlation(inp['in1'], inp['in2'], md, s2, F64, 'leaky', 0.1)
    assert np.array_equal(lk, np.where(got64 > 0, got64, got64 * F64(F32(0.1)))) and np.array_equal(np.signbit(lk), np.signbit(got64))


# ------------------------------------------------------------------------------------------------ 2. inputs and bounds of every case
@pytest.mark.parametrize('c', K.CASES, ids=K.case_id)
def test_every_case_has_inputs_without_zeros_and_its_bound_under_the_cap(c):
    ref = K.reference(c)
    L = K.layout(c)
    a, b = ref['inp']['in1'], ref['inp']['in2']
    assert a.shape == b.shape == (c['N'], c['H'], c['W'], c['C']) and a.dtype == b.dtype == F32
    assert (a != 0).all() and (b != 0).all() and np.isfinite(a).all() and np.isfinite(b).all()
    assert max(np.abs(a).max(), np.abs(b).max()) < 65504                       # inside the fp16 range: the status word must stay 0
    if c['N'] > 1:                                                             # another distribution per image: most of in1 positive in image 0, negative in image 1
        assert (a[0] > 0).mean() > 0.5 > (a[1] > 0).mean() and (b[0] > 0).mean() < 0.5 < (b[1] > 0).mean()
    assert ref['r64'].shape == ref['outside'].shape == (c['N'], c['H'], c['W'], L['ND'])
    assert (ref['r64'][~ref['outside']] != 0).all() and not ref['r64'][ref['outside']].any()
    bnd, dist, floor, cap = K.bound(c, ref)
    print('%s: float32 vs float64 %.3g, floor %.3g, bound %.3g, cap %.3g' % (c['id'], dist, floor, bnd, cap))
    assert 0 < bnd <= cap, 'bound %.3g (float32 vs float64 %.3g, floor %.3g) above the cap %.3g' % (bnd, dist, floor, cap)
    # tests/tolerances.py CORR_MEASURED is a record of these figures: it follows the inputs (numpy's summation order may move the distance a little)
    from tolerances import CORR_MEASURED
    rec = CORR_MEASURED[c['route']][c['id']]
    assert abs(rec[0] - dist) <= 0.25 * dist and abs(rec[1] - bnd) <= 0.25 * bnd and rec[2] <= rec[1]
    if K.expected_route(c) != K.MFMA:
        assert bnd == max(floor, 4 * dist) and floor == float(np.spacing(F32(np.abs(ref['r64']).max())))
    # windows: multiples of 4 as the entry points demand, the shared layout's two windows apart
    assert not any(L[k] & 3 for k in ('ld1', 'ld2', 'coff1', 'coff2'))
    assert L['coff1'] + c['C'] <= L['ld1'] and L['coff2'] + c['C'] <= L['ld2'] and L['out_coff'] + L['ND'] <= L['out_ld']
    if L['shared']:
        assert L['ld1'] == L['ld2'] and L['coff1'] + c['C'] < L['coff2']
        m1, m2 = K.wide_inputs(c, ref['inp'])
        assert m2 is None and int((m1 == K.JUNK).sum()) == m1.size - 2 * a.size


@pytest.mark.parametrize('c', K.CASES, ids=K.case_id)
def test_every_case_tells_a_wrong_kernel_from_a_right_one(c):
    """on the very inputs the GPU test uses, more than ten times the bound it applies: in2 taken from the other image (N = 2) or one
    column further on (N = 1), and the displacement index transposed ((ti, tj) for (tj, ti))"""
    ref = K.reference(c)
    bnd = K.bound(c, ref)[0]
    a, b, r64 = ref['inp']['in1'], ref['inp']['in2'], ref['r64']
    wrong = b[::-1] if c['N'] == 2 else np.roll(b, 1, axis=2)
    bad, _ = R.correlation(a, wrong, c['md'], c['s2'], F64, c['act'], K.SLOPE)
    assert np.abs(bad - r64).max() > 10 * bnd
    D = 2 * (c['md'] // c['s2']) + 1
    if D > 1:
        t = r64.reshape(r64.shape[:3] + (D, D)).swapaxes(-1, -2).reshape(r64.shape)
        assert np.abs(t - r64).max() > 10 * bnd
    # a leak into an out-of-image displacement is no matter of bounds: whatever is read there is not zero
    assert ref['outside'].any() == (c['md'] >= c['s2']) and (np.abs(a).min() > 0 and np.abs(b).min() > 0)


# ------------------------------------------------------------------------------------------------ 3. routes
# (N, H, W, C, max_disp, stride2) that each default-reachable route must at least hold
LISTED = {
    K.GENERIC: [(2, 5, 7, 4, 0, 1), (2, 5, 7, 12, 3, 1), (1, 9, 11, 64, 4, 1), (2, 12, 20, 256, 20, 2), (2, 7, 9, 8, 6, 3), (1, 512, 516, 4, 1, 1)],
    K.GENERIC2: [(2, 4, 6, 260, 4, 1), (1, 4, 6, 512, 2, 1)],
    K.GENERIC4: [(2, 3, 5, 516, 2, 1), (1, 3, 5, 1024, 4, 1), (1, 3, 5, 772, 1, 1)],
    K.CORR4: [(2, 5, 8, 4, 20, 2), (2, 7, 24, 128, 20, 2), (1, 3, 40, 256, 20, 2), (1, 4, 16, 36, 20, 2), (1, 2, 256, 36, 20, 2)],
    K.HALF1: [(2, 5, 4, 4, 4, 1), (2, 9, 12, 128, 4, 1), (1, 6, 8, 100, 4, 1), (2, 96, 172, 8, 4, 1)],
    K.HALF2: [(2, 6, 8, 132, 4, 1), (1, 10, 16, 200, 4, 1), (2, 4, 12, 256, 4, 1)],
    K.LDS: [(2, 3, 256, 32, 20, 2), (2, 3, 256, 96, 20, 2), (1, 2, 512, 64, 20, 2), (2, 23, 256, 32, 20, 2), (1, 1, 256, 32, 20, 2)],
    K.MFMA: [(2, 3, 128, 256, 20, 2), (2, 2, 256, 256, 20, 2), (1, 1, 128, 256, 20, 2)],
}


def _shape(c):
    return (c['N'], c['H'], c['W'], c['C'], c['md'], c['s2'])


def test_expected_route_gives_every_case_the_kernel_its_row_claims():
    ids = [c['id'] for c in K.CASES]
    assert len(set(ids)) == len(ids)
    for c in K.CASES:
        assert K.expected_route(c) == c['route'], (c['id'], K.expected_route(c))
        assert c['route'] not in K.ENV_ONLY
        assert (c['route'] == K.MFMA) == (c['entry'] == 'f16' and not c['fallback'])


def test_every_default_reachable_route_has_its_listed_cases():
    assert {c['route'] for c in K.CASES} == set(LISTED)
    for route, shapes in LISTED.items():
        have = [_shape(c) for c in K.CASES if c['route'] == route and (c['entry'] == 'f16') == (route == K.MFMA)]
        assert set(have) >= set(shapes), (route, set(shapes) - set(have))
    by = lambda **kw: [c for c in K.CASES if all(c[k] == v for k, v in kw.items())]
    # the matrix-core route: both activations at N = 2, input windows (ld 264, coff 4) with an output window
    assert {c['act'] for c in by(route=K.MFMA, N=2, H=3, W=128)} == {None, 'leaky'}
    assert any(K.layout(c)['ld1'] == 264 and K.layout(c)['coff1'] == 4 and c['lay'][2] == 'w' for c in by(route=K.MFMA, W=256))
    # the two fallbacks of vps_correlation_f16
    assert {_shape(c) for c in K.CASES if c['fallback']} == {(1, 4, 128, 128, 20, 2), (1, 4, 64, 256, 4, 1)}
    # windows where the table names them, the shared buffer on the three-stage LDS case
    for route, shape in ((K.CORR4, (2, 7, 24, 128, 20, 2)), (K.HALF1, (2, 9, 12, 128, 4, 1)), (K.HALF2, (1, 10, 16, 200, 4, 1))):
        assert any(_shape(c) == shape and c['lay'] == 'www' for c in by(route=route))
    assert any(_shape(c) == (2, 3, 256, 96, 20, 2) and c['lay'][:2] == 'ss' for c in by(route=K.LDS))
    # every route sees N = 2, a non-tight input and a non-tight output somewhere; the three input layouts and both activations exist
    for route in LISTED:
        cs = by(route=route)
        assert any(c['N'] == 2 for c in cs) and any(c['lay'][:2] != 'tt' for c in cs) and any(c['lay'][2] == 'w' for c in cs), route
    assert {c['lay'][0] for c in K.CASES} == set('tws') and {c['act'] for c in K.CASES} == {None, 'leaky'}
    # the grid-stride rounds: more pixels than 65536 blocks x 4 waves (generic), more 4-pixel groups than 2048 x 4 (half-wavefront)
    assert any(c['N'] * c['H'] * c['W'] > 4 * 65536 for c in by(route=K.GENERIC))
    assert any(c['N'] * c['H'] * c['W'] // 4 > 4 * 2048 for c in by(route=K.HALF1))
    # small: the two grid-stride cases apart, under 20k pixels
    assert sorted(c['N'] * c['H'] * c['W'] for c in K.CASES)[-3] < 20000


# ------------------------------------------------------------------------------------------------ 4. argument refusals
def _refusals():
    """(id, expected VPS_EARG index, overrides of a valid argument list)"""
    out = [('null_%s' % k, 1, {k: None}) for k in ('in1', 'in2', 'out')]
    out += [('%s_%d' % (k, v), 1, {k: v}) for k in 'NHW' for v in (0, -1)]
    out += [('C_%d' % v, 2, dict(C=v)) for v in (0, 6, 1028)]
    out += [('%s_%d' % (k, v), 2, {k: v}) for k, v in (('ld1', 10), ('ld2', 14), ('coff1', 2), ('coff2', 1))]
    out += [('stride2_0', 3, dict(s2=0)), ('stride2_-1', 3, dict(s2=-1)), ('max_disp_-1', 3, dict(md=-1))]
    return out


@pytest.mark.parametrize('entry', ['vps_correlation', 'vps_correlation_f16'])
def test_argument_refusals(entry):
    """VPS_EARG(x) = -1000 - x, returned before anything is launched (no stream is even looked at)"""
    lib = hip.load()
    dev = 'cuda:0' if torch.cuda.is_available() else 'cpu'              # no launch happens; device memory where there is a device
    keep = [torch.zeros(4096, dtype=torch.float32, device=dev) for _ in range(3)] + [torch.zeros(4, dtype=torch.int32, device=dev)]
    base = dict(in1=keep[0].data_ptr(), ld1=8, coff1=0, in2=keep[1].data_ptr(), ld2=8, coff2=0, out=keep[2].data_ptr(), out_ld=12, out_coff=0,
                N=1, H=4, W=4, C=8, md=1, s2=1, act=0, slope=0.1, status=keep[3].data_ptr())
    order = ['in1', 'ld1', 'coff1', 'in2', 'ld2', 'coff2', 'out', 'out_ld', 'out_coff', 'N', 'H', 'W', 'C', 'md', 's2', 'act', 'slope']
    cases = _refusals() + ([('null_status', 1, dict(status=None))] if entry.endswith('f16') else [])
    for name, code, over in cases:
        a = dict(base, **over)
        args = [a[k] for k in order] + ([a['status']] if entry.endswith('f16') else []) + [None]
        rc = getattr(lib, entry)(*args)                                         # (the binding declares the argument types)
        assert rc == -1000 - code, '%s(%s) returned %d' % (entry, name, rc)
    if dev != 'cpu':
        torch.cuda.synchronize()
        assert all(not t.any() for t in keep)
