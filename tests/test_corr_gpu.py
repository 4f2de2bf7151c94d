"""Kernel-level tests of the correlation kernels - the correlation half of vps_amd/csrc/flow_ops.hip (correlation_kernel<1|2|4>,
correlation4_kernel<2,10,1>, correlation_lds_kernel<2,10>), vps_amd/csrc/corr_half.hip (correlation4h_kernel<4,1|2>) and
vps_amd/csrc/corr_mfma.hip (corr_mfma_kernel<2,10,8>) - against tests/corr_restate.py (a plain numpy restatement, pinned to the oracle on
the CPU by tests/test_corr_restate.py) on the cases of tests/corr_cases.py: every kernel instance that vps_correlation and
vps_correlation_f16 launch at their default switch values, with N = 2, channel windows on the inputs (two windows of one buffer among
them) and on the output, C up to 1024, off-path radii and strides, and the grid-stride rounds of the two capped grids. What is
deliberately NOT covered (the routes behind environment switches, the 65536-block caps of the LDS and correlation4 kernels): the
docstring of tests/corr_cases.py. Which kernel ran is not observed here; tests/test_corr_restate.py checks the table's intent against a
restatement of the dispatch.

Both entry points are called through the C ABI (hip.load().vps_correlation, vps_correlation_f16), inputs and outputs move with torch and
numpy on the host. Per case:
  * guards: inputs sit in buffers of their own leading dimension with 1e30 beside their window and are unchanged, bit for bit, after the
    call; the output buffer, a guard row before and after included, is pre-filled with a quiet-NaN sentinel and everything outside
    [coff, coff + D D) still holds it; the return code (and the status word of vps_correlation_f16) is 0;
  * out-of-image displacements are +0.0 BITWISE, with and without the activation, on the matrix-core route too. The inputs hold no zero:
    a value leaking in from the neighbouring row (x wrapping round), the neighbouring image (N = 2) or the 1e30 beside the window shows
    here exactly, under no tolerance;
  * everything else against the float64 restatement - the exact routes under bound = max(one float32 ulp of the largest |reference|,
    4 x max|float32 restatement - float64 restatement|), derived from the case's own inputs and asserted on the CPU not to exceed what
    tests/test_hip_ops.py allows these kernels; the matrix-core route under the project's figure for it, 2e-6 of the largest |reference|;
  * every N = 2 case again on image 1 alone (N = 1, pointers advanced by one image): bitwise the second half of the N = 2 result.
Measured figures: tests/tolerances.py (CORR_MEASURED)."""
import ctypes

import numpy as np
import pytest
import torch

import corr_cases as K
from kernel_buf import SENT, Buf, written_outside
from vps_amd import hip

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _run(dev, c, image=None, entry=None):
    """one call on fresh buffers -> (return code, status word or None, output Buf, input Bufs). image = 1: N = 1 on image 1 alone,
    inside the buffers of the whole case; entry overrides the case's entry point"""
    L, inp = K.layout(c), K.reference(c)['inp']
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    m1, m2 = K.wide_inputs(c, inp)
    b1 = Buf(dev, m1, N * H * W, L['ld1'])
    b2 = b1 if m2 is None else Buf(dev, m2, N * H * W, L['ld2'])
    o = Buf(dev, None, N * H * W, L['out_ld'])
    skip = 0 if image is None else image * H * W
    args = [b1.p(skip * L['ld1']), L['ld1'], L['coff1'], b2.p(skip * L['ld2']), L['ld2'], L['coff2'], o.p(skip * L['out_ld']), L['out_ld'],
            L['out_coff'], N if image is None else 1, H, W, C, c['md'], c['s2'], hip.ACT_LEAKY if c['act'] else hip.ACT_NONE, K.SLOPE]
    if (entry or c['entry']) == 'f16':
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        rc = hip.load().vps_correlation_f16(*args, ctypes.c_void_p(st.data_ptr()), hip.stream_ptr())
    else:
        st = None
        rc = hip.load().vps_correlation(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, (None if st is None else st.cpu().numpy()), o, ([b1] if b2 is b1 else [b1, b2])


def _window(c, o):
    """the guards of the output buffer, then its window as int32 bit patterns [N, H, W, D D]"""
    L = K.layout(c)
    got = o.bits()
    nout = written_outside(got, [(L['out_coff'], L['ND'])])
    assert nout == 0, '%d elements outside the window written' % nout
    return got[1:-1, L['out_coff']:L['out_coff'] + L['ND']].reshape(c['N'], c['H'], c['W'], L['ND'])


@pytest.mark.parametrize('c', K.CASES, ids=K.case_id)
def test_correlation(dev, c):
    ref = K.reference(c)
    rc, st, o, ins = _run(dev, c)
    assert rc == 0, 'return code %d' % rc
    assert st is None or not st.any(), 'status word %s' % st
    for b in ins:
        assert b.unchanged(), 'an input buffer was written'
    w = _window(c, o)
    outside = ref['outside']
    bad = outside & (w != 0)
    assert not bad.any(), '%d of %d out-of-image displacements are not +0.0, first at (n, y, x, d) %s: %s' % (
        int(bad.sum()), int(outside.sum()), np.argwhere(bad)[:4].tolist(), w.view(F32)[bad][:4])
    err = np.abs(w.view(F32).astype(F64) - ref['r64'])
    assert not np.isnan(err).any(), '%d NaN (sentinel left or computed)' % int(np.isnan(err).sum())
    bnd, dist, floor, cap = K.bound(c, ref)
    print('correlation %s [%s]: max err %.3g, float32 vs float64 %.3g, floor %.3g, bound %.3g' % (c['id'], c['route'], float(err.max()), dist, floor, bnd))
    assert float(err.max()) <= bnd, 'max err %.3g > bound %.3g (float32 vs float64 restatement %.3g), at (n, y, x, d) %s' % (
        float(err.max()), bnd, dist, np.unravel_index(int(err.argmax()), err.shape))
    if c['fallback']:
        rc2, _, o2, _ = _run(dev, c, entry='f32')
        assert rc2 == 0 and np.array_equal(o2.bits(), o.bits()), 'vps_correlation_f16 without an instance is not vps_correlation'


@pytest.mark.parametrize('c', [c for c in K.CASES if c['N'] == 2], ids=K.case_id)
def test_image_1_alone_is_the_second_half_of_the_batch(dev, c):
    """N = 1 with every pointer advanced by one image: the kernels' decode of (n, y, x), and every bound that depends on N, against
    the same kernel at N = 2 - bitwise, under no tolerance"""
    rc, st, o, _ = _run(dev, c)
    rc1, st1, o1, ins1 = _run(dev, c, image=1)
    assert rc == 0 and rc1 == 0 and (st is None or not (st.any() or st1.any()))
    for b in ins1:
        assert b.unchanged()
    both, alone = _window(c, o), _window(c, o1)
    assert (alone[0] == SENT).all(), 'image 0 written by a call on image 1'
    diff = both[1] != alone[1]
    assert not diff.any(), '%d of %d elements of image 1 differ, first at (y, x, d) %s' % (int(diff.sum()), diff.size, np.argwhere(diff)[:4].tolist())
