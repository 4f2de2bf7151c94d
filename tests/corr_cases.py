"""The case table of tests/test_corr_gpu.py (vps_correlation / vps_correlation_f16 on the GPU against tests/corr_restate.py) and of
tests/test_corr_restate.py (the same inputs on the CPU: the restatement is the oracle's operator, every derived bound stays under the
cap, expected_route gives every case the kernel its row claims).

A case is a dict: route (the kernel instance its row is there for), entry ('f32' = vps_correlation, 'f16' = vps_correlation_f16), N, H,
W, C, md (max_disp), s2 (stride2), act (None / 'leaky', slope 0.1) and lay, three letters for in1, in2 and out:
    t  tight: ld == C (out: ld == D D), coff == 0
    w  a window: ld = C + 8, coff = 4 (out: ld = D D rounded up to 4, + 8; coff = 4)
    s  in1 and in2 are the windows [4, 4 + C) and [C + 8, 2 C + 8) of ONE buffer with ld = 2 C + 12 - how the path uses the kernels
Inputs are seeded per case, hold no exact zero, follow another distribution in every image and operand, and a quarter of the channels
is scaled by exp(1.5 randn) (as in test_correlation_split_fp16_on_mfma_equals_the_exact_kernels): a read from the wrong image, row,
column or channel cannot cancel. Outside their window the input buffers hold 1e30.

NOT covered, deliberately:
  * the routes that exist only behind a process-wide environment switch read once into a `static` (A/B code): VPS_CORR_LDS=2
    (correlation_lds_kernel<1,4>), VPS_CORR_LDS=0, VPS_CORR_HALF=0 (correlation4_kernel<1,4,1>: by default the half-wavefront kernel
    takes every call that would reach it) and VPS_CORR_MFMA bit 1 (corr_mfma_kernel<1,4,8>);
  * the 65536-block caps of correlation_lds_kernel<2,10> and correlation4_kernel<2,10,1> and the >= 4 GB refusals of the buffer-load
    kernels: not reachable at a test-sized shape (441 outputs for more than a million pixels)."""
import zlib

import numpy as np

import corr_restate as R
from nn_cases import JUNK, wide
from nn_restate import derive_bound

F32, F64 = np.float32, np.float64
SLOPE = 0.1
CAP = (1e-5, 1e-5)             # (atol, rtol) of test_correlation_matches_oracle in tests/test_hip_ops.py: the exact kernels
MFMA_REL = 2e-6                # of max|reference|: tests/test_hip_ops.py and tests/test_ref_native_gpu.py for the split-fp16 route

GENERIC, GENERIC2, GENERIC4 = 'correlation_kernel<1>', 'correlation_kernel<2>', 'correlation_kernel<4>'
CORR4, HALF1, HALF2 = 'correlation4_kernel<2,10,1>', 'correlation4h_kernel<4,1>', 'correlation4h_kernel<4,2>'
LDS, MFMA = 'correlation_lds_kernel<2,10>', 'corr_mfma_kernel<2,10,8>'
ENV_ONLY = ('correlation4_kernel<1,4,1>',)         # returned by expected_route only for a call of 4 GB or more


def _case(route, N, H, W, C, md, s2, lay='ttt', act=None, entry='f32', fallback=False):
    cid = '%s_N%d_%dx%d_C%d_md%d_s%d_%s%s' % (entry, N, H, W, C, md, s2, lay, '_leaky' if act else '')
    return dict(route=route, id=cid, entry=entry, N=N, H=H, W=W, C=C, md=md, s2=s2, lay=lay, act=act, fallback=fallback)


CASES = [
    # the generic kernel: r = 0 (one output), ND = 49 < 64, W % 4 != 0 at the half kernel's radius, W % 8 != 0 at the FlowNetC radius
    # (ND = 441 = 6 full passes of 64 + 57), stride2 = 3, and more than 65536 blocks x 4 pixels: a second grid-stride round
    _case(GENERIC, 2, 5, 7, 4, 0, 1, 'ttt'),
    _case(GENERIC, 2, 5, 7, 12, 3, 1, 'www', 'leaky'),
    _case(GENERIC, 1, 9, 11, 64, 4, 1, 'sst'),
    _case(GENERIC, 2, 12, 20, 256, 20, 2, 'twt', 'leaky'),
    _case(GENERIC, 2, 7, 9, 8, 6, 3, 'wtw'),
    _case(GENERIC, 1, 512, 516, 4, 1, 1, 'ttt'),
    # two float4 chunks per lane: only lane 0 holds a second chunk; all of them
    _case(GENERIC2, 2, 4, 6, 260, 4, 1, 'wwt'),
    _case(GENERIC2, 1, 4, 6, 512, 2, 1, 'ttw', 'leaky'),
    # four chunks: the first lane of the third; all four full; the third partly filled and the fourth empty
    _case(GENERIC4, 2, 3, 5, 516, 2, 1, 'ssw'),
    _case(GENERIC4, 1, 3, 5, 1024, 4, 1, 'ttt'),
    _case(GENERIC4, 1, 3, 5, 772, 1, 1, 'wtt', 'leaky'),
    # four pixels per wavefront at the FlowNetC radius where the lane-per-pixel kernel does not apply: one group pair per row; C % 32 != 0
    # with W % 256 == 0 must stay off the LDS route
    _case(CORR4, 2, 5, 8, 4, 20, 2, 'ttt'),
    _case(CORR4, 2, 7, 24, 128, 20, 2, 'www'),
    _case(CORR4, 1, 3, 40, 256, 20, 2, 'sst', 'leaky'),
    _case(CORR4, 1, 4, 16, 36, 20, 2, 'ttw'),
    _case(CORR4, 1, 2, 256, 36, 20, 2, 'wtt'),
    # half a wavefront per dot product, one float4 per lane: one group per row (every displacement row partly outside), a window, idle
    # lanes, and more than 2048 blocks x 4 groups: a second grid-stride round
    _case(HALF1, 2, 5, 4, 4, 4, 1, 'ttt'),
    _case(HALF1, 2, 9, 12, 128, 4, 1, 'www'),
    _case(HALF1, 1, 6, 8, 100, 4, 1, 'sst', 'leaky'),
    _case(HALF1, 2, 96, 172, 8, 4, 1, 'ttt'),
    # two float4 per lane
    _case(HALF2, 2, 6, 8, 132, 4, 1, 'ttw'),
    _case(HALF2, 1, 10, 16, 200, 4, 1, 'www', 'leaky'),
    _case(HALF2, 2, 4, 12, 256, 4, 1, 'sst'),
    # one lane per pixel, 32-channel stages two deep: one stage, three, two segments per row; a map taller than the 21 displacement rows
    # reach (interior rows see no out-of-image row); a single row
    _case(LDS, 2, 3, 256, 32, 20, 2, 'ttt'),
    _case(LDS, 2, 3, 256, 96, 20, 2, 'ssw'),
    _case(LDS, 1, 2, 512, 64, 20, 2, 'wwt', 'leaky'),
    _case(LDS, 2, 23, 256, 32, 20, 2, 'ttw'),
    _case(LDS, 1, 1, 256, 32, 20, 2, 'twt'),
    # split fp16 on the matrix cores
    _case(MFMA, 2, 3, 128, 256, 20, 2, 'ttt', entry='f16'),
    _case(MFMA, 2, 2, 256, 256, 20, 2, 'www', entry='f16'),
    _case(MFMA, 1, 1, 128, 256, 20, 2, 'sst', entry='f16'),
    _case(MFMA, 2, 3, 128, 256, 20, 2, 'ttw', 'leaky', entry='f16'),
    # vps_correlation_f16 where no matrix-core instance exists by default: the exact kernels, bitwise
    _case(CORR4, 1, 4, 128, 128, 20, 2, 'ttt', entry='f16', fallback=True),
    _case(HALF2, 1, 4, 64, 256, 4, 1, 'ttw', entry='f16', fallback=True),
]


def case_id(c):
    return c['id']


def layout(c):
    """-> dict(ld1, coff1, ld2, coff2, shared, ND, out_ld, out_coff)"""
    C, r = c['C'], c['md'] // c['s2']
    ND = (2 * r + 1) ** 2
    l1, l2, lo = c['lay']
    assert (l1 == 's') == (l2 == 's') and l1 in 'tws' and l2 in 'tws' and lo in 'tw'
    if l1 == 's':
        d = dict(ld1=2 * C + 12, coff1=4, ld2=2 * C + 12, coff2=C + 8, shared=True)
    else:
        d = dict(ld1=C + 8 * (l1 == 'w'), coff1=4 * (l1 == 'w'), ld2=C + 8 * (l2 == 'w'), coff2=4 * (l2 == 'w'), shared=False)
    d.update(ND=ND, out_ld=ND if lo == 't' else (ND + 3) // 4 * 4 + 8, out_coff=0 if lo == 't' else 4)
    return d


def expected_route(c):
    """The kernel instance a case's call launches at the DEFAULT switch values (no VPS_CORR_* set) - a pure-Python restatement of the
    dispatch, to be kept in step with, in this order:
      vps_correlation_f16 (vps_amd/csrc/flow_ops.hip) -> vpsi_launch_corr_mfma (corr_mfma.hip), else vps_correlation;
      vps_correlation (flow_ops.hip): the LDS kernel, correlation4_kernel<2,10,1>, vpsi_launch_corr4h (corr_half.hip),
      correlation4_kernel<1,4,1>, correlation_kernel<1|2|4>."""
    L = layout(c)
    N, H, W, C, s2 = c['N'], c['H'], c['W'], c['C'], c['s2']
    r = c['md'] // s2
    below4g = N * H * W * L['ld1'] * 4 < 0xFFFFFFF0 and N * H * W * L['ld2'] * 4 < 0xFFFFFFF0
    if c['entry'] == 'f16':
        # vpsi_launch_corr_mfma: VPS_CORR_MFMA defaults to 1 = the stride-2 instance alone
        if s2 == 2 and C == 256 and below4g and r == 10 and W % 128 == 0:
            return MFMA
    # vps_correlation
    if below4g and C % 32 == 0 and s2 == 2 and r == 10 and W % 256 == 0:
        return LDS
    if s2 == 2 and r == 10 and W % 8 == 0 and C <= 256:
        return CORR4
    # vpsi_launch_corr4h
    if s2 == 1 and r == 4 and W % 4 == 0 and C <= 256 and below4g and N * H * (W // 4) < 0x7fffffff:
        return HALF1 if C <= 128 else HALF2
    if s2 == 1 and r == 4 and W % 4 == 0 and C <= 256:
        return ENV_ONLY[0]
    return GENERIC if C <= 256 else GENERIC2 if C <= 512 else GENERIC4


# ------------------------------------------------------------------------------------------------ inputs and the shared reference
def inputs(c):
    """{in1, in2}: [N, H, W, C] float32, no exact zero"""
    g = np.random.default_rng(zlib.crc32(('correlation/' + c['id']).encode()))
    N, H, W, C = c['N'], c['H'], c['W'], c['C']
    scale = np.where(g.random(C) < 0.25, np.exp(1.5 * g.standard_normal(C)), 1.0)
    out = {}
    for name, sig, mu in (('in1', (1.0, 1.6), (0.6, -0.9)), ('in2', (0.8, 1.3), (-0.5, 0.8))):
        a = np.stack([(g.standard_normal((H, W, C)) * sig[n] + mu[n]) * scale for n in range(N)]).astype(F32)
        a[a == 0] = F32(0.5)
        out[name] = a
    return out


def wide_inputs(c, inp):
    """the host maps of the input buffers, [N, H, W, ld] with 1e30 outside the windows -> (map of in1, map of in2 or None = the same)"""
    L = layout(c)
    if L['shared']:
        m = wide(inp['in1'], L['ld1'], L['coff1'])
        m[..., L['coff2']:L['coff2'] + c['C']] = inp['in2']
        return m, None
    return wide(inp['in1'], L['ld1'], L['coff1']), wide(inp['in2'], L['ld2'], L['coff2'])


_REFERENCE = {}


def reference(c):
    """-> dict(inp, r32, r64, outside): computed ONCE per case and shared by every test that needs it (read-only arrays)"""
    if c['id'] not in _REFERENCE:
        inp = inputs(c)
        r32, o32 = R.correlation(inp['in1'], inp['in2'], c['md'], c['s2'], F32, c['act'], SLOPE)
        r64, outside = R.correlation(inp['in1'], inp['in2'], c['md'], c['s2'], F64, c['act'], SLOPE)
        assert np.array_equal(o32, outside)
        d = dict(inp=inp, r32=r32, r64=r64, outside=outside)
        for a in (inp['in1'], inp['in2'], r32, r64, outside):
            a.setflags(write=False)
        _REFERENCE[c['id']] = d
    return _REFERENCE[c['id']]


def bound(c, ref):
    """-> (bound, float32-vs-float64 distance, floor, cap). The exact routes: the project's recipe, max(one float32 ulp of the largest
    |reference|, 4 x max|float32 restatement - float64 restatement|), cap = what tests/test_hip_ops.py allows them. The matrix-core
    route: the project's figure for it, 2e-6 of the largest |reference| (its own cap)."""
    b, dist, floor = derive_bound(ref['r32'], ref['r64'])
    top = float(np.abs(ref['r64']).max())
    if expected_route(c) == MFMA:
        return MFMA_REL * top, dist, floor, MFMA_REL * top
    return b, dist, floor, CAP[0] + CAP[1] * top


assert JUNK == F32(1e30)
