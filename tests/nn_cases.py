"""The case table of tests/test_nn_ops_gpu.py (the kernels on the GPU) and tests/test_nn_restate.py (the same inputs on the CPU: the
derived bound of every case stays under its cap, and a deliberately wrong restatement is told apart on exactly these inputs).

A case is a dict: op, id, the shapes / windows (leading dimensions `*_ld`, channel offsets `*_coff`), `exact` (compared bitwise with the
float64 restatement cast to float32) and `wrong` (the wrong variants that must be noticed). inputs(case) builds the numpy inputs from the
case's seed - input maps WIDE, i.e. with their leading dimension, JUNK outside the channel window - and reference(case, inp, dtype,
wrong) evaluates tests/nn_restate.py on the windows -> {output name: array}."""
import zlib

import numpy as np

import nn_restate as R

F32 = np.float32
JUNK = F32(1e30)            # what input buffers hold outside their channel window: finite (a max would not hide it), and ruinous when read

# what tests/test_hip_ops.py allows the same kernel today, as (atol, rtol); flow_prep: its isolation test, 1e-5 absolute (mean: 1e-4)
CAPS = dict(resize=(1e-6, 1e-6), pool=(1e-6, 1e-6), gather=(1e-6, 1e-6), scatter=(1e-6, 1e-6), scatter_all=(1e-6, 1e-6),
            resample2d=(1e-6, 1e-6), tcea_modulate=(1e-6, 1e-6), channelnorm=(1e-7, 1e-6), groupnorm=(1e-5, 1e-5),
            tcea_temporal=(1e-5, 1e-5), flow_stage=(1e-5, 1e-5), flow_stage_full=(1e-5, 1e-5), flow_warp=(1e-4, 1e-4),
            flow_prep=(1e-5, 0.0))


def _rng(case):
    return np.random.default_rng(zlib.crc32(('%s/%s' % (case['op'], case['id'])).encode()))


def _n(g, *shape, scale=1.0, shift=0.0):
    return (g.standard_normal(shape) * scale + shift).astype(F32)


def wide(a, ld, coff):
    """a [..., C] -> [..., ld] with a in channels [coff, coff + C) and JUNK elsewhere"""
    out = np.full(a.shape[:-1] + (ld,), JUNK, dtype=F32)
    out[..., coff:coff + a.shape[-1]] = a
    return out


def win(a, coff, C, shift=0):
    """the channel window [coff, coff + C) of a wide map; shift: the WRONG window, `shift` channels further on (cyclic)"""
    return np.roll(a, -shift, axis=-1)[..., coff:coff + C]


# ------------------------------------------------------------------------------------------------ the table
def _resize_cases():
    shapes = [(7, 5, 12, 9), (33, 17, 17, 9), (5, 9, 13, 4), (1, 6, 3, 11), (6, 1, 4, 1), (8, 12, 8, 12)]
    layouts = dict(c8w=dict(C=8, in_ld=16, in_coff=4, out_ld=24, out_coff=8),        # float4 path, windows on both sides
                   c8s=dict(C=8, in_ld=8, in_coff=0, out_ld=19, out_coff=4),         # C % 4 == 0 but a misaligned out_ld: scalar path
                   c3=dict(C=3, in_ld=5, in_coff=1, out_ld=7, out_coff=2))
    out, k = [], 0
    for mode in ('bilinear', 'nearest'):
        for s in shapes:
            for ln, lay in layouts.items():
                alpha = (1.0, 0.25, -20.0)[k % 3]; k += 1
                wrong = ['batch'] + (['shift4'] if ln == 'c8w' else [])
                if mode == 'bilinear' and s[:2] != s[2:]:
                    wrong.append('align_corners')
                out.append(dict(op='resize', id='%s_%dx%d_%dx%d_%s_a%g' % ((mode,) + s + (ln, alpha)), mode=mode, N=2, Hi=s[0], Wi=s[1], Ho=s[2],
                                Wo=s[3], alpha=alpha, exact=mode == 'nearest', wrong=wrong, **lay))
    return out


def _pool_cases():
    layouts = dict(c4w=dict(C=4, in_ld=8, in_coff=4, out_ld=12, out_coff=4), c3=dict(C=3, in_ld=5, in_coff=1, out_ld=4, out_coff=1))
    out = []
    for mode, datas in (('max', ('normal', 'negative', 'special')), ('avg', ('normal', 'negative'))):
        for Hi, Wi in ((1, 1), (1, 7), (2, 2), (2, 9), (9, 2), (17, 9)):
            for ln, lay in layouts.items():
                for data in datas:
                    wrong = ['batch'] + (['exclude_pad'] if mode == 'avg' else ['zero_pad'] if data != 'normal' else [])
                    out.append(dict(op='pool', id='%s_%dx%d_%s_%s' % (mode, Hi, Wi, ln, data), mode=mode, N=2, Hi=Hi, Wi=Wi, data=data,
                                    exact=mode == 'max', wrong=wrong, **lay))
    return out


def _gather_cases():
    out = [dict(op='gather', id='L%d' % L, ratios=tuple(1 << l for l in range(L)), H0=16, W0=48) for L in (1, 2, 3, 5)]
    out.append(dict(op='gather', id='r1_3', ratios=(1, 3), H0=12, W0=24))
    for c in out:
        c.update(N=2, C=8, lvl_ld=12, out_ld=16, out_coff=4, exact=False, wrong=['batch'] + (['div5'] if len(c['ratios']) != 5 else []))
    return out


def _scatter_cases():
    out = [dict(op='scatter', id='r%d' % r, r=r, N=2, C=8, H0=24, W0=48, ld=12, exact=True, wrong=['batch'] + (['window'] if r > 1 else []))
           for r in (1, 2, 3, 4, 8)]
    out += [dict(op='scatter_all', id='L%d' % L, L=L, N=2, C=32, H0=16, W0=32, ld=36, exact=True, wrong=['batch', 'window']) for L in (2, 3, 5)]
    return out


def _groupnorm_cases():
    out = []

    def add(C, G, npix, relu, wide_in, path, data='normal', entry='relu', nrep=1):
        lay = dict(out_ld=C + 8, out_coff=4) if path == 'v' else dict(out_ld=C + 3, out_coff=1)      # 'v': float4 path where 4 | C
        cnt, cpg = npix * C // G, C // G
        wrong = (['unbiased'] if cnt > 1 else []) + (['per_channel'] if cpg > 1 else [])
        if entry == 'apply':
            wrong = ['unbiased', 'relu_flip']
        if data == 'constant' or not wrong:
            wrong = ['relu_flip']                                             # the statistics cannot matter: the output is beta
        if data == 'far_mean':
            wrong = ['relu_flip', 'float32_stats']
        out.append(dict(op='groupnorm', id='%s_C%d_G%d_p%d_relu%d_%s%s_%s%s' % (entry, C, G, npix, relu, 'ld+4' if wide_in else 'ld', path, data,
                                                                             '_rep%d' % nrep if entry == 'apply' else ''),
                        C=C, G=G, npix=npix, relu=relu, in_ld=C + 4 * wide_in, data=data, entry=entry, nrep=nrep, exact=False,
                        ill=data == 'far_mean', wrong=wrong, **lay))
    for k, (C, G) in enumerate([(256, 32), (64, 32), (32, 32), (16, 4), (8, 8), (4, 1), (4, 4), (2, 1), (1, 1), (128, 1)]):
        add(C, G, 37, k & 1, (k >> 1) & 1, 'vs'[(k >> 2) & 1 if C > 2 else 1])
    for k, npix in enumerate((1, 3, 560)):
        add(64, 32, npix, (k + 1) & 1, k & 1, 'vs'[k == 1])
        add(2, 1, npix, k & 1, (k + 1) & 1, 's')
    add(64, 32, 37, 1, 1, 'v'); add(64, 32, 37, 0, 0, 's'); add(2, 1, 37, 0, 0, 's')
    add(64, 32, 37, 1, 0, 'v', 'constant'); add(16, 4, 3, 0, 1, 's', 'constant'); add(2, 1, 37, 0, 0, 's', 'constant')
    add(64, 32, 560, 1, 0, 'v', 'far_mean'); add(2, 1, 560, 0, 1, 's', 'far_mean')
    for nrep in (1, 3):
        for path in 'vs':
            for relu in (0, 1):
                add(16, 4, 37, relu, nrep == 3, path, entry='apply', nrep=nrep)
    return out


def _tcea_cases():
    out = [dict(op='tcea_temporal', id='C%d_p%d' % (C, npix), C=C, npix=npix, gain=1.0, ill=False) for C in (4, 64, 256, 512) for npix in (1, 5, 67)]
    out.append(dict(op='tcea_temporal', id='C64_p67_saturated', C=64, npix=67, gain=50.0, ill=True))
    for c in out:
        C = c['C']
        c.update(emb_ld=2 * C + 8, ref_ld=C, f0_ld=C + 8, f0_coff=4, f1_ld=C + 4, out_ld=2 * C + 4, exact=False, wrong=['swap_frames', 'shift4'])
    out += [dict(op='tcea_modulate', id='flat_n%d' % n, entry='flat', npix=n, C=1, lds=(1, 1, 1, 1), exact=False, wrong=['no_factor_2']) for n in (1, 1027)]
    out.append(dict(op='tcea_modulate', id='ld_C8_p37', entry='ld', npix=37, C=8, lds=(12, 16, 20, 24), exact=False, wrong=['no_factor_2']))
    return out


def _axpb_cases():
    return [dict(op='axpb', id='a%g_b%g' % (a, b), a=a, b=b, C=3, in_ld=8, in_coff=3, out_ld=12, out_coff=5, npix=77, exact=True, wrong=['shift1'])
            for a, b in ((1.0, 0.0), (20.0, 0.0), (-0.05, 3.0))]


def _transpose_cases():
    out = []
    for N, C, H, W in ((1, 1, 1, 1), (2, 3, 5, 7), (2, 33, 9, 11), (1, 64, 8, 8), (3, 40, 1, 67)):
        wrong = ['batch'] if N > 1 else ['hw_swap'] if H * W > 1 else ['negate']
        for Cpad in (C, C + 5):
            out.append(dict(op='nchw_to_nhwc', id='%dx%dx%dx%d_pad%d' % (N, C, H, W, Cpad), N=N, C=C, H=H, W=W, Cpad=Cpad, out_coff=3,
                            out_ld=Cpad + 7, exact=True, wrong=wrong))
        out.append(dict(op='nhwc_to_nchw', id='%dx%dx%dx%d' % (N, C, H, W), N=N, C=C, H=H, W=W, in_coff=3, in_ld=C + 7, exact=True, wrong=wrong))
    return out


def _resample_cases():
    out, k = [], 0
    for C in (1, 3, 5):
        for flows in ('normal', 'integer', 'edges'):
            for lay in ('ccc', 'hhh', ('hch', 'chc', 'cch')[k % 3]):               # c: NCHW strides, h: NHWC window; input, flow, output
                k += 1
                out.append(dict(op='resample2d', id='C%d_%s_%s' % (C, flows, lay), B=2, C=C, H=9, W=13, flows=flows, lay=lay, exact=False,
                                wrong=['zero_pad', 'swap_xy', 'batch']))
        for lay in ('cc', 'hh', 'hc', 'ch'):
            out.append(dict(op='channelnorm', id='C%d_%s' % (C, lay), B=2, C=C, H=9, W=13, lay=lay, exact=False, wrong=['batch'] + (['l1'] if C > 1 else [])))
    return out


def _flow_warp_cases():
    out = []
    for N, H, W, C in ((2, 9, 7, 8), (1, 24, 40, 64), (1, 2, 2, 4), (2, 5, 16, 12)):
        for flows in ('normal', 'zero', 'outside', 'edge'):
            wrong = ['border', 'align_corners'] + (['batch'] if N > 1 and flows in ('normal', 'edge') else []) + (['swap_xy'] if flows == 'normal' else [])
            if flows == 'outside':
                wrong = ['border']
            out.append(dict(op='flow_warp', id='%dx%dx%dx%d_%s' % (N, H, W, C, flows), N=N, H=H, W=W, C=C, flows=flows, flow_ld=8, flow_coff=4,
                            in_ld=C + 8, in_coff=4, out_ld=C + 12, out_coff=8, exact=flows == 'outside', wrong=wrong))
    return out


STAGE_OFFSETS = dict(img=0, flow=4, warp=7, diffnorm=11, flownorm=13)          # non-overlapping in out_ld = 16
STAGE_WIDTH = dict(img=3, flow=2, warp=3, diffnorm=1, flownorm=1)


def _flow_stage_cases():
    out, k = [], 0
    sets = [tuple(STAGE_OFFSETS), ('flow',), ('warp',), ('diffnorm',), ('flownorm',), ('img',)]
    for H, W in ((4, 4), (8, 12), (20, 36)):
        for up_mode in (0, 1):
            for div_mode in (0, 1):
                outs = sets[k % 6]
                wrong = ['img2'] if outs == ('img',) else ['mul_div'] + (['swap_xy'] if set(outs) & {'flow', 'warp', 'diffnorm'} else [])
                out.append(dict(op='flow_stage', id='%dx%d_up%d_div%d_%s_x%d_od%d' % (H, W, up_mode, div_mode, '+'.join(outs) if len(outs) < 5 else 'all',
                                                                                    (6, 8)[(k >> 1) & 1], (0, 20)[k & 1]),
                                H=H, W=W, up_mode=up_mode, div_mode=div_mode, flow_out_div=(0.0, 20.0)[k & 1], x_ld=(6, 8)[(k >> 1) & 1], outs=outs,
                                mul=20.0, flo_ld=4, flo_coff=2, out_ld=16, exact=False, wrong=wrong))
                k += 1
    for mode in (0, 1):
        for H, W in ((4, 4), (8, 12)):
            out.append(dict(op='flow_stage_full', id='mode%d_%dx%d' % (mode, H, W), H=H, W=W, mode=mode, mul=20.0, a_ld=4, a_coff=2, b_ld=2, b_coff=0,
                            exact=False, wrong=['mul_div', 'swap_xy']))
    return out


def _flow_prep_cases():
    out, k = [], 0
    for H, W, Hp, Wp in ((5, 7, 5, 7), (5, 7, 8, 16), (16, 16, 64, 64)):
        for nblk in (1, 4, 64):
            out.append(dict(op='flow_prep', id='%dx%d_%dx%d_nblk%d_ld%d' % (H, W, Hp, Wp, nblk, (8, 12)[k & 1]), H=H, W=W, Hp=Hp, Wp=Wp, nblk=nblk,
                            out_ld=(8, 12)[k & 1], exact=False, wrong=['mean_unpadded' if (Hp, Wp) != (H, W) else 'swap_frames']))
            k += 1
    return out


CASES = (_resize_cases() + _pool_cases() + _gather_cases() + _scatter_cases() + _groupnorm_cases() + _tcea_cases() + _axpb_cases() +
         _transpose_cases() + _resample_cases() + _flow_warp_cases() + _flow_stage_cases() + _flow_prep_cases())


def cases(*ops):
    return [c for c in CASES if c['op'] in ops]


def case_id(c):
    return c['id']


# ------------------------------------------------------------------------------------------------ inputs
def _quarter_steps(g, *shape):
    """quarter-step values (ties between window members), a +0.0 / -0.0 pair in one window, one -inf"""
    a = (np.round(g.standard_normal(shape) * 4) / 4).astype(F32)
    a[a == 0] = F32(0.25)
    a[0, 0, 0, :4] = F32(-0.0); a[0, 0, 1, :4] = F32(0.0); a[-1, 1, 1, 5] = F32(-np.inf)
    return a


def _weird_bits(g, *shape):
    """int32 bit patterns of float32 values with NaN payloads (quiet and signalling), -0.0, denormals, infinities"""
    a = g.standard_normal(shape).astype(F32).view(np.int32).reshape(-1).copy()
    special = np.array([0x7fc00001, 0x7fc12345, -0x00312345, 0x7f800001, -0x80000000, 0x00000001, 0x007fffff, -0x7ffffffe, 0x7f800000,
                        -0x00800000], dtype=np.int64).astype(np.int32)
    idx = g.permutation(a.size)[:min(a.size, 3 * len(special))]
    a[idx] = special[np.arange(len(idx)) % len(special)]
    return a.reshape(shape)


def _edge_targets(n, k):
    """sample positions exactly at n - 1, at n - 1 + 0.5, at -0.5, at -7 and at n + 7"""
    return np.array([n - 1, n - 1 + 0.5, -0.5, -7, n + 7], dtype=F32)[k % 5]


def inputs(c):
    g, op = _rng(c), c['op']
    if op == 'resize':
        return dict(x=wide(_n(g, c['N'], c['Hi'], c['Wi'], c['C']), c['in_ld'], c['in_coff']))
    if op == 'pool':
        x = _n(g, c['N'], c['Hi'], c['Wi'], c['C'])
        if c['data'] != 'normal':
            x = -np.abs(x) - 1
        if c['data'] == 'special':                                             # -0.0 is then the largest value of its windows
            f = x.reshape(-1)
            f[::5] = F32(-0.0); f[-1] = F32(-np.inf); f[f.size // 2] = F32(-np.inf)
        return dict(x=wide(x, c['in_ld'], c['in_coff']))
    if op == 'gather':
        return dict(levels=[wide(_n(g, c['N'], c['H0'] // r, c['W0'] // r, c['C']), c['lvl_ld'], 0) for r in c['ratios']])
    if op == 'scatter':
        return dict(bsf=wide(_quarter_steps(g, c['N'], c['H0'], c['W0'], c['C']), c['ld'], 0),
                    level=wide(_n(g, c['N'], c['H0'] // c['r'], c['W0'] // c['r'], c['C']), c['ld'], 0))
    if op == 'scatter_all':
        return dict(bsf=wide(_quarter_steps(g, c['N'], c['H0'], c['W0'], c['C']), c['ld'], 0),
                    levels=[wide(_n(g, c['N'], c['H0'] >> l, c['W0'] >> l, c['C']), c['ld'], 0) for l in range(c['L'])])
    if op == 'groupnorm':
        C, npix = c['C'], c['npix']
        x = dict(normal=lambda: _n(g, npix, C, scale=2.0, shift=0.5), constant=lambda: np.full((npix, C), 3.25, dtype=F32),
                 far_mean=lambda: _n(g, npix, C, scale=0.01, shift=1000.0))[c['data']]()
        d = dict(x=wide(x, c['in_ld'], 0), gamma=(g.random(C) + 0.5).astype(F32), beta=_n(g, C, scale=0.2))
        d['beta'][::2] = -np.abs(d['beta'][::2]); d['beta'][1::2] = np.abs(d['beta'][1::2])   # both signs, whatever C is
        if c['entry'] == 'apply':
            tot = R.group_sums(x, c['G'])
            # the float64 sums split unevenly over the copies: one is all zeros, one carries a negative part
            d['sums'] = tot[None] if c['nrep'] == 1 else np.stack([tot * 1.75, np.zeros_like(tot), tot - tot * 1.75])
        return d
    if op == 'tcea_temporal':
        C, npix = c['C'], c['npix']
        return dict(emb=wide(_n(g, npix, 2 * C, scale=0.2 * c['gain']), c['emb_ld'], 0), emb_ref=wide(_n(g, npix, C, scale=0.2 * c['gain']), c['ref_ld'], 0),
                    fea0=wide(_n(g, npix, C), c['f0_ld'], c['f0_coff']), fea1=wide(_n(g, npix, C), c['f1_ld'], 0))
    if op == 'tcea_modulate':
        fea, att, add = _n(g, c['npix'], c['C']), _n(g, c['npix'], c['C'], scale=3.0), _n(g, c['npix'], c['C'])
        att.reshape(-1)[::7] = F32(100.0); att.reshape(-1)[3::11] = F32(-100.0)
        return dict(fea=wide(fea, c['lds'][0], 0), att=wide(att, c['lds'][1], 0), add=wide(add, c['lds'][2], 0))
    if op == 'axpb':
        return dict(x=wide(_n(g, c['npix'], c['C']), c['in_ld'], c['in_coff']))
    if op == 'nchw_to_nhwc':
        return dict(x=_weird_bits(g, c['N'], c['C'], c['H'], c['W']))
    if op == 'nhwc_to_nchw':
        x = _weird_bits(g, c['N'], c['H'], c['W'], c['in_ld'])                 # the channels beside the window hold patterns of their own
        return dict(x=x)
    if op in ('resample2d', 'channelnorm'):
        B, C, H, W = c['B'], c['C'], c['H'], c['W']
        d = dict(img=_n(g, B, C, H, W))
        if op == 'resample2d':
            if c['flows'] == 'normal':
                d['flow'] = _n(g, B, 2, H, W, scale=3.0)
            elif c['flows'] == 'integer':                                      # alpha = beta = 0 everywhere; some leave the map
                d['flow'] = g.integers(-5, 6, size=(B, 2, H, W)).astype(F32)
            else:
                ys, xs = np.mgrid[0:H, 0:W]
                fx = _edge_targets(W, xs + ys) - xs.astype(F32)
                fy = _edge_targets(H, xs + 2 * ys + 1) - ys.astype(F32)
                d['flow'] = np.stack([np.stack([fx, fy]), np.stack([fx[::-1, ::-1], fy[::-1, ::-1]])]).astype(F32)
        return d
    if op == 'flow_warp':
        N, H, W, C = c['N'], c['H'], c['W'], c['C']
        ys, xs = np.mgrid[0:H, 0:W]
        if c['flows'] == 'normal':
            f = _n(g, N, H, W, 2, scale=2.0)
        elif c['flows'] == 'zero':
            f = np.zeros((N, H, W, 2), dtype=F32)
        elif c['flows'] == 'outside':                                          # every sample beyond the map by more than one pixel, on all four sides
            sx, sy = np.where((xs + ys) & 1, 1, -1), np.where(ys & 1, -1, 1)
            f = np.broadcast_to(np.stack([sx * 2.0 * W, sy * 2.0 * H], axis=-1).astype(F32), (N, H, W, 2)).copy()
        else:                                                                  # samples at ix in (-1, 0) and (W - 1, W), iy in (-1, 0) and (H - 1, H)
            bx = (R.linspace_m1_p1(W, np.float64)[None, :] + 1) * W / 2 - 0.5
            by = (R.linspace_m1_p1(H, np.float64)[:, None] + 1) * H / 2 - 0.5
            tx = np.where((xs + ys) & 1, -0.6, W - 0.4); ty = np.where(ys & 1, H - 0.7, -0.3)
            f = np.broadcast_to(np.stack([(tx - bx) * (W - 1) / W, (ty - by) * (H - 1) / H], axis=-1).astype(F32), (N, H, W, 2)).copy()
            f[..., 1] = np.where((xs % 3 == 0)[None], F32(0), f[..., 1])        # every third column: only x leaves (one COLUMN of corners outside)
        return dict(x=wide(_n(g, N, H, W, C), c['in_ld'], c['in_coff']), flow=wide(f, c['flow_ld'], c['flow_coff']))
    if op == 'flow_stage':
        H, W = c['H'], c['W']
        px = min(4.0, H / 3) / 4                                               # flows of +-4 pixels after mul (+-1.3 on the 4 x 4 map): some samples leave the map
        lo = _n(g, H // 4, W // 4, 2, scale=(80.0 if c['div_mode'] else 0.2) * px)
        return dict(x6=wide(_n(g, H, W, 6, scale=0.25), c['x_ld'], 0), flo=wide(lo, c['flo_ld'], c['flo_coff']))
    if op == 'flow_stage_full':
        H, W = c['H'], c['W']
        return dict(x6=wide(_n(g, H, W, 6, scale=0.25), 8, 0), fa=wide(_n(g, H // 4, W // 4, 2, scale=0.2 * min(4.0, H / 3) / 4), c['a_ld'], c['a_coff']),
                    fb=wide(_n(g, H // 4, W // 4, 2, scale=80.0 * min(4.0, H / 3) / 4), c['b_ld'], c['b_coff']))
    if op == 'flow_prep':
        return dict(img=_n(g, 3, c['H'], c['W']), ref=_n(g, 3, c['H'], c['W']), mean3=np.array([123.675, 116.28, 103.53], dtype=F32),
                    std3=np.array([58.395, 57.12, 57.375], dtype=F32))
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ the restatement on a case's inputs
def reference(c, inp, dtype, wrong=None):
    """{output name: array} - NHWC / pixel-major windows as the kernels write them. Exact cases: dtype float64 cast to float32 is the
    expected bit pattern (the transposes work on int32 patterns and ignore dtype)."""
    op = c['op']
    s4 = 4 if wrong == 'shift4' else 0
    w = None if wrong in ('shift4', 'shift1') else wrong
    if op == 'resize':
        return dict(out=R.resize(win(inp['x'], c['in_coff'], c['C'], s4), c['Ho'], c['Wo'], c['mode'], c['alpha'], dtype, w))
    if op == 'pool':
        return dict(out=R.pool3x3s2(win(inp['x'], c['in_coff'], c['C']), c['mode'], dtype, w))
    if op == 'gather':
        return dict(out=R.bfp_gather([win(l, 0, c['C']) for l in inp['levels']], c['ratios'], dtype, w))
    if op == 'scatter':
        return dict(out=R.bfp_scatter(win(inp['bsf'], 0, c['C']), win(inp['level'], 0, c['C']), c['r'], dtype, w))
    if op == 'scatter_all':
        return {'out%d' % l: R.bfp_scatter(win(inp['bsf'], 0, c['C']), win(inp['levels'][l], 0, c['C']), 1 << l, dtype, w if l or w == 'batch' else None)
                for l in range(c['L'])}
    if op == 'groupnorm':
        return dict(out=R.groupnorm(win(inp['x'], 0, c['C']), c['G'], inp['gamma'], inp['beta'], 1e-5, c['relu'], dtype, inp.get('sums'), w))
    if op == 'tcea_temporal':
        C = c['C']
        return dict(out=R.tcea_temporal(win(inp['emb'], 0, 2 * C), win(inp['emb_ref'], 0, C), win(inp['fea0'], c['f0_coff'], C, s4),
                                        win(inp['fea1'], 0, C), dtype, w))
    if op == 'tcea_modulate':
        C = c['C']
        return dict(out=R.tcea_modulate(win(inp['fea'], 0, C), win(inp['att'], 0, C), win(inp['add'], 0, C), dtype, w))
    if op == 'axpb':
        return dict(out=R.axpb(win(inp['x'], c['in_coff'], c['C'], 1 if wrong == 'shift1' else 0), c['a'], c['b'], dtype))
    if op in ('nchw_to_nhwc', 'nhwc_to_nchw'):
        x = inp['x'] if op == 'nchw_to_nhwc' else np.ascontiguousarray(win(inp['x'], c['in_coff'], c['C']))
        if wrong == 'batch':
            x = np.broadcast_to(x[:1], x.shape)
        if wrong == 'negate':
            x = x ^ np.int32(-0x80000000)
        if wrong == 'hw_swap':
            x = x.reshape(x.shape[0], x.shape[1], -1)[:, :, ::-1].reshape(x.shape) if op == 'nchw_to_nhwc' else x[:, ::-1, ::-1]
        return dict(out=R.nchw_to_nhwc(x, c['Cpad']) if op == 'nchw_to_nhwc' else R.nhwc_to_nchw(x))
    if op == 'resample2d':
        return dict(out=R.resample2d(inp['img'], inp['flow'], dtype, w))
    if op == 'channelnorm':
        return dict(out=R.channelnorm(inp['img'], dtype, w))
    if op == 'flow_warp':
        return dict(out=R.flow_warp(win(inp['x'], c['in_coff'], c['C']), win(inp['flow'], c['flow_coff'], 2), dtype, w))
    if op == 'flow_stage':
        x6 = win(inp['x6'], 0, 6)
        s = R.flow_stage(x6, win(inp['flo'], c['flo_coff'], 2), c['up_mode'], c['mul'], c['div_mode'], c['flow_out_div'], dtype, None if w == 'img2' else w)
        if w == 'img2':
            s['img'] = x6[..., 3:6].astype(dtype)
        return {k: (s[k] if s[k].ndim == 3 else s[k][..., None]) for k in c['outs']}
    if op == 'flow_stage_full':
        return dict(out=R.flow_stage_full(win(inp['x6'], 0, 6), win(inp['fa'], c['a_coff'], 2), win(inp['fb'], c['b_coff'], 2), c['mode'], c['mul'], dtype, w))
    if op == 'flow_prep':
        out, mean = R.flow_prep(inp['img'], inp['ref'], inp['mean3'], inp['std3'], c['Hp'], c['Wp'], dtype, w)
        # channels 6 .. out_ld of the output are zeroed: +0.0 exactly (bound 0: no float32-vs-float64 distance, and |reference| = 0)
        return dict(out=out, zeros=np.zeros(out.shape[:2] + (c['out_ld'] - 6,), dtype=dtype), rgb_mean=mean)
    raise KeyError(op)


def expected_bits(c, r64):
    """the float32 value an EXACT case must produce, from the float64 restatement; axpb follows the library's build: hipcc contracts
    x * a + b into one fma (no -ffp-contract flag in vps_amd/csrc/Makefile: the HIP default is fast), so one rounding - which is
    what float64 arithmetic cast to float32 gives (R.axpb(fma=True))"""
    return {k: (v if v.dtype == np.int32 else v.astype(F32)) for k, v in r64.items()}


def bounds(c, r32, r64):
    """{output name: (bound, distance, floor, cap)} of a bounded case; cap = atol + rtol max|reference| of what tests/test_hip_ops.py
    allows the kernel (rgb_mean of flow_prep: 1e-4 absolute)"""
    atol, rtol = CAPS[c['op']]
    out = {}
    for k in r64:
        b, dist, floor = R.derive_bound(r32[k], r64[k])
        cap = 1e-4 if k == 'rgb_mean' else atol + rtol * float(np.abs(r64[k][np.isfinite(r64[k])]).max())
        out[k] = (b, dist, floor, cap)
    return out


def groupnorm_affine_bound(c, inp):
    """The far-mean GroupNorm cases (mean 1000, std 0.01) are there to show that the STATISTICS are taken in float64: a float32 sum of
    squares loses the variance altogether (the float32 restatement is off by whole units, and so is the bound derived from it). What
    float64 statistics leave, from the number formats alone:
      * the float32 affine (x - mean) sc + beta: x - float(mean) is exact, sc, the shift and the result are each rounded once
        -> 4 float32 ulp of the largest |output|;
      * sum of squares / count - mean^2 cancels mean^2 against the variance. A float64 sum of n = npix cpg terms is off by at most
        (n - 1) 2^-53 of the sum of their magnitudes, whatever the order: (n - 1) 2^-53 mean^2 in the mean of squares and twice that in
        mean^2, so 3 (n - 1) 2^-53 mean^2 / (var + eps) relative in var + eps and half of it in 1 / sqrt(var + eps); the kernel and the
        yardstick each -> 3 (n - 1) 2^-53 x mean^2 / (var + eps) x the largest |output - beta|."""
    x = win(inp['x'], 0, c['C']).astype(np.float64)
    xg = x.reshape(c['npix'], c['G'], -1)
    mean, var = xg.mean(axis=(0, 2)), xg.var(axis=(0, 2))
    cpg = c['C'] // c['G']
    norm = np.abs((x - np.repeat(mean, cpg)) * np.repeat(1 / np.sqrt(var + 1e-5), cpg) * inp['gamma'])
    out = norm + np.abs(inp['beta'])
    n = c['npix'] * cpg
    return 4 * float(np.spacing(F32(out.max()))) + 3 * (n - 1) * 2.0 ** -53 * float((mean * mean / (var + 1e-5)).max()) * float(norm.max())
