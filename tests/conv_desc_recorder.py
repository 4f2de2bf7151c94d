"""Which vps_conv_desc the Python side hands to vps_conv2d, and what PackedConv packs: recorded on the CPU with every launch stubbed
(the stubs of tests/test_host_dryrun.py), compared by tests/test_conv_desc.py with tests/conv_desc_cases.json.

    python tests/conv_desc_recorder.py <commit the tree is at>      rewrites the fixture from the tree it runs in

tests/conv_plan_cases.json pins what the planner does WITH a descriptor; this pins which descriptors it gets: tile_n, ksplit, the
GroupNorm fields, the w_thin hand-off, the f16x3 status slot of every layer, in launch order."""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_desc_cases.json')

# (name, config, arithmetic, H, W), two frames each. The small clip reaches split counts 1..32 with uneven chunk splits, only the
# full-size ones the 256-column deformable tile and the GroupNorm sums in the epilogue.
CONFIGS = [
    ('fusetrack f16x3 128x256', 'cityscapes/fusetrack.py', 'f16x3', 128, 256),
    ('fusetrack f32 128x256', 'cityscapes/fusetrack.py', 'f32', 128, 256),
    ('fusetrack bf16x6 128x256', 'cityscapes/fusetrack.py', 'bf16x6', 128, 256),
    ('fuse f16x3 128x256', 'cityscapes/fuse.py', 'f16x3', 128, 256),
    ('track f16x3 128x256', 'cityscapes/track.py', 'f16x3', 128, 256),
    ('fusetrack f16x3 1024x2048', 'cityscapes/fusetrack.py', 'f16x3', 1024, 2048),
    ('fusetrack bf16x6 1024x2048', 'cityscapes/fusetrack.py', 'bf16x6', 1024, 2048),
    ('fusetrack_r101 f16x3 1088x1920', 'viper/fusetrack_r101.py', 'f16x3', 1088, 1920),
]
FRAMES = 2
# the module-level switches of vps_amd/nhwc.py that the packing and the geometry read, at their defaults: they are set from VPS_*
# environment variables at import, and the record must not depend on the environment it is replayed in
SWITCHES = dict(SPLITK_TARGET_BLOCKS=256, SPLITK_LAST_BLOCK=False, SMALL_ON_MFMA=False, THIN_KERNEL=True, DCN256=[True], DCN256_MIN_TILES=256)
MODES = ('f32', 'bf16', 'bf16x3', 'bf16x6', 'f16x3')


def _fields():
    from vps_amd import hip
    ints, ptrs = [], []
    for name, typ in hip.ConvDesc._fields_:
        if typ is ctypes.c_void_p:
            if name != 'status':
                ptrs.append(name)
        elif typ is ctypes.c_int32:
            ints.append(name)
        elif typ is not ctypes.c_float:
            ints += ['%s[%d]' % (name, i) for i in range(typ._length_)]
    return ints, ptrs


def _row(d, ints, ptrs, status_base):
    vals = []
    for f in ints:
        vals.append(getattr(d, f[:-3])[int(f[-2])] if f.endswith(']') else getattr(d, f))
    return dict(d=vals, slope=d.slope, p=[int(bool(getattr(d, f))) for f in ptrs]), -1 if not d.status else (d.status - status_base) // 4


@contextlib.contextmanager
def default_switches():
    from vps_amd import nhwc
    saved = {k: getattr(nhwc, k) for k in SWITCHES}
    for k, v in SWITCHES.items():
        setattr(nhwc, k, list(v) if isinstance(v, list) else v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(nhwc, k, v)


@contextlib.contextmanager
def _stubbed(prec, on_conv=None):
    """the launch stubs of tests/test_host_dryrun.py, `prec` as the default arithmetic, the switches at their defaults, and a slot
    numbering that starts afresh"""
    from test_host_dryrun import _RecordingLib
    from vps_amd import hip, nhwc
    lib = _RecordingLib()
    status = torch.zeros(nhwc.F16_SLOTS, dtype=torch.int32)
    saved_hip = {k: getattr(hip, k) for k in ('load', 'ptr', 'stream_ptr', 'conv2d')}
    saved = (nhwc.f16_status, nhwc.DEFAULT_PREC, nhwc._F16_NEXT[0], dict(nhwc._F16_LAYERS), nhwc.F16_FALLBACKS[0])
    hip.load = lambda: lib
    hip.ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    hip.stream_ptr = lambda: None
    hip.conv2d = (lambda d: None) if on_conv is None else (lambda d: on_conv(d, status.data_ptr()))
    nhwc.f16_status = lambda device: status
    nhwc.DEFAULT_PREC = nhwc.PREC_NAMES[prec]
    nhwc._F16_NEXT[0] = 1
    nhwc._F16_LAYERS.clear()
    try:
        with default_switches():
            yield
    finally:
        for k, v in saved_hip.items():
            setattr(hip, k, v)
        nhwc.f16_status, nhwc.DEFAULT_PREC, nhwc._F16_NEXT[0] = saved[:3]
        nhwc._F16_LAYERS.clear()
        nhwc._F16_LAYERS.update(saved[3])
        nhwc.F16_FALLBACKS[0] = saved[4]


def record_launches(config, prec, H, W, frames=FRAMES):
    """-> (row = dict d, slope, p; status slot or -1) per vps_conv2d launch of `frames` frames of the detector of configs/<config>"""
    import vps_amd
    from test_host_dryrun import _FakeCuda
    from vps_amd import synth
    ints, ptrs = _fields()
    rows = []
    with _stubbed(prec, lambda d, base: rows.append(_row(d, ints, ptrs, base))):
        cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', config))
        m = vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
        m.overlap_streams = False                      # torch.cuda streams need a device
        synth.load_synth(m, 0)
        fr = synth.synth_clip(H, W, frames, 0)
        for t in range(frames):
            m(return_loss=False, rescale=True, img=[fr[t].as_subclass(_FakeCuda)], img_meta=[[synth.img_meta(H, W, 10001 + t)]],
              ref_img=[fr[t - 1 if t else 0]])
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------------------
def _values(*shape, salt=0):
    """reproducible fp32 values in [-0.5, 0.5) from integer arithmetic alone (no random generator whose stream could change)"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64) + 7919 * salt + 1
    return ((i * 2654435761 % 4294967296).double() / 4294967296 - 0.5).float().view(*shape)


def _bn(c):
    return dict(weight=_values(c, salt=11) + 1.5, bias=_values(c, salt=12), running_mean=_values(c, salt=13),
                running_var=_values(c, salt=14) + 1.0, eps=1e-5)


def _layers(prec):
    """name -> PackedConv, built on the CPU in arithmetic `prec`; the order is part of the record (f16x3 layers take status slots in it)"""
    from vps_amd import hip, nhwc
    P = nhwc.PackedConv
    yield '3x3 tap-major 8->40', P(_values(40, 8, 3, 3), _values(40, salt=1), padding=1, act=hip.ACT_RELU, device='cpu', prec=prec)
    yield '3x3 chunk-major 64->72', P(_values(72, 64, 3, 3, salt=2), None, padding=1, device='cpu', prec=prec)
    yield '1x1 48->130', P(_values(130, 48, 1, 1, salt=3), _values(130, salt=4), device='cpu', prec=prec)
    yield '7x7 s2 thin 3->64', P(_values(64, 3, 7, 7, salt=5), None, stride=2, padding=3, device='cpu', prec=prec)
    yield '4x4 s2 transposed 36->20', P(_values(36, 20, 4, 4, salt=6), _values(20, salt=7), stride=2, padding=1, transposed=True, act=hip.ACT_LEAKY,
                                        device='cpu', prec=prec)
    yield 'deformable 3x3 chunk-major 64->64', P(_values(64, 64, 3, 3, salt=8), None, padding=1, deform=True, device='cpu', prec=prec)
    yield 'deformable 3x3 tap-major 16->32', P(_values(32, 16, 3, 3, salt=9), None, padding=1, deform=True, device='cpu', prec=prec)
    yield 'linear chw 6x4 -> 50', nhwc.pack_linear(_values(50, 24, salt=10), _values(50, salt=15), act=hip.ACT_RELU, device='cpu', chw=(6, 4), prec=prec)
    yield 'from_matrix 37x64', P.from_matrix(_values(37, 64, salt=16), prec=prec)
    yield 'small 3x3 64->2', P(_values(2, 64, 3, 3, salt=17), _values(2, salt=18), padding=1, device='cpu', prec=prec)
    yield '3x3 with BN 32->64', P(_values(64, 32, 3, 3, salt=19), None, bn=_bn(64), padding=1, act=hip.ACT_RELU, device='cpu', prec=prec)


def _tensor(t):
    if t is None:
        return None
    t = t.contiguous()
    return dict(shape=list(t.shape), dtype=str(t.dtype).replace('torch.', ''), sha256=hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


PACK_INTS = ('prec', 'korder', 'cin', 'cin_pad', 'cout', 'cout_pad', 'kpad', 'tile_n', 'KH', 'KW', 'stride', 'nclass', 'f16_slot')


def _packed(pc):
    rec = {k: int(getattr(pc, k)) for k in PACK_INTS}
    rec.update(pad_y=list(pc.pad_y), pad_x=list(pc.pad_x), has_scale=bool(pc.has_scale), can_fall_back=pc._fb is not None)
    for k in ('w', 'w_split', 'w_thin', 'scale', 'shift'):
        rec[k] = _tensor(getattr(pc, k, None))          # (getattr: at the commit of the fixture's `source` a layer without split weights has no w_thin)
    return rec


def record_packing():
    """-> {mode: {layer: record}}; 'f16x3' also holds the BN layer after `use_fallback`"""
    from vps_amd import nhwc
    out = {}
    for mode in MODES:
        with _stubbed(mode):
            layers = list(_layers(nhwc.PREC_NAMES[mode]))
            out[mode] = {name: _packed(pc) for name, pc in layers}
            if mode == 'f16x3':
                pc = dict(layers)['3x3 with BN 32->64']
                assert pc.use_fallback('cpu') == 1
                out[mode]['3x3 with BN 32->64, after use_fallback'] = _packed(pc)
    return out


def main(commit):
    ints, ptrs = _fields()
    rows, index, configs = [], {}, {}
    for name, config, prec, H, W in CONFIGS:
        seq, status = [], []
        for r, slot in record_launches(config, prec, H, W):
            key = json.dumps(r, sort_keys=True)
            if key not in index:
                index[key] = len(rows)
                rows.append(r)
            seq.append(index[key])
            status.append(slot)
        configs[name] = dict(rows=seq, status=status)
        print('%-34s %4d launches, %3d distinct rows so far' % (name, len(seq), len(rows)))
    table = dict(source='Recorded with tests/conv_desc_recorder.py on the CPU (every launch stubbed) from commit %s, the parent of the PackedConv '
                        'refactor: the vps_conv_desc of every vps_conv2d launch of two frames of each configuration (distinct `rows`, and per configuration the '
                        'sequence of row indices and of f16x3 status slots, -1 = none), and what PackedConv packs for '
                        'a list of small layers in every arithmetic.' % commit,
                 int_fields=ints, pointers=ptrs, frames=FRAMES, rows=rows, configs=configs, packing=record_packing())
    with open(FIXTURE, 'w') as f:
        f.write('{\n')
        for k, v in table.items():
            if k == 'rows':
                f.write('"rows": [\n%s\n],\n' % ',\n'.join(json.dumps(r, separators=(',', ':')) for r in v))
            elif k == 'packing':
                f.write('"packing": {\n%s\n}\n' % ',\n'.join('%s: {\n%s\n}' % (json.dumps(mode), ',\n'.join(
                    '%s: %s' % (json.dumps(name), json.dumps(r, separators=(',', ':'))) for name, r in layers.items())) for mode, layers in v.items()))
            else:
                f.write('%s: %s,\n' % (json.dumps(k), json.dumps(v, separators=(',', ':') if k == 'configs' else None)))
        f.write('}\n')
    json.load(open(FIXTURE))


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    main(sys.argv[1])
