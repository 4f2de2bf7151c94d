"""BASELINE config 3 plumbing (VERDICT r4 missing #1, #3): `load_checkpoint` with mmcv's semantics and tools/run_config3.py on
synthetic artefacts in the reference's file layout (the tools/test_vpq.py loop over the vps_amd loader and wrapper: tests/test_dataloader.py)."""
import io
import json
import os
import subprocess
import sys
from collections import OrderedDict
from contextlib import redirect_stdout

import pytest
import torch

import vps_amd
from vps_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    cfg = vps_amd.Config.fromfile(os.path.join(ROOT, 'configs', 'cityscapes', 'fusetrack.py'))
    return vps_amd.build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)


def test_load_checkpoint_semantics(tmp_path):
    """mmcv.runner.load_checkpoint as tools/test_vpq.py:135-137 uses it: 'state_dict' entry or bare OrderedDict, 'module.' prefix,
    strict=False reports (not raises) missing / unexpected keys, a shape mismatch raises, the checkpoint object is returned, and the
    packed HIP weights are invalidated by the in-place copy"""
    m = _model()
    sd = synth.synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, 3)
    f1 = str(tmp_path / 'latest.pth')
    torch.save({'meta': {'CLASSES': ('a', 'b')}, 'state_dict': OrderedDict(('module.' + k, v) for k, v in sd.items()), 'optimizer': {}}, f1)
    m.backbone._packed_device = torch.device('cpu')                  # as if it had been packed before
    ck = vps_amd.load_checkpoint(m, f1, map_location='cpu')
    assert ck['meta']['CLASSES'] == ('a', 'b')
    assert ck['_vps_load_report'] == dict(unexpected=[], missing=[], loaded=len(sd))
    assert m.backbone._packed_device is None
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    # a bare OrderedDict without prefix; one key missing, one unexpected: reported, not fatal
    f2 = str(tmp_path / 'bare.pth')
    part = OrderedDict((k, v) for k, v in sd.items() if k != 'bbox_head.fc_cls.bias')
    part['not.in.the.model'] = torch.zeros(1)
    torch.save(part, f2)
    buf = io.StringIO()
    with redirect_stdout(buf):
        vps_amd.load_checkpoint(_model(), f2, map_location='cpu')
    assert 'unexpected key in source state_dict: not.in.the.model' in buf.getvalue()
    assert 'missing keys in source state_dict: bbox_head.fc_cls.bias' in buf.getvalue()
    with pytest.raises(RuntimeError, match='missing keys'):
        vps_amd.load_checkpoint(_model(), f2, map_location='cpu', strict=True)
    # no state_dict at all / a shape mismatch
    f3 = str(tmp_path / 'junk.pth')
    torch.save({'meta': {}}, f3)
    with pytest.raises(RuntimeError, match='No state_dict found'):
        vps_amd.load_checkpoint(_model(), f3)
    bad = OrderedDict(sd); bad['bbox_head.fc_cls.bias'] = torch.zeros(3)
    f4 = str(tmp_path / 'bad.pth')
    torch.save({'state_dict': bad}, f4)
    with pytest.raises(RuntimeError, match='While copying the parameter named bbox_head.fc_cls.bias'):
        vps_amd.load_checkpoint(_model(), f4)


def test_run_config3_check_only_on_synthetic_artefacts():
    """tools/run_config3.py --dry-run --check-only: a synthetic latest.pth ('module.' prefix + meta) and FlowNet2_checkpoint.pth.tar in
    the reference's layout load with no missing / unexpected key, the dataset json is listed; a missing artefact is ONE JSON error"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_config3.py'), '--dry-run', '--check-only'], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert j['checkpoint']['missing'] == [] and j['checkpoint']['unexpected'] == [] and j['checkpoint']['loaded'] == 629
    assert j['dataset'] == dict(frames=16, videos=1, labelled_frames=4, img_prefix=j['dataset']['img_prefix'])
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_config3.py'), '--check-only', '--checkpoint', '/nonexistent/latest.pth'],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and 'missing artefact' in json.loads(p.stdout.strip().splitlines()[-1])['error']


@pytest.mark.gpu
def test_run_config3_dry_run_end_to_end(dev):
    """the whole chain of BASELINE config 3 on the synthetic stand-ins (files -> ClipFeeder -> detector with the loaded checkpoint ->
    unifier -> PNGs + pred.json -> eval_vpq): the prediction scored against itself is 100 in the reference's metric"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_config3.py'), '--dry-run'], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert j['run']['frames'] == 16 and j['run']['decodes'] == 16 and j['run']['png_files'] == 4
    assert j['vpq_final'][0] == 'vpq_all:100.0000', j['vpq_final']
