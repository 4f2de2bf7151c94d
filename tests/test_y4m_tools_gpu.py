"""GPU: the Y4M options of the tools. `tools/run_config3.py --dry-run --video` runs one clip that it writes itself through `Y4mWriter`
and writes every frame's PNGs, pred.json and the overlay stream; `tools/run_vps_synthetic.py --overlay-video` adds one stream per video
and leaves every other output of the run byte for byte what it is without the option."""
import filecmp
import json
import os
import subprocess
import sys

import pytest

from vps_amd import y4m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(p):
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1])


def test_run_config3_dry_run_from_a_y4m_clip(dev, tmp_path):
    ov, jd = str(tmp_path / 'overlay.y4m'), str(tmp_path / 'jpg')
    env = dict(os.environ, VPS_KEEP_DRY_RUN='1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_config3.py'), '--dry-run', '--dry-frames', '6', '--video', 'clip.y4m',
                        '--overlay-video', ov, '--overlay-video-sampling', '420mpeg2', '--overlay', jd, '--tubes'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    rep = _report(p)
    try:
        v = rep['video']
        assert (v['frames'], v['size'], v['sampling'], v['native_y4m'], v['dropped_partial_frames']) == (6, [128, 256], '420jpeg', 6, 0)
        assert os.path.basename(v['file']) == 'clip.y4m' and rep['run']['frames'] == rep['run']['decodes'] == rep['run']['png_files'] == 6
        out = rep['run']['output_dir']
        names = ['clip_%06d.png' % f for f in range(6)]                              # every frame is a result frame
        assert sorted(os.listdir(os.path.join(out, 'pan_pred'))) == sorted(os.listdir(os.path.join(out, 'pan_2ch'))) == names
        assert len(json.load(open(os.path.join(out, 'pred.json')))['annotations']) == 6 and os.path.exists(os.path.join(out, 'tubes.json'))
        assert 'vpq_final' not in rep                                                # a clip from a file has no ground truth
        assert rep['overlay_video']['files'] == [ov] and rep['overlay']['files'] == 6 and len(os.listdir(jd)) == 6
        r = y4m.Y4mReader(ov)
        assert len(r) == 6 and r.dropped == 0 and r.info.sampling == '420mpeg2' and r.info.W == 2 * r.info.H
        assert rep['overlay_video']['bytes'] == r.info.header_bytes + 6 * (6 + r.info.frame_bytes)
        r.close()
    finally:
        import shutil
        shutil.rmtree(os.path.dirname(rep['video']['file']), ignore_errors=True)      # the scratch directory of the dry run


def test_run_vps_synthetic_overlay_video_leaves_the_other_outputs_alone(dev, tmp_path):
    def run(tag, extra):
        out = str(tmp_path / tag)
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'run_vps_synthetic.py'), '--videos', '2', '--frames', '25', '--height', '128',
                            '--width', '256', '--out', out, '--overlay', os.path.join(out, 'ov')] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        return out, _report(p)
    a, ra = run('plain', [])
    b, rb = run('video', ['--overlay-video', str(tmp_path / 'video' / 'clip.y4m')])
    assert 'overlay_video' not in ra and len(rb['overlay_video']['files']) == 2
    for sub in ('ov', os.path.join('pred', 'pan_pred'), os.path.join('pred', 'pan_2ch')):
        fa = sorted(os.listdir(os.path.join(a, sub)))
        assert fa and fa == sorted(os.listdir(os.path.join(b, sub)))
        match, mismatch, errors = filecmp.cmpfiles(os.path.join(a, sub), os.path.join(b, sub), fa, shallow=False)
        assert not mismatch and not errors, (sub, mismatch, errors)
    assert open(os.path.join(a, 'pred', 'pred.json'), 'rb').read() == open(os.path.join(b, 'pred', 'pred.json'), 'rb').read()
    for f in rb['overlay_video']['files']:
        r = y4m.Y4mReader(f)
        assert len(r) == 25 and r.dropped == 0 and r.info.sampling == '420jpeg' and r.info.W == 2 * r.info.H
        r.close()
    assert rb['overlay_video']['files'][0] != rb['overlay_video']['files'][1]
