"""CPU: the NumPy restatement of the flow colour coding (tests/flow_vis_restate.py) against the reference's own images
(tests/golden/flow_vis_cases.npz, written by tests/golden/make_flow_vis_golden.py from the real `vis_flow` / `writeFlow`), and the
.flo reader / writer of vps_amd/flowvis.py against the reference's file bytes. The GPU tests (tests/test_flow_vis_gpu.py) compare the
kernels with the same golden images and with this restatement."""
import numpy as np
import pytest

import flow_vis_restate as F
from vps_amd import flowvis

CASES, NUMPY_VERSION = F.load_golden()


def test_golden_has_the_cases_and_the_special_pixels():
    assert {c: v['flow'].shape for c, v in CASES.items()} == {'1x1_zero': (1, 1, 2), '3x5': (3, 5, 2), '67x131': (67, 131, 2),
                                                              '96x160_smooth': (96, 160, 2)}
    assert NUMPY_VERSION
    for c in ('67x131', '96x160_smooth'):
        row = CASES[c]['flow'][0, :9]
        assert row[0].tolist() == [0, 0] and row[7, 0] > 1e9 and row[8, 1] > 1e9 and np.signbit(row[5, 1]) and row[5, 1] == 0


@pytest.mark.parametrize('case', sorted(CASES))
def test_restatement_equals_the_float64_golden(case):
    c = CASES[case]
    got = F.colour(c['flow'])
    assert got.dtype == np.uint8 and np.array_equal(got, c['rgb64']), int((got != c['rgb64']).sum())


@pytest.mark.parametrize('case', sorted(CASES))
def test_restatement_is_within_one_level_of_the_float32_golden(case):
    c = CASES[case]
    d = np.abs(F.colour(c['flow']).astype(np.int32) - c['rgb32'].astype(np.int32))
    assert d.max() <= 1 and (d.max(-1) > 0).mean() <= 1e-3, (int(d.max()), float((d.max(-1) > 0).mean()))


@pytest.mark.parametrize('case', sorted(CASES))
def test_restatement_through_a_strided_view_and_with_a_perturbed_arctan2(case):
    c = CASES[case]
    for ld, coff in ((4, 0), (8, 2)):
        wide = F.strided(c['flow'], ld, coff)
        assert F.max_radius(wide, ld, coff) == F.max_radius(c['flow'])
        assert np.array_equal(F.colour(wide, None, ld, coff), c['rgb64'])
    for ulps in (-2, 2):                                                         # the device's atan2 may round differently: no level moves

        def moved(y, x, n=ulps):
            a = np.arctan2(y, x)
            for _ in range(abs(n)):
                a = np.nextafter(a, np.where(a == np.pi, a, np.inf) if n > 0 else np.where(a == -np.pi, a, -np.inf))
            return a
        assert np.array_equal(F.colour(c['flow'], atan2=moved), c['rgb64']), ulps


def test_fixed_normaliser():
    flow = CASES['96x160_smooth']['flow']
    own = F.max_radius(flow)
    assert np.array_equal(F.colour(flow, own), CASES['96x160_smooth']['rgb64'])
    small = F.colour(flow, own / 4)                                               # most pixels beyond the normaliser: the darkened branch
    u, v = F.known(flow)
    beyond = np.sqrt(u * u + v * v) / (own / 4 + np.finfo(np.float64).eps) > 1
    assert 0.3 < beyond.mean() < 1 and small[beyond].max() <= 191                 # floor(255 * 0.75)


SPECIAL = [(0, 0), (2.5, 0), (-2.5, 0), (0, 1.5), (0, -1.5), (2.5, -0.0), (1.25, 1.25)]


def test_colour_wheel_has_55_rows_and_its_ramps():
    cw = F.colour_wheel()
    assert cw.shape == (55, 3) and cw.dtype == np.float64
    assert cw[0].tolist() == [255, 0, 0] and cw[15].tolist() == [255, 255, 0] and cw[21].tolist() == [0, 255, 0]
    assert cw[25].tolist() == [0, 255, 255] and cw[36].tolist() == [0, 0, 255] and cw[49].tolist() == [255, 0, 255]
    assert ((cw == 0) | (cw == 255)).any(1).all() and (cw.max(1) == 255).all() and (cw == np.floor(cw)).all()
    # (the other 49 rows are pinned by the whole-image equalities above: every row is used by the 67x131 and 96x160 cases)
    for case in ('67x131', '96x160_smooth'):
        u, v = F.known(CASES[case]['flow'])
        pos = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
        assert set(np.unique(pos.astype(np.int64)).tolist()) == set(range(55)), case


@pytest.mark.parametrize('case', ['67x131', '96x160_smooth'])
def test_colour_wheel_entries_recovered_from_the_goldens_special_pixels(case):
    """What the special pixels of the first row determine. A pixel of radius r <= 1 shows floor(255 * (1 - r * (1 - hue))), so a level L
    of the reference's image bounds the hue: 1 - (1 - L / 255) / r <= hue < 1 - (1 - (L + 1) / 255) / r. Three of the pixels sit ON
    wheel entries (u = 2.5, v = +0: entry 0; u = -2.5: entry 27; u = 2.5, v = -0: entry 54 -> 0 with weight 0), where hue = entry / 255:
    the recovered interval of 255 * hue must hold the wheel's entry. The others sit between two entries (13 | 14, 40 | 41, 6 | 7): the
    interval must hold the interpolated value."""
    cw = F.colour_wheel()
    c = CASES[case]
    flow, rgb = c['flow'], c['rgb64'].astype(np.float64)
    den = F.max_radius(flow) + np.finfo(np.float64).eps
    seen = {}
    for x, (u, v) in enumerate(SPECIAL):
        assert flow[0, x].tolist() == [u, v]
        if (u, v) == (0, 0):
            assert rgb[0, x].tolist() == [255, 255, 255]                         # radius 0: white whatever the wheel holds
            continue
        u, v = np.float64(u) / den, np.float64(v) / den
        r = np.sqrt(u * u + v * v)
        assert 0 < r < 1
        lo = 255 * (1 - (1 - rgb[0, x] / 255) / r)                               # recovered from the golden alone
        hi = 255 * (1 - (1 - (rgb[0, x] + 1) / 255) / r)
        pos = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54
        k0 = int(pos)
        f = pos - k0
        entry = (1 - f) * cw[k0] + f * cw[(k0 + 1) % 55]
        assert ((lo - 1e-9 <= entry) & (entry < hi + 1e-9)).all(), (x, k0, f, lo.tolist(), entry.tolist(), hi.tolist())
        seen[k0] = f
    assert set(seen) == {0, 27, 54, 13, 40, 6} and seen[0] == 0 and seen[27] == 0 and seen[54] == 0, seen
    assert c['rgb64'][0, 7].tolist() == [255, 255, 255] and c['rgb64'][0, 8].tolist() == [255, 255, 255]    # unknown flow: zero flow, white


@pytest.mark.parametrize('case', sorted(CASES))
def test_flo_bytes_equal_the_references_file(case):
    c = CASES[case]
    assert flowvis.flo_bytes(c['flow']) == c['flo']
    assert flowvis.flo_bytes(np.ascontiguousarray(c['flow'].transpose(2, 0, 1))[None]) == c['flo']      # [1,2,H,W]
    import torch
    assert flowvis.flo_bytes(torch.from_numpy(c['flow'])) == c['flo']


def test_flo_round_trip_and_bad_files(tmp_path):
    for case, c in CASES.items():
        name = flowvis.write_flo(c['flow'], str(tmp_path / 'sub' / (case + '.flo')))
        back = flowvis.read_flo(name)
        assert back.dtype == np.float32 and back.shape == c['flow'].shape
        assert back.tobytes() == c['flow'].tobytes()                             # bit for bit, the sign of -0 included
    bad = tmp_path / 'bad.flo'
    bad.write_bytes(b'\x00' * 20)
    with pytest.raises(ValueError):
        flowvis.read_flo(str(bad))
    short = tmp_path / 'short.flo'
    short.write_bytes(CASES['3x5']['flo'][:-4])
    with pytest.raises(ValueError):
        flowvis.read_flo(str(short))
    assert flowvis.flow_name('out', 'a/b/0001_newImg8bit.png', 'flo') == 'out/0001_newImg8bit.flo'
