"""Which descriptors the Python side of the convolution produces (vps_amd/nhwc.py: PackedConv, conv_geometry), no GPU:
tests/conv_desc_cases.json was recorded by tests/conv_desc_recorder.py from the commit named in its `source`; the tree reproduces
every launch of every configuration and every packed tensor exactly, conv_geometry sizes the split-K buffers for what the planner
of csrc/conv_plan.cpp launches, and the planner takes every recorded descriptor."""
import json
import types

import pytest

import conv_desc_recorder as rec
from test_conv_plan import POINTERS, SWITCHES, TABLE, _plans
from vps_amd import hip, nhwc


@pytest.fixture(scope='module')
def table():
    return json.load(open(rec.FIXTURE))


@pytest.fixture(scope='module')
def plans(table, tmp_path_factory):
    """(kernel, grid, block, reduce, err) of every row from the stand-alone planner driver of tests/test_conv_plan.py"""
    assert table['int_fields'][0] == 'N'
    names = ['inp' if p == 'in' else p for p in POINTERS]
    rows = [dict(d=r['d'], p=[16 * r['p'][table['pointers'].index(n)] for n in names], sw=[1] * len(SWITCHES)) for r in table['rows']]
    got = _plans(tmp_path_factory.mktemp('conv_desc'), dict(int_fields=table['int_fields'], limits=json.load(open(TABLE))['limits'], rows=rows))
    assert len(got) == len(rows)
    return [(g[0], int(g[1]), int(g[2]), int(g[3]), int(g[4])) for g in got]


def _layer(f, p):
    """what conv_geometry reads of a PackedConv, from a recorded row. tile_n and small are the layer's, not the launch's, and no row
    holds them: they are derived as PackedConv derives them with SMALL_ON_MFMA off, which the recorder pins (an MFMA twin, narrow
    but not `small`, never launches then) - a fixture recorded with twins would have to record `small`."""
    assert rec.SWITCHES['SMALL_ON_MFMA'] is False
    deform = bool(p['offset'])
    return types.SimpleNamespace(deform=deform, prec=f['prec'], korder=f['korder'], cout=f['cout'], cout_pad=f['cout_pad'], kpad=f['kpad'],
                                 KH=f['KH'], KW=f['KW'], nclass=f['nclass'], tile_n=nhwc._tile_n(f['cout']), small=f['cout'] <= 4 and not deform)


def test_the_fixture_names_its_source_and_covers_what_it_is_for(table):
    assert '94c6d96' in table['source']
    assert [c[0] for c in rec.CONFIGS] == list(table['configs'])
    ints = table['int_fields']
    col = lambda name: [r['d'][ints.index(name)] for r in table['rows']]
    assert set(col('ksplit')) >= {1, 2, 3, 4, 7, 8, 16, 32} and 256 in col('tile_n') and sum(1 for c in col('gn_cpg') if c) >= 6
    assert any(r['p'][table['pointers'].index('w_thin')] for r in table['rows'])
    assert all(len(c['rows']) == len(c['status']) and len(c['rows']) > 200 for c in table['configs'].values())


@pytest.mark.parametrize('name,config,prec,H,W', rec.CONFIGS, ids=[c[0].replace(' ', '-') for c in rec.CONFIGS])
def test_the_detector_launches_the_recorded_descriptors_in_the_recorded_order(table, name, config, prec, H, W):
    want = table['configs'][name]
    got = rec.record_launches(config, prec, H, W, table['frames'])
    assert len(got) == len(want['rows'])
    for i, ((row, slot), w, s) in enumerate(zip(got, want['rows'], want['status'])):
        assert row == table['rows'][w] and slot == s, (i, dict(zip(table['int_fields'], row['d'])), row, slot, 'want', table['rows'][w], s)


def test_packed_tensors_hash_as_recorded(table):
    got = rec.record_packing()
    assert list(got) == list(table['packing']) == list(rec.MODES)
    for mode, layers in table['packing'].items():
        assert list(got[mode]) == list(layers)
        for name, want in layers.items():
            assert got[mode][name] == want, (mode, name)


def test_conv_geometry_reproduces_every_row_and_sizes_the_split_buffers_for_the_planned_tiles(table, plans):
    ints, ptrs, split = table['int_fields'], table['pointers'], 0
    for r, (kernel, grid, block, reduce, err) in zip(table['rows'], plans):
        f, p = dict(zip(ints, r['d'])), dict(zip(ptrs, r['p']))
        with rec.default_switches():
            geo = nhwc.conv_geometry(_layer(f, p), f['N'], f['Qh'], f['Qw'], f['out_ld'], f['out_coff'], bool(p['res']),
                                     f['cout'] // f['gn_cpg'] if f['gn_cpg'] else None)
        assert (geo.tile_n, geo.ksplit, geo.gn_cpg) == (f['tile_n'], f['ksplit'], f['gn_cpg']), (f, geo)
        assert bool(p['ws']) == (f['ksplit'] > 1) and bool(p['gn_stats']) == (f['gn_cpg'] > 0) and f['gn_rep'] == (nhwc.GN_REP if f['gn_cpg'] else 0)
        if f['ksplit'] == 1:
            assert (geo.scratch_floats, geo.tickets) == (0, 0)
            continue
        split += 1
        assert geo.scratch_floats == f['ksplit'] * f['nclass'] * f['N'] * f['Qh'] * f['Qw'] * f['cout_pad']
        # one ticket per tile: the planner's grid is tiles x splits
        assert reduce == 1 and grid % f['ksplit'] == 0 and geo.tickets >= grid // f['ksplit'], (f, kernel, grid, geo)
    assert split >= 50


def test_the_library_takes_every_recorded_descriptor(table, plans):
    bad = [(dict(zip(table['int_fields'], r['d'])), g) for r, g in zip(table['rows'], plans) if g[4] != 0]
    assert not bad, '%d of %d descriptors rejected by vpsi_conv_check / the planner, first: %s' % (len(bad), len(plans), bad[:3])
    # f16x3 launches report into the layer's own slot, the others carry no status word
    prec = table['int_fields'].index('prec')
    for c in table['configs'].values():
        assert all((s >= 0) == (table['rows'][i]['d'][prec] == hip.PREC_F16X3) for i, s in zip(c['rows'], c['status']))
