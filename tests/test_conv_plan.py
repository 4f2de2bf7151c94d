"""Which kernel a vps_conv2d launch gets: vps_amd/csrc/conv_plan.cpp is plain C++, so it is compiled here with a small driver
(no GPU, no HIP) and asked for the plan of every descriptor in tests/conv_plan_cases.json. The expected kernel, grid, block size and
split-K reduce launch in that table were recorded from the commit BEFORE the planner existed (see the table's `source`), i.e. the
table pins the routing of every CONV_CASES / transposed / A/B-test shape of tests/test_hip_ops.py and of one FuseTrack frame."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vps_amd', 'csrc')
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_plan_cases.json')

POINTERS = ('in', 'w', 'out', 'res', 'offset', 'ws', 'w_split', 'gn_stats', 'tile_counter', 'w_thin')
SWITCHES = ('pw', 'h8p', 'n16t', 'n32', 's2_halo', 'thin')

DRIVER = r'''
#include <cstdio>
#include <cstdint>
#include "conv_plan.h"
static bool rd(int& v) { return scanf("%%d", &v) == 1; }
template <class T> static void ptr(T*& p) { int f = 0; rd(f); p = f ? reinterpret_cast<T*>((uintptr_t)0x100000 + (f - 16)) : nullptr; }   // 0 = NULL, 16 + the low address bits
int main() {
    conv_limits lim = {};
    rd(lim.cus); rd(lim.pw_per_cu[0]); rd(lim.pw_per_cu[1]);
    for (int i = 0; i < 4; ++i) rd(lim.thin_per_cu[i]);
    for (;;) {
        vps_conv_desc d = {};
        if (!rd(d.%s)) break;
        %s
        %s
        int s[6];
        for (int i = 0; i < 6; ++i) rd(s[i]);
        conv_switches sw = {s[0] != 0, s[1] != 0, s[2] != 0, s[3] != 0, s[4] != 0, s[5] != 0, false};
        int err = vpsi_conv_check(d);
        conv_plan p = {};
        if (!err) { p = vpsi_conv_plan(d, lim, sw); err = p.err; }
        printf("%%s %%u %%u %%d %%d\n", vpsi_conv_kernel_name(p.kernel), p.grid, p.block, (int)p.needs_reduce, err);
    }
    return 0;
}
'''


def _plans(tmp_path, table):
    ints = table['int_fields']
    src = tmp_path / 'plan_driver.cpp'
    src.write_text(DRIVER % (ints[0], ' '.join('rd(d.%s);' % f for f in ints[1:]), ' '.join('ptr(d.%s);' % f for f in POINTERS)))
    exe = tmp_path / 'plan_driver'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-I', CSRC, str(src), os.path.join(CSRC, 'conv_plan.cpp'), '-o', str(exe)])
    lim = table['limits']
    words = [lim['cus']] + lim['pw_per_cu'] + lim['thin_per_cu']
    for r in table['rows']:
        assert len(r['d']) == len(ints) and len(r['p']) == len(POINTERS) and len(r['sw']) == len(SWITCHES)
        words += r['d'] + r['p'] + r['sw']
    out = subprocess.run([str(exe)], input=' '.join(str(w) for w in words), capture_output=True, text=True, check=True).stdout
    return [ln.split() for ln in out.splitlines()]


def test_the_planner_routes_every_recorded_launch_as_the_commit_before_it(tmp_path):
    table = json.load(open(TABLE))
    assert table['pointers'] == list(POINTERS) and table['switches'] == list(SWITCHES)
    rows = table['rows']
    assert 100 <= len(rows) <= 600
    got = _plans(tmp_path, table)
    assert len(got) == len(rows)
    bad = []
    for r, (name, grid, block, reduce, err) in zip(rows, got):
        if (name, int(grid), int(block), int(reduce), int(err)) != (r['kernel'], r['grid'], r['block'], r['reduce'], 0):
            bad.append((r['what'], dict(zip(table['int_fields'], r['d'])), 'want', (r['kernel'], r['grid'], r['block'], r['reduce']),
                        'got', (name, grid, block, reduce, err)))
    assert not bad, '%d of %d launches re-routed, first: %s' % (len(bad), len(rows), bad[:3])
    # the table reaches every family (a family without a row is a family nobody would see re-routed)
    assert {r['kernel'] for r in rows} >= {'small3x3v', 'small_batched', 'small', 'thin', 'dcn256', 'n16t', 'n32', 'n16', 'h8s2', 'h8p', 'h8', 'halo',
                                           'pw', 'q', 'f32', 'bf16p'}


def test_the_ab_switches_move_a_layer_between_exactly_the_two_kernels_their_tests_compare():
    """rows of the four bitwise A/B tests of tests/test_hip_ops.py: both values of the switch are in the table"""
    rows = json.load(open(TABLE))['rows']
    for i, (sw, on, off) in enumerate((('pw', 'pw', 'q'), ('h8p', 'h8p', 'h8'), ('n16t', 'n16t', 'n16'), ('n32', 'n32', 'halo'))):
        by_desc = {}
        for r in rows:
            by_desc.setdefault((tuple(r['d']), tuple(r['p'])), {})[r['sw'][i]] = r['kernel']
        pairs = [v for v in by_desc.values() if len(v) == 2 and v[0] != v[1]]
        assert pairs, sw
        assert all((v[1], v[0]) == (on, off) for v in pairs), (sw, pairs[:3])
