"""CPU half of the Y4M work (vps_amd/y4m.py, csrc/y4m_host.cpp): the container parser on valid, refused, truncated and damaged headers,
`Y4mReader` on real files, the NumPy restatement of the colour arithmetic (tests/y4m_restate.py) against the real-valued conversion
over the whole colour cube and against answers worked out by hand, and the parser under the address / undefined-behaviour sanitizers
as a stand-alone program. The device kernels are compared with the restatement in tests/test_y4m_gpu.py."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import y4m_restate as R
from vps_amd import hip, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |decode444(encode444(x)) - x| of the RESTATEMENT over the whole BGR cube, per (matrix, range): half a level of rounding in each of
# Y, Cb, Cr, and a level of Cb is worth up to 1.772 (bt709: 1.856) levels of B - times 255 / 224 in limited range, which keeps 219 / 224
# of the 255 levels. Computed by test_round_trip_bound_of_the_restatement below, from the restatement alone;
# tests/test_y4m_gpu.py holds the device round trip to it.
ROUND_TRIP_BOUND = {('bt601', 'limited'): 2, ('bt601', 'full'): 1, ('bt709', 'limited'): 2, ('bt709', 'full'): 1}


def _code(e):
    return int(str(e.value).rsplit('code ', 1)[1].rstrip(')'))


# ---------------------------------------------------------------------------------------------- parser

@pytest.mark.parametrize('c, sampling, cw, ch', [(None, '420jpeg', 9, 6), ('420jpeg', '420jpeg', 9, 6), ('420', '420jpeg', 9, 6),
                                                 ('420mpeg2', '420mpeg2', 9, 6), ('422', '422', 9, 11), ('444', '444', 17, 11),
                                                 ('mono', 'mono', 0, 0)])
def test_valid_headers_for_every_supported_colour_space_and_odd_sizes(c, sampling, cw, ch):
    tags = ['W17', 'H11'] + (['C' + c] if c else [])
    info = y4m.y4m_info(('YUV4MPEG2 ' + ' '.join(tags) + '\n').encode() + b'FRAME\n')
    assert (info.W, info.H, info.sampling, info.CW, info.CH) == (17, 11, sampling, cw, ch)
    assert info.frame_bytes == 17 * 11 + 2 * cw * ch == R.frame_bytes(11, 17, sampling)
    assert info.range == 'limited' and info.fps == (0, 0) and info.aspect == (0, 0) and not info.progressive
    assert info.header_bytes == len('YUV4MPEG2 ' + ' '.join(tags)) + 1


def test_optional_tags_in_any_order():
    tags = ['W64', 'H48', 'F30000:1001', 'A1:1', 'Ip', 'C420mpeg2', 'XCOLORRANGE=FULL', 'XYSCSS=420MPEG2']
    for perm in itertools.islice(itertools.permutations(tags), 0, 40320, 97):
        info = y4m.y4m_info(('YUV4MPEG2 ' + ' '.join(perm) + '\n').encode())
        assert (info.W, info.H, info.fps, info.aspect, info.progressive, info.sampling, info.range) == \
            (64, 48, (30000, 1001), (1, 1), True, '420mpeg2', 'full')
    assert y4m.y4m_info(b'YUV4MPEG2 W2 H2 I? A0:0 XCOLORRANGE=LIMITED\n').range == 'limited'
    assert y4m.y4m_info(b'YUV4MPEG2  H2   W3 \n').W == 3                      # runs of blanks between and behind the tags


@pytest.mark.parametrize('header, code', [
    (b'YUV4MPEG3 W4 H4\n', 2), (b'RIFF....', 2), (b'', 3), (b'YUV4MPEG2 H4\n', 5), (b'YUV4MPEG2 W4\n', 5), (b'YUV4MPEG2 W0 H4\n', 6),
    (b'YUV4MPEG2 W4 H-4\n', 6), (b'YUV4MPEG2 W99999999999 H4\n', 7), (b'YUV4MPEG2 W4 H' + b'9' * 40 + b'\n', 7), (b'YUV4MPEG2 W65536 H32768\n', 7), (b'YUV4MPEG2 W4x H4\n', 4),
    (b'YUV4MPEG2 W H4\n', 4), (b'YUV4MPEG2 W4 H4 F30\n', 4), (b'YUV4MPEG2 W4 H4 F30:x\n', 4), (b'YUV4MPEG2 W4 H4 It\n', 8),
    (b'YUV4MPEG2 W4 H4 Ib\n', 8), (b'YUV4MPEG2 W4 H4 Im\n', 8), (b'YUV4MPEG2 W4 H4 Iq\n', 14), (b'YUV4MPEG2 W4 H4 C420paldv\n', 9),
    (b'YUV4MPEG2 W4 H4 C420p10\n', 10), (b'YUV4MPEG2 W4 H4 C444p16\n', 10), (b'YUV4MPEG2 W4 H4 Cmono12\n', 10),
    (b'YUV4MPEG2 W4 H4 C444alpha\n', 11), (b'YUV4MPEG2 W4 H4 C411\n', 12), (b'YUV4MPEG2 W4 H4 XCOLORRANGE=WIDE\n', 13),
    (b'YUV4MPEG2 W4 H4 X' + b'y' * 240 + b'\n', 3), (b'YUV4MPEG2 W4 H4', 3)])
def test_every_refusal_has_its_code_and_its_words(header, code):
    with pytest.raises(ValueError) as e:
        y4m.y4m_info(header)
    assert _code(e) == -1000 - code and y4m.REFUSALS[code] in str(e.value)


def test_the_largest_size_the_parser_takes_and_the_256_byte_limit():
    assert y4m.y4m_info(b'YUV4MPEG2 W65535 H32768 Cmono\n').frame_bytes == 65535 * 32768
    head = b'YUV4MPEG2 W4 H4 X'
    ok = head + b'y' * (255 - len(head)) + b'\n'
    assert len(ok) == 256 and y4m.y4m_info(ok).header_bytes == 256
    with pytest.raises(ValueError):
        y4m.y4m_info(head + b'y' * (256 - len(head)) + b'\n')


def test_truncation_at_every_byte_of_a_valid_header_is_refused():
    header = b'YUV4MPEG2 W640 H480 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n'
    assert y4m.y4m_info(header).header_bytes == len(header)
    for n in range(len(header)):
        with pytest.raises(ValueError):
            y4m.y4m_info(header[:n])


@pytest.mark.parametrize('sampling', R.SAMPLINGS)
@pytest.mark.parametrize('rng', ['limited', 'full'])
def test_written_header_parses_back_to_the_same_info(sampling, rng):
    for W, H, fps, aspect, prog in ((1, 1, (0, 0), (0, 0), False), (1919, 1081, (30000, 1001), (128, 117), True),
                                    (2048, 1024, (30, 1), (0, 0), True)):
        info = y4m.make_info(W, H, fps, sampling, rng, aspect, prog)
        assert (info.W, info.H, info.fps, info.aspect, info.progressive, info.sampling, info.range) == (W, H, fps, aspect, prog, sampling, rng)
        line = y4m.y4m_header(info)
        assert line.startswith(b'YUV4MPEG2 W%d H%d' % (W, H)) and line.endswith(b'\n') and len(line) == info.header_bytes
        assert y4m.y4m_info(line) == info and y4m.y4m_header(y4m.y4m_info(line)) == line
    d = y4m.make_info(8, 8).desc()
    out, n = (ctypes.c_char * 256)(), ctypes.c_int32(-7)
    assert hip.load_host().vps_y4m_write_header(ctypes.byref(d), out, 10, ctypes.byref(n)) == -1031 and n.value == -7 and out.raw == bytes(256)
    d.W = 0
    assert hip.load_host().vps_y4m_write_header(ctypes.byref(d), out, 256, ctypes.byref(n)) == -1030


def test_frame_lines():
    assert y4m.frame_header(b'FRAME\n' + bytes(10)) == 6
    assert y4m.frame_header(b'FRAME Ip Xabc=1\nrest') == 16
    assert y4m.frame_header(b'FRAME ' + b'x' * 73 + b'\n') == 80
    for bad, code in ((b'FRAME', 21), (b'FRAME Ip', 21), (b'FRAME ' + b'x' * 74 + b'\n', 21), (b'FRAMX\n', 20), (b'FRAMES\n', 20),
                      (b'frame\n', 20), (b'', 21), (b'FRA', 21), (b'YUV4MPEG2 W4 H4\n', 20)):
        with pytest.raises(ValueError) as e:
            y4m.frame_header(bad)
        assert _code(e) == -1000 - code, bad


# ---------------------------------------------------------------------------------------------- reader

def _clip(path, W, H, sampling, n, params=(), tail=b''):
    rs = np.random.RandomState(5)
    info = y4m.make_info(W, H, (25, 1), sampling)
    frames = [rs.randint(0, 256, info.frame_bytes, dtype=np.uint8) for _ in range(n)]
    with open(path, 'wb') as f:
        f.write(y4m.y4m_header(info))
        for t, fr in enumerate(frames):
            f.write(b'FRAME' + (b' ' + params[t] if t < len(params) and params[t] else b'') + b'\n' + fr.tobytes())
        f.write(tail)
    return info, frames


@pytest.mark.parametrize('tail_bytes', [0, 1, 5, 6, 7, 100])
def test_reader_drops_and_counts_a_truncated_last_frame(tmp_path, tail_bytes):
    tail = (b'FRAME\n' + bytes(range(200)))[:tail_bytes]
    info, frames = _clip(tmp_path / 'c.y4m', 13, 7, '420jpeg', 3, tail=tail)
    r = y4m.Y4mReader(tmp_path / 'c.y4m')
    assert len(r) == 3 and r.dropped == (tail_bytes > 0) and r.info == info
    slot = np.zeros(info.frame_bytes + 3, dtype=np.uint8)
    for t in (2, 0, 1):
        assert r.readinto(t, slot) == info.frame_bytes
        assert np.array_equal(slot[:info.frame_bytes], frames[t]) and not slot[info.frame_bytes:].any()
    r.close()
    r.close()


def test_reader_takes_frame_parameters_and_refuses_a_damaged_frame_line(tmp_path):
    info, frames = _clip(tmp_path / 'p.y4m', 8, 6, '444', 4, params=(b'', b'Ip', b'', b'Xkey=value Ip'))
    r = y4m.Y4mReader(str(tmp_path / 'p.y4m'))
    assert len(r) == 4 and r.dropped == 0
    import torch
    slot = torch.zeros(info.frame_bytes, dtype=torch.uint8)
    for t in range(4):
        r.readinto(t, slot)
        assert np.array_equal(slot.numpy(), frames[t])
    data = bytearray(open(tmp_path / 'p.y4m', 'rb').read())
    at = info.header_bytes + 6 + info.frame_bytes
    assert data[at:at + 5] == b'FRAME'
    data[at + 4] = ord('X')
    open(tmp_path / 'bad.y4m', 'wb').write(data)
    with pytest.raises(ValueError, match='frame 1'):
        y4m.Y4mReader(tmp_path / 'bad.y4m')
    with pytest.raises(ValueError, match='bad magic'):
        open(tmp_path / 'no.y4m', 'wb').write(b'not a video')
        y4m.Y4mReader(tmp_path / 'no.y4m')


# ---------------------------------------------------------------------------------------------- arithmetic

@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
@pytest.mark.parametrize('rng', ['limited', 'full'])
def test_restatement_is_within_one_level_of_the_real_valued_conversion_over_the_cube(matrix, rng):
    """the 16-bit coefficient error times 3 * 255 is far below a level, so only rounding ties can differ: at most one level, anywhere"""
    worst_d = worst_e = 0
    for a, b, c in R.cube_slabs():
        a, b, c = np.broadcast_arrays(a, b, c)
        got, want = R.decode_pixels(a, b, c, matrix, rng), R.decode_real(a, b, c, matrix, rng)         # (Y, Cb, Cr) cube, 4:4:4
        worst_d = max(worst_d, max(int(np.abs(g.astype(np.int64) - w).max()) for g, w in zip(got, want)))
        got, want = R.encode_pixels(a, b, c, matrix, rng), R.encode_real(a, b, c, matrix, rng)         # (B, G, R) cube
        worst_e = max(worst_e, max(int(np.abs(g - w).max()) for g, w in zip(got, want)))
    print('%s %s: decode differs by at most %d, encode by at most %d level(s)' % (matrix, rng, worst_d, worst_e))
    assert worst_d <= 1 and worst_e <= 1


@pytest.mark.parametrize('matrix, rng', sorted(ROUND_TRIP_BOUND))
def test_round_trip_bound_of_the_restatement(matrix, rng):
    got = R.round_trip_error(matrix, rng)
    print('%s %s: round trip differs by at most %d level(s)' % (matrix, rng, got))
    assert got == ROUND_TRIP_BOUND[(matrix, rng)]


def test_integer_coefficients_are_the_published_ones():
    d, e = R.int_coefficients('bt601', 'limited')                   # the familiar three-decimal constants of the "studio swing" matrices
    for k, v in dict(ky=1.164, cr_r=1.596, cb_g=-0.392, cr_g=-0.813, cb_b=2.017).items():
        assert abs(d[k] / 65536.0 - v) < 6e-4, k
    for got, v in zip(e['y'] + e['cb'] + e['cr'], (0.257, 0.504, 0.098, -0.148, -0.291, 0.439, 0.439, -0.368, -0.071)):
        assert abs(got / 65536.0 - v) < 6e-4
    d, e = R.int_coefficients('bt709', 'limited')
    for k, v in dict(ky=1.164, cr_r=1.793, cb_g=-0.213, cr_g=-0.533, cb_b=2.112).items():
        assert abs(d[k] / 65536.0 - v) < 6e-4, k
    d, e = R.int_coefficients('bt601', 'full')
    assert d['ky'] == 65536 and e['cb'][2] == 32768 and sum(e['y']) == 65536


def test_known_answers():
    def dec(y, cb, cr, **kw):
        return [int(v) for v in np.concatenate(R.decode_pixels(*(np.array([v]) for v in (y, cb, cr)), **kw))]

    def enc(b, g, r, **kw):
        return [int(v[0]) for v in R.encode_pixels(*(np.array([v]) for v in (b, g, r)), **kw)]
    assert dec(16, 128, 128) == [0, 0, 0] and dec(235, 128, 128) == [255, 255, 255]            # limited black, white
    assert dec(126, 128, 128) == [128, 128, 128]                                               # (126 - 16) * 255 / 219 = 128.08
    assert dec(0, 128, 128) == [0, 0, 0] and dec(255, 128, 128) == [255, 255, 255]             # below / above nominal: clamped
    assert dec(0, 128, 128, rng='full') == [0, 0, 0] and dec(255, 128, 128, rng='full') == [255, 255, 255]
    assert enc(0, 0, 0) == [16, 128, 128] and enc(255, 255, 255) == [235, 128, 128] and enc(128, 128, 128) == [126, 128, 128]
    # 16 + 219 * (0.299, 0.587, 0.114) = 81.48, 144.55, 40.97; chroma 128 +- 112 on its own primary,
    # 128 - 224 * 0.299 / 1.772 = 90.20, 128 - 224 * 0.587 / 1.772 = 53.80, 128 - 224 * 0.587 / 1.402 = 34.21, 128 - 224 * 0.114 / 1.402 = 109.79
    assert enc(0, 0, 255) == [81, 90, 240] and enc(0, 255, 0) == [145, 54, 34] and enc(255, 0, 0) == [41, 240, 110]
    assert enc(0, 0, 255, rng='full') == [76, 85, 255] and enc(255, 0, 0, rng='full') == [29, 255, 107]   # 128 + 127.5 rounds to 256: clamped
    for b, g, r in ((0, 0, 255), (0, 255, 0), (255, 0, 0)):
        assert max(abs(x - y) for x, y in zip(dec(*enc(b, g, r)), (b, g, r))) <= 1


# the weights of every position of a 4-sample axis on its 2 chroma samples, written out by hand (denominator 4):
CENTRE = np.array([[4, 0], [3, 1], [1, 3], [0, 4]])        # 420jpeg both axes, 420mpeg2 rows: position 0 and 3 have their far sample clamped onto the near one
COSITED = np.array([[4, 0], [2, 2], [0, 4], [0, 4]])       # 420mpeg2 / 422 columns: even positions sit on a sample, position 3 is half-way to a clamped one


@pytest.mark.parametrize('sampling, av, ah', [('420jpeg', CENTRE, CENTRE), ('420mpeg2', CENTRE, COSITED), ('422', 4 * np.eye(4, dtype=np.int64), COSITED)])
def test_upsampling_weights_on_a_two_sample_axis(sampling, av, ah):
    rs = np.random.RandomState(3)
    for c in (np.array([[0, 255], [255, 0]]), np.array([[10, 20], [30, 40]]), rs.randint(0, 256, (2, 2))):
        c = np.repeat(c, 2, axis=0)[[0, 1, 2, 3]] if sampling == '422' else c                   # 422: a plane of 4 rows
        want = (av @ c @ ah.T + 8) >> 4
        assert np.array_equal(R.upsample(c.astype(np.uint8), 4, 4, sampling), want)
    assert np.array_equal(R.upsample(np.array([[7]], dtype=np.uint8), 1, 1, '420jpeg'), [[7]])          # all border
    assert np.array_equal(R.upsample(np.array([[0, 200]], dtype=np.uint8), 1, 3, '420mpeg2'), [[0, 100, 200]])
    assert np.array_equal(R.upsample(np.array([[0, 200]], dtype=np.uint8), 1, 3, '420jpeg'), [[0, 50, 150]])


def test_chroma_reduction_by_hand():
    c = np.array([[0, 8, 16, 24, 40], [8, 16, 24, 32, 48], [100, 100, 100, 100, 100]], dtype=np.int64)      # 3 x 5: clamped right and bottom
    assert np.array_equal(R.reduce_chroma(c, '420jpeg'), [[8, 24, 44], [100, 100, 100]])
    # (1, 2, 1) on columns -1(=0), 0, 1 | 1, 2, 3 | 3, 4, 5(=4) of the row sums 8, 24, 40, 56, 88
    assert np.array_equal(R.reduce_chroma(c, '420mpeg2'), [[(8 + 16 + 24 + 4) >> 3, (24 + 80 + 56 + 4) >> 3, (56 + 176 + 88 + 4) >> 3], [100, 100, 100]])
    assert R.reduce_chroma(c, '444') is c


def test_overlay_videos_are_named_after_their_frames():
    from vps_amd.postprocess import overlay_video_name, video_name_of
    city = ['%04d_%04d_frankfurt_000000_%06d_newImg8bit.png' % (5, 25 + f, 1736 + f) for f in range(6)]
    assert video_name_of(city, 0) == '0005' and video_name_of(['dir/clip_%03d.png' % f for f in range(3)], 1) == 'clip'
    assert video_name_of(['a.png', 'b.png'], 2) == 'v002' and video_name_of(['only_frame.png'], 0) == 'only_frame'
    assert overlay_video_name('out/ov.y4m', '0005', 1) == 'out/ov.y4m' and overlay_video_name('out/ov.y4m', '0005', 3) == 'out/ov.0005.y4m'
    assert overlay_video_name('ov.y4m', 'clip', 2, taken=['ov.clip.y4m']) == 'ov.clip-2.y4m'


def test_feeder_refuses_a_y4m_clip_on_a_host_stand_in(tmp_path):
    """the documented choice: the conversion exists on the device only, a host `prep` is refused when the feeder is made"""
    import torch
    from vps_amd.pipeline import ClipFeeder
    _clip(tmp_path / 'c.y4m', 16, 8, '420jpeg', 2)

    class HostPrep:
        device = torch.device('cpu')
    with pytest.raises(hip.VpsHipError, match='no host path'):
        ClipFeeder(str(tmp_path / 'c.y4m'), HostPrep())


# ---------------------------------------------------------------------------------------------- sanitizers

SAN_MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "vps_hip.h"

static int cases = 0;

// every call gets a heap buffer of exactly n bytes: a read past the length the parser was given is a sanitizer report
static int info_of(const char* s, size_t n, vps_y4m_desc* d) {
    uint8_t* b = (uint8_t*)malloc(n ? n : 1);
    memcpy(b, s, n);
    if (!n) { free(b); b = (uint8_t*)malloc(1); }
    const int st = vps_y4m_info(n ? b : b + 0, (int64_t)n, d);
    int32_t len = 0;
    vps_y4m_frame_header(b, (int64_t)n, &len);
    free(b);
    ++cases;
    return st;
}

int main() {
    const char* valid[] = {
        "YUV4MPEG2 W640 H480 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n", "YUV4MPEG2 W17 H11\n", "YUV4MPEG2 H2 W3 Cmono\n",
        "YUV4MPEG2 W1919 H1081 F30000:1001 I? A128:117 C444 XYSCSS=444 XCOLORRANGE=LIMITED\n", "YUV4MPEG2 C422 W8 H8 A0:0\n"};
    for (const char* v : valid) {
        const size_t n = strlen(v);
        vps_y4m_desc d;
        if (info_of(v, n, &d) != 0 || d.header_bytes != (int)n) { printf("valid header refused: %s", v); return 1; }
        for (size_t k = 0; k < n; ++k)
            if (info_of(v, k, &d) == 0) { printf("truncated header accepted at %zu: %s", k, v); return 1; }
        char* m = (char*)malloc(n);
        for (size_t k = 0; k < n; ++k)
            for (int bit = 0; bit < 8; ++bit) {
                memcpy(m, v, n);
                m[k] ^= (char)(1 << bit);
                vps_y4m_desc e;
                if (info_of(m, n, &e) == 0 && (e.W <= 0 || e.H <= 0 || e.frame_bytes <= 0 || e.header_bytes > (int)n)) { printf("bad info\n"); return 1; }
            }
        free(m);
        // the header written back into exactly sized buffers, and into every shorter one
        uint8_t* exact = (uint8_t*)malloc(256);
        int32_t len = 0;
        if (vps_y4m_write_header(&d, exact, 256, &len) != 0) { printf("write refused\n"); return 1; }
        for (int cap = 0; cap <= len; ++cap) {
            uint8_t* o = (uint8_t*)malloc(cap ? cap : 1);
            int32_t l2 = 0;
            const int st = vps_y4m_write_header(&d, o, cap, &l2);
            if ((st == 0) != (cap == len)) { printf("capacity %d of %d: %d\n", cap, len, st); return 1; }
            if (st == 0) {
                vps_y4m_desc back;
                if (vps_y4m_info(o, cap, &back) != 0 || back.W != d.W || back.H != d.H || back.sampling != d.sampling || back.range != d.range ||
                    back.frame_bytes != d.frame_bytes) { printf("round trip\n"); return 1; }
            }
            free(o);
            ++cases;
        }
        free(exact);
    }
    const char* lines[] = {"FRAME\n", "FRAME Ip Xa=b\n", "FRAME", "FRAMES\n", "FRAME xxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxxx\n"};
    for (const char* v : lines)
        for (size_t k = 0; k <= strlen(v); ++k) {
            uint8_t* b = (uint8_t*)malloc(k ? k : 1);
            memcpy(b, v, k);
            int32_t len = -1;
            const int st = vps_y4m_frame_header(b, (int64_t)k, &len);
            if (st == 0 && (len <= 0 || len > (int)k || b[len - 1] != '\n')) { printf("bad frame line length\n"); return 1; }
            free(b);
            ++cases;
        }
    printf("OK %d\n", cases);
    return 0;
}
'''


def test_parser_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, no Python) built with y4m_host.cpp under -fsanitize=address,undefined: valid, truncated and
    bit-flipped headers in exactly sized heap buffers"""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no C++ compiler')
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    base = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g', '-O1', '-std=c++17']
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libsan'], []):
        flags = base + extra
        if subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True).returncode == 0 and \
                subprocess.run([str(tmp_path / 'probe')], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip('the compiler has no sanitizer runtime')
    src = tmp_path / 'y4m_san.cpp'
    src.write_text(SAN_MAIN)
    exe = tmp_path / 'y4m_san'
    subprocess.check_call([cxx] + flags + ['-I', os.path.join(ROOT, 'include'), str(src), os.path.join(ROOT, 'vps_amd', 'csrc', 'y4m_host.cpp'), '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('OK '), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
