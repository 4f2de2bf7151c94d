"""Writes tests/golden/jpeg_cases.npz: small JPEG files (their bytes, as uint8 arrays) and the BGR arrays PIL decodes from them.

    python tests/golden/make_jpeg_golden.py

The files are encoded and decoded with PIL (Pillow 12.2 on libjpeg-turbo, API 6.2, when the committed archive was written): the
expected pixels are libjpeg-turbo's default decode (slow-integer IDCT, fancy upsampling), which is what cv2.imread runs too.
Keys: `file/<case>` + `bgr/<case>` for the files the native path takes, `refuse/<case>` for those it must hand to `imread`.
Images: seeded low-pass-filtered noise over the full 0..255 range, and one hard-edged pattern of saturated colours whose ringing
leaves 0..255 after the inverse DCT, so that the range limiter and the colour clamp take part."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SUB = {'444': 0, '422': 1, '420': 2}
SIZES = [(64, 96), (40, 56), (37, 53), (31, 47), (1, 1), (8, 17)]
NARROW = [(9, 2), (9, 3), (9, 4), (9, 5), (2, 9), (3, 6)]          # down-sampled widths 1, 2 (box filter) and 3 (the first fancy one)


def smooth_noise(h, w, seed):
    rng = np.random.RandomState(seed)
    a = rng.rand(h // 4 + 3, w // 4 + 3, 3)
    a = np.kron(a, np.ones((4, 4, 1)))
    for _ in range(2):                                                # 3x3 box filter, twice
        p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode='edge')
        a = sum(p[i:i + a.shape[0], j:j + a.shape[1]] for i in range(3) for j in range(3)) / 9.0
    a = a[2:2 + h, 2:2 + w]
    a = (a - a.min()) / max(a.max() - a.min(), 1e-9)
    a = a * 1.2 - 0.1 + rng.randn(h, w, 3) * 0.02                     # overshoots 0..1: some saturated areas
    return np.clip(a * 255.0 + 0.5, 0, 255).astype(np.uint8)


def hard_edges(h, w):
    y, x = np.mgrid[:h, :w]
    a = np.zeros((h, w, 3), np.uint8)
    a[..., 0] = np.where((x // 3 + y // 5) % 2, 255, 0)
    a[..., 1] = np.where((x // 7) % 2, 0, 255)
    a[..., 2] = np.where((x + 2 * y) % 11 < 4, 255, 0)
    return a


def encode(rgb, sub, **kw):
    im = Image.fromarray(rgb[..., 0].copy(), 'L') if sub == 'grey' else Image.fromarray(rgb, 'RGB')
    b = io.BytesIO()
    if sub != 'grey':
        kw['subsampling'] = SUB[sub]
    im.save(b, 'JPEG', **kw)
    return b.getvalue()


def decode_bgr(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def main():
    out = {}

    def add(name, data):
        assert 'file/' + name not in out, name
        out['file/' + name] = np.frombuffer(data, dtype=np.uint8)
        out['bgr/' + name] = decode_bgr(data)

    seed = 0
    for sub in ('444', '422', '420', 'grey'):
        for (h, w) in SIZES:
            seed += 1
            add('%s_%dx%d_q90' % (sub, h, w), encode(smooth_noise(h, w, seed), sub, quality=90))
        for q in (50, 100):
            seed += 1
            add('%s_37x53_q%d' % (sub, q), encode(smooth_noise(37, 53, seed), sub, quality=q))
            add('%s_40x56_edges_q%d' % (sub, q), encode(hard_edges(40, 56), sub, quality=q))
        seed += 1
        add('%s_40x56_optimize' % sub, encode(smooth_noise(40, 56, seed), sub, quality=90, optimize=True))
        add('%s_37x53_rst_blocks4' % sub, encode(smooth_noise(37, 53, seed), sub, quality=90, restart_marker_blocks=4))
        add('%s_64x96_rst_rows1' % sub, encode(smooth_noise(64, 96, seed), sub, quality=75, restart_marker_rows=1, optimize=True))
    for sub in ('422', '420'):
        for (h, w) in NARROW:
            seed += 1
            add('%s_%dx%d_narrow' % (sub, h, w), encode(smooth_noise(h, w, seed), sub, quality=95))

    base = smooth_noise(40, 56, 99)
    out['refuse/progressive'] = np.frombuffer(encode(base, '420', quality=90, progressive=True), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(np.concatenate([base, base[..., :1]], 2), 'CMYK').save(b, 'JPEG', quality=90)
    out['refuse/cmyk'] = np.frombuffer(b.getvalue(), dtype=np.uint8)
    ex = Image.Exif()
    ex[0x0112] = 6
    out['refuse/exif_orientation6'] = np.frombuffer(encode(base, '420', quality=90, exif=ex), dtype=np.uint8)
    whole = encode(base, '420', quality=90)
    out['refuse/truncated'] = np.frombuffer(whole[:len(whole) * 3 // 5], dtype=np.uint8)

    path = os.path.join(HERE, 'jpeg_cases.npz')
    np.savez_compressed(path, **out)
    print('%s: %d accepted cases, %d refusal cases, %d bytes' % (path, sum(k.startswith('file/') for k in out),
                                                                   sum(k.startswith('refuse/') for k in out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
