"""NumPy float64 restatement of what `vps_flow_max_radius` / `vps_flow_colour` (csrc/flow_vis_ops.hip) compute: the colour coding of the
reference's `vis_flow(flow.astype(np.float64))`, written from its published algorithm (the Middlebury colour wheel), with the two things
the device adds: a fixed normaliser (`max_rad`) and a flow addressed inside a wider NHWC map (`ld`, `coff`).
tests/test_flow_vis.py pins it to the reference's images (tests/golden/flow_vis_cases.npz) level for level."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flow_vis_cases.npz')
RAMPS = (15, 6, 4, 11, 13, 6)            # RY, YG, GC, CB, BM, MR
UNKNOWN_FLOW_THRESH = 1e9


def colour_wheel():
    """float64 [55,3] RGB, 0..255: red -> yellow -> green -> cyan -> blue -> magenta -> red, each ramp floor(255 * j / N)"""
    rows = []
    # (channel held at 255, channel that ramps, rising?) per segment
    plan = ((0, 1, True), (1, 0, False), (1, 2, True), (2, 1, False), (2, 0, True), (0, 2, False))
    for n, (full, ramp, rising) in zip(RAMPS, plan):
        for j in range(n):
            c = [0.0, 0.0, 0.0]
            c[full] = 255.0
            step = float(np.floor(255 * j / n))
            c[ramp] = step if rising else 255.0 - step
            rows.append(c)
    return np.asarray(rows, dtype=np.float64)


def strided(flow, ld, coff, fill=777.0):
    """the flow [H,W,2] inside a float32 [H,W,ld] map at channel offset coff; the other channels hold `fill`"""
    H, W = flow.shape[:2]
    wide = np.full((H, W, ld), fill, dtype=np.float32)
    wide[:, :, coff:coff + 2] = flow
    return wide


def known(flow, ld=2, coff=0):
    """float64 (u, v) with the unknown-flow rule: u > 1e9 or v > 1e9 -> both 0"""
    f = np.asarray(flow).reshape(flow.shape[0], flow.shape[1], ld)[:, :, coff:coff + 2].astype(np.float64)
    u, v = f[..., 0].copy(), f[..., 1].copy()
    unk = (u > UNKNOWN_FLOW_THRESH) | (v > UNKNOWN_FLOW_THRESH)
    u[unk] = 0
    v[unk] = 0
    return u, v


def max_radius(flow, ld=2, coff=0):
    u, v = known(flow, ld, coff)
    return np.float64(np.max(np.sqrt(u * u + v * v)))


def colour(flow, max_rad=None, ld=2, coff=0, atan2=np.arctan2):
    """-> RGB uint8 [H,W,3]. max_rad None: the frame's own maximum radius. `atan2`: replaceable, to show that its last ulps move nothing.
    Every line is one rounded float64 operation of the kernel, in its order."""
    u, v = known(flow, ld, coff)
    if max_rad is None:
        max_rad = max_radius(flow, ld, coff)
    den = np.float64(max_rad) + np.finfo(np.float64).eps
    u = u / den
    v = v / den
    wheel = colour_wheel() / 255                                   # the table the kernel keeps in LDS
    entries = wheel.shape[0]
    radius = np.sqrt(u * u + v * v)
    turn = atan2(-v, -u) / np.pi                                   # -1 .. 1 round the wheel
    pos = (turn + 1) / 2 * (entries - 1)                           # 0 .. 54
    lower = np.clip(pos.astype(np.int64), 0, entries - 1)          # pos >= 0: truncation is the floor
    upper = np.where(lower + 1 == entries, 0, lower + 1)           # the wheel closes
    frac = pos - lower
    in_range = radius <= 1
    img = np.empty(u.shape + (3,), dtype=np.uint8)
    for ch in range(3):
        hue = (1 - frac) * wheel[lower, ch] + frac * wheel[upper, ch]
        shade = np.where(in_range, 1 - radius * (1 - hue), hue * 0.75)      # saturation grows with the radius; beyond it: darkened
        img[..., ch] = np.floor(255 * shade).astype(np.uint8)
    return img


def load_golden():
    """{case: dict(flow, rgb64, rgb32, flo bytes)}, numpy version of the recording"""
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith('flow/'))
    return {n: dict(flow=z['flow/' + n], rgb64=z['rgb64/' + n], rgb32=z['rgb32/' + n], flo=z['flo/' + n].tobytes()) for n in names}, str(z['numpy_version'])
