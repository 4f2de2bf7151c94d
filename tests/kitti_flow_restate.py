"""The KITTI flow coding, restated from memory of the KITTI devkit's io_flow.h in NumPy, sharing no code with vps_amd/kittiflow.py or the
kernels (the file format itself is tests/png16_cases.py). What pins the rules are the known answers below, written out by hand.

    read    valid iff B > 0 (the 16-bit value); u = (R - 32768) / 64, v = (G - 32768) / 64; an invalid pixel reads as u = v = 0
    write   R = (uint16) max(min(u * 64.0f + 32768.0f, 65535.0f), 0.0f), every operation in fp32, the cast truncating behind the clamp;
            G likewise from v; B = 1 where valid, 0 otherwise
    own     (this repository, not the kit) a pixel whose u or v is NaN or +-inf is written R = G = B = 0
    mask    vps_flow_error's codes from the two ground-truth files of a pair: 1 valid in flow_occ and in flow_noc, 2 valid in flow_occ
            only (occluded), 0 invalid in flow_occ; without a flow_noc file 1 / 0
"""
import numpy as np

import png16_cases as P

F = np.float32

# R (or G) -> u (or v), by hand: (R - 32768) / 64
KNOWN_READ = ((0, -512.0), (1, -511.984375), (32767, -0.015625), (32768, 0.0), (32769, 0.015625), (65535, 511.984375))
# B -> valid. 256 has a zero low byte and 1 a zero high byte: a test on one byte gets one of them wrong
KNOWN_VALID = ((0, False), (1, True), (256, True), (65535, True))
# u -> R: 1/128 * 64 = 0.5 -> 32768.5 truncates to 32768; -1/128 -> 32767.5 -> 32767; 512 -> 65536 clamps to 65535; -513 -> -64 clamps to 0
KNOWN_WRITE = ((1.0 / 128, 32768), (-1.0 / 128, 32767), (512.0, 65535), (-513.0, 0), (0.0, 32768), (-512.0, 0), (511.984375, 65535), (1.0, 32832))


def decode(rgb):
    """uint16 [H,W,3] -> (flow float32 [H,W,2], valid bool [H,W])"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint16 and rgb.ndim == 3 and rgb.shape[2] == 3
    valid = rgb[..., 2] > 0
    uv = (rgb[..., :2].astype(np.int64) - 32768).astype(np.float64) / 64.0            # multiples of 1/64 below 2^9: exact in fp32 too
    flow = np.where(valid[..., None], uv, 0.0).astype(F)
    assert np.array_equal(flow.astype(np.float64), np.where(valid[..., None], uv, 0.0))
    return flow, valid


def mask_codes(valid_occ, valid_noc=None):
    valid_occ = np.asarray(valid_occ, dtype=bool)
    if valid_noc is None:
        return valid_occ.astype(np.uint8)
    return np.where(valid_occ, np.where(np.asarray(valid_noc, dtype=bool), 1, 2), 0).astype(np.uint8)


def encode(flow, valid=None):
    """float32 [H,W,2] (+ bool / uint8 [H,W]) -> uint16 [H,W,3]"""
    flow = np.asarray(flow)
    assert flow.dtype == F and flow.ndim == 3 and flow.shape[2] == 2
    H, W = flow.shape[:2]
    valid = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    finite = np.isfinite(flow).all(axis=2)
    with np.errstate(all='ignore'):
        q = flow * F(64.0)
        assert q.dtype == F
        q = q + F(32768.0)
        q = np.maximum(np.minimum(q, F(65535.0)), F(0.0))
        assert q.dtype == F
    q = np.where(finite[..., None], q, F(0.0))
    rgb = np.zeros((H, W, 3), np.uint16)
    rgb[..., :2] = np.trunc(q).astype(np.uint16)
    rgb[..., 2] = (valid & finite).astype(np.uint16)
    rgb[~finite] = 0
    return rgb


def quantised(flow, valid=None):
    """what a reader makes of the file a writer makes of (flow, valid): (flow, valid)"""
    return decode(encode(flow, valid))


def read_file(data):
    """file bytes -> (flow, valid)"""
    return decode(P.rgb16(P.read_raw(data)))


def write_file(flow, valid=None, types=None, idat_parts=1):
    """-> file bytes; `types`: filter type per row (default: all Paeth)"""
    raw = P.raw_of(encode(flow, valid))
    return P.encode(raw, [4] * raw.shape[0] if types is None else types, idat_parts)[0]


def self_check():
    for R, u in KNOWN_READ:
        f, v = decode(np.array([[[R, R, 1]]], np.uint16))
        assert v[0, 0] and f[0, 0, 0] == F(u) and f[0, 0, 1] == F(u), (R, u, f)
    for B, ok in KNOWN_VALID:
        f, v = decode(np.array([[[40000, 30000, B]]], np.uint16))
        assert bool(v[0, 0]) == ok and (f[0, 0, 0] != 0) == ok, (B, ok)
    for u, R in KNOWN_WRITE:
        rgb = encode(np.array([[[u, -u]]], F))
        assert rgb[0, 0, 0] == R and rgb[0, 0, 2] == 1, (u, R, rgb)
    for bad in (np.nan, np.inf, -np.inf):
        assert encode(np.array([[[bad, 1.0]]], F)).tolist() == [[[0, 0, 0]]] and encode(np.array([[[1.0, bad]]], F)).tolist() == [[[0, 0, 0]]]
    assert encode(np.array([[[1.0, 2.0]]], F), np.array([[0]], np.uint8)).tolist() == [[[32832, 32896, 0]]]


self_check()
