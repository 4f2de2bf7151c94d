"""KITTI flow files: optical flow as a 16-bit RGB PNG, read and written with the un-filter, the filter, the deflate and the flow coding on
the device. The format is restated from memory of the KITTI devkit's `io_flow.h`; tests/kitti_flow_restate.py and its
known answers pin it.

    file    non-interlaced PNG, colour type 2, bit depth 16; samples big-endian in the order R, G, B
    read    valid iff B > 0; u = (R - 32768) / 64, v = (G - 32768) / 64; an invalid pixel reads as (0, 0)
    write   R = (uint16) max(min(u * 64.0f + 32768.0f, 65535.0f), 0.0f) in fp32, the cast truncating; G likewise from v; B = 1 where valid
    own     a pixel whose u or v is NaN or +-inf is written invalid, R = G = B = 0 (not in the kit)

Ground truth comes as two files per pair: `flow_occ` holds every labelled pixel, `flow_noc` only the non-occluded ones. `read_kitti_flow`
takes both and returns the mask byte of `vps_flow_error`: 1 valid and not occluded, 2 valid and occluded, 0 invalid.

Input: `vps_png16_inflate` on the host (no interpreter lock), then `vps_kitti_flow_reconstruct`: the skewed-wavefront un-filter of the 8-bit
input path at 6 bytes per pixel with the decode fused. Output: `vps_kitti_flow_encode`, then `vps_png_deflate_bpp` (the filter / deflate
chain of the panoptic PNG writer with Sub reaching back 6 bytes); signature, IHDR, IEND and the CRCs on the host. No CPU path."""
import ctypes
import os
import struct
import zlib

import numpy as np
import torch

from . import flowvis, hip

PNG_SIG = b'\x89PNG\r\n\x1a\n'


def _cbuf(data):
    if isinstance(data, (bytearray, memoryview)):
        return (ctypes.c_char * len(data)).from_buffer(data)
    return (ctypes.c_char * len(data)).from_buffer_copy(data)


def png16_info(data):
    """header of a non-interlaced 16-bit RGB PNG -> (H, W); None for any other file (`vps_png16_info`)"""
    H, W, C = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    if hip.load_host().vps_png16_info(_cbuf(data), len(data), ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)) != 0:
        return None
    return H.value, W.value


def png16_inflate(data, out=None):
    """bytes of a 16-bit RGB PNG -> (uint8 [H * (1 + 6 W)] filtered scanlines as zlib delivers them, H, W) through `vps_png16_inflate`
    (host, no interpreter lock). `out`: a host uint8 tensor or array to inflate into (a pinned staging slot). Any other file raises."""
    hw = png16_info(data)
    if hw is None:
        raise ValueError('not a non-interlaced 16-bit RGB PNG (the KITTI flow flavour)')
    H, W = hw
    n = H * (1 + 6 * W)
    if out is None:
        out = np.empty(n, dtype=np.uint8)
    arr = out.numpy() if torch.is_tensor(out) else out
    assert arr.dtype == np.uint8 and arr.ndim == 1 and arr.size >= n and arr.flags['C_CONTIGUOUS'], 'a flat uint8 buffer of %d bytes' % n
    hip.check(hip.load_host().vps_png16_inflate(_cbuf(data), len(data), arr.ctypes.data_as(ctypes.c_void_p), arr.size), 'vps_png16_inflate')
    return out[:n], H, W


def kitti_flow_reconstruct(scan, H, W, noc_valid=None, ws=None):
    """device uint8 buffer with the filtered scanlines of a KITTI flow file (at any byte offset of its storage) -> (flow device fp32
    [H,W,2], mask device uint8 [H,W]) on the current stream, no sync (`vps_kitti_flow_reconstruct`). noc_valid: device uint8 [H,W],
    non-zero = valid in the pair's flow_noc file; the mask then has the codes 1 / 2 / 0, without it 1 / 0."""
    lib = hip.load()
    need = ctypes.c_int64()
    hip.check(lib.vps_kitti_flow_reconstruct_ws(H, W, ctypes.byref(need)), 'vps_kitti_flow_reconstruct_ws')
    assert scan.is_cuda and scan.dtype == torch.uint8 and scan.is_contiguous() and scan.numel() >= H * (1 + 6 * W), \
        'filtered scanlines of H * (1 + 6 W) bytes expected'
    if noc_valid is not None:
        assert noc_valid.is_cuda and noc_valid.dtype == torch.uint8 and noc_valid.is_contiguous() and tuple(noc_valid.shape) == (H, W)
    if ws is None or ws.numel() < need.value:
        ws = torch.empty(need.value, dtype=torch.uint8, device=scan.device)
    flow = torch.empty(H, W, 2, dtype=torch.float32, device=scan.device)
    mask = torch.empty(H, W, dtype=torch.uint8, device=scan.device)
    hip.check(lib.vps_kitti_flow_reconstruct(hip.ptr(scan), H, W, hip.ptr(noc_valid), hip.ptr(flow), flow.numel() * 4, hip.ptr(mask), hip.ptr(ws),
                                             ws.numel(), hip.stream_ptr()), 'vps_kitti_flow_reconstruct')
    return flow, mask


def _device_valid(valid, H, W, device):
    if valid is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(valid)) if isinstance(valid, np.ndarray) else valid
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if not (t.dtype == torch.uint8 and tuple(t.shape) == (H, W)):
        raise ValueError('valid is uint8 or bool [%d,%d] like the flow, got %s %s' % (H, W, t.dtype, tuple(t.shape)))
    return t.to(device).contiguous()


def kitti_flow_encode(flow, valid=None, out=None):
    """a device flow (what `flowvis.flow_colour` takes: FMap, [H,W,2] or [1,2,H,W]) -> device uint8 [H, 6 W]: the big-endian RGB16 image
    of the write rule, on the current stream, no sync (`vps_kitti_flow_encode`). valid: None (all valid) or uint8 / bool [H,W]."""
    t, ld, coff, H, W = flowvis._flow_view(flow)
    valid = _device_valid(valid, H, W, t.device)
    if out is None:
        out = torch.empty(H, 6 * W, dtype=torch.uint8, device=t.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (H, 6 * W)
    hip.check(hip.load().vps_kitti_flow_encode(hip.ptr(t), ld, coff, hip.ptr(valid), H, W, hip.ptr(out), hip.stream_ptr()), 'vps_kitti_flow_encode')
    return out


def png_encode_bound_bpp(H, rowbytes, bpp):
    """(worst-case stream bytes, workspace bytes) of `vps_png_deflate_bpp`"""
    cap, wsb = ctypes.c_int64(0), ctypes.c_int64(0)
    hip.check(hip.load().vps_png_encode_bound_bpp(H, rowbytes, bpp, ctypes.byref(cap), ctypes.byref(wsb)), 'vps_png_encode_bound_bpp')
    return cap.value, wsb.value


def png_deflate_bpp(img, bpp, out=None, ws=None, size=None, huffman='fixed'):
    """filter + deflate a dense device uint8 [H, rowbytes] image whose pixels are bpp bytes (`vps_png_deflate_bpp_h`) on the current
    stream, no sync -> (device uint8 buffer, device int64 [1] size); size -1 = `out` was too small. huffman: 'fixed' (the bytes of
    `vps_png_deflate_bpp`) or 'dynamic' (a segment in a Huffman code of its own where that is shorter), as `postprocess.png_deflate`"""
    from .postprocess import png_huffman
    huffman = png_huffman(huffman)
    assert img.is_cuda and img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous()
    H, rowbytes = int(img.shape[0]), int(img.shape[1])
    if out is None or ws is None:
        cap, wsb = png_encode_bound_bpp(H, rowbytes, bpp)
        out = torch.empty(cap, dtype=torch.uint8, device=img.device) if out is None else out
        ws = torch.empty(wsb, dtype=torch.uint8, device=img.device) if ws is None else ws
    if size is None:
        size = torch.empty(1, dtype=torch.int64, device=img.device)
    hip.check(hip.load().vps_png_deflate_bpp_h(hip.ptr(img), H, rowbytes, bpp, rowbytes, hip.ptr(out), out.numel(), hip.ptr(size),
                                               hip.ptr(ws), ws.numel(), hip.stream_ptr(), huffman), 'vps_png_deflate_bpp_h')
    return out, size


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)


def png16_container(stream_bytes, H, W):
    """the file around one zlib stream: signature, IHDR (16 bit, colour type 2, no interlace), one IDAT, IEND; CRCs on the host"""
    return PNG_SIG + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 16, 2, 0, 0, 0)) + _chunk(b'IDAT', bytes(stream_bytes)) + _chunk(b'IEND', b'')


def read_kitti_flow(path_occ, path_noc=None, device='cuda'):
    """a KITTI flow file -> (flow device fp32 [H,W,2], mask device uint8 [H,W]). With the pair's flow_noc file the mask separates the
    occluded pixels (2) from the others (1); the noc file is decoded first and its mask feeds the decode of the occ file."""
    device = torch.device(device)

    def upload(path):
        with open(path, 'rb') as f:
            data = f.read()
        try:
            scan, H, W = png16_inflate(bytearray(data))
        except ValueError as e:
            raise ValueError('%s: %s' % (path, e))
        return torch.from_numpy(scan).to(device), H, W
    noc_valid = None
    if path_noc is not None:
        scan, Hn, Wn = upload(path_noc)
        _, noc_valid = kitti_flow_reconstruct(scan, Hn, Wn)
    scan, H, W = upload(path_occ)
    if noc_valid is not None and (Hn, Wn) != (H, W):
        raise ValueError('%s is %d x %d, %s is %d x %d' % (path_noc, Hn, Wn, path_occ, H, W))
    return kitti_flow_reconstruct(scan, H, W, noc_valid)


def kitti_flow_bytes(flow, valid=None, huffman='fixed'):
    """the complete file of a device flow (synchronises: one download of the stream and its size)"""
    t, _, _, H, W = flowvis._flow_view(flow)
    out, size = png_deflate_bpp(kitti_flow_encode(flow, valid), 6, huffman=huffman)
    n = int(size.item())
    if n < 0:
        raise hip.VpsHipError('vps_png_deflate_bpp: the stream did not fit its worst-case bound')
    return png16_container(out[:n].cpu().numpy().tobytes(), H, W)


def write_kitti_flow(flow, name, valid=None, huffman='fixed'):
    os.makedirs(os.path.dirname(name) or '.', exist_ok=True)
    with open(name, 'wb') as f:
        f.write(kitti_flow_bytes(flow, valid, huffman))
    return name
