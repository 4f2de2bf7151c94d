"""Plain numpy restatement of the correlation kernels (vps_correlation / vps_correlation_f16: vps_amd/csrc/flow_ops.hip, corr_half.hip,
corr_mfma.hip; the reference's correlation_cuda_kernel.cu with kernel_size 1, stride1 1, pad_size == max_displacement), NHWC:

    out[n, y, x, (tj + r) D + (ti + r)] = act( 1/C  sum_c in1[n, y, x, c]  in2[n, y + tj s2, x + ti s2, c] ),   r = max_disp // s2, D = 2 r + 1

with zero for a sample outside the image. dtype-generic: float32 (products and sums in float32, numpy's pairwise order) gives the
distance that the bound of tests/test_corr_gpu.py is derived from, float64 is the yardstick. Pinned to oracle.ops.correlation by
tests/test_corr_restate.py."""
import numpy as np

F32 = np.float32


def correlation(in1, in2, max_disp, stride2, dtype, act=None, slope=0.1):
    """in1, in2 [N, H, W, C] -> (out [N, H, W, D D] of dtype, outside [N, H, W, D D] bool: the in2 sample lies outside the image).
    act: None or 'leaky' (v > 0 ? v : v slope, slope the float32 the kernel is handed)"""
    a, b = np.asarray(in1, dtype=dtype), np.asarray(in2, dtype=dtype)
    N, H, W, C = a.shape
    r = max_disp // stride2
    D = 2 * r + 1
    out = np.zeros((N, H, W, D * D), dtype=dtype)
    outside = np.ones((N, H, W, D * D), dtype=bool)
    inv = dtype(1) / dtype(C)
    for tj in range(-r, r + 1):
        dy = tj * stride2
        y0, y1 = max(0, -dy), min(H, H - dy)
        for ti in range(-r, r + 1):
            dx = ti * stride2
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            k = (tj + r) * D + (ti + r)
            out[:, y0:y1, x0:x1, k] = (a[:, y0:y1, x0:x1] * b[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]).sum(axis=-1, dtype=dtype) * inv
            outside[:, y0:y1, x0:x1, k] = False
    if act == 'leaky':
        out = np.where(out > 0, out, out * dtype(F32(slope)))
    else:
        assert act is None
    return out, outside
