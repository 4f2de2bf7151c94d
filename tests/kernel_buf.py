"""What the kernel-level GPU tests share (tests/test_nn_ops_gpu.py, tests/test_corr_gpu.py): the sentinel-framed device buffer and the check
that a kernel wrote nothing outside its output windows."""
import ctypes

import numpy as np
import torch

F32 = np.float32
SENT = np.int32(0x7fc05a5a)                 # a quiet NaN with a payload: equal to nothing, told from any NaN a kernel could compute


class Buf:
    """a float32 device buffer of `rows` rows of `ld` elements with one guard row before and one after; .p(off) = pointer to element off
    of row 0"""

    def __init__(self, dev, host, rows, ld):
        self.rows, self.ld = rows, ld
        self.host = np.full((rows + 2, ld), SENT, dtype=np.int32)
        if host is not None:
            self.host[1:-1] = np.ascontiguousarray(host, dtype=F32).view(np.int32).reshape(rows, ld)
        self.t = torch.from_numpy(self.host.copy()).to(dev)

    def p(self, off=0):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (self.ld + off))

    def bits(self):
        return self.t.cpu().numpy()

    def unchanged(self):
        return np.array_equal(self.bits(), self.host)


def written_outside(bits, windows):
    """bits: Buf.bits() of an output buffer, windows: [(coff, C)] - the number of elements outside every window [coff, coff + C) of rows
    1 .. rows (guard rows included) that no longer hold the sentinel"""
    frame = bits.copy()
    for coff, C in windows:
        frame[1:-1, coff:coff + C] = SENT
    return int((frame != SENT).sum())
