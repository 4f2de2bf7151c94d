"""What the per-pair evaluators share on the host (`FlowEvaluator` of floweval.py, `PhotoEvaluator` and `CensusEvaluator` of
flowphoto.py): the device tables that pairs are counted into between two downloads, and the checks of their inputs. The messages
are the callers': every check takes the words that caller has always raised."""
import json
import os

import numpy as np
import torch

from . import hip

BLOCK = 16


class PairTables:
    """Device tables for pairs that come one by one: one row per pair in blocks of `BLOCK` rows (per_pair), or one row that every pair
    adds to. specs: [(cells shape, torch dtype)], one per table. Nothing is synchronised before `download`."""

    def __init__(self, device, per_pair, specs):
        self.device, self.per_pair, self.specs = device, bool(per_pair), specs
        self.n, self._blocks = 0, []

    def row(self):
        """the tensors (one per table) the next pair adds to"""
        i = self.n if self.per_pair else 0
        if i >= BLOCK * len(self._blocks):               # pairs come one by one: rows in blocks, still one download
            rows = BLOCK if self.per_pair else 1
            self._blocks.append([torch.zeros((rows,) + shape, dtype=dtype, device=self.device) for shape, dtype in self.specs])
        return [t[i % BLOCK] for t in self._blocks[i // BLOCK]]

    def download(self):
        """the one download (and synchronisation) -> (n, host arrays: [n, cells] each with per_pair, else [cells]); empty afterwards"""
        n, blocks = self.n, self._blocks
        self.n, self._blocks = 0, []
        host = [(torch.cat(ts) if len(ts) > 1 else ts[0]).cpu().numpy() for ts in zip(*blocks)]
        return n, [a[:n] if self.per_pair else a[0] for a in host]

    def zeros(self):
        """host tables of no pair at all"""
        return [torch.zeros(shape, dtype=dtype).numpy() for shape, dtype in self.specs]


def device_or_raise(device, message):
    device = torch.device(device)
    if device.type != 'cuda' or not torch.cuda.is_available():
        raise hip.VpsHipError(message)
    return device


def _host_or_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a


def _got(t):
    return getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))


def frame(f, H, W, device, what):
    """a uint8 [H,W,3] frame, host or device -> contiguous on the device"""
    t = _host_or_tensor(f)
    if not (torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (H, W, 3)):
        raise ValueError('%s is a uint8 [%d,%d,3] frame of the flow\'s H, W, got %s %s' % ((what, H, W) + _got(t)))
    return t.to(device).contiguous()


def byte_map(m, H, W, device, what, like):
    """None, or a uint8 [H,W] map `like` the flow(s): a host map is uploaded, a contiguous map on `device` is used where it lies (it
    may be the map the same call writes)"""
    if m is None:
        return None
    t = _host_or_tensor(m)
    if not (torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (H, W)):
        raise ValueError('%s is uint8 [%d,%d] like the %s, got %s %s' % ((what, H, W, like) + _got(t)))
    return t.to(device).contiguous()


def out_map(t, shape, message):
    """None, or a caller-owned contiguous device uint8 tensor of `shape` that a kernel writes"""
    if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(message)
    return t


def write_result(result, out_dir, stem, text):
    """<stem>.txt (`text`) and <stem>.json (`result`) in `out_dir`"""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, stem + '.txt'), 'w') as f:
        f.write(text)
    with open(os.path.join(out_dir, stem + '.json'), 'w') as f:
        json.dump(result, f, indent=1)
