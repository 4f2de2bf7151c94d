"""Golden fixtures under tests/golden/ whose archive would exceed the 1 MiB limit of a committed file are stored in parts:
NAME.npz is kept as NAME.part0.npz, NAME.part1.npz, ... (compressed, disjoint key sets, each under PART_BYTES). `load(path)` opens
either form and returns one read-only mapping with the interface of np.lib.npyio.NpzFile (`files`, `[key]`, `in`, `keys()`, ...);
`save(path, arrays)` writes the single file when it fits, the parts otherwise (the generators under tests/golden/ use it)."""
import glob
import io
import os
import re
import zipfile

import numpy as np

PART_BYTES = 960 * 1024


def _parts(path):
    stem = path[:-len('.npz')] if path.endswith('.npz') else path
    found = glob.glob(glob.escape(stem) + '.part*.npz')
    idx = lambda p: int(re.search(r'\.part(\d+)\.npz$', p).group(1))
    return sorted((p for p in found if re.search(r'\.part\d+\.npz$', p)), key=idx)


class _Parts:
    def __init__(self, parts):
        self._parts = parts
        self._where = {}
        for p in parts:
            for k in p.files:
                assert k not in self._where, 'key %s in two parts' % k
                self._where[k] = p
        self.files = list(self._where)

    def __getitem__(self, k):
        if k not in self._where and k.endswith('.npy'):
            k = k[:-len('.npy')]
        return self._where[k][k]

    def __contains__(self, k):
        return k in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return list(self.files)

    def values(self):
        return [self[k] for k in self.files]

    def items(self):
        return [(k, self[k]) for k in self.files]

    def get(self, k, default=None):
        return self[k] if k in self._where else default

    def close(self):
        for p in self._parts:
            p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load(path, **kw):
    if os.path.exists(path):
        return np.load(path, **kw)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    return _Parts([np.load(p, **kw) for p in parts])


def _member_bytes(name, a):
    """compressed size of one array as a member of an .npz archive"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        with z.open(name + '.npy', 'w') as f:
            np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)
    return buf.tell()


def save(path, arrays):
    """np.savez_compressed(path, **arrays), split into parts (key order kept) when one archive would exceed PART_BYTES"""
    for p in _parts(path):
        os.remove(p)
    if os.path.exists(path):
        os.remove(path)
    sizes = {k: _member_bytes(k, v) for k, v in arrays.items()}
    if sum(sizes.values()) <= PART_BYTES:
        np.savez_compressed(path, **arrays)
        return [path]
    groups, cur, n = [], {}, 0
    for k, v in arrays.items():
        assert sizes[k] <= PART_BYTES, '%s alone takes %d bytes compressed' % (k, sizes[k])
        if cur and n + sizes[k] > PART_BYTES:
            groups.append(cur)
            cur, n = {}, 0
        cur[k] = v
        n += sizes[k]
    groups.append(cur)
    stem = path[:-len('.npz')]
    out = []
    for i, g in enumerate(groups):
        out.append('%s.part%d.npz' % (stem, i))
        np.savez_compressed(out[-1], **g)
    return out
