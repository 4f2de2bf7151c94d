"""The two device steps of the PQ / VPQ / boundary evaluators restated in NumPy, and the fixture that puts them in place of the device
ones: `evaluate.pair_table` (the only caller of `vps_pair_count`) and `boundary.boundary_band`. With them the host logic of
vps_amd/evaluate.py, ipq.py and boundary.py runs without a GPU (`device='cpu'`)."""
import numpy as np
import pytest
import torch

import boundary_restate as R


def numpy_pair_table(g, p, gt_ids, pred_ids, dev):
    """the definition of `evaluate.pair_table`: int64 [ngt+1][npred+1], row / column n collects the ids that are not listed"""
    gi, pi = R.ids_of(g.cpu().numpy()), R.ids_of(p.cpu().numpy())
    r = np.searchsorted(gt_ids, gi); r[(r >= len(gt_ids)) | (gt_ids[np.minimum(r, len(gt_ids) - 1)] != gi)] = len(gt_ids)
    c = np.searchsorted(pred_ids, pi); c[(c >= len(pred_ids)) | (pred_ids[np.minimum(c, len(pred_ids) - 1)] != pi)] = len(pred_ids)
    tab = np.zeros((len(gt_ids) + 1, len(pred_ids) + 1), dtype=np.int64)
    np.add.at(tab, (r, c), 1)
    return tab


@pytest.fixture
def numpy_device(monkeypatch):
    """the two device steps (band, pair count) replaced by their NumPy definitions: the host logic around them runs without a GPU"""
    from vps_amd import boundary, evaluate
    monkeypatch.setattr(evaluate, 'pair_table', numpy_pair_table)
    monkeypatch.setattr(boundary, 'boundary_band', lambda pan, d=None, ratio=0.02, device='cpu': torch.from_numpy(R.band_map(pan.cpu().numpy(), d)))
