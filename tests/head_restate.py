"""Plain-numpy restatements of the contracts of the detection-head kernels (vps_amd/csrc/head_ops.hip), written from the reference's
host code and the oracle, NOT from the kernels: what tests/test_head_ops_gpu.py compares the kernels with, and what
tests/test_head_restate.py pins to oracle/fusetrack.py on the CPU. No GPU, no vps_amd.hip. Reference paths relative to mmdet/.

Every function returns what the kernel must WRITE; what it must leave alone (rows past the count, spare header words) is the
caller's sentinel."""
import numpy as np
import torch

from oracle import fusetrack as OF

SORT_CAP = 8192          # candidates the select / collect kernels can sort (64 KB of 64-bit keys)


def rpn_collect(boxes, keep, nkeep, nms_post, max_num):
    """rpn_head.py:94-104: `proposals[:nms_post]` of every level concatenated, then the max_num best by score. boxes [nlv][nmax][5]
    (each level in descending score order), keep [nlv][nmax] kept positions (ascending = descending score), nkeep [nlv].
    Equal scores: the earlier position of the concatenation first (a stable descending sort; torch.topk leaves it open).
    -> (out [max_num][5] with rows >= n zero, n)"""
    boxes = np.asarray(boxes, dtype=np.float32)
    cat = [boxes[l][np.asarray(keep[l][:min(int(nkeep[l]), nms_post)], dtype=np.int64)] for l in range(boxes.shape[0])]
    cat = np.concatenate(cat, 0) if cat else np.zeros((0, 5), np.float32)
    order = np.argsort(-cat[:, 4].astype(np.float64), kind='stable')
    n = min(max_num, cat.shape[0])
    out = np.zeros((max_num, 5), dtype=np.float32)
    out[:n] = cat[order[:n]]
    return out, n


def maskroi_select(rois, delta, prob, n_valid, nc, thr, weights, im_hw, dtype=np.float32):
    """utils/mask_roi.py:43-95 (class_agnostic, clip_boxes): bbox_transform (bbox_transform.py:290-330) + clip_boxes (:45-60) of the
    first nv = min(n_valid, n) rois, candidate q = roi * (nc - 1) + (cls - 1) for the foreground classes, those with prob > thr
    (strict, in the probabilities' own precision), in the order gpu_nms.pyx:23-38 walks them: `scores.argsort()[::-1]`, i.e.
    descending score and among equal scores the LARGER q first (a stable ascending sort reversed).
    -> (dets [m][5], cand [m] int32, [m, overflow, nv]); m is capped at SORT_CAP (which candidates fill the slots is then open)."""
    n = rois.shape[0]
    nv = n if n_valid is None else min(int(n_valid), n)
    rois = np.asarray(rois, dtype=dtype)[:nv]
    delta = np.ascontiguousarray(np.asarray(delta, dtype=dtype)[:nv])
    boxes = OF._clip_boxes_np(OF._bbox_transform_np(rois[:, 1:5], delta, weights), im_hw).reshape(nv, nc, 4)
    p = np.asarray(prob, dtype=np.float32)[:nv, 1:].reshape(-1)
    q = np.nonzero(p > np.float32(thr))[0]
    q = q[np.lexsort((-q, -p[q].astype(np.float64)))]
    overflow = int(q.shape[0] > SORT_CAP)
    q = q[:SORT_CAP]
    r, c = q // (nc - 1), q % (nc - 1) + 1
    dets = np.concatenate([boxes[r, c].astype(dtype), p[q].astype(dtype)[:, None]], 1).reshape(-1, 5)
    return dets, q.astype(np.int32), [int(q.shape[0]), overflow, nv]


def maskroi_finish(dets, cand, m_in, keep, nkeep, nc, max_det, kcap):
    """utils/mask_roi.py:96-147: the post-NMS list dets[keep[:nkeep]] (descending score), cut to the max_det best BY VALUE
    (`image_thresh = np.sort(scores)[-max_det]`, `scores >= image_thresh`: ties with the max_det-th stay), or the dummy row
    (score 1, box 0, class 0; :136-142). m_in = [candidates, overflow, valid rois] as maskroi_select left it.
    -> (header [K, candidates, post-NMS count, status, valid rois], rows [K][8] = 0, x1, y1, x2, y2, score, class, q);
    status bit 0: more than SORT_CAP candidates, bit 1: more than kcap rows (cut to kcap)."""
    nk = int(nkeep)
    sel = np.asarray(keep[:nk], dtype=np.int64)
    scores = np.asarray(dets, dtype=np.float32)[sel, 4]
    if max_det > 0 and nk > max_det:
        image_thresh = np.sort(scores)[-max_det]
        sel = sel[np.where(scores >= image_thresh)[0]]
    status = 1 if m_in[1] else 0
    if sel.shape[0] > kcap:
        status |= 2
        sel = sel[:kcap]
    if nk == 0:
        rows = np.array([[0, 0, 0, 0, 0, 1, 0, 0]], dtype=np.float32)
    else:
        q = np.asarray(cand, dtype=np.int64)[sel]
        rows = np.zeros((sel.shape[0], 8), dtype=np.float32)
        rows[:, 1:6] = np.asarray(dets, dtype=np.float32)[sel]
        rows[:, 6] = q % (nc - 1) + 1
        rows[:, 7] = q
    return np.array([rows.shape[0], m_in[0], nk, status, m_in[2]], dtype=np.float32), rows


def track_assign(comp, M, emb, box, label, prev_emb, prev_box, prev_label):
    """detectors/panoptic_fusetrack.py:424-469: oracle.fusetrack.greedy_assign (row arg-max = FIRST maximum, greedy assignment with
    undo, new ids) and its update list applied, in order, to copies of the memory arrays (:441-443 / :467-469 append embedding, box
    and label; :458-459 overwrite embedding and box of a matched entry, whose label stays). prev_* have room for M + K rows.
    -> (ids int32 [K], new M, prev_emb, prev_box, prev_label)"""
    ids, updates = OF.greedy_assign(torch.from_numpy(np.ascontiguousarray(comp, dtype=np.float32)), M)
    pe, pb, pl = prev_emb.copy(), prev_box.copy(), prev_label.copy()
    mem = M
    for u in updates:
        if u[0] == 'add':
            pe[mem] = emb[u[1]]; pb[mem] = box[u[1], :4]; pl[mem] = label[u[1]]
            mem += 1
        else:
            pe[u[1]] = emb[u[2]]; pb[u[1]] = box[u[2], :4]
    return np.asarray(ids, dtype=np.int32), mem, pe, pb, pl


def seg_crop(row):
    """utils/unary_logits.py:96-106 as oracle.fusetrack.seg_term evaluates it on boxes * 4 * 0.25 (== the boxes, exactly, in fp32):
    [int(x1), int(round(x2) + 1)) x [int(y1), int(round(y2) + 1)), numpy's round (half to even) -> (sx0, sy0, sx1, sy1)"""
    b = np.asarray(row, dtype=np.float32)[1:5] * np.float32(4.0) * np.float32(1 / 4.0)
    return int(b[0]), int(b[1]), int(b[2].round() + 1), int(b[3].round() + 1)


def pan_instances(order, flags, rows, tbox, class_mapping):
    """utils/mask_removal.py:81-91 (kept list in walk order; nothing kept -> keep = [0], all-zero mask logits = an empty paste box)
    + the SegTerm crop of every kept detection. order [n]: detection at walk position p, flags [n]: kept at p, rows [n][8] as
    maskroi_finish writes them, tbox [n][4]: int32 boxes in walk order, class_mapping {class: semantic channel}; order / flags /
    tbox None = the dummy-row call. -> (inst [k][10] int32 = sx0, sy0, sx1, sy1, seg_ch, bx1, by1, bx2, by2, mask_idx; keep [k];
    [k, masks_valid])"""
    def seg(row):
        c = int(row[6])
        return [0, 0, 0, 0, 0] if c == 0 else list(seg_crop(row)) + [int(class_mapping[c])]
    inst, keep = [], []
    for p in range(rows.shape[0] if flags is not None else 0):
        if flags[p]:
            i = int(order[p])
            inst.append(seg(rows[i]) + [int(v) for v in tbox[p]] + [i])
            keep.append(i)
    valid = 1
    if not keep:
        inst, keep, valid = [seg(rows[0]) + [0, 0, -1, -1, 0]], [0], 0
    return np.array(inst, dtype=np.int32), np.array(keep, dtype=np.int32), [len(keep), valid]


def frame_tail(tail, kinfo, keep, ids, mem_count, f16_status, nslots, K, kcap):
    """the end-of-frame record: `tail` (the buffer as it was) with words 0..3 = kinfo, 4 = mem_count (0 when None), 5 = the largest
    of the first nslots status words (0 when nslots = 0), 8 .. 8+K = keep[:K], 8+kcap .. 8+kcap+K = ids[:K] (left alone when ids is
    None); every other word as it was"""
    t = np.array(tail, dtype=np.int32, copy=True)
    t[0:4] = kinfo[0:4]
    t[4] = 0 if mem_count is None else int(mem_count)
    t[5] = max([0] + [int(v) for v in f16_status[:nslots]]) if nslots > 0 else 0
    t[8:8 + K] = keep[:K]
    if ids is not None:
        t[8 + kcap:8 + kcap + K] = ids[:K]
    return t
