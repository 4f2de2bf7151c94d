"""Inputs of the STQ tests (tests/test_stq.py, tests/test_stq_gpu.py): the five hand-derived cases of the definition, seeded random
videos, the 64x96 frame that exercises every per-pixel rule, and the two-video set with an id switch, a merged pair and a crowd region.
A frame is `(gt_json_ann, pred_json_ann, gt_pan, pred_pan)` as `StqEvaluator.add_video` takes it."""
import numpy as np

ROAD, CAR = 7, 26
CATS2 = {ROAD: {'id': ROAD, 'name': 'road', 'isthing': 0}, CAR: {'id': CAR, 'name': 'car', 'isthing': 1}}
# five classes with gaps between the ids: class index != category id
CATS5 = {3: {'id': 3, 'name': 'road', 'isthing': 0}, 8: {'id': 8, 'name': 'sky', 'isthing': 0}, 11: {'id': 11, 'name': 'person', 'isthing': 1},
         12: {'id': 12, 'name': 'car', 'isthing': 1}, 20: {'id': 20, 'name': 'bus', 'isthing': 1}}
MAX_ID = (1 << 24) - 1


def pan_of(ids):
    """uint8 [H,W,3] map of an integer id map: R + 256 G + 65536 B"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def seg(sid, cat, iscrowd=0):
    return {'id': int(sid), 'category_id': cat, 'iscrowd': iscrowd, 'area': 0}


def frame(gt_ids, pred_ids, gt_segs, pred_segs):
    return ({'segments_info': list(gt_segs)}, {'segments_info': [{k: v for k, v in s.items() if k != 'iscrowd'} for s in pred_segs]},
            pan_of(gt_ids), pan_of(pred_ids))


def hand_cases():
    """{name: (frames of one video, expected {'aq', 'sq', 'stq'} - None where the issue derives no value)}: one 1x4 frame each"""
    row = lambda *v: np.array([v])
    return {
        'equal': ([frame(row(1, 1, 5, 5), row(1, 1, 5, 5), [seg(1, ROAD), seg(5, CAR)], [seg(1, ROAD), seg(5, CAR)])], dict(aq=1.0, sq=1.0, stq=1.0)),
        'split': ([frame(row(5, 5, 5, 5), row(8, 8, 9, 9), [seg(5, CAR)], [seg(8, CAR), seg(9, CAR)])], dict(aq=0.5, sq=1.0, stq=0.7071067811865476)),
        'merged': ([frame(row(5, 5, 6, 6), row(8, 8, 8, 8), [seg(5, CAR), seg(6, CAR)], [seg(8, CAR)])], dict(aq=0.5, sq=None, stq=None)),
        'crowd': ([frame(row(5, 5, 6, 6), row(8, 8, 8, 8), [seg(5, CAR, 1), seg(6, CAR)], [seg(8, CAR)])], dict(aq=1.0, sq=None, stq=None)),
        'stuff': ([frame(row(1, 1, 1, 1), row(1, 1, 1, 8), [seg(1, ROAD)], [seg(1, ROAD), seg(8, CAR)])], dict(aq=0.0, sq=0.375, stq=0.0)),
    }


def _paint(rng, H, W, ids, n_rect):
    m = np.zeros((H, W), dtype=np.int64)
    for _ in range(n_rect):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, max(2, H // 2))), int(rng.integers(1, max(2, W // 2)))
        m[y0:y0 + h, x0:x0 + w] = ids[int(rng.integers(0, len(ids)))]
    return m


def random_video(seed, nframes=3, H=6, W=8, cats=CATS5):
    """a small video of overlapping rectangles: 6 gt and 6 predicted segments of random categories (one gt segment crowd if a thing), VOID"""
    rng = np.random.default_rng(seed)
    cat_ids = sorted(cats)
    gt_segs = [seg(i, cat_ids[int(rng.integers(0, len(cat_ids)))]) for i in rng.choice(np.arange(1, 400), 6, replace=False)]
    pred_segs = [seg(i, cat_ids[int(rng.integers(0, len(cat_ids)))]) for i in rng.choice(np.arange(1, 400), 6, replace=False)]
    gt_segs[0]['iscrowd'] = 1
    frames = []
    for _ in range(nframes):
        g = _paint(rng, H, W, [0] + [s['id'] for s in gt_segs], 8)
        p = _paint(rng, H, W, [0] + [s['id'] for s in pred_segs], 8)
        frames.append(frame(g, p, gt_segs, pred_segs))
    return frames


RICH_GT = [seg(1, 3), seg(MAX_ID, 12), seg(300, 11), seg(70000, 11, 1), seg(5, 8), seg(77, 20), seg(1000, 12, 1), seg(65536, 12)]
RICH_PRED = [seg(1, 12), seg(MAX_ID, 3), seg(9, 11), seg(400, 8), seg(65537, 12), seg(12, 20), seg(13, 11), seg(500, 3)]
RICH_GT_UNLISTED, RICH_PRED_UNLISTED = 4242, 99999


def rich_frame(seed=0, H=64, W=96, unlisted_pred=False, extra_gt=0, extra_pred=0):
    """64x96 maps of overlapping rectangles: 8 gt and 8 predicted segments of stuff / thing / crowd with ids 1 and 2^24-1, VOID on either
    side, a painted gt id that is not listed, thing on stuff and stuff on thing; `unlisted_pred` also paints a predicted id that is not
    listed. `extra_gt` / `extra_pred` listed but unpainted segments widen the tables (ids from 2000 / 3000 up)."""
    rng = np.random.default_rng(seed)
    g = _paint(rng, H, W, [0] + [s['id'] for s in RICH_GT] + [RICH_GT_UNLISTED], 40)
    p = _paint(rng, H, W, [0] + [s['id'] for s in RICH_PRED] + ([RICH_PRED_UNLISTED] if unlisted_pred else []), 40)
    g[0, :7] = 0; p[0, 3:9] = 0                                                   # VOID on either side whatever the seed paints
    g[1, :4] = RICH_GT_UNLISTED
    g[2, :6] = 1; p[2, :3] = 1; p[2, 3:6] = MAX_ID                                # stuff under thing and under stuff
    g[3, :6] = MAX_ID; p[3, :3] = MAX_ID; p[3, 3:6] = 65537                       # thing under stuff and under thing
    g[4, :6] = 70000; p[4, :6] = 9                                                # crowd under a thing
    if unlisted_pred:
        p[5, :5] = RICH_PRED_UNLISTED
    cats = sorted(CATS5)
    gt_segs = RICH_GT + [seg(2000 + i, cats[i % 5], int(i % 7 == 0)) for i in range(extra_gt)]
    pred_segs = RICH_PRED + [seg(3000 + i, cats[i % 5]) for i in range(extra_pred)]
    return frame(g, p, gt_segs, pred_segs)


def two_videos(H=32, W=64):
    """2 videos of 3 frames: video 0 has a car track (id 10) whose predicted id switches from 20 to 21 in the last frame, two persons
    (11, 12) predicted as one (22) and a crowd region (13) partly covered by the prediction; video 1 is nearly right, with a road /
    sky boundary off by two rows and an unmatched predicted bus"""
    vids = []
    gt_segs = [seg(1, 3), seg(2, 8), seg(10, 12), seg(11, 11), seg(12, 11), seg(13, 11, 1)]
    pred_segs = [seg(1, 3), seg(2, 8), seg(20, 12), seg(21, 12), seg(22, 11)]
    frames = []
    for t in range(3):
        g = np.full((H, W), 1, dtype=np.int64); g[:H // 2] = 2
        p = g.copy()
        g[10:20, 4 + 3 * t:16 + 3 * t] = 10
        p[10:20, 4 + 3 * t:16 + 3 * t] = 21 if t == 2 else 20
        g[14:26, 30:36] = 11; g[14:26, 36:43] = 12
        p[14:26, 30:43] = 22
        g[4:12, 50:62] = 13
        p[6:12, 52:60] = 22
        frames.append(frame(g, p, gt_segs, pred_segs))
    vids.append(frames)
    gt_segs = [seg(1, 3), seg(2, 8), seg(30, 20)]
    pred_segs = [seg(1, 3), seg(2, 8), seg(30, 20), seg(31, 20)]
    frames = []
    for t in range(3):
        g = np.full((H, W), 1, dtype=np.int64); g[:H // 2] = 2
        p = np.full((H, W), 1, dtype=np.int64); p[:H // 2 + 2] = 2
        g[8:24, 10 + t:40 + t] = 30; p[8:24, 11 + t:40 + t] = 30
        p[26:30, 50:56] = 31
        g[0, :5] = 0
        frames.append(frame(g, p, gt_segs, pred_segs))
    vids.append(frames)
    return vids


def self_scored(videos):
    """the same videos with the ground truth as the prediction"""
    return [[(f[0], {'segments_info': [{k: v for k, v in s.items() if k != 'iscrowd'} for s in f[0]['segments_info']]}, f[2], f[2]) for f in frames]
            for frames in videos]
