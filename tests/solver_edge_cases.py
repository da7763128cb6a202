"""Deterministic frames for tests/test_solver_edges.py: inputs built to sit on the edges of csrc/track_solver.hip and
csrc/nms.hip (sort ties, suppression chains as deep as the frame, 63 / 64 / 65 rows and the 64-bit word boundaries, small
frames on full id tables, scores exactly on a threshold, ids in neither table), with the answer of the literal
restatement of the reference's solver (oracle/solver_oracle.py) computed ONCE per case and shared by the CPU and the
GPU tests.  Nothing here touches a device."""
import copy
import functools

import numpy as np

from oracle import solver_oracle as SO

IMAGE_WH = (1280, 704)
SCORE_GRID = 16                          # scores are k / 16: ties everywhere, exact 0.25 / 0.375 / 0.5 / 1.0
THRESHOLDS = ((0.375, 0.5, 0.25),        # (track, start, resume): resume below track, all exactly representable
              (0.4, 0.6, 0.4),
              (0.3, 0.5, 0.4))
MAX_DORMANT = (1, 3)
SHAPES = ((1, 0, 0), (2, 3, 0), (10, 500, 500), (63, 40, 100), (64, 64, 0), (65, 500, 10),
          (127, 100, 300), (128, 100, 300), (129, 100, 300), (255, 200, 200), (256, 200, 200), (257, 200, 200),
          (511, 300, 100), (512, 340, 512))          # (rows per frame M, active ids, dormant ids)
FRAMES = 3
STRANGERS = 5                            # ids the tracker still propagates although the pool has killed them
CAPACITY = 512                           # ids per table of the device-resident pool (TrackPool.DEVICE_CAPACITY)
# how the frame reaches the solver, by case number: "one" = a single concatenated BoxList through solver([boxlist]),
# "nolabels" = two segments without a labels field, "two" = two segments (detections, tracks) with labels
VARIANTS = ("one", "nolabels", "two", "two", "two")
CASES = [(M, na, nd, mdf, t) for (M, na, nd) in SHAPES for mdf in MAX_DORMANT for t in range(len(THRESHOLDS))]
EVENTS = ("start", "resume", "resume_and_suspend", "suspend_by_score", "suspend_by_nms", "expire", "stranger_kept",
          "tie_kept_vs_suppressed")


def case_id(c):
    return "M%d-a%d-d%d-mdf%d-thr%d" % c


def variant_of(c):
    return VARIANTS[CASES.index(c) % len(VARIANTS)]


def chain_boxes(n):
    """Box i = [30 i, 0, 30 i + 100, 100]: neighbours overlap with +1-IoU 71 / 131 > 0.5, next-neighbours with
    41 / 161 < 0.5 — in score order along the chain every box hangs on its predecessor: suppression depth n."""
    x = 30.0 * np.arange(n, dtype=np.float32)
    return np.stack((x, np.zeros(n, np.float32), x + 100, np.full(n, 100, np.float32)), 1).astype(np.float32)


def overlaps(box, others, thresh):
    """+1-convention "IoU > thresh" of one box against many, in the fp32 operations of SO.nms_indices."""
    one = np.float32(1)
    w = np.maximum(np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]) + one, 0)
    h = np.maximum(np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]) + one, 0)
    inter = (w * h).astype(np.float32)
    area = (others[:, 2] - others[:, 0] + one) * (others[:, 3] - others[:, 1] + one)
    a0 = (box[2] - box[0] + one) * (box[3] - box[1] + one)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a0 + area - inter) > np.float32(thresh)


def frame_boxes(rs, M):
    """A third of the rows form one chain, a third sit in tight clusters, the rest are isolated; shuffled over the rows."""
    n_chain = M // 3
    n_clu = M // 3
    n_iso = M - n_chain - n_clu
    chain = chain_boxes(n_chain)                                   # y 0 .. 100
    centres = np.stack((rs.uniform(100, 3000, max(M // 12, 1)), rs.uniform(400, 900, max(M // 12, 1))), 1)
    c = centres[rs.randint(0, len(centres), n_clu)] + rs.normal(0, 8, (n_clu, 2))
    wh = rs.uniform(40, 90, (n_clu, 2))
    clu = np.concatenate((c - wh / 2, c + wh / 2), 1)              # y 300 .. 1000
    k = np.arange(n_iso)
    x0, y0 = 150.0 * (k % 32), 1300.0 + 150.0 * (k // 32)          # 150 px apart, sides 100: no overlap at all
    iso = np.stack((x0, y0, x0 + 100, y0 + 100), 1)
    boxes = np.concatenate((chain, clu, iso), 0).astype(np.float32)
    return boxes[rs.permutation(M)]


def make_pool(rs, n_active, n_dormant, max_dormant_frames):
    """A TrackPool brought to (n_active, n_dormant) with the host mutators only, and the ids it killed on the way."""
    from siammot_amd.solver import TrackPool
    pool = TrackPool(max_dormant_frames=max_dormant_frames)
    for _ in range(n_active + n_dormant + STRANGERS):
        pool.start_track()
    pool.increment_frame(max_dormant_frames + 3)
    ids = rs.permutation(n_active + n_dormant + STRANGERS)
    strangers = [int(i) for i in ids[:STRANGERS]]
    for i in strangers:
        pool.kill_track(i)
    for i in ids[STRANGERS:STRANGERS + n_dormant]:
        pool.suspend_track(int(i))
        # some of these expire in the first frames, some survive all of them
        pool._dormant_ids[int(i)] = pool._frame_idx - 1 - int(rs.randint(0, max_dormant_frames + 1))
    return pool, strangers


def make_frame(rs, pool, strangers, M):
    """One frame of M rows from the pool's CURRENT state: detections (id -1) first, then the boxes the tracker propagated
    (scores carry the +1 of the track segment in `scores`; `raw` is what the segments hold before the solver's bias).
    Ids are unique within a frame and scores are never NaN: the reference leaves both undefined."""
    universe = sorted(pool.get_active_ids()) + sorted(pool.get_dormant_ids()) + list(strangers)
    n_trk = min(2 * M // 3, len(universe))
    n_det = M - n_trk
    trk = rs.choice(np.array(universe, dtype=np.int64), n_trk, replace=False) if n_trk else np.zeros(0, np.int64)
    ids = np.concatenate((np.full(n_det, -1, np.int64), trk.astype(np.int64)))
    raw = (rs.randint(1, SCORE_GRID + 1, M) / float(SCORE_GRID)).astype(np.float32)
    scores = raw.copy()
    scores[n_det:] += np.float32(1.0)
    labels = rs.randint(1, 4, M).astype(np.int64)
    return dict(boxes=frame_boxes(rs, M), ids=ids, raw=raw, scores=scores, labels=labels, n_det=n_det)


def solve_with_oracle(pool, frame, thresholds, strangers=()):
    """Run the restatement of the reference on `frame` (mutates `pool`); adds the expected results, the pool afterwards and
    the event counts of the frame to it."""
    boxes, ids = frame["boxes"], frame["ids"]
    active0, dormant0 = set(pool.get_active_ids()), dict(pool._dormant_ids)
    kill0, max0 = set(pool._kill_ids), pool._max_id
    banded = frame["scores"].copy()
    keep, out_ids, out_scores = SO.solve(pool, boxes, ids.copy(), banded, *thresholds)
    track, start, resume = (np.float32(t) for t in thresholds)
    kin = ids[keep]                                               # the ids the kept rows came in with
    is_dorm = np.array([int(i) in dormant0 for i in kin], bool)
    is_act = np.array([int(i) in active0 for i in kin], bool)
    removed = set(ids[ids >= 0].tolist()) - set(kin[kin >= 0].tolist())
    ev = dict.fromkeys(EVENTS, 0)
    ev["start"] = pool._max_id - max0
    ev["resume"] = int((is_dorm & (out_scores >= resume)).sum())
    ev["resume_and_suspend"] = int((is_dorm & (out_scores >= resume) & (out_scores < track)).sum())
    ev["suspend_by_score"] = int((is_act & (out_scores < track)).sum())
    ev["suspend_by_nms"] = len(removed & active0)
    ev["expire"] = len(pool._kill_ids - kill0)
    ev["stranger_kept"] = int(np.isin(out_ids, np.array(list(strangers) or [-2])).sum())
    dead = np.ones(len(ids), bool)
    dead[keep] = False
    for j in np.nonzero(dead)[0]:
        same = keep[banded[keep] == banded[j]]
        if len(same) and overlaps(boxes[j], boxes[same], 0.5).any():
            ev["tie_kept_vs_suppressed"] += 1
    active1 = set(pool.get_active_ids())
    # ids resumed and suspended in this frame that are still dormant after it (the solver kernel's record counts them)
    again = [int(i) for i in kin[is_dorm & (out_scores >= resume) & (out_scores < track)] if int(i) in pool._dormant_ids]
    frame.update(
        keep=keep, again=again, out_ids=out_ids, out_scores=out_scores, banded=banded, events=ev,
        active=active1, dormant=list(pool._dormant_ids.items()), kill=set(pool._kill_ids), max_id=pool._max_id,
        frame_idx=pool._frame_idx, tables_unchanged=(active1 == active0 and dict(pool._dormant_ids) == dormant0),
        act_rows=np.nonzero(np.array([int(i) in active1 for i in out_ids], bool))[0])
    return frame


@functools.lru_cache(maxsize=None)
def case(M, n_active, n_dormant, max_dormant_frames, thr):
    """(pool before the first frame, stranger ids, FRAMES frames with their expected results).  Every frame is built from
    the ORACLE pool's state only, so a solver under test never needs a host-side look at (or edit of) its own pool
    between frames.  Cached: treat the result as read-only and deep-copy the pool."""
    rs = np.random.RandomState(1000003 * M + 1009 * n_active + 17 * n_dormant + 5 * max_dormant_frames + thr)
    pool0, strangers = make_pool(rs, n_active, n_dormant, max_dormant_frames)
    twin = copy.deepcopy(pool0)
    frames = [solve_with_oracle(twin, make_frame(rs, twin, strangers, M), THRESHOLDS[thr], strangers)
              for _ in range(FRAMES)]
    return pool0, strangers, frames


def chain_frame(M, scores_kind, seed=0):
    """M detections that are nothing but the chain.  'descending': strictly falling scores along the chain; 'equal': one
    score for all (the stable order is the row order); 'permuted': the descending frame with its rows shuffled."""
    boxes = chain_boxes(M)
    if scores_kind == "equal":
        scores = np.full(M, 0.75, np.float32)
    else:
        scores = (0.25 + (M - np.arange(M)) / 1024.0).astype(np.float32)    # exact, distinct, in (0.25, 0.75]
    if scores_kind == "permuted":
        perm = np.random.RandomState(seed).permutation(M)
        boxes, scores = boxes[perm], scores[perm]
    return dict(boxes=boxes, ids=np.full(M, -1, np.int64), raw=scores.copy(), scores=scores.copy(),
                labels=np.ones(M, np.int64), n_det=M)


def state_array(pool, cap, guard=0, fill=0):
    """The int32 pool state of smot_track_solve_fwd for a table capacity `cap`, with `guard` words behind it."""
    h = np.full(8 + 3 * cap + guard, fill, np.int32)
    h[:8] = 0
    h[0], h[1], h[2], h[3] = pool._max_id, pool._frame_idx, len(pool._active_ids), len(pool._dormant_ids)
    h[8:8 + len(pool._active_ids)] = sorted(pool._active_ids)
    dorm = sorted(pool._dormant_ids.items())
    h[8 + cap:8 + cap + len(dorm)] = [d[0] for d in dorm]
    h[8 + 2 * cap:8 + 2 * cap + len(dorm)] = [d[1] for d in dorm]
    return h
