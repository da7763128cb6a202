"""The one-launch track solver (csrc/track_solver.hip) and the stand-alone NMS (csrc/nms.hip) against the literal
restatement of the reference (oracle/solver_oracle.py) on inputs built for their edges: tied scores, suppression chains
as deep as the frame, 63 / 64 / 65 rows and the 64-bit word boundaries, small frames on full id tables, resume below
track threshold, scores exactly on a threshold (1.0 included), ids in neither table, table overflow, a table capacity
below 512, NMS beyond 4,096 boxes.  Everything is integers, or fp32 values both sides compute with the same
operations: every comparison is exact.  The cases and their expected results come from tests/solver_edge_cases.py."""
import copy

import numpy as np
import pytest
import torch

import solver_edge_cases as E
from oracle import solver_oracle as SO
from test_solver import _numpy_mask


def _boxlist(dev, boxes, ids, scores, labels):
    from siammot_amd.structures import BoxList
    b = BoxList(torch.from_numpy(np.ascontiguousarray(boxes)).to(dev).reshape(-1, 4), E.IMAGE_WH, mode="xyxy")
    b.add_field("ids", torch.from_numpy(ids.copy()).to(dev))
    b.add_field("scores", torch.from_numpy(scores.copy()).to(dev))
    if labels is not None:
        b.add_field("labels", torch.from_numpy(labels.copy()).to(dev))
    return b


def _check_pool(pool, f, where):
    assert pool._active_ids == f["active"], where
    assert list(pool._dormant_ids.items()) == f["dormant"], where       # the ORDER too: it orders the next track memory
    assert pool._kill_ids == f["kill"], where
    assert (pool._max_id, pool._frame_idx) == (f["max_id"], f["frame_idx"]), where


# ---- CPU: the generator's conditions, and the host path of the product against the oracle -------------------------
@pytest.mark.parametrize("c", E.CASES, ids=E.case_id)
def test_host_solver_equals_the_oracle_on_edge_frames(c):
    from siammot_amd.solver import TrackSolver
    pool0, _, frames = E.case(*c)
    pool = copy.deepcopy(pool0)
    solver = TrackSolver(pool, *E.THRESHOLDS[c[4]], nms_mask_fn=_numpy_mask)
    for k, f in enumerate(frames):
        where = "%s frame %d" % (E.case_id(c), k)
        bl = _boxlist("cpu", f["boxes"], f["ids"], f["scores"], f["labels"])
        out = solver([bl])[0]
        assert np.array_equal(out.get_field("ids").numpy(), f["out_ids"]), where
        assert np.array_equal(out.get_field("scores").numpy(), f["out_scores"]), where
        assert np.array_equal(out.bbox.numpy(), f["boxes"][f["keep"]]), where
        assert np.array_equal(out.get_field("labels").numpy(), f["labels"][f["keep"]]), where
        assert np.array_equal(np.asarray(out.host_ids), f["out_ids"]), where
        assert np.array_equal(bl.get_field("scores").numpy(), f["banded"]), where      # banded in place
        _check_pool(pool, f, where)
        assert len(f["active"]) <= E.CAPACITY and len(f["dormant"]) <= E.CAPACITY, where     # fits the device tables


@pytest.mark.parametrize("c", E.CASES, ids=E.case_id)
def test_mirror_follows_the_oracle_pool_from_synthesised_records(c):
    """``TrackPool._mirror`` alone, without a device: the record the kernel would hand back (layout: include/smot_emm.h)
    is written from the oracle's results, the tables sorted as no particular order is promised — but for the ids resumed
    and suspended in the frame, which the record counts and puts last (word 6, bits 8 and up).  The mirror must end up
    as the oracle's pool, the insertion order of the dormant ids included — with hundreds of rows, ids resumed and
    suspended in one frame, and ids that are in neither table."""
    pool0, _, frames = E.case(*c)
    pool = copy.deepcopy(pool0)
    cap = pool.DEVICE_CAPACITY
    pool._last_tables = None
    for k, f in enumerate(frames):
        M, K = len(f["ids"]), len(f["keep"])
        rec = np.zeros(8 + 4 * M + 3 * cap, dtype=np.int32)
        rec[0], rec[1], rec[2], rec[3] = K, len(f["act_rows"]), f["max_id"], f["frame_idx"]
        rec[4], rec[5], rec[7] = len(f["active"]), len(f["dormant"]), M
        rec[6] = (4 if f["tables_unchanged"] else 0) | (len(f["again"]) << 8)     # (csrc/track_solver.hip, record word 6)
        rec[8:8 + K] = f["keep"]
        rec[8 + M:8 + M + K] = f["out_ids"]
        base = 8 + 3 * M
        rec[base:base + rec[4]] = sorted(f["active"])
        d = sorted(x for x in f["dormant"] if x[0] not in f["again"]) + sorted(x for x in f["dormant"] if x[0] in f["again"])
        rec[base + cap:base + cap + len(d)] = [i for i, _ in d]
        rec[base + 2 * cap:base + 2 * cap + len(d)] = [v for _, v in d]
        rec[base + 3 * cap:] = f["ids"]
        pool._mirror(rec, M)
        _check_pool(pool, f, "%s frame %d" % (E.case_id(c), k))


def test_edge_frames_contain_every_event_class():
    """A condition on the INPUTS of this module: every decision the solver can take is taken somewhere in the
    parametrisation, the rare ones included.  If a class is missing the generator is to be changed, not this test."""
    total = dict.fromkeys(E.EVENTS, 0)
    unchanged = 0
    for c in E.CASES:
        for f in E.case(*c)[2]:
            for e in E.EVENTS:
                total[e] += f["events"][e]
            unchanged += bool(f["tables_unchanged"])
            assert len(set(f["ids"][f["ids"] >= 0].tolist())) == int((f["ids"] >= 0).sum())      # ids unique in a frame
    print("events over %d frames: %s, %d frames leave the tables unchanged" % (len(E.CASES) * E.FRAMES, total, unchanged))
    for e in E.EVENTS:
        assert total[e] > 0, "no frame with the event %r" % e
    assert unchanged > 0 and unchanged < len(E.CASES) * E.FRAMES
    assert {E.variant_of(c) for c in E.CASES} == set(E.VARIANTS)


@pytest.mark.parametrize("n", [64, 65, 512])
def test_the_chain_keeps_exactly_its_even_positions(n):
    """The chain is as deep as it is long: box i falls to box i - 1 only if that one was kept, so the greedy pass keeps
    0, 2, 4, ... — in any row order."""
    f = E.chain_frame(n, "descending")
    assert SO.nms_indices(f["boxes"], f["scores"], 0.5).tolist() == list(range(0, n, 2))
    g = E.chain_frame(n, "permuted", seed=n)
    kept = SO.nms_indices(g["boxes"], g["scores"], 0.5)
    assert sorted((g["boxes"][kept, 0] / 30).astype(int).tolist()) == list(range(0, n, 2))
    e = E.chain_frame(n, "equal")                      # all tied: the stable sort leaves the row order
    assert SO.nms_indices(e["boxes"], e["scores"], 0.5).tolist() == list(range(0, n, 2))


# ---- GPU: the one-launch kernel --------------------------------------------------------------------------------------
DEV = "cuda:0"


class _Launches(object):
    """Counts ops.track_solve launches and keeps what the last one returned (the record on the device)."""

    def __enter__(self):
        import siammot_amd.ops as ops
        self.ops, self.real, self.n, self.last = ops, ops.track_solve, 0, None

        def counted(*a, **k):
            self.n += 1
            self.last = self.real(*a, **k)
            return self.last
        ops.track_solve = counted
        return self

    def __exit__(self, *exc):
        self.ops.track_solve = self.real


def _device_tables(pool):
    st = pool._dev_state.cpu().numpy()
    cap = pool.DEVICE_CAPACITY
    na, nd = int(st[2]), int(st[3])
    return st[:5].tolist(), st[8:8 + na].tolist(), list(zip(st[8 + cap:8 + cap + nd].tolist(),
                                                             st[8 + 2 * cap:8 + 2 * cap + nd].tolist()))


def _solve_and_check(solver, pool, f, variant, where, launches, equal_nan=False):
    """One frame through the device path; every output, the mirror and the device-resident state against the oracle's
    results in `f`.  Returns (kept rows, record, output BoxList)."""
    import siammot_amd.ops as ops
    n_det = f["n_det"]
    labels = None if variant == "nolabels" else f["labels"]
    want_labels = np.ones(len(f["ids"]), np.int64) if labels is None else labels
    before = launches.n
    if variant == "one":
        segs = [_boxlist(DEV, f["boxes"], f["ids"], f["scores"], labels)]
        assert solver._device_path(segs[0]), where
        out = solver(segs)[0]
    else:
        det = _boxlist(DEV, f["boxes"][:n_det], f["ids"][:n_det], f["raw"][:n_det],
                       None if labels is None else labels[:n_det]) if n_det else None
        trk = _boxlist(DEV, f["boxes"][n_det:], f["ids"][n_det:], f["raw"][n_det:],
                       None if labels is None else labels[n_det:]) if n_det < len(f["ids"]) else None
        segs = [s for s in (det, trk) if s is not None]
        assert solver._device_path(det, trk), where
        out = solver.solve(det, trk, 1.0)
    assert launches.n == before + 1, where
    rec = ops.track_solve_record(launches.last[2])
    M, K = len(f["ids"]), len(f["keep"])
    assert (int(rec[0]), int(rec[7])) == (K, M), where
    kept = rec[8:8 + K].astype(np.int64)
    # the output rows
    assert kept.tolist() == f["keep"].tolist(), where
    assert np.array_equal(out.get_field("ids").cpu().numpy(), f["out_ids"]), where
    assert np.array_equal(out.get_field("scores").cpu().numpy(), f["out_scores"], equal_nan=equal_nan), where
    assert np.array_equal(out.bbox.cpu().numpy(), f["boxes"][f["keep"]]), where
    assert np.array_equal(out.get_field("labels").cpu().numpy(), want_labels[f["keep"]]), where
    assert np.array_equal(np.asarray(out.host_ids), f["out_ids"]), where
    # the inputs, banded in place
    got = np.concatenate([s.get_field("scores").cpu().numpy() for s in segs])
    assert np.array_equal(got, f["banded"], equal_nan=equal_nan), where
    # the rows whose id is active after the update, in output order
    rows, act = f["act_rows"], out.active_rows
    assert int(rec[1]) == len(rows) == len(act), where
    assert np.array_equal(act.get_field("ids").cpu().numpy(), f["out_ids"][rows]), where
    assert np.array_equal(act.get_field("scores").cpu().numpy(), f["out_scores"][rows], equal_nan=equal_nan), where
    assert np.array_equal(act.bbox.cpu().numpy(), f["boxes"][f["keep"]][rows]), where
    assert np.array_equal(act.get_field("labels").cpu().numpy(), want_labels[f["keep"]][rows]), where
    assert list(act.host_ids) == f["out_ids"][rows].tolist(), where
    # the host mirror, and the state the NEXT launch reads
    _check_pool(pool, f, where)
    hdr, d_active, d_dormant = _device_tables(pool)
    assert hdr == [f["max_id"], f["frame_idx"], len(f["active"]), len(f["dormant"]), len(rows)], where
    assert len(d_active) == len(set(d_active)) and set(d_active) == f["active"], where
    assert len(d_dormant) == len(dict(d_dormant)) and dict(d_dormant) == dict(f["dormant"]), where
    assert not rec[6] & 1, where
    assert bool(rec[6] & 4) == bool(f["tables_unchanged"]), where
    assert int(rec[6]) >> 8 == len(f["again"]), where            # ids resumed and suspended in this frame, still dormant
    return kept, rec, out


def _written(rec):
    """The words of a record the kernel writes (the row blocks are allocated for M rows and filled for K / A)."""
    M, K, A = int(rec[7]), int(rec[0]), int(rec[1])
    return rec[:8].tolist(), rec[8:8 + K].tolist(), rec[8 + M:8 + M + K].tolist(), rec[8 + 2 * M:8 + 2 * M + A].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("c", E.CASES, ids=E.case_id)
def test_one_launch_solver_equals_the_oracle_on_edge_frames(c):
    import siammot_amd.ops as ops
    from siammot_amd.solver import TrackSolver
    pool0, _, frames = E.case(*c)
    pool = copy.deepcopy(pool0)
    solver = TrackSolver(pool, *E.THRESHOLDS[c[4]])
    with _Launches() as launches:
        for k, f in enumerate(frames):
            where = "%s frame %d" % (E.case_id(c), k)
            kept, _, _ = _solve_and_check(solver, pool, f, E.variant_of(c), where, launches)
            # the two device implementations of the greedy pass agree with each other as well
            mask = ops.nms_keep_mask(torch.from_numpy(f["boxes"]).to(DEV), torch.from_numpy(f["banded"]).to(DEV), 0.5)
            assert mask.nonzero().flatten().cpu().tolist() == kept.tolist(), where
        assert launches.n == len(frames)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["descending", "equal", "permuted"])
@pytest.mark.parametrize("M", [512, 511, 65, 64])
def test_one_launch_solver_resolves_a_chain_as_deep_as_the_frame(M, kind):
    """Box j of the chain is decided only after j rounds of the kernel's fixed-point iteration: its loop bound and the
    rotation of its "changed" flags are at their limit."""
    from siammot_amd.solver import TrackPool, TrackSolver
    thresholds = E.THRESHOLDS[1]
    runs = []
    for _ in range(2 if (M, kind) == (512, "descending") else 1):        # twice, back to back, on fresh pools
        f = E.solve_with_oracle(TrackPool(max_dormant_frames=3), E.chain_frame(M, kind, seed=M), thresholds)
        if kind != "permuted":
            assert f["keep"].tolist() == list(range(0, M, 2))
        pool = TrackPool(max_dormant_frames=3)
        with _Launches() as launches:
            _, rec, _ = _solve_and_check(TrackSolver(pool, *thresholds), pool, f, "two", "chain %d %s" % (M, kind), launches)
        runs.append(_written(rec))
    assert all(r == runs[0] for r in runs)


@pytest.mark.gpu
def test_track_solve_with_a_small_table_capacity_stays_inside_its_tables():
    """pool_capacity is an argument of the kernel: with 16 ids per table the three tables are 16 words apart, a frame that
    fits gives the oracle's tables, one that does not says so (record word 6, bit 0) and writes nothing past a table."""
    import siammot_amd.ops as ops
    CAP, GUARD, SENTINEL = 16, 64, -77777
    thr = E.THRESHOLDS[0]
    rs = np.random.RandomState(16)
    pool, strangers = E.make_pool(rs, 6, 3, 3)
    f = E.solve_with_oracle(copy.deepcopy(pool), E.make_frame(rs, pool, strangers, 12), thr, strangers)
    assert 0 < len(f["dormant"]) and f["events"]["start"] > 0 and not f["tables_unchanged"]      # (conditions on the input)

    def launch(state, frame):
        n_det = frame["n_det"]
        seg = lambda a, b: (torch.from_numpy(frame["boxes"][a:b]).to(DEV), torch.from_numpy(frame["raw"][a:b]).to(DEV),
                            torch.from_numpy(frame["ids"][a:b]).to(DEV), torch.from_numpy(frame["labels"][a:b]).to(DEV))
        fbuf, ibuf, rec, M = ops.track_solve(seg(0, n_det) if n_det else None,
                                             seg(n_det, len(frame["ids"])) if n_det < len(frame["ids"]) else None,
                                             1.0, thr, 0.5, 3, state, CAP)
        return ops.track_solve_record(rec), ibuf

    h0 = E.state_array(pool, CAP, GUARD, SENTINEL)
    state = torch.from_numpy(h0).to(DEV)
    rec, ibuf = launch(state, f)
    st = state.cpu().numpy()
    na, nd = len(f["active"]), len(f["dormant"])
    assert not rec[6] & 1 and (int(rec[4]), int(rec[5])) == (na, nd) and rec[0] == len(f["keep"])
    assert rec[8:8 + rec[0]].tolist() == f["keep"].tolist() and ibuf[:rec[0]].cpu().tolist() == f["out_ids"].tolist()
    assert st[:4].tolist() == [f["max_id"], f["frame_idx"], na, nd]
    assert set(st[8:8 + na].tolist()) == f["active"] and na == len(set(st[8:8 + na].tolist()))
    assert dict(zip(st[8 + CAP:8 + CAP + nd].tolist(), st[8 + 2 * CAP:8 + 2 * CAP + nd].tolist())) == dict(f["dormant"])
    # the record's snapshot of the tables is the state's
    base = 8 + 3 * len(f["ids"])
    assert rec[base:base + na].tolist() == st[8:8 + na].tolist()
    assert rec[base + CAP:base + CAP + nd].tolist() == st[8 + CAP:8 + CAP + nd].tolist()
    assert rec[base + 2 * CAP:base + 2 * CAP + nd].tolist() == st[8 + 2 * CAP:8 + 2 * CAP + nd].tolist()
    # words of a table that neither the old nor the new count covers still hold the fill, the guard words all do
    for t, (old, new) in enumerate(((int(h0[2]), na), (int(h0[3]), nd), (int(h0[3]), nd))):
        assert (st[8 + t * CAP + max(old, new):8 + (t + 1) * CAP] == SENTINEL).all(), "table %d" % t
    assert (st[8 + 3 * CAP:] == SENTINEL).all() and len(st) == 8 + 3 * CAP + GUARD

    # a frame that starts more ids than the table takes: 6 active ids that stay (none of them is in the frame), no dormant
    # ids, 14 isolated detections above the start threshold
    from siammot_amd.solver import TrackPool
    pool = TrackPool(max_dormant_frames=3)
    for _ in range(6):
        pool.start_track()
    pool.increment_frame(4)
    n = 14
    x0 = 150.0 * np.arange(n)
    over = dict(boxes=np.stack((x0, 0 * x0, x0 + 100, 0 * x0 + 100), 1).astype(np.float32), ids=np.full(n, -1, np.int64),
                raw=np.full(n, 0.9375, np.float32), labels=np.ones(n, np.int64), n_det=n)
    state = torch.from_numpy(E.state_array(pool, CAP, GUARD, SENTINEL)).to(DEV)
    rec, ibuf = launch(state, over)
    st = state.cpu().numpy()
    assert rec[6] & 1 and 0 <= rec[4] <= CAP and 0 <= rec[5] <= CAP and rec[0] == n
    assert ibuf[:n].cpu().tolist() == list(range(6, 6 + n))                    # the rows themselves got their new ids
    assert 0 <= st[2] <= CAP and 0 <= st[3] <= CAP and st[0] == 5 + n
    assert set(st[8:8 + st[2]].tolist()) <= set(range(6 + n)) and len(set(st[8:8 + st[2]].tolist())) == st[2]
    assert (st[8 + CAP:8 + 3 * CAP] == SENTINEL).all(), "the active table spilled into the dormant tables"
    assert (st[8 + 3 * CAP:] == SENTINEL).all()


@pytest.mark.gpu
def test_overflowing_id_tables_raise_through_the_solver():
    from siammot_amd.solver import TrackPool, TrackSolver
    pool = TrackPool(max_dormant_frames=3)
    for _ in range(500):
        pool.start_track()
    pool.increment_frame(4)
    n = 100
    x0, y0 = 150.0 * (np.arange(n) % 10), 150.0 * (np.arange(n) // 10)
    det = _boxlist(DEV, np.stack((x0, y0, x0 + 100, y0 + 100), 1).astype(np.float32), np.full(n, -1, np.int64),
                   np.full(n, 0.9375, np.float32), np.ones(n, np.int64))
    solver = TrackSolver(pool, *E.THRESHOLDS[1])
    assert solver._device_path(det, None)
    with pytest.raises(RuntimeError, match="overflowed"):
        solver.solve(det, None, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [40, 100])
def test_a_nan_track_score_is_reported_and_disturbs_no_other_row(M):
    """A propagated track with a NaN score (what a head writes whose order hint failed) sets record word 6 bit 1.  NaN
    compares false with everything: the reference's sort puts the row last and none of its threshold tests fires, so the
    row keeps its id if NMS keeps it — and every other row is decided as if it were not there."""
    from siammot_amd.solver import TrackSolver
    rs = np.random.RandomState(M)
    thr = E.THRESHOLDS[1]
    pool0, strangers = E.make_pool(rs, 30, 20, 3)
    f = E.make_frame(rs, pool0, strangers, M)
    isolated = np.nonzero((f["boxes"][:, 1] >= 1300) & (f["ids"] >= 0))[0]     # a track row with a box that touches no other
    assert len(isolated) > 0
    f["raw"][isolated[0]] = f["scores"][isolated[0]] = np.nan
    f = E.solve_with_oracle(copy.deepcopy(pool0), f, thr, strangers)
    assert isolated[0] in f["keep"] and np.isnan(f["out_scores"]).sum() == 1
    pool = copy.deepcopy(pool0)
    with _Launches() as launches:
        _, rec, out = _solve_and_check(TrackSolver(pool, *thr), pool, f, "two", "NaN row, M=%d" % M, launches,
                                       equal_nan=True)
    assert rec[6] & 2 and out.nan_track_scores is True


# ---- GPU: the stand-alone NMS ----------------------------------------------------------------------------------------
def _tied_boxes(n):
    rs = np.random.RandomState(n)
    centers = rs.uniform(0, 600, (max(n // 6, 1), 2))                       # clustered: plenty of overlaps
    c = centers[rs.randint(0, len(centers), n)] + rs.normal(0, 12, (n, 2))
    wh = rs.uniform(20, 120, (n, 2))
    boxes = np.concatenate((c - wh / 2, c + wh / 2), 1).astype(np.float32)
    scores = (rs.randint(1, 65, n) / 64.0).astype(np.float32)                # 64 levels: ties everywhere
    return boxes, scores


def _nms_both_ways(boxes, scores, thresh=0.5):
    import siammot_amd.ops as ops
    b, s = torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV)
    idx = ops.nms(b, s, thresh).cpu().numpy()
    mask = ops.nms_keep_mask(b, s, thresh).cpu().numpy()
    assert mask.dtype == np.bool_ and np.nonzero(mask)[0].tolist() == idx.tolist()
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 300, 2500, 4096, 4097, 6000, 8192])
def test_nms_with_tied_scores_equals_the_oracle(n):
    boxes, scores = _tied_boxes(n)
    ref = SO.nms_indices(boxes, scores, 0.5)
    assert len(np.unique(scores)) < n                                        # (a condition on the input: there are ties)
    if n == 8192:
        # a condition on the input: the second 64-word register of the scan kernel's `removed` set decides something.  Among
        # the suppressed boxes at sorted positions >= 4096 some have kept suppressors only at positions >= 4096, and some
        # have one below
        order = np.argsort(-scores.astype(np.float64), kind="stable")
        pos = np.empty(n, np.int64)
        pos[order] = np.arange(n)
        kept_pos = np.sort(pos[ref])
        sb = boxes[order]
        only_high = with_low = 0
        dead = np.ones(n, bool)
        dead[kept_pos] = False
        for j in np.nonzero(dead)[0]:
            if j < 4096:
                continue
            by = kept_pos[:np.searchsorted(kept_pos, j)]
            by = by[E.overlaps(sb[j], sb[by], 0.5)]
            assert len(by) > 0
            only_high += by.min() >= 4096
            with_low += by.min() < 4096
        print("n=8192: %d kept, %d late boxes fall to late kept boxes only, %d to an early one"
              % (len(ref), only_high, with_low))
        assert only_high > 0 and with_low > 0
    assert _nms_both_ways(boxes, scores).tolist() == ref.tolist()
    assert 0 < len(ref) < n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4097, 8192])
def test_nms_resolves_a_chain_through_every_slab(n):
    boxes = E.chain_boxes(n)
    scores = ((n - np.arange(n)) / 8192.0).astype(np.float32)                # exact and strictly descending
    assert _nms_both_ways(boxes, scores).tolist() == list(range(0, n, 2))
    perm = np.random.RandomState(n).permutation(n)
    kept = _nms_both_ways(boxes[perm], scores[perm])
    assert kept.tolist() == SO.nms_indices(boxes[perm], scores[perm], 0.5).tolist()
    assert sorted(perm[kept].tolist()) == list(range(0, n, 2))
    tied = np.full(n, 0.5, np.float32)                                       # all tied: stable order = row order
    assert _nms_both_ways(boxes, tied).tolist() == list(range(0, n, 2))


@pytest.mark.gpu
def test_nms_refuses_more_boxes_than_its_slab_holds():
    import siammot_amd.ops as ops
    n = 8193
    boxes = torch.from_numpy(E.chain_boxes(n)).to(DEV)
    scores = torch.linspace(1.0, 0.0, n, device=DEV)
    with pytest.raises(RuntimeError):
        ops.nms_keep_mask(boxes, scores, 0.5)
    with pytest.raises(RuntimeError):
        ops.nms(boxes, scores, 0.5)
