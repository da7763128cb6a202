"""Several cameras on one GPU, the device side: the batched track solver (csrc/track_solver.hip,
track_solve_batched_kernel — one workgroup per image) against the oracle's edge frames and, bit for bit, against the
single launch on a copy of the same pool; every image inside its own buffers; and ``MultiCameraTrackingLoop`` with the real
HIP head against independent ``TrackingLoop``s.  Integers and fp32 values that both sides compute with the same operations:
every comparison is exact."""
import copy

import numpy as np
import pytest
import torch

import solver_edge_cases as E
from test_multi_camera import _same_pool
from test_solver_edges import _boxlist, _check_pool, _written

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the cameras of a call: (rows, active ids, dormant ids, max dormant frames, thresholds) — 1 row, the 63 / 64 / 65 boundary,
# small frames on full id tables; thresholds and dormancy mixed; the segments with and without labels in turn
CAMERAS = ((1, 0, 0, 1, 0), (2, 3, 0, 3, 1), (63, 40, 100, 1, 2), (64, 64, 0, 3, 0), (65, 500, 10, 1, 1), (10, 500, 500, 3, 2))
VARIANTS = ("nolabels", "two")


class _Counted(object):
    """Counts the calls of the library's batched entry point (one call = ceil(images with rows / 16) launches: the loop
    over chunks is inside it), of the single-image binding and of the stream synchronisations; keeps the last records."""

    def __enter__(self):
        import siammot_amd.ops as ops
        self.ops, self.lib = ops, ops.load_library()
        self.real = (self.lib.smot_track_solve_batched_fwd, ops.track_solve, ops.track_solve_records, torch.cuda.Stream.synchronize)
        self.entry = self.images = self.single = self.syncs = 0
        self.records = self.single_rec = None

        def entry(num_images, *a):
            self.entry += 1
            self.images = num_images
            return self.real[0](num_images, *a)

        def single(*a, **k):
            self.single += 1
            r = self.real[1](*a, **k)
            self.single_rec = r[2]
            return r

        def records(rec, offsets):
            self.records = self.real[2](rec, offsets)
            return self.records

        def sync(stream):
            self.syncs += 1
            return self.real[3](stream)
        self.lib.smot_track_solve_batched_fwd, ops.track_solve, ops.track_solve_records = entry, single, records
        torch.cuda.Stream.synchronize = sync
        return self

    def __exit__(self, *exc):
        self.lib.smot_track_solve_batched_fwd, self.ops.track_solve, self.ops.track_solve_records = self.real[:3]
        torch.cuda.Stream.synchronize = self.real[3]


def _segments(f, variant):
    n_det = f["n_det"]
    labels = None if variant == "nolabels" else f["labels"]
    cut = lambda a, b: _boxlist(DEV, f["boxes"][a:b], f["ids"][a:b], f["raw"][a:b], None if labels is None else labels[a:b])
    return (cut(0, n_det) if n_det else None), (cut(n_det, len(f["ids"])) if n_det < len(f["ids"]) else None)


def _fields(b):
    return [b.bbox] + [b.get_field(k) for k in ("ids", "scores", "labels")]


def _same_rows(a, b, where):
    assert len(a) == len(b), where
    for x, y in zip(_fields(a), _fields(b)):
        assert x.dtype == y.dtype and torch.equal(x, y), where


def _check_image(out, segs, rec, pool, f, variant, where):
    """One image of a batched call against the oracle's frame (what tests/test_solver_edges.py checks of a single launch)."""
    want_labels = np.ones(len(f["ids"]), np.int64) if variant == "nolabels" else f["labels"]
    M, K = len(f["ids"]), len(f["keep"])
    assert (int(rec[0]), int(rec[7])) == (K, M), where
    assert rec[8:8 + K].tolist() == f["keep"].tolist(), where
    assert np.array_equal(out.get_field("ids").cpu().numpy(), f["out_ids"]), where
    assert np.array_equal(out.get_field("scores").cpu().numpy(), f["out_scores"]), where
    assert np.array_equal(out.bbox.cpu().numpy(), f["boxes"][f["keep"]]), where
    assert np.array_equal(out.get_field("labels").cpu().numpy(), want_labels[f["keep"]]), where
    assert np.array_equal(np.asarray(out.host_ids), f["out_ids"]), where
    got = np.concatenate([s.get_field("scores").cpu().numpy() for s in segs if s is not None])
    assert np.array_equal(got, f["banded"]), where                      # the inputs, banded in place
    rows, act = f["act_rows"], out.active_rows
    assert int(rec[1]) == len(rows) == len(act), where
    assert np.array_equal(act.get_field("ids").cpu().numpy(), f["out_ids"][rows]), where
    assert np.array_equal(act.get_field("scores").cpu().numpy(), f["out_scores"][rows]), where
    assert np.array_equal(act.bbox.cpu().numpy(), f["boxes"][f["keep"]][rows]), where
    assert np.array_equal(act.get_field("labels").cpu().numpy(), want_labels[f["keep"]][rows]), where
    assert list(act.host_ids) == f["out_ids"][rows].tolist(), where
    _check_pool(pool, f, where)
    assert not rec[6] & 1 and bool(rec[6] & 4) == bool(f["tables_unchanged"]) and int(rec[6]) >> 8 == len(f["again"]), where
    assert not out.nan_track_scores, where


@pytest.mark.parametrize("B", [1, 2, 5, 17, 64])
def test_batched_solver_equals_the_oracle_and_the_single_launch_on_edge_frames(B):
    """B = 17 crosses the 16 images of a launch by one, B = 64 is the most a call takes (cases repeated on pools of their
    own).  In the B = 5 call camera 2 has no rows in the middle step: it is not launched, its pool and its last outputs
    stand, and it goes on with its next frame one step later."""
    import siammot_amd.ops as ops
    from siammot_amd.solver import TrackSolver, solve_batched
    cams = [CAMERAS[b % len(CAMERAS)] for b in range(B)]
    frames = [E.case(*c)[2] for c in cams]
    variants = [VARIANTS[b % 2] for b in range(B)]
    pools = [copy.deepcopy(E.case(*c)[0]) for c in cams]                 # the batched call's
    twins = [copy.deepcopy(E.case(*c)[0]) for c in cams]                 # ... and the single launches'
    solvers = [TrackSolver(p, *E.THRESHOLDS[c[4]]) for p, c in zip(pools, cams)]
    singles = [TrackSolver(p, *E.THRESHOLDS[c[4]]) for p, c in zip(twins, cams)]
    pos = [0] * B
    idle = 2 if B == 5 else -1
    with _Counted() as n:
        for step in range(E.FRAMES):
            live = [b for b in range(B) if not (b == idle and step == 1)]
            segs = [_segments(frames[b][pos[b]], variants[b]) if b in live else (None, None) for b in range(B)]
            if idle >= 0 and step == 1:
                state_before = pools[idle]._dev_state.clone()
                prev_before = [t.clone() for t in _fields(prev_idle)] + [t.clone() for t in _fields(prev_idle.active_rows)]
                mirror_before = copy.deepcopy((pools[idle]._active_ids, pools[idle]._dormant_ids, pools[idle]._frame_idx))
            entry, syncs = n.entry, n.syncs
            outs = solve_batched(solvers, [s[0] for s in segs], [s[1] for s in segs], 1.0)
            # one call of the library entry — ceil(images with rows / 16) launches — and one synchronisation, whatever B is
            assert (n.entry, n.syncs, n.single) == (entry + 1, syncs + 1, 0) and n.images == B, (B, step)
            assert -(-len(live) // ops.TRACK_SOLVE_CHUNK) == (2 if B == 17 else 4 if B == 64 else 1)
            recs = n.records
            assert len(outs) == len(recs) == B
            for b in live:
                f, where = frames[b][pos[b]], "B=%d image %d (%s, %s) step %d" % (B, b, E.case_id(cams[b]), variants[b], step)
                _check_image(outs[b], segs[b], recs[b], pools[b], f, variants[b], where)
                # ... and bit for bit the single launch on a copy of the pool
                det, trk = _segments(f, variants[b])
                want = singles[b].solve(det, trk, 1.0)
                _same_rows(outs[b], want, where)
                _same_rows(outs[b].active_rows, want.active_rows, where)
                assert np.array_equal(outs[b].host_ids, want.host_ids) and outs[b].active_rows.host_ids == want.active_rows.host_ids
                assert _written(recs[b]) == _written(ops.track_solve_record(n.single_rec)), where
                for s_, w_ in zip(segs[b], (det, trk)):
                    assert s_ is None or torch.equal(s_.get_field("scores"), w_.get_field("scores")), where
                _same_pool(pools[b], twins[b], where)
                assert torch.equal(pools[b]._dev_state, twins[b]._dev_state), where        # what the next launch reads
                pos[b] += 1
            n.single = 0
            if idle >= 0 and step == 1:
                assert outs[idle] is None and len(recs[idle]) == 0
                assert torch.equal(pools[idle]._dev_state, state_before)
                now = _fields(prev_idle) + _fields(prev_idle.active_rows)
                assert all(torch.equal(x, y) for x, y in zip(now, prev_before))
                assert (pools[idle]._active_ids, pools[idle]._dormant_ids, pools[idle]._frame_idx) == mirror_before
            if idle >= 0:
                prev_idle = outs[idle] if outs[idle] is not None else prev_idle
    assert pos == [E.FRAMES - (b == idle) for b in range(B)]


def _guarded(words, dtype, guard, fill):
    """One tensor holding arrays of `words` elements each with `guard` elements of `fill` before, between and behind them;
    returns it and the arrays' offsets."""
    offs, n = [], guard
    for w in words:
        offs.append(n)
        n += w + guard
    return torch.full((n,), fill, dtype=dtype, device=DEV), offs


def _guards_intact(t, offs, words, guard, fill):
    h = t.cpu().numpy()
    mask = np.ones(len(h), bool)
    for o, w in zip(offs, words):
        mask[o:o + w] = False
    return bool((h[mask] == fill).all()) and int(mask.sum()) == guard * (len(words) + 1)


def test_batched_solver_keeps_every_image_inside_its_own_buffers():
    """Three images of 512, 65 and 1 rows on id tables of 16 entries: the big frames start more ids than a table takes
    (record word 6, bit 0).  Guard words around each image's pool state, each of its eight output arrays and its record
    segment are untouched, and what is inside them is what the single launch writes."""
    import siammot_amd.ops as ops
    lib = ops.load_library()
    CAP, G, SENT, FSENT = 16, 64, -77777, -12345.0
    thr = E.THRESHOLDS[0]
    rs = np.random.RandomState(16)
    images = []
    for M in (512, 65, 1):
        pool, strangers = E.make_pool(rs, 6, 3, 3)
        images.append((pool, E.make_frame(rs, pool, strangers, M)))
    B = len(images)
    ptr = np.zeros((18, B), np.uint64)
    ints = np.zeros((4, B), np.int32)
    flt = np.zeros((5, B), np.float32)
    rec_words = [ops.FrameBuffers.record_words(len(f["ids"]), CAP) for _, f in images]
    rec, rec_offs = _guarded(rec_words, torch.int32, G, SENT)
    keep, per_image, singles = [], [], []
    for b, (pool, f) in enumerate(images):
        M, n_det = len(f["ids"]), f["n_det"]
        seg = lambda a, z: [torch.from_numpy(f[k][a:z].copy()).to(DEV) for k in ("boxes", "raw", "ids", "labels")]
        det, trk = (seg(0, n_det) if n_det else None), (seg(n_det, M) if n_det < M else None)
        h0 = E.state_array(pool, CAP)
        state, st_off = _guarded([len(h0)], torch.int32, G, SENT)
        state[st_off[0]:st_off[0] + len(h0)] = torch.from_numpy(h0).to(DEV)
        fw, iw = [4 * M, 4 * M, M, M], [M, M, M, M]
        fbuf, fo = _guarded(fw, torch.float32, G, FSENT)     # out_boxes, act_boxes, out_scores, act_scores
        ibuf, io = _guarded(iw, torch.int64, G, SENT)        # out_ids, out_labels, act_ids, act_labels
        for k, s_ in enumerate((det, trk)):
            if s_ is not None:
                ptr[4 * k:4 * k + 4, b] = [t.data_ptr() for t in s_]
        fp, ip = fbuf.data_ptr(), ibuf.data_ptr()
        ptr[8, b] = state.data_ptr() + 4 * st_off[0]
        ptr[9:17, b] = [fp + 4 * fo[0], fp + 4 * fo[2], ip + 8 * io[0], ip + 8 * io[1], fp + 4 * fo[1], ip + 8 * io[2],
                        ip + 8 * io[3], fp + 4 * fo[3]]
        ptr[17, b] = rec.data_ptr() + 4 * rec_offs[b]
        ints[:, b] = n_det, M - n_det, 3, CAP
        flt[:, b] = 1.0, thr[0], thr[1], thr[2], 0.5
        keep.append((det, trk, state, fbuf, ibuf))
        per_image.append((state, st_off, len(h0), fbuf, fo, fw, ibuf, io, iw))
        # the single launch on copies of the same inputs
        cp = lambda s_: None if s_ is None else tuple(t.clone() for t in s_)
        st1 = torch.from_numpy(h0).to(DEV)
        f1, i1, r1, _ = ops.track_solve(cp(det), cp(trk), 1.0, thr, 0.5, 3, st1, CAP)
        singles.append((st1, f1, i1, ops.track_solve_record(r1)))
    row = lambda a, k: a.ctypes.data + k * a.strides[0]
    P, I, F = (lambda k: row(ptr, k)), (lambda k: row(ints, k)), (lambda k: row(flt, k))
    rc = lib.smot_track_solve_batched_fwd(B, P(0), P(1), P(2), P(3), I(0), P(4), P(5), P(6), P(7), I(1), F(0), F(1), F(2), F(3),
                                          F(4), I(2), P(8), I(3), *[P(k) for k in range(9, 18)], ops._stream(torch.device(DEV)))
    assert rc == 0, lib.smot_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(rec, rec_offs, rec_words, G, SENT)
    recs = rec.cpu().numpy()
    overflowed = 0
    for b, (state, st_off, ns, fbuf, fo, fw, ibuf, io, iw) in enumerate(per_image):
        where = "image %d" % b
        assert _guards_intact(state, st_off, [ns], G, SENT), where
        assert _guards_intact(fbuf, fo, fw, G, FSENT), where
        assert _guards_intact(ibuf, io, iw, G, SENT), where
        st1, f1, i1, r1 = singles[b]
        M = len(images[b][1]["ids"])
        r = recs[rec_offs[b]:rec_offs[b] + rec_words[b]]
        assert _written(r) == _written(r1), where
        K, A = int(r[0]), int(r[1])
        assert torch.equal(state[st_off[0]:st_off[0] + ns], st1), where
        one = ops.FrameBuffers(f1, i1, M)
        got_f = [fbuf[fo[0]:fo[0] + 4 * K].view(K, 4), fbuf[fo[2]:fo[2] + K], fbuf[fo[1]:fo[1] + 4 * A].view(A, 4), fbuf[fo[3]:fo[3] + A]]
        got_i = [ibuf[io[0]:io[0] + K], ibuf[io[1]:io[1] + K], ibuf[io[2]:io[2] + A], ibuf[io[3]:io[3] + A]]
        kb, ki, ks, kl = one.kept(K)
        ab, ai, as_, al = one.active(A)
        for x, y in zip(got_f + got_i, [kb, ks, ab, as_, ki, kl, ai, al]):
            assert torch.equal(x, y), where
        overflowed += int(r[6]) & 1
    assert overflowed >= 1                       # (a condition on the input: a frame that does not fit its tables is among them)


def test_a_chain_as_deep_as_the_frame_among_other_images():
    """The fixed-point loop of the middle image runs 512 rounds while its neighbours are long done: nothing of one
    workgroup's progress reaches another."""
    from siammot_amd.solver import TrackPool, TrackSolver, solve_batched
    cams = (CAMERAS[2], None, CAMERAS[4])
    chain = E.chain_frame(512, "permuted", seed=512)
    frames = [E.case(*cams[0])[2][0], chain, E.case(*cams[2])[2][0]]
    pools = [copy.deepcopy(E.case(*cams[0])[0]), TrackPool(max_dormant_frames=3), copy.deepcopy(E.case(*cams[2])[0])]
    twins = copy.deepcopy(pools)
    thr = [E.THRESHOLDS[cams[0][4]], E.THRESHOLDS[1], E.THRESHOLDS[cams[2][4]]]
    segs = [_segments(f, "two") for f in frames]
    outs = solve_batched([TrackSolver(p, *t) for p, t in zip(pools, thr)], [s[0] for s in segs], [s[1] for s in segs], 1.0)
    kept = outs[1].bbox.cpu().numpy()
    assert sorted((kept[:, 0] / 30).astype(int).tolist()) == list(range(0, 512, 2))          # its even positions, exactly
    for b in range(3):
        det, trk = _segments(frames[b], "two")
        want = TrackSolver(twins[b], *thr[b]).solve(det, trk, 1.0)
        _same_rows(outs[b], want, "image %d" % b)
        _same_rows(outs[b].active_rows, want.active_rows, "image %d" % b)
        _same_pool(pools[b], twins[b], "image %d" % b)
        assert torch.equal(pools[b]._dev_state, twins[b]._dev_state)


# ---- the loop -----------------------------------------------------------------------------------------------------------
def _cfg():
    from siammot_amd.config import get_default_cfg
    cfg = get_default_cfg(channels=32)
    cfg.MODEL.TRACK_HEAD.MAX_DORMANT_FRAMES = 2
    cfg.MODEL.TRACK_HEAD.TRACK_THRESH = 0.35
    cfg.MODEL.TRACK_HEAD.RESUME_TRACK_THRESH = 0.5
    return cfg


def _loops(B, refine=False):
    """(the multi-camera loop, B independent loops) on one set of weights, the predictor's scaled by 20."""
    import siammot_amd.ops as ops
    from siammot_amd.multi_camera import build_multi_camera_tracking_loop
    from siammot_amd.track_head import build_tracking_loop
    cfg = _cfg()
    multi = build_multi_camera_tracking_loop(cfg, B, device=DEV, refine_tracks=refine)
    with torch.no_grad():
        for name in ("cls", "center", "reg"):
            getattr(multi.emm.predictor, name).weight.mul_(20.0)
    # (the tower's filters are packed once per weight set, with a synchronisation of its own: here, not in a counted step)
    ops.tower_packed(multi.emm.predictor.param_dict())
    singles = [build_tracking_loop(cfg, device=DEV, refine_tracks=refine) for _ in range(B)]
    for lp in singles:
        lp.track.tracker.load_state_dict(multi.emm.state_dict())
    return multi, singles


@pytest.fixture(scope="module")
def maps():
    """Four sets of [3, 32, H_l, W_l] maps with different contents per camera (read-only)."""
    import golden_inputs as gi
    rs = np.random.RandomState(9)
    shapes = gi.feature_shapes((1280, 704), 32)
    return [tuple(torch.from_numpy(rs.standard_normal((3,) + tuple(s[1:])).astype(np.float32)).to(DEV) for s in shapes)
            for _ in range(4)]


def _starved(d, f):
    if f < 3 or 7 <= f < 11:
        d.add_field("scores", torch.full_like(d.get_field("scores"), 0.05))       # nothing starts; tracks starve
        d = d[:0] if f in (8, 9) else d                                           # ... and frames with no row at all
    return d


def _same_camera(multi, b, out, single, want, where):
    _same_rows(out, want, where)
    _same_pool(multi.solvers[b].track_pool, single.solver.track_pool, where)
    ma, mb = multi.track_memory[b], single.track_memory
    assert len(ma[2][0]) == len(mb[2][0]), where
    if len(mb[2][0]):
        assert torch.equal(ma[0], mb[0]), where                                    # templates
        assert torch.equal(ma[1][0].bbox, mb[1][0].bbox) and torch.equal(ma[2][0].bbox, mb[2][0].bbox), where
        assert torch.equal(ma[2][0].get_field("ids"), mb[2][0].get_field("ids")), where


def _run(multi, singles, maps_of, frames, dets_of, counted, expect_batched=True):
    import siammot_amd.ops as ops
    B = len(singles)
    seen = dict(dormant=False, killed=False, rowless=False)
    for f in range(frames):
        feats = maps_of(f)
        dets = [dets_of(b, f) for b in range(B)]
        had_rows = [len(dets[b]) > 0 or (multi.track_memory[b] is not None and len(multi.track_memory[b][2][0]) > 0) for b in range(B)]
        entry, syncs, fb = counted.entry, counted.syncs, ops.FALLBACKS["multi_camera_per_camera"]
        outs = multi(feats, [d.to(DEV) for d in dets])
        if expect_batched and any(had_rows):
            # one solver launch (B <= 16), one synchronisation, no camera-by-camera step
            assert (counted.entry, counted.syncs, ops.FALLBACKS["multi_camera_per_camera"]) == (entry + 1, syncs + 1, fb), f
        seen["rowless"] |= not all(had_rows) and any(had_rows)
        for b in range(B):
            want = singles[b](tuple(x[b:b + 1] for x in feats), dets_of(b, f).to(DEV))
            _same_camera(multi, b, outs[b], singles[b], want, "camera %d, frame %d" % (b, f))
            pool = multi.solvers[b].track_pool
            seen["dormant"] |= bool(pool._dormant_ids)
            seen["killed"] |= bool(pool._kill_ids)
    return seen


def _traffic(seeds, frames, starved=1):
    """dets_of(b, f): ``fake_tracker.detections`` of camera b's own stream, the same on every call for a (b, f)."""
    from fake_tracker import detections
    made = {}
    for b, seed in enumerate(seeds):
        rs = np.random.RandomState(seed)
        for f in range(frames):
            d = detections(rs, f)
            made[b, f] = _starved(d, f) if b == starved else d
    return lambda b, f: copy.deepcopy(made[b, f])


def test_multi_camera_loop_equals_independent_loops_with_the_real_head(maps):
    from fake_tracker import detections
    multi, singles = _loops(3)
    dets_of = _traffic((5, 6, 7), 40)
    with _Counted() as n:
        seen = _run(multi, singles, lambda f: maps[f % 4], 40, dets_of, n)
        assert seen["dormant"] and seen["killed"], seen
        # camera 1 restarts its video on a frame without detections: a camera without rows beside two with rows
        multi.reset(camera=1)
        singles[1].reset()
        rs = np.random.RandomState(77)
        last = {b: detections(rs, 3) for b in range(3)}
        last[1] = last[1][:0]
        seen = _run(multi, singles, lambda f: maps[0], 1, lambda b, f: copy.deepcopy(last[b]), n)
        assert seen["rowless"]
        # fp16 channels-last maps, all cameras from the start
        multi.reset()
        for lp in singles:
            lp.reset()
        half = [tuple(x.half().contiguous(memory_format=torch.channels_last) for x in m) for m in maps[:2]]
        _run(multi, singles, lambda f: half[f % 2], 12, dets_of, n)


def test_a_camera_beyond_the_solver_capacity_sends_one_step_camera_by_camera(maps):
    import siammot_amd.ops as ops
    from siammot_amd.structures import BoxList
    multi, singles = _loops(3)
    dets_of = _traffic((5, 6, 7), 4, starved=-1)
    gx, gy = np.meshgrid(np.arange(27), np.arange(19))
    x0, y0 = 10.0 + 45.0 * gx.reshape(-1), 10.0 + 35.0 * gy.reshape(-1)
    grid = BoxList(torch.from_numpy(np.stack((x0, y0, x0 + 40, y0 + 30), 1).astype(np.float32)), (1280, 704), mode="xyxy")
    grid.add_field("ids", torch.full((513,), -1, dtype=torch.int64))
    grid.add_field("labels", torch.ones(513, dtype=torch.int64))
    grid.add_field("scores", torch.full((513,), 0.3))                  # below the start threshold: no track comes of them
    assert len(grid) == 513
    pick = lambda b, f: copy.deepcopy(grid) if (b, f) == (0, 2) else dets_of(b, f)
    with _Counted() as n:
        for f in range(4):
            fb = ops.FALLBACKS["multi_camera_per_camera"]
            _run(multi, singles, lambda _f, f=f: maps[f % 4], 1, lambda b, _f, f=f: pick(b, f), n, expect_batched=f != 2)
            assert ops.FALLBACKS["multi_camera_per_camera"] == fb + (f == 2), f


def test_refinement_camera_by_camera_and_one_camera_restarting(maps):
    from siammot_amd.structures import BoxList

    def refine(features, tracks):
        assert features[0].shape[0] == 1
        t = tracks[0]
        out = BoxList(t.bbox + 1.0, t.size, mode=t.mode)
        out.add_field("ids", t.get_field("ids"))
        out.add_field("labels", t.get_field("labels"))
        out.add_field("scores", 1.0 + 0.5 * t.get_field("scores"))
        return [out]
    multi, singles = _loops(3, refine=refine)
    dets_of = _traffic((5, 6, 7), 10, starved=-1)
    with _Counted() as n:
        _run(multi, singles, lambda f: maps[f % 4], 6, dets_of, n)
        assert multi.solvers[2].track_pool._max_id >= 0
        multi.reset(camera=2)
        singles[2].reset()
        assert multi.solvers[2].track_pool._max_id == -1 and multi.solvers[0].track_pool._max_id >= 0
        _run(multi, singles, lambda f: maps[(f + 6) % 4], 4, lambda b, f: dets_of(b, f + 6), n)
