"""CPU: sessions that join and leave a running batcher -- serving.RowPool against a bitmap model, slot and row reuse in a LipBatcher with a fake generator
(max_sessions= / pool_rows=), vacant slots in a step, and add_session / flush / remove_session of the schedulers on injected clocks and events: a leaver's rows
stay allocated until its last batch in flight has retired.  Nothing here needs a device."""
import random

import numpy as np
import pytest
import torch

from mere_fusion_amd import lip_driver as D
from mere_fusion_amd import serving as S
from serving_fakes import FakeRing

B = 2
COUNTS = (3, 4, 5)


# ---- RowPool -------------------------------------------------------------------------------------------------------------------------------------------
class BitmapPool:
    """the brute-force model: one flag per row, alloc scans for the lowest run of n free rows"""

    def __init__(self, capacity):
        self.used_rows, self.ranges = [False] * capacity, {}

    def alloc(self, n):
        run = 0
        for i, u in enumerate(self.used_rows):
            run = 0 if u else run + 1
            if run == n:
                off = i - n + 1
                self.used_rows[off:i + 1] = [True] * n
                self.ranges[off] = n
                return off
        return None

    def free(self, off):
        n = self.ranges.pop(off)
        self.used_rows[off:off + n] = [False] * n

    def largest_gap(self):
        best = run = 0
        for u in self.used_rows:
            run = 0 if u else run + 1
            best = max(best, run)
        return best


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_pool_equals_a_bitmap_model_over_random_operations(seed):
    rng = random.Random(seed)
    pool, model = S.RowPool(64), BitmapPool(64)
    refused = 0
    for _ in range(400):
        if model.ranges and rng.random() < 0.45:
            off = rng.choice(sorted(model.ranges))
            model.free(off)
            pool.free(off)
        else:
            n = rng.randint(1, 12)
            want = model.alloc(n)
            if want is None:
                refused += 1
                with pytest.raises(RuntimeError, match=f"RowPool: no gap of {n} rows: the largest free gap has {model.largest_gap()} of 64"):
                    pool.alloc(n)
            else:
                assert pool.alloc(n) == want
        assert pool.used() == sum(model.used_rows) and pool.largest_gap() == model.largest_gap() and pool.taken == model.ranges
        assert pool.gaps == sorted(pool.gaps) and all(a + n < b for (a, n), (b, _) in zip(pool.gaps, pool.gaps[1:]))      # sorted, coalesced
    assert refused > 0                                                   # the sequence did reach a pool too full or too fragmented


def test_row_pool_takes_the_lowest_gap_coalesces_and_refuses_when_fragmented():
    p = S.RowPool(12)
    assert [p.alloc(3), p.alloc(3), p.alloc(3), p.alloc(3)] == [0, 3, 6, 9] and p.largest_gap() == 0
    p.free(3)
    p.free(9)
    assert p.used() == 6 and p.largest_gap() == 3
    with pytest.raises(RuntimeError, match="no gap of 4 rows: the largest free gap has 3 of 12 rows"):      # 6 rows free, no 4 together: no compaction
        p.alloc(4)
    assert p.alloc(2) == 3 and p.alloc(1) == 5 and p.alloc(2) == 9      # the LOWEST gap that fits, each time
    p.free(3), p.free(5), p.free(6)                                      # neighbours on both sides join: [3, 9)
    assert p.gaps == [(3, 6), (11, 1)] and p.alloc(6) == 3
    with pytest.raises(RuntimeError, match="free\\(4\\): no range starts there"):
        p.free(4)
    with pytest.raises(RuntimeError):
        S.RowPool(0)


# ---- a LipBatcher whose sessions come and go (fake generator, CPU tensors) ----------------------------------------------------------------------------------
class FakeModel:
    def __init__(self):
        self.calls = []

    def parameters(self):
        yield torch.zeros(1)

    def forward_u8_rows(self, mel, pool, rows):
        self.calls.append(list(rows))
        return pool[torch.tensor(rows)].float()


class FakeAvatar:
    H, W = 4, 6

    def __init__(self, n):
        self.n = n

    def paste(self, res, indices):
        return res.to(torch.uint8)

    def source(self, i):
        return ("cached", i)


def _faces(s, n):
    return torch.stack([torch.full((96, 96, 3), 16 * s + i, dtype=torch.uint8) for i in range(n)])


def _session(m, s, n, paste=False):
    return D.LipSession(m, _faces(s, n), avatar_frames=FakeAvatar(n) if paste else None)


def _mel():
    return torch.zeros(B, 1, 80, 16)


def _batcher(paste=False, **kw):
    m = FakeModel()
    sessions = [_session(m, s, n, paste) for s, n in enumerate(COUNTS)]
    return m, sessions, D.LipBatcher(m, sessions, batch_size=B, paste=paste, device="cpu", **kw)


def test_without_max_sessions_nothing_changes_and_add_session_refuses():
    m, sessions, bat = _batcher()
    assert bat.sessions == sessions and all(a is b for a, b in zip(bat.sessions, sessions))
    assert [s.pool_offset for s in sessions] == [0, 3, 7] and bat.row_pool is None and bat.live() == [0, 1, 2]
    assert torch.equal(bat.pool, torch.cat([s.faces for s in sessions])) and bat.pool.shape[0] == 12
    with pytest.raises(RuntimeError, match="LipBatcher: add_session: .*fixed list of sessions.*max_sessions="):
        bat.add_session(_session(m, 3, 2))
    with pytest.raises(RuntimeError, match="LipBatcher: remove_session: .*max_sessions="):
        bat.remove_session(0)
    assert bat.sessions == sessions
    sch = S.SessionScheduler(bat, clock=lambda: 0.0, sync=lambda: None)
    with pytest.raises(RuntimeError, match="max_sessions="):
        sch.add_session(_session(m, 3, 2))


def test_joiners_take_the_lowest_vacant_slot_and_the_lowest_gap():
    m, sessions, bat = _batcher(max_sessions=5, pool_rows=16, max_sessions_per_step=3)
    ptr = bat.pool.data_ptr()
    assert bat.sessions == sessions + [None, None] and [s.pool_offset for s in sessions] == [0, 3, 7]      # the offsets of the concatenation
    assert bat.pool.shape == (16, 96, 96, 3) and torch.equal(bat.pool[:12], torch.cat([s.faces for s in sessions])) and bat.live() == [0, 1, 2]
    c = _session(m, 3, 2)
    assert bat.add_session(c) == 3 and c.pool_offset == 12 and torch.equal(bat.pool[12:14], c.faces)
    assert bat.remove_session(1) is sessions[1] and sessions[1].pool_offset is None and bat.live() == [0, 2, 3] and bat.row_pool.used() == 10
    d = _session(m, 4, 3)
    assert bat.add_session(d) == 1 and d.pool_offset == 3                # slot 1 before slot 4; rows [3, 6) before the tail
    e = _session(m, 5, 2)
    assert bat.add_session(e) == 4 and e.pool_offset == 14               # 1 row free at 6, 2 at 14
    out = bat.step([None, _mel(), None, None, _mel()])
    assert m.calls[-1] == [3, 4, 14, 15] and [int(f[0, 0, 0]) for f in out[1][0]] == [64, 65] and [int(f[0, 0, 0]) for f in out[4][0]] == [80, 81]
    # refusals change nothing: a full batcher, rows that fit nowhere, crops of the wrong type, a frame cache of another length
    state = lambda: ([None if s is None else (id(s), s.pool_offset) for s in bat.sessions], dict(bat.row_pool.taken), bat.pool.clone())
    before = state()
    with pytest.raises(RuntimeError, match="all 5 session slots are taken"):
        bat.add_session(_session(m, 6, 1))
    bat.remove_session(4)
    before = state()
    for bad, text in ((_session(m, 6, 4), "no gap of 4 rows: the largest free gap has 2 of 16 rows"), (D.LipSession(m, _faces(6, 2).float()), "session 4: .*uint8"),
                      (D.LipSession(m, _faces(6, 2), avatar_frames=FakeAvatar(3)), "session 4: one cached full frame")):
        with pytest.raises(RuntimeError, match=text):
            bat.add_session(bad)
        after = state()
        assert after[:2] == before[:2] and torch.equal(after[2], before[2]) and bad.pool_offset is None
    with pytest.raises(RuntimeError, match="remove_session\\(4\\): no session there"):
        bat.remove_session(4)
    assert bat.pool.data_ptr() == ptr
    with pytest.raises(RuntimeError, match="pool_rows=11: the 3 initial sessions have 12 rows"):
        _batcher(pool_rows=11)
    with pytest.raises(RuntimeError, match="max_sessions=2 for 3 initial sessions"):
        _batcher(max_sessions=2)
    assert _batcher(max_sessions=4)[2].pool.shape[0] == 12               # pool_rows defaults to what the initial sessions need


def test_a_vacant_slot_is_absent_from_a_step_and_refused_before_any_index_moves():
    m, sessions, bat = _batcher(max_sessions=4, pool_rows=16)
    bat.remove_session(1)
    for kw, text in ((dict(mel_chunks=[_mel(), None, _mel(), None], only=[0, 1]), "slots \\[1\\] are vacant"),
                     (dict(mel_chunks=[_mel(), None, _mel(), None], only=[3]), "slots \\[3\\] are vacant"),
                     (dict(mel_chunks=[_mel(), _mel(), _mel(), None]), "slots \\[1\\] are vacant: their entries must be None"),
                     (dict(mel_chunks=[_mel(), None, _mel(), _mel()], only=[0]), "slots \\[3\\] are vacant: their entries must be None"),
                     (dict(mel_chunks=[_mel(), None, _mel()]), "3 entries for 4 sessions")):
        with pytest.raises(RuntimeError, match=text):
            bat.step(**kw)
        assert [s.index for s in sessions] == [0, 0, 0] and not m.calls, kw
    out = bat.step([_mel(), None, None, None])                           # only=None: every LIVE session; the vacant slots have no entry
    assert out[1] is None and out[3] is None and out[0][1] == [0, 1] and out[2] == (None, [0, 1]) and m.calls == [[0, 1]]


# ---- schedulers ----------------------------------------------------------------------------------------------------------------------------------------------
class Events:
    """torch.cuda.Event for a box without a device, completed by the test: `finish()` completes every event recorded so far"""

    def __init__(self, monkeypatch):
        self.all = []
        outer = self

        class Event:
            def __init__(self, *a, **k):
                self.done = False
                outer.all.append(self)

            def record(self, *a):
                pass

            def query(self):
                return self.done

            def synchronize(self):
                self.done = True

        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: None)

    def finish(self):
        for e in self.all:
            e.done = True


def test_session_scheduler_add_flush_remove_and_slot_reuse():
    m, sessions, bat = _batcher(max_sessions=4, pool_rows=16, max_sessions_per_step=4)
    now = [0.0]
    sch = S.SessionScheduler(bat, clock=lambda: now[0], hold_s=0.0, sync=lambda: None)
    assert [q is not None for q in sch.queues] == [True, True, True, False]
    with pytest.raises(RuntimeError, match="submit\\(3\\): no session there \\(live sessions: \\[0, 1, 2\\]\\)"):
        sch.submit(3, _mel())
    with pytest.raises(RuntimeError, match="flush\\(3\\): no session there"):
        sch.flush(3)
    with pytest.raises(RuntimeError, match="ring=None, frontend=None"):
        sch.add_session(_session(m, 3, 2), ring=FakeRing(4))
    assert bat.live() == [0, 1, 2]
    c = _session(m, 3, 2)
    assert sch.add_session(c) == 3 and bat.sessions[3] is c and len(sch.queues[3]) == 0
    for j in range(3):
        sch.submit(3, _mel(), 0.1 * j)
    sch.submit(0, _mel(), 0.05)
    now[0] = 1.0
    done = sch.run_once()
    assert sorted(k for k, *_ in done) == [0, 3] and c.index == B and sch.backlog() == 2
    assert sch.flush(3) == 2 and c.index == B and sch.flush(3) == 0 and sch.pending() == {} and sch.next_due() is None       # the walk has not moved for them
    sch.submit(3, _mel(), 1.0)
    sch.remove_session(3)                                                # nothing in flight in this scheduler: released at once, the queued batch dropped
    assert bat.sessions[3] is None and sch.queues[3] is None and c.pool_offset is None and sch.run_once(2.0) == [] and sch.backlog() == 0
    sch.remove_session(0)
    d = _session(m, 4, 3)
    assert sch.add_session(d) == 0 and d.pool_offset == 0                # the lowest vacant slot, and session 0's old rows
    sch.submit(0, _mel(), 2.0)
    (k, fr, idx, lat), = sch.run_once(3.0)
    assert k == 0 and idx == [0, 1] and [int(f[0, 0, 0]) for f in fr] == [64, 65]


def test_remove_session_keeps_the_rows_until_the_last_batch_in_flight_has_retired(monkeypatch):
    events = Events(monkeypatch)
    m, sessions, bat = _batcher(max_sessions=4, pool_rows=16, max_sessions_per_step=4)
    now = [0.0]
    sch = S.PipelinedScheduler(bat, clock=lambda: now[0], hold_s=0.0, depth=2)                   # rings=None: no stream, no device
    for j in range(3):
        sch.submit(0, _mel(), 0.01 * j)
    sch.submit(1, _mel(), 0.0)
    now[0] = 1.0
    assert sch.run_once() == [] and sch.run_once() == [] and len(sch.inflight) == 2              # two steps in flight, both with a batch of session 0
    assert sessions[0].index == 2 * B and len(sch.queues[0]) == 1
    sch.remove_session(0)                                                                        # the queued batch is dropped, the two in flight are not
    assert sch.leaving == {0} and sch.queues[0] is not None and len(sch.queues[0]) == 0
    assert bat.sessions[0] is sessions[0] and sessions[0].pool_offset == 0 and bat.row_pool.taken == {0: 3, 3: 4, 7: 5}
    for what in (lambda: sch.submit(0, _mel()), lambda: sch.flush(0), lambda: sch.remove_session(0)):
        with pytest.raises(RuntimeError, match="the session is leaving"):
            what()
    joiner = _session(m, 3, 3)
    assert sch.add_session(joiner) == 3 and joiner.pool_offset == 12                             # NOT slot 0, NOT rows [0, 3): a step may still read them
    assert sch.run_once() == [] and sch.leaving == {0}                                           # nothing has completed yet
    events.finish()
    done = sch.run_once()
    assert [k for k, *_ in done].count(0) == 2 and [idx for k, _, idx, _ in done if k == 0] == [[0, 1], [2, 2]]      # both batches in flight are delivered
    assert sch.leaving == set() and sch.queues[0] is None and bat.sessions[0] is None and bat.row_pool.taken == {3: 4, 7: 5, 12: 3}
    with pytest.raises(RuntimeError, match="submit\\(0\\): no session there"):
        sch.submit(0, _mel())
    late = _session(m, 4, 2)
    assert sch.add_session(late) == 0 and late.pool_offset == 0                                  # now the slot and the rows are free
    sch.submit(0, _mel(), 1.0)
    sch.run_once(2.0)
    assert [k for k, *_ in sch.drain()] == [0] and m.calls[-1] == [0, 1]
    sch.close()


class FakeCustomVideos:
    def __init__(self):
        self.custom_index, self.lengths, self.checked = {2: 0}, {2: 5}, []

    def check_size(self, H, W, who):
        self.checked.append((H, W, who))

    def source(self, ty, j):
        return ("custom", ty, j)


def test_flush_drops_only_unpicked_batches_and_leaves_the_walks_alone(monkeypatch):
    from mere_fusion_amd import ops
    events = Events(monkeypatch)
    gathered = []
    monkeypatch.setattr(ops, "gather_frames", lambda srcs, dst, out, fmt, order: gathered.append((list(srcs), list(dst))))
    m, sessions, bat = _batcher(paste=True, max_sessions=4, pool_rows=16, max_sessions_per_step=4)
    cv = FakeCustomVideos()
    sessions[0].custom_videos = cv
    rings = [FakeRing(8 * B), FakeRing(8 * B), FakeRing(8 * B), None]
    now = [0.0]
    sch = S.PipelinedScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, depth=2, single_stream=True, idle_frames=True)
    assert sch.rings is not rings and sch.rings == rings
    custom = [(np.zeros(4, np.float32), 2)] * (2 * B)                                            # a custom video's audio: B frames of the custom walk per batch
    for j in range(4):
        sch.submit(0, None, 0.01 * j, pairs=custom)
    sch.submit(1, _mel(), 0.0, pairs=[(np.zeros(4, np.float32), 0)] * (2 * B))
    now[0] = 1.0
    assert sch.run_once() == []                                                                  # one batch of session 0 is picked and in flight ...
    assert sessions[0].index == B and cv.custom_index == {2: B} and gathered[0] == ([("custom", 2, 0), ("custom", 2, 1)], [0, 1])
    assert sch.flush(0) == 3                                                                     # ... three are dropped
    assert sessions[0].index == B and cv.custom_index == {2: B} and sch.flush(0) == 0 and sch.flush(1) == 0
    events.finish()
    done = sch.run_once()
    assert sorted(k for k, *_ in done) == [0, 1] and len(rings[0].msgs) == B and [msg[1] for msg in rings[0].msgs] == [0, 1]      # the batch in flight is delivered
    sch.submit(0, None, 2.0, pairs=custom)                                                       # the session talks on from where it was
    now[0] = 3.0
    sch.run_once()
    assert sessions[0].index == 2 * B and cv.custom_index == {2: 2 * B} and gathered[-1][0] == [("custom", 2, 2), ("custom", 2, 3)]
    # a joiner's ring and custom videos are checked as the constructor checks them, before anything is stored
    with pytest.raises(RuntimeError, match="a ring per session"):
        sch.add_session(_session(m, 3, 2, paste=True))
    with pytest.raises(RuntimeError, match="idle_frames=True: session 3 has no AvatarFrames"):
        sch.add_session(_session(m, 3, 2), ring=FakeRing(4))
    assert bat.live() == [0, 1, 2] and sch.rings[3] is None and sch.queues[3] is None
    joiner, ring = _session(m, 3, 2, paste=True), FakeRing(4 * B)
    joiner.custom_videos = FakeCustomVideos()
    assert sch.add_session(joiner, ring=ring) == 3 and sch.rings[3] is ring and joiner.custom_videos.checked == [(4, 6, "PipelinedScheduler: session 3")]
    events.finish()
    sch.drain()
    sch.remove_session(3)
    assert sch.rings[3] is None and bat.sessions[3] is None
    sch.close()


def test_i420_joiner_needs_a_ring_of_its_frames_planes():
    """the per-session half of _check_frame_format, with the constructor's words"""
    S.PipelinedScheduler._check_session_format(2, type("R", (), {"frame_shape": (6, 6)})(), (4, 6))          # the right ring: accepted
    with pytest.raises(RuntimeError, match="PipelinedScheduler: frame_format='i420': ring 2 has slots of shape \\(4, 6, 3\\); session 2's 4 x 6 frames need \\(6, 6\\)"):
        S.PipelinedScheduler._check_session_format(2, type("R", (), {"frame_shape": (4, 6, 3)})(), (4, 6))
    with pytest.raises(RuntimeError, match="session 2's frames are 5 x 6 \\(H x W\\); 4:2:0 needs even sizes"):
        S.PipelinedScheduler._check_session_format(2, type("R", (), {"frame_shape": (6, 6)})(), (5, 6))
    with pytest.raises(RuntimeError, match="ring 2 has slots of shape \\(4, 6, 3\\), which is no"):
        S.PipelinedScheduler._check_session_format(2, type("R", (), {"frame_shape": (4, 6, 3)})(), None)


def test_lip_scheduler_needs_a_window_for_every_slot():
    m, sessions, bat = _batcher(max_sessions=4, pool_rows=16)
    with pytest.raises(RuntimeError, match="no CPU path"):                                      # the dynamic window pool pushes through mf_windows_push
        bat.frontends()
    pool = D.LipWindowPool(3, B, device="cpu")
    with pytest.raises(RuntimeError, match="needs a window for every slot: LipWindowPool\\(..., max_sessions=4\\)"):
        D.LipEndToEndScheduler(bat, [D.LipASRDeviceFrontend(pool, k) for k in range(3)] + [None])
    with pytest.raises(RuntimeError, match="max_sessions=2 for 3 sessions"):
        D.LipWindowPool(3, B, device="cpu", max_sessions=2)
