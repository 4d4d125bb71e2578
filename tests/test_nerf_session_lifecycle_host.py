"""CPU: ER-NeRF sessions that join and leave a running batcher (mere_fusion_amd/nerf_serving.py with max_sessions=) -- the feature pool's rows that are taken
and given back, with the three launches replaced by restatements of what include/merefusion.h says they do (the two of tests/test_nerf_serving_host.py and
the new mf_nerf_feat_rows_load); `NerfBatcher`'s slots with the stand-in sessions of that file; `NerfEndToEndScheduler` on injected clocks and events: a
leaver's pool row and slot stay taken until its last batch in flight has retired; and the C ABI of the new entry (header, exports, ctypes table, argument
checks that never launch).  Nothing here needs a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import nerf_serving_util as U
from serving_fakes import FakeRing
from nerf_featpool_ref import emu_rows_load as _emu_rows_load, emu_scatter as _emu_scatter, emu_windows as _emu_windows
from test_nerf_serving_host import FakeModel, FakeSession, _inp
from test_session_lifecycle_host import Events

B = 4
DIM = 5


# ---- the three launches, restated from the header (host tensors): tests/nerf_featpool_ref.py ---------------------------------------------------------
@pytest.fixture
def host_ops(monkeypatch):
    from mere_fusion_amd import nerf_serving as S
    calls = []
    monkeypatch.setattr(S.ops, "nerf_feat_scatter", lambda *a, **k: (calls.append(("scatter", list(a[4]), list(a[5]))), _emu_scatter(*a, **k))[1])
    monkeypatch.setattr(S.ops, "nerf_feat_windows", lambda *a, **k: (calls.append(("windows", list(a[2]), list(a[5]))), _emu_windows(*a, **k))[1])
    monkeypatch.setattr(S, "host_rows_load", lambda *a, **k: (calls.append(("rows_load", list(a[2]), len(a) > 3 and a[3] is not None)), _emu_rows_load(*a, **k))[1])
    return calls


class BiasNet(U.StubNet):
    """the stub net plus a value per net frame, so that silence does not come out as zeros and a warmed-up ring differs from a reset one; still elementwise"""

    def __call__(self, x):
        res = super().__call__(x)
        t = res.last_hidden_state if self.hidden else res.logits
        t += 1.0 + 0.5 * torch.arange(t.shape[1], dtype=torch.float32)[None, :, None]
        return res


def _blocks(ks, step):
    return [sum((U.pcm(k, B * step + b) for b in range(B)), []) for k in ks]


def _host_state(pool, k):
    return (U.pool_counters(pool, k), pool.head[k], pool.first[k], list(pool.win_fronts[k]), pool.pcm[k].copy())


def _same_state(a, b):
    return a[:4] == b[:4] and np.array_equal(a[4], b[4])


# ---- the pool --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("att", [2, 0])
def test_a_row_that_joins_at_a_step_boundary_is_a_warmed_up_session(host_ops, att):
    """Three live rows of a four-row pool run 40 frames (ten steps of B = 4); row 3 joins after the fifth step.  Its next 12 frames of `auds` are those of a fresh
    one-row pool after warm_up() fed the same chunks, the other rows' outputs are those of a run without the join, and the join is one rows_load launch and no
    net call.  The stub net is elementwise, so a window's rows are the same bits whatever else shares the call."""
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    net = BiasNet(DIM, "cpu")
    pool = NerfFeaturePool(3, net, DIM, att=att, device="cpu", max_sessions=4)
    assert pool.n_sessions == 4 and pool.live() == [0, 1, 2] and pool.vacant == {3} and pool.rings.shape[0] == 5 and pool.scratch == 4
    pool.warm_up()
    assert net.calls == [3, 3]
    pool.warm_state()
    assert net.calls == [3, 3, 1, 1]                                    # exactly what warm_up([row]) runs: S = 1 net calls, on the scratch row
    plain = NerfFeaturePool(3, BiasNet(DIM, "cpu"), DIM, att=att, device="cpu")
    plain.warm_up()
    alone = NerfFeaturePool(1, BiasNet(DIM, "cpu"), DIM, att=att, device="cpu")
    alone.warm_up()
    joined = 0
    for step in range(10):
        if step == 5:
            n_net, n_launch = len(net.calls), pool.launches
            del host_ops[:]
            assert pool.join([3]) == [3]
            assert host_ops == [("rows_load", [3], True)] and len(net.calls) == n_net and pool.launches == n_launch + 1
            assert pool.live() == [0, 1, 2, 3] and _same_state(_host_state(pool, 3), _host_state(alone, 0))
            assert torch.equal(pool.rings[3], alone.rings[0]) and (att == 0 or torch.equal(pool.hist[3], alone.hist[0]))
        ks = [0, 1, 2] if step < 5 or step >= 8 else [0, 1, 2, 3]
        want = plain.step([0, 1, 2], _blocks([0, 1, 2], step), B)
        del host_ops[:]
        got = pool.step(ks, _blocks([0, 1, 2], step) + (_blocks([3], step - 5) if 3 in ks else []), B)
        assert torch.equal(got[:3], want), step
        assert [c[0] for c in host_ops] == ["windows", "windows", "scatter", "windows", "windows"] and host_ops[2][1] == ks     # the joiner is in phase
        if 3 in ks:
            assert torch.equal(got[3], alone.step([0], _blocks([3], step - 5), B)[0]), step
            assert U.pool_counters(pool, 3) == U.pool_counters(alone, 0)
            joined += B
    assert joined == 12 and float(got.abs().max()) > 0.5


def test_warm_state_is_computed_once_however_many_joins_follow(host_ops):
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    net = BiasNet(DIM, "cpu")
    pool = NerfFeaturePool(1, net, DIM, device="cpu", max_sessions=3)
    assert pool._warm is None and net.calls == []
    pool.join([1])                                                       # lazily, at the first join
    assert net.calls == [1, 1] and pool._warm is not None
    w = pool.warm_state()
    ring, hist = pool.rings[pool.scratch].clone(), pool.hist[pool.scratch].clone()
    assert float(ring.abs().max()) > 0.5 and float(hist.abs().max()) == 0.0                    # (warm_up runs no get_next_feat: the history is still zeros)
    for rnd in range(3):
        pool.join([2])
        pool.step([1, 2], _blocks([1, 2], rnd), B)                       # the joined rows move on; the snapshot does not
        pool.leave(2)
        pool.leave(1)
        del host_ops[:]
        pool.join([2, 1])                                                # two rows, one launch
        assert host_ops == [("rows_load", [2, 1], True)]
        pool.leave(2)
        assert pool.warm_state() is w
        assert _same_state(_host_state(pool, 1), ((22, 2, 24, 8), 4, True, [-1] * 4, w["pcm"]))
        assert torch.equal(pool.rings[pool.scratch], ring) and torch.equal(pool.hist[pool.scratch], hist)
    assert net.calls[:2] == [1, 1] and all(n == 2 for n in net.calls[2:]) and len(net.calls) == 2 + 3
    # warm=False: the state NerfASR.__init__ leaves, through the same launch with no source
    fresh = NerfFeaturePool(1, BiasNet(DIM, "cpu"), DIM, device="cpu")
    pool.rings[2] = 7.0
    pool.hist[2] = 7.0
    del host_ops[:]
    pool.join([2], warm=False)
    assert host_ops == [("rows_load", [2], False)] and _same_state(_host_state(pool, 2), _host_state(fresh, 0))
    assert torch.equal(pool.rings[2], fresh.rings[0]) and torch.equal(pool.hist[2], fresh.hist[0])
    # reset() goes through that launch too, once for all its rows, with the results of the two zero_() calls per row it replaces
    pool.rings[:3] = 3.0
    pool.hist[:3] = 3.0
    del host_ops[:]
    assert pool.reset([1, 2]) == [1, 2]
    assert host_ops == [("rows_load", [1, 2], False)] and float(pool.rings[1:3].abs().max()) == 0.0 and float(pool.hist[1:3].abs().max()) == 0.0
    assert float(pool.rings[0].min()) == 3.0 and U.pool_counters(pool, 1) == (10, 0, 24, 8)


def test_a_vacant_row_is_refused_before_any_state_moves(host_ops):
    from mere_fusion_amd.nerf_serving import NerfASRDeviceFrontend, NerfFeaturePool
    net = BiasNet(DIM, "cpu")
    pool = NerfFeaturePool(2, net, DIM, device="cpu", max_sessions=3)
    pool.warm_up()
    pool.warm_state()
    state = lambda: [_host_state(pool, k) for k in range(4)]
    before, n_net = state(), len(net.calls)
    del host_ops[:]
    silence = np.zeros(U.CHUNK, np.float32)
    for what in (lambda: pool.step([0, 2], _blocks([0, 2], 0), B), lambda: pool.step([2], _blocks([2], 0), B), lambda: pool.next_feat([1, 2]),
                 lambda: pool.run_step([2, 0], [silence, silence]), lambda: pool.reset([2]), lambda: pool.warm_up(2),
                 lambda: NerfASRDeviceFrontend(pool, 2).get_next_feat()):
        with pytest.raises(RuntimeError, match=r"NerfFeaturePool.*rows \[2\] are vacant \(live rows: \[0, 1\]\)"):
            what()
        assert all(_same_state(a, b) for a, b in zip(state(), before)) and not host_ops and len(net.calls) == n_net
    for what, text in ((lambda: pool.step([3], _blocks([3], 0), B), "rows run from 0 to 2"),                 # the scratch row is never handed out
                       (lambda: pool.join([3]), "distinct rows from 0 to 2"), (lambda: pool.join([2, 2]), "distinct rows"), (lambda: pool.join([]), "distinct rows"),
                       (lambda: pool.join([1]), r"rows \[1\] hold a session \(vacant rows: \[2\]\)"), (lambda: pool.join([2, 0]), r"rows \[0\] hold a session"),
                       (lambda: pool.leave(2), r"row 2: no session there \(live rows: \[0, 1\]\)"), (lambda: pool.leave(3), "row 3: no session there")):
        with pytest.raises(RuntimeError, match="NerfFeaturePool.*" + text):
            what()
        assert all(_same_state(a, b) for a, b in zip(state(), before)) and not host_ops and pool.vacant == {2}
    with pytest.raises(RuntimeError, match="max_sessions=1 for 2 initial sessions"):
        NerfFeaturePool(2, net, DIM, device="cpu", max_sessions=1)
    # without max_sessions nothing changes, and the new entries refuse by name
    fixed = NerfFeaturePool(2, net, DIM, device="cpu")
    assert fixed.rings.shape[0] == 2 and fixed.n_sessions == 2 and fixed.live() == [0, 1] and fixed.vacant == set() and fixed.scratch is None
    for what in (lambda: fixed.join([1]), lambda: fixed.leave(1), lambda: fixed.warm_state()):
        with pytest.raises(RuntimeError, match=r"NerfFeaturePool: (join|leave|warm_state): .*fixed list of sessions.*max_sessions="):
            what()


# ---- NerfBatcher ---------------------------------------------------------------------------------------------------------------------------
class RenderingModel(FakeModel):
    def render_frames(self, jobs, **kw):
        raise AssertionError("never rendered here")


class BatchableSession(FakeSession):
    """a stand-in with the entry points of the batched and frame-batched routes (never stepped through them here): what a frame batch is sized for"""

    def __init__(self, model, value, render_hw, **kw):
        super().__init__(model, value, **kw)
        self.H, self.W = render_hw

    begin = end = bind_aabb = set_background = lambda self, *a, **k: None

    def out_key(self):
        return (self.H, self.W, self.GH, self.GW)

    def bg_key(self):
        return (self.H, self.W)


def _slots(bat):
    return [None if s is None else id(s) for s in bat.sessions], list(bat.out_shape), list(bat.enc_a)


def test_batcher_slots_joins_and_refusals():
    from mere_fusion_amd.nerf_serving import NerfBatcher
    shared = FakeModel()
    ss = [FakeSession(shared, 10), FakeSession(shared, 20), FakeSession(FakeModel(), 30)]
    bat = NerfBatcher(ss[:2], device="cpu", max_sessions=4)
    assert bat.sessions == ss[:2] + [None, None] and bat.out_shape == [(6, 4, 3)] * 2 + [None] * 2 and bat.enc_a == [None] * 4
    assert bat.live() == [0, 1] and bat.max_sessions_per_step == 4 and bat.vacant_slot() == 2
    most = bat._most_frames(shared)
    assert most == 16 == bat._most_frames(ss[2].model)                   # batch_size x max_sessions_per_step, whoever is present
    out = bat.step([_inp(1), _inp(2), None, None])
    assert out[2] is None and out[3] is None and bat.enc_a[0] is not None
    assert bat.add_session(ss[2]) == 2 and bat.live() == [0, 1, 2] and bat.out_shape[2] == (6, 4, 3) and bat._most_frames(shared) == most
    assert bat.remove_session(0) is ss[0] and bat.sessions[0] is None and bat.out_shape[0] is None and bat.enc_a[0] is None
    ema1 = bat.enc_a[1]
    bat.enc_a[0] = 99.0                                                  # (whatever a leaver's EMA left in the slot)
    late = FakeSession(shared, 40)
    assert bat.add_session(late) == 0 and bat.enc_a[0] is None and bat.enc_a[1] == ema1 and bat._most_frames(shared) == most      # the LOWEST vacant slot
    out = bat.step([_inp(3), None, None, None], only=[0])
    alone = FakeSession(FakeModel(), 40)
    want = torch.stack([alone.step(torch.full((8, 3, 16), 3.0)).clone() for _ in range(B)])
    assert torch.equal(out[0][0], want) and late.seen == alone.seen      # not smoothed against the leaver's EMA
    # a step leaves a vacant slot out and refuses it before any index moves
    for kw, text in ((dict(inputs=[_inp(1), _inp(1), _inp(1), _inp(1)]), r"slots \[3\] are vacant: their entries must be None"),
                     (dict(inputs=[_inp(1), None, None, None], only=[0, 3]), r"slots \[3\] are vacant")):
        idx = [s.index for s in (late, ss[1], ss[2])]
        with pytest.raises(RuntimeError, match=text):
            bat.step(**kw)
        assert [s.index for s in (late, ss[1], ss[2])] == idx
    # refusals store nothing: a custom-video frame of another size, a full batcher, a batcher built for a fixed list
    wrong = FakeSession(FakeModel(), 1, cycle={2: [torch.zeros(6, 4, 3, dtype=torch.uint8), torch.zeros(6, 5, 3, dtype=torch.uint8)]})
    before = _slots(bat)
    with pytest.raises(RuntimeError, match=r"NerfBatcher: session 3: custom_img_cycle\[2\] holds a 5 x 6 frame, the session's frames are 4 x 6"):
        bat.add_session(wrong)
    no_step = type("S", (), dict(model=FakeModel(), fullbody_frames=None, GH=6, GW=4, custom_img_cycle={}))()
    with pytest.raises(RuntimeError, match="session 3: neither begin / end / bind_aabb over a model with render_frames nor step"):
        bat.add_session(no_step)
    assert _slots(bat) == before
    assert bat.add_session(FakeSession(shared, 50)) == 3
    before = _slots(bat)
    with pytest.raises(RuntimeError, match="NerfBatcher: add_session: all 4 session slots are taken"):
        bat.add_session(FakeSession(shared, 60))
    with pytest.raises(RuntimeError, match=r"remove_session\(4\): no session there \(live sessions: \[0, 1, 2, 3\]\)"):
        bat.remove_session(4)
    assert _slots(bat) == before
    fixed = NerfBatcher(ss[:2], device="cpu")
    assert fixed.sessions == ss[:2] and fixed.enc_a == [None] * 2 and fixed.out_shape == [(6, 4, 3)] * 2 and fixed._most_frames(shared) == 0
    with pytest.raises(RuntimeError, match="NerfBatcher: add_session: .*fixed list of sessions.*max_sessions="):
        fixed.add_session(ss[2])
    with pytest.raises(RuntimeError, match="NerfBatcher: remove_session: .*max_sessions="):
        fixed.remove_session(0)
    assert fixed.sessions == ss[:2]
    with pytest.raises(RuntimeError, match="max_sessions=1 for 2 initial sessions"):
        NerfBatcher(ss[:2], device="cpu", max_sessions=1)
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="a feature pool of 2 rows for 4 sessions"):       # the pool has max_sessions rows
        NerfBatcher(ss[:2], device="cpu", max_sessions=4, pool=SimpleNamespace(n_sessions=2))


def test_a_joiner_with_more_pixels_than_the_frame_batch_holds_is_refused_with_that_number():
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m = RenderingModel()
    first = [BatchableSession(m, 1, (6, 4)), BatchableSession(m, 2, (3, 4)), FakeSession(FakeModel(), 3)]
    bat = NerfBatcher(first, device="cpu", max_sessions=5)
    assert bat.max_pixels == 24 and bat._most_frames(m) == 20            # the default: the largest initial session that takes the frame-batched route
    before = _slots(bat)
    with pytest.raises(RuntimeError, match=r"NerfBatcher: session 3: its frames are rendered at 5 x 5 = 25 pixels; the frame batch was sized for 24 .*max_pixels="):
        bat.add_session(BatchableSession(m, 4, (5, 5)))
    assert _slots(bat) == before
    assert bat.add_session(BatchableSession(m, 4, (4, 6))) == 3 and bat._most_frames(m) == 20
    big = FakeSession(FakeModel(), 5, hw=(60, 40))                       # a session on its own launches takes no place in the frame batch
    assert bat.add_session(big) == 4 and bat.out_shape[4] == (60, 40, 3)
    roomy = NerfBatcher(first, device="cpu", max_sessions=4, max_pixels=30)
    assert roomy.add_session(BatchableSession(m, 4, (5, 5))) == 3 and roomy.max_pixels == 30
    with pytest.raises(RuntimeError, match="max_pixels=20: an initial session renders 24 pixels per frame"):
        NerfBatcher(first, device="cpu", max_sessions=4, max_pixels=20)


# ---- the end-to-end scheduler ------------------------------------------------------------------------------------------------------------------
class ShapedRing(FakeRing):
    def __init__(self, places, frame_shape=(6, 4, 3)):
        super().__init__(places)
        self.frame_shape = tuple(frame_shape)


def _batch(k, j):
    return sum((U.pcm(k, B * j + b) for b in range(B)), [])


def _scheduler(n, clock, frame_format="packed", shape=(6, 4, 3)):
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfEndToEndScheduler, NerfFeaturePool
    net = U.StubNet(3, "cpu")
    pool = NerfFeaturePool(n, net, 3, device="cpu", max_sessions=4)
    pool.warm_up()
    ss = [FakeSession(FakeModel(), 10 * k) for k in range(n)]
    bat = NerfBatcher(ss, pool=pool, device="cpu", max_sessions=4)
    bat.prewarm()                                                        # the joiners' audio state is computed here, not at a join
    assert pool._warm is not None
    rings = [ShapedRing(8 * B, shape) for _ in range(n)] + [None] * (4 - n)
    return NerfEndToEndScheduler(bat, rings=rings, clock=clock, hold_s=0.0, depth=2, single_stream=True, frame_format=frame_format), pool, bat, ss, net


def test_a_leaver_keeps_its_row_and_slot_until_its_last_batch_in_flight_has_retired(host_ops, monkeypatch):
    events = Events(monkeypatch)
    now = [0.0]
    sch, pool, bat, ss, net = _scheduler(3, lambda: now[0])
    assert [q is not None for q in sch.queues] == [True, True, True, False]
    for j in range(3):
        sch.submit(0, _batch(0, j), 0.01 * j)
    sch.submit(1, _batch(1, 0), 0.0)
    now[0] = 1.0
    assert sch.run_once() == [] and sch.run_once() == [] and len(sch.inflight) == 2              # two steps in flight, both with a batch of session 0
    moved = U.pool_counters(pool, 0)
    assert ss[0].index == 2 * B and len(sch.queues[0]) == 1
    sch.remove_session(0)                                                                        # the queued batch is dropped, the two in flight are not
    assert sch.leaving == {0} and bat.sessions[0] is ss[0] and pool.vacant == {3} and sch.rings[0] is not None and len(sch.queues[0]) == 0
    for what in (lambda: sch.submit(0, _batch(0, 3)), lambda: sch.flush(0), lambda: sch.remove_session(0)):
        with pytest.raises(RuntimeError, match="the session is leaving"):
            what()
    for what in (lambda: sch.submit(3, _batch(0, 0)), lambda: sch.flush(3)):
        with pytest.raises(RuntimeError, match=r"\(3\): no session there \(live sessions: \[0, 1, 2\]\)"):
            what()
    n_net = len(net.calls)
    del host_ops[:]
    joiner, ring = FakeSession(FakeModel(), 70), ShapedRing(8 * B)
    assert sch.add_session(joiner, ring=ring) == 3                                               # NOT slot 0, NOT pool row 0: a step may still read them
    assert host_ops == [("rows_load", [3], True)] and len(net.calls) == n_net and pool.vacant == set() and sch.rings[3] is ring and bat.sessions[3] is joiner
    assert U.pool_counters(pool, 3) == (22, 2, 24, 8) and U.pool_counters(pool, 0) == moved
    with pytest.raises(RuntimeError, match="add_session: all 4 session slots are taken"):
        sch.add_session(FakeSession(FakeModel(), 80), ring=ShapedRing(8 * B))
    assert sch.run_once() == [] and sch.leaving == {0}                                           # nothing has completed yet
    events.finish()
    done = sch.run_once()
    assert [k for k, *_ in done].count(0) == 2 and [idx for k, _, idx, _ in done if k == 0] == [[0, 1, 2, 3], [4, 4, 3, 2]]      # both batches in flight are delivered
    assert sch.leaving == set() and sch.queues[0] is None and bat.sessions[0] is None and pool.vacant == {0} and sch.rings[0] is None
    for what in (lambda: sch.submit(0, _batch(0, 3)), lambda: sch.flush(0)):
        with pytest.raises(RuntimeError, match=r"\(0\): no session there"):
            what()
    bat.enc_a[0] = 5.0
    late = FakeSession(FakeModel(), 90)
    del host_ops[:]
    assert sch.add_session(late, ring=ShapedRing(8 * B)) == 0 and host_ops == [("rows_load", [0], True)]      # now the row and the slot are free
    assert U.pool_counters(pool, 0) == (22, 2, 24, 8) and pool.first[0] and bat.enc_a[0] is None and len(net.calls) == n_net
    # flush: features advance when a batch is picked, so the dropped batches' audio never enters the context
    sch.submit(0, _batch(5, 0), 2.0)
    sch.submit(0, _batch(5, 1), 2.1)
    assert sch.flush(0) == 2 and U.pool_counters(pool, 0) == (22, 2, 24, 8) and late.index == 0
    sch.submit(0, _batch(5, 2), 2.2)
    sch.submit(3, _batch(6, 0), 2.2)
    now[0] = 3.0
    sch.run_once()
    assert [k for k, *_ in sch.drain()] == [0, 3] and late.index == B and joiner.index == B
    fresh = _fresh_row(_batch(5, 2))
    assert torch.equal(sch.rings[0].msgs[0][0], late_frame(90, fresh)) and U.pool_counters(pool, 0) == U.pool_counters(pool, 3)
    sch.close()


def _fresh_row(chunks):
    """the windows of one batch through a fresh one-row pool after warm_up()"""
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    alone = NerfFeaturePool(1, U.StubNet(3, "cpu"), 3, device="cpu")
    alone.warm_up()
    return alone.step([0], [chunks], B)[0]


def late_frame(value, auds):
    return FakeSession(FakeModel(), value).step(auds[0]).clone()


@pytest.mark.parametrize("frame_format, good, bad", [("packed", (6, 4, 3), (6, 6, 3)), ("packed", (6, 4, 3), (9, 4)), ("i420", (9, 4), (6, 4, 3)), ("i420", (9, 4), (9, 6))])
def test_a_joiners_ring_is_checked_like_the_constructors_before_anything_is_stored(host_ops, monkeypatch, frame_format, good, bad):
    from mere_fusion_amd.nerf_serving import NerfEndToEndScheduler
    Events(monkeypatch)
    sch, pool, bat, ss, net = _scheduler(2, lambda: 0.0, frame_format=frame_format, shape=good)
    del host_ops[:]
    state = lambda: (_slots(bat), set(pool.vacant), list(sch.rings), [q is not None for q in sch.queues])
    before = state()
    joiner = FakeSession(FakeModel(), 70)
    for ring, text in ((None, "add_session: a ring per session"), (ShapedRing(8 * B, bad), r"ring 2 has slots of shape .*session 2's 6 x 4 frames need " +
                                                                    str(good).replace("(", r"\(").replace(")", r"\)"))):
        with pytest.raises(RuntimeError, match="NerfEndToEndScheduler: .*" + text):
            sch.add_session(joiner, ring=ring)
        assert state() == before and not host_ops
    with pytest.raises(RuntimeError, match="frontend=None"):
        sch.add_session(joiner, ring=ShapedRing(8 * B, good), frontend=object())
    wrong = FakeSession(FakeModel(), 1, cycle={2: [torch.zeros(6, 5, 3, dtype=torch.uint8)]})
    with pytest.raises(RuntimeError, match=r"NerfBatcher: session 2: custom_img_cycle\[2\]"):    # the batcher's checks run before the pool's row is written
        sch.add_session(wrong, ring=ShapedRing(8 * B, good))
    assert state() == before and not host_ops
    assert sch.add_session(joiner, ring=ShapedRing(8 * B, good)) == 2 and host_ops == [("rows_load", [2], True)]
    sch.remove_session(2)                                                # nothing in flight: released at once
    assert pool.vacant == {2, 3} and bat.sessions[2] is None and sch.rings[2] is None
    sch.close()
    # a scheduler over a pool or a batcher built for a fixed list refuses by name
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfFeaturePool
    fixed_pool = NerfFeaturePool(3, U.StubNet(3, "cpu"), 3, device="cpu")
    room = NerfBatcher(ss[:2], pool=fixed_pool, device="cpu", max_sessions=3)
    with pytest.raises(RuntimeError, match=r"live rows \[0, 1, 2\] are not the batcher's live sessions \[0, 1\]"):
        NerfEndToEndScheduler(room)
    fixed = NerfEndToEndScheduler(NerfBatcher(ss[:2], pool=NerfFeaturePool(2, U.StubNet(3, "cpu"), 3, device="cpu"), device="cpu"))
    with pytest.raises(RuntimeError, match="NerfBatcher: add_session: .*fixed list of sessions"):
        fixed.add_session(joiner)
    with pytest.raises(RuntimeError, match="NerfBatcher: remove_session: .*fixed list of sessions"):
        fixed.remove_session(0)


def test_session_scheduler_takes_joiners_without_a_pool():
    """NerfSessionScheduler's code is serving.SessionScheduler's: the batcher's four entry points are all it needs"""
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfSessionScheduler
    ss = [FakeSession(FakeModel(), 1), FakeSession(FakeModel(), 2)]
    bat = NerfBatcher(ss, device="cpu", max_sessions=3)
    now = [0.0]
    sch = NerfSessionScheduler(bat, clock=lambda: now[0], hold_s=0.0, sync=lambda: None)
    late = FakeSession(FakeModel(), 3)
    assert sch.add_session(late) == 2
    sch.submit(2, _inp(1), 0.0)
    sch.remove_session(0)
    assert bat.live() == [1, 2] and sch.queues[0] is None
    (k, fr, idx, lat), = sch.run_once(1.0)
    assert k == 2 and idx == [0, 1, 2, 3] and tuple(fr.shape) == (4, 6, 4, 3)
    assert sch.add_session(FakeSession(FakeModel(), 4)) == 0


# ---- the C ABI of the new entry ----------------------------------------------------------------------------------------------------------------
def test_header_exports_and_ctypes_table_agree_for_the_new_symbol(lib_built):
    from mere_fusion_amd import _lib
    declared = _lib.HEADER.functions
    lib = C.CDLL(lib_built)
    n = "mf_nerf_feat_rows_load"
    assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES
    assert len(declared[n][1]) == len(_lib.SIGNATURES[n][1]) == 10
    assert sorted(_lib.SIGNATURES) == sorted(declared)


def test_argument_checks_that_never_launch(lib_built):
    """every call is refused with MF_ERR_INVALID before a pointer is read or anything is enqueued (this box has no device)"""
    from mere_fusion_amd import _lib
    l = _lib.lib()
    ints = lambda *v: (C.c_int * len(v))(*v)
    N, R, dim = 3, 32, 44
    ring_b, hist_b = R * dim * 4, 8 * dim * 16 * 4
    rings, hist = 1 << 20, 1 << 24                                       # non-null, 16-byte aligned, never dereferenced; row N of each is a scratch row
    ptr = lambda v: None if v is None else C.c_void_p(v)

    def load(rings=rings, hist=hist, N=N, R=R, dim=dim, S=2, rows=ints(0, 2), src_ring=rings + 3 * ring_b, src_hist=hist + 3 * hist_b):
        return l.mf_nerf_feat_rows_load(ptr(rings), ptr(hist), N, R, dim, S, rows, ptr(src_ring), ptr(src_hist), None)

    for kw, needle in ((dict(rings=None), b"null"), (dict(rows=None), b"null"), (dict(hist=None), b"null history"), (dict(dim=0), b"dim"), (dict(dim=1025), b"dim"),
                       (dict(dim=-3), b"dim"), (dict(R=15), b"ring"), (dict(R=1 << 30), b"ring"), (dict(R=18), b"ring"), (dict(N=0), b"pool"), (dict(N=1 << 30), b"pool"),
                       (dict(S=0), b"picked"), (dict(S=4), b"picked"), (dict(S=-1), b"picked"), (dict(rows=ints(0, 3)), b"out of range"),
                       (dict(rows=ints(-1, 0)), b"out of range"), (dict(rows=ints(1 << 30, 0)), b"out of range"), (dict(rows=ints(2, 2)), b"twice"),
                       (dict(rings=rings + 4), b"aligned"), (dict(hist=hist + 8), b"aligned"), (dict(src_ring=rings + 3 * ring_b + 4), b"aligned"),
                       (dict(src_hist=hist + 3 * hist_b + 12), b"aligned"),
                       (dict(src_ring=rings), b"ring source overlaps session row 0"), (dict(src_ring=rings + 2 * ring_b), b"ring source overlaps session row 2"),
                       (dict(src_ring=rings + ring_b + 16), b"ring source overlaps session row 2"), (dict(src_ring=rings - 16), b"ring source overlaps session row 0"),
                       (dict(src_hist=hist + 2 * hist_b), b"history source overlaps session row 2"), (dict(src_hist=hist + hist_b - 16), b"history source overlaps session row 0"),
                       (dict(src_hist=hist + 3 * hist_b - 16), b"history source overlaps session row 2")):
        assert load(**kw) == -1 and needle in l.mf_last_error(), (kw, l.mf_last_error())
