"""CPU: the model-agnostic serving loop (mere_fusion_amd/serving.py) with a counting stage, fake rings and a fake batcher -- advance-once across failed
steps, reservations and queue order after a failure, deferral (the numbers of the ADVICE r04 test in test_muse_driver.py), the waiter thread's life, the `only=`
and submit helpers -- and MuseBatcher's two refusals through the pooled step with a fake forward."""
import numpy as np
import pytest
import torch

from mere_fusion_amd import muse_driver as D
from mere_fusion_amd import serving as S
from serving_fakes import FakeBatcher, FakeRing, fake_cuda_events

B = 2


class CountingScheduler(S.PipelinedScheduler):
    """the smallest model: a session's audio state is a counter, a batch's input is the counter's value when the batch advanced it"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.state, self.advances = [0] * len(self.queues), []

    def _advance(self, ks, payloads):
        self.advances.append(list(ks))
        for k in ks:
            self.state[k] += 1
            payloads[k]["input"] = self.state[k]

    def _inputs(self, ks, payloads, dev):
        return [payloads[k]["input"] if k in ks else None for k in range(len(self.queues))]


def test_a_batch_whose_step_fails_twice_advances_once_and_is_delivered_once(monkeypatch):
    fake_cuda_events(monkeypatch)
    bat = FakeBatcher(2, 2, batch_size=B)
    good_step, failures, seen = bat.step, [2], []

    def step(inputs, only=None):
        seen.append(list(inputs))
        if failures[0]:
            failures[0] -= 1
            raise RuntimeError("step failed")
        return good_step(inputs, only=only)

    bat.step = step
    rings = [FakeRing(2 * B), FakeRing(2 * B)]
    sch = CountingScheduler(bat, rings=rings, clock=lambda: 1.0, hold_s=0.0, single_stream=True)
    sch.submit(0, {"name": "a0"}, 0.1, ["p0", "p1", "p2", "p3"])
    sch.submit(0, {"name": "b0"}, 0.5, ["q0", "q1", "q2", "q3"])
    sch.submit(1, {"name": "a1"}, 0.2, ["r0", "r1", "r2", "r3"])
    for attempt in range(2):
        with pytest.raises(RuntimeError, match="step failed"):
            sch.run_once()
        assert all(r.taken == 0 and not r.open and not r.begun for r in rings)            # every reservation went back
        assert [[e[0] for e in q] for q in sch.queues] == [[0.1, 0.5], [0.2]]            # both batches back at the HEAD of their queues, order kept
        assert [q[0][1][0]["name"] for q in sch.queues] == ["a0", "a1"]
        assert [len(e) for e in sch.queues[0]] == [3, 2] and sch.queues[1][0][2] is True   # the tried batches carry the mark, the one behind does not
        assert sch.steps == 0 and sch.sessions_served == 0 and not sch.inflight and sch._waiter is None
    done = sch.run_once() + sch.drain()
    assert sch.advances == [[0, 1]] and sch.state == [1, 1]                               # the stage advanced ONCE for the batch that was tried three times
    assert seen == [[1, 1]] * 3                                                          # ... and every try stepped on what that one advance produced
    assert sorted(k for k, *_ in done) == [0, 1] and sch.steps == 1 and sch.sessions_served == 2
    assert [len(r.msgs) for r in rings] == [B, B] and [len(r.begun) for r in rings] == [1, 1]      # delivered once
    assert rings[0].msgs[0][1:] == (0, ["p0", "p1"]) and rings[0].msgs[1][1:] == (1, ["p2", "p3"])
    done = sch.run_once() + sch.drain()                                                   # session 0's second batch: its own advance
    assert [k for k, *_ in done] == [0] and sch.advances == [[0, 1], [0]] and sch.state == [2, 1] and seen[-1] == [2, None]
    assert [m[1] for m in rings[0].msgs] == [0, 1, 2, 3]
    sch.close()


def test_a_deferred_session_is_left_out_of_pending_and_offered_again():
    """ADVICE r04 on the agnostic scheduler, with the numbers of test_end_to_end_scheduler_leaves_a_deferred_session_out_until_its_ring_has_room"""
    now = [1.0]
    rings = [FakeRing(0), FakeRing(16)]
    sch = S.PipelinedScheduler(FakeBatcher(2, 2, batch_size=8), rings=rings, clock=lambda: now[0], single_stream=True)    # built without a device
    assert sch.copy_stream is None and (sch.capacity, sch.hold, sch.period) == (2, pytest.approx(0.08), pytest.approx(0.32))
    sch.submit(0, "win", 0.2)
    sch.submit(1, "win", 0.9)
    sch._deferred = {0: 1.05}                                       # session 0 was deferred at t = 0.97 (+ period / 4)
    assert sch.pending() == {1: 0.9}                                # the stalled session does not age the order ...
    assert sch.next_due() == pytest.approx(0.98)                    # ... session 1's own hold decides (0.9 + 0.08), not a time in the past
    sch.queues[1].clear()
    assert sch.pending() == {} and sch.next_due() == 1.05           # nothing else queued: wake up when the back-off ends, do not spin
    now[0] = 1.06
    assert sch.pending() == {0: 0.2} and 0 not in sch._deferred     # back-off over: offered again (and counted as a new episode if still full)
    sch._deferred = {0: 9.0}
    rings[0].places = 8
    assert sch.pending() == {0: 0.2}                                # ... or as soon as the consumer has freed a batch's worth of slots


def test_a_full_ring_defers_its_session_in_run_once_and_counts_one_episode(monkeypatch):
    fake_cuda_events(monkeypatch)
    now = [1.0]
    rings = [FakeRing(0), FakeRing(2 * B)]
    bat = FakeBatcher(2, 2, batch_size=B)
    sch = S.PipelinedScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, single_stream=True)
    sch.submit(0, "x0", 0.2)
    sch.submit(1, "x1", 0.9)
    done = sch.run_once() + sch.drain()
    assert [k for k, *_ in done] == [1] and bat.steps == [([1], [None, "mel"])]           # (the default stage: the payload is the batcher's input)
    assert sch.ring_full == 1 and sch._deferred == {0: pytest.approx(1.0 + sch.period / 4)} and len(sch.queues[0]) == 1
    assert sch.pending() == {} and sch.next_due() == pytest.approx(1.0 + sch.period / 4) and sch.run_once() == [] and sch.ring_full == 1
    rings[0].places = B                                                                   # the consumer has read: offered at once, no new episode
    done = sch.run_once() + sch.drain()
    assert [k for k, *_ in done] == [0] and sch.ring_full == 1 and not sch._deferred and bat.index == [B, B]
    sch.close()


def test_the_waiter_thread_exists_from_the_first_step_to_close(monkeypatch):
    fake_cuda_events(monkeypatch)
    sch = S.PipelinedScheduler(FakeBatcher(1, 1, batch_size=B), clock=lambda: 1.0, hold_s=0.0)        # rings=None: no stream, no device
    assert sch._waiter is None and sch.copy_stream is None
    sch.submit(0, "x", 0.5)
    assert sch._waiter is None                                                            # queued, not stepped: no thread yet
    assert sch.run_once() == [] and len(sch.inflight) == 1                                # the step is in flight ...
    waiter = sch._waiter
    assert waiter is not None and waiter.is_alive()                                       # ... and its event has gone to the waiter
    done = sch.drain()
    assert [d[0] for d in done] == [0] and done[0][2] == [0, 1] and done[0][3] == pytest.approx(0.5)
    sch.close()
    assert sch._waiter is None and not waiter.is_alive()
    sch.close()                                                                           # (twice is fine)


def test_step_sessions_refuses_bad_numbers_and_steps_over_capacity():
    bat = FakeBatcher(3, 2, batch_size=B)
    x = object()
    assert S.step_sessions(bat, [x, None, x], None) == ([0, 1, 2], [0, 2])                # a None input is picked (its walk moves) but not active
    assert S.step_sessions(bat, [x, x, x], [2, 0]) == ([0, 2], [0, 2])
    assert S.step_sessions(bat, [x, x, x], range(1)) == ([0], [0])
    assert S.step_sessions(bat, [x, None, None], [0, 1], skip_none=False) == ([0, 1], [0, 1])
    for inputs, only, kw, text in (([x, x], None, {}, "2 entries for 3 sessions"), ([x, x, x], [0, 3], {}, "session numbers run from 0 to 2"),
                                   ([x, x, x], [-1], {}, "session numbers run from 0 to 2"), ([x, x, x], None, {}, "3 active sessions in one step"),
                                   ([x, None, None], None, dict(skip_none=False), "3 active sessions in one step")):
        with pytest.raises(RuntimeError, match="FakeBatcher: .*" + text):
            S.step_sessions(bat, inputs, only, **kw)


def test_split_batch_classifies_silent_mixed_and_bare_batches():
    c = [np.full(4, i, np.float32) for i in range(4)]
    chunks, pairs, types = S.split_batch(c, "t")                                          # bare arrays: all speech
    assert chunks == c and types == [0, 0, 0, 0] and all(p[0] is a and p[1] == 0 for p, a in zip(pairs, c)) and not S.all_silent(types)
    chunks, pairs, types = S.split_batch([(a, 1) for a in c], "t")                        # all silent (type 1)
    assert all(a is b for a, b in zip(chunks, c)) and types == [1] * 4 and S.all_silent(types)
    chunks, pairs, types = S.split_batch([(c[0], 1), c[1], (c[2], 2), (c[3], 1)], "t")    # mixed: one type-0 chunk makes it a spoken batch
    assert types == [1, 0, 2, 1] and not S.all_silent(types) and pairs[1][0] is c[1] and pairs[2] == (c[2], 2)
    assert S.all_silent([2, 1]) and S.all_silent([])                                      # a custom video's audio (type > 1) is not speech either
    with pytest.raises(RuntimeError, match="who: expected chunks or"):
        S.split_batch([(c[0], 0, 0)], "who")


class HostMuseBatcher(D.MuseBatcher):
    """MuseBatcher's step without its handles: the constructor (which needs a device) and the forward are replaced, the input check takes host tensors"""

    def __init__(self, sessions, paste):
        self.sessions, self.batch_size, self.paste, self.device, self.max_sessions_per_step = list(sessions), B, paste, torch.device("cpu"), len(sessions)
        self._lay_out_pool()
        self.forwards = []

    def _check_input(self, k, ch):
        if ch.shape[0] != self.batch_size:
            raise RuntimeError(f"session {k}: expected {self.batch_size} whisper chunks")

    def _forward(self, chunks, rows):
        self.forwards.append(list(rows))
        return torch.zeros(len(rows), 4, 4, 3, dtype=torch.uint8)


class FakeAvatar:
    def __init__(self, n):
        self.n = n

    def paste(self, res, indices):
        return res


def test_muse_batcher_refuses_before_any_index_moves():
    lat = [torch.zeros(1, 8, 32, 32)] * 3
    ch = torch.zeros(B, 50, 384)
    # a session without AvatarFrames, paste=True: refused although it comes AFTER sessions that could have been walked
    ss = [D.MuseSession(lat, avatar_frames=FakeAvatar(3)), D.MuseSession(lat, avatar_frames=FakeAvatar(3)), D.MuseSession(lat)]
    bat = HostMuseBatcher(ss, paste=True)
    assert [s.pool_offset for s in ss] == [0, 3, 6]
    with pytest.raises(RuntimeError, match="session 2 has no AvatarFrames"):
        bat.step([ch, ch, ch])
    assert [s.index for s in ss] == [0, 0, 0] and not bat.forwards
    out = bat.step([ch, ch, None])                                                        # silent: nothing to paste, nothing to refuse
    assert [s.index for s in ss] == [B, B, B] and out[2] == (None, [0, 1]) and bat.forwards == [[0, 1, 3, 4]]
    # an input list that is not one entry per session (it used to end the zip early and skip sessions)
    ss = [D.MuseSession(lat) for _ in range(3)]
    bat = HostMuseBatcher(ss, paste=False)
    for short in ([ch, ch], [ch, ch, ch, ch], []):
        with pytest.raises(RuntimeError, match=f"{len(short)} entries for 3 sessions"):
            bat.step(short)
        with pytest.raises(RuntimeError, match=f"{len(short)} entries for 3 sessions"):
            bat.step(short, only=[0])
        assert [s.index for s in ss] == [0, 0, 0] and not bat.forwards
