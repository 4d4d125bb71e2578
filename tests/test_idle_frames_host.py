"""CPU: the host side of idle and custom-video frames from the device -- serving.choose_frames against the reference consumer's branch written out
(tests/idle_frames_ref.py), mf_frames_gather's refusals through ctypes (none touches a device), what PipelinedScheduler(idle_frames=True) refuses when it is
built, and the scheduler's bookkeeping around the gather (which frames it asks for, when the custom walk moves) with the launch itself replaced by a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

from idle_frames_ref import RefConsumer, typed
from mere_fusion_amd import serving as S
from serving_fakes import FakeBatcher, FakeRing, fake_cuda_events


# ---- choose_frames ------------------------------------------------------------------------------------------------------------------------
def _check_batch(ref, ci, lengths, idx, pairs):
    """one batch through both; the scheduler's part (applying the increments) is done here"""
    before = dict(ci)
    got, inc = S.choose_frames(pairs, idx, ci, lengths)
    assert ci == before                                                     # the call itself moves nothing
    want = ref.batch(idx, pairs)
    assert got == want, (got, want)
    assert inc == {t: sum(1 for c in want if c[0] == "custom" and c[1] == t) for t in inc} and all(n > 0 for n in inc.values())
    for t, n in inc.items():
        ci[t] += n
    assert ci == ref.custom_index
    return got


@pytest.mark.parametrize("n_cycle", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 4, 8])
def test_choose_frames_equals_the_reference_branch(B, n_cycle):
    """seeded type sequences over {0, 1, 2, 3}; a custom video for type 2 only, so type 3 shows the idle frame; six batches, the dict reset after the third"""
    rng = np.random.default_rng(100 * B + n_cycle)
    lengths = {2: n_cycle}
    ci, ref = {2: 0}, RefConsumer(lengths, {2: 0})
    seen, walk = set(), 0
    for j in range(6):
        if j == 3:                                                          # set_curr_state(2, reinit=True) / init_customindex() between two batches
            ci[2] = 0
            ref.custom_index[2] = 0
        types = rng.integers(0, 4, 2 * B) if j % 2 else np.repeat(rng.integers(0, 4, B), 2)          # per-chunk and per-frame sequences
        if j == 4:
            types = np.full(2 * B, 2)                                       # a whole batch of the custom video: the mirror walk turns around inside it
        idx = [S.mirror_index(7, walk + i) for i in range(B)]
        walk += B
        got = _check_batch(ref, ci, lengths, idx, typed(types))
        seen.update(c[0] for c in got)
        if j == 4:
            assert [c[2] for c in got] == [S.mirror_index(n_cycle, ci[2] - B + i) for i in range(B)]
    if B > 1:
        assert seen == {"speech", "idle", "custom"}


def test_choose_frames_named_cases():
    lengths, ci = {2: 5}, {2: 3}
    ref = RefConsumer(lengths, dict(ci))
    pairs = typed([2, 1,      # first chunk custom type, second plain silence: non-speech, audiotype 2
                   1, 2,      # the other way round: non-speech, audiotype 1 -> idle
                   0, 2,      # one speech chunk: speech
                   2, 0,      # one speech chunk: speech
                   3, 3,      # a custom type without a video: idle
                   2, 2, 2, 2, 2, 2])
    got = _check_batch(ref, ci, lengths, [10, 11, 12, 13, 14, 15, 16, 17], pairs)
    assert got == [("custom", 2, 3), ("idle", 11), ("speech", 12), ("speech", 13), ("idle", 14), ("custom", 2, 4), ("custom", 2, 4), ("custom", 2, 3)]
    assert ci == {2: 7}
    # no custom videos at all: silence is the idle frame, nothing to move
    assert S.choose_frames(typed([1, 1, 2, 2]), [0, 1], {}, {}) == ([("idle", 0), ("idle", 1)], {})
    with pytest.raises(RuntimeError, match="3 .pcm, type. pairs for 2 frames"):
        S.choose_frames(typed([1, 1, 1]), [0, 1], {}, {})
    with pytest.raises(RuntimeError, match="no custom video of that type is attached"):
        S.choose_frames(typed([4, 4]), [0], {4: 0}, {2: 5})


# ---- mf_frames_gather: refusals ----------------------------------------------------------------------------------------------------------------
def test_abi_refusals_name_the_value_and_launch_nothing(lib_built):
    """every refusal comes before the launch, so none needs a device; the pointers are never read"""
    from mere_fusion_amd import _lib
    l = _lib.lib()
    src, out = (C.c_uint8 * 256)(), (C.c_uint8 * 256)()
    ps, po = C.addressof(src), C.addressof(out)

    def table(*entries):
        arr = (_lib.MfFrameSrc * len(entries))()
        for a, (frame, dst) in zip(arr, entries):
            a.frame, a.dst = frame, dst
        return arr

    one = table((ps, 0))
    for args, text in (((None, 1, 4, 4, 0, 0, po, 4), b"srcs is a null pointer"), ((one, 1, 4, 4, 0, 0, None, 4), b"out is a null pointer"),
                       ((one, 0, 4, 4, 0, 0, po, 4), b"n 0"), ((one, -3, 4, 4, 0, 0, po, 4), b"n -3"), ((one, 1, 4, 4, 0, 0, po, 0), b"out_frames 0"),
                       ((one, 1, 0, 4, 0, 0, po, 4), b"frame size 0 x 4"), ((one, 1, 4, -4, 1, 0, po, 4), b"frame size 4 x -4"),
                       ((one, 1, 4, 4, 2, 0, po, 4), b"format 2"), ((one, 1, 4, 4, -1, 0, po, 4), b"format -1"), ((one, 1, 4, 4, 0, 2, po, 4), b"rgb_order 2"),
                       ((one, 1, 5, 4, 1, 0, po, 4), b"H 5 is odd"), ((one, 1, 4, 7, 1, 1, po, 4), b"W 7 is odd"),
                       ((table((ps, 0), (None, 1)), 2, 4, 4, 0, 0, po, 4), b"source 1: frame is a null pointer"),
                       ((table((ps, 4)), 1, 4, 4, 0, 0, po, 4), b"source 0: dst 4 is outside [0, 4)"),
                       ((table((ps, 0), (ps + 48, -1)), 2, 4, 4, 1, 0, po, 4), b"source 1: dst -1 is outside [0, 4)"),
                       ((table((ps, 1), (ps + 48, 0), (ps + 96, 1)), 3, 4, 4, 0, 0, po, 4), b"sources 0 and 2 both name dst 1"),
                       ((table((ps, 0), (po + 48, 1)), 2, 4, 4, 0, 0, po, 4), b"source 1 lies inside out")):
        assert l.mf_frames_gather(*args, None) == -1, args
        assert text in l.mf_last_error(), (args, l.mf_last_error())
    assert bytes(src) == bytes(256) and bytes(out) == bytes(256)
    assert l.mf_abi_version() == 4                                          # an entry point was added, none changed


# ---- PipelinedScheduler(idle_frames=True): what it refuses when it is built ------------------------------------------------------------------------
class _Cycles:
    """the surface of paste.CustomVideos the scheduler uses, on the host"""

    def __init__(self, cycles, custom_index):
        self.cycles, self.custom_index, self.lengths = cycles, custom_index, {t: len(c) for t, c in cycles.items()}

    def source(self, t, i):
        return self.cycles[t][i]

    def check_size(self, H, W, who="CustomVideos"):
        for t, c in self.cycles.items():
            if tuple(c.shape[1:3]) != (H, W):
                raise RuntimeError(f"{who}: custom video {t!r} holds {c.shape[1]} x {c.shape[2]} frames (H x W), the avatar's frames are {H} x {W}")


class _Session:
    def __init__(self, frames, custom_videos=None):
        self.frames, self.custom_videos = frames, custom_videos


class _IdleBatcher(FakeBatcher):
    """FakeBatcher with cached full frames [n, 4, 4, 3] per session: its generated frames are filled with 200 + the session's number; a step can fail once"""
    frame_order, paste = "bgr", True

    def __init__(self, sessions, batch_size, fail_steps=()):
        super().__init__(len(sessions), len(sessions), batch_size=batch_size)
        self.sessions, self.fail_steps, self.calls = list(sessions), set(fail_steps), 0

    def frame_hw(self, k):
        return (4, 4) if self.paste and self.sessions[k].frames is not None else None

    def idle_source(self, k, i):
        return self.sessions[k].frames[i]

    def step(self, chunks, only=None):
        self.calls += 1
        if self.calls in self.fail_steps:
            raise RuntimeError("step failed")
        out = super().step(chunks, only)
        return [None if o is None else (None if o[0] is None else torch.full((self.batch_size, 4, 4, 3), 200 + k, dtype=torch.uint8), o[1]) for k, o in enumerate(out)]


def _frames(n, base):
    return torch.stack([torch.full((4, 4, 3), base + i, dtype=torch.uint8) for i in range(n)])


def test_constructor_refusals_of_idle_frames():
    B = 2
    rings = [FakeRing(2 * B), FakeRing(2 * B)]
    good = _IdleBatcher([_Session(_frames(3, 10)), _Session(_frames(3, 20))], B)
    with pytest.raises(RuntimeError, match="idle_frames=True fills the tuples the rings carry; without rings"):
        S.PipelinedScheduler(good, single_stream=True, idle_frames=True)
    with pytest.raises(RuntimeError, match="1 rings for 2 sessions"):
        S.PipelinedScheduler(good, rings=rings[:1], single_stream=True, idle_frames=True)
    with pytest.raises(RuntimeError, match=r"FakeBatcher has no idle_source\(k, i\)"):
        S.PipelinedScheduler(FakeBatcher(2, 2, batch_size=B), rings=rings, single_stream=True, idle_frames=True)
    unpasted = _IdleBatcher([_Session(_frames(3, 10)), _Session(_frames(3, 20))], B)
    unpasted.paste = False
    with pytest.raises(RuntimeError, match="_IdleBatcher was built with paste=False"):
        S.PipelinedScheduler(unpasted, rings=rings, single_stream=True, idle_frames=True)
    with pytest.raises(RuntimeError, match="session 1 has no AvatarFrames"):
        S.PipelinedScheduler(_IdleBatcher([_Session(_frames(3, 10)), _Session(None)], B), rings=rings, single_stream=True, idle_frames=True)
    other = _Cycles({2: torch.zeros((2, 6, 4, 3), dtype=torch.uint8)}, {2: 0})
    with pytest.raises(RuntimeError, match=r"session 0: custom video 2 holds 6 x 4 frames \(H x W\), the avatar's frames are 4 x 4"):
        S.PipelinedScheduler(_IdleBatcher([_Session(_frames(3, 10), other), _Session(_frames(3, 20))], B), rings=rings, single_stream=True, idle_frames=True)
    S.PipelinedScheduler(good, rings=rings, single_stream=True, idle_frames=True).close()
    # the default looks at none of this
    sch = S.PipelinedScheduler(FakeBatcher(2, 2, batch_size=B), single_stream=True)
    assert sch.idle_frames is False
    sch.close()


# ---- the scheduler's bookkeeping, with the launch replaced by a host copy -----------------------------------------------------------------------
def _host_gather(calls):
    def gather(sources, dst, out, fmt="packed", order="bgr"):
        assert fmt == "packed" and order == "bgr" and len(set(dst)) == len(dst) == len(sources) > 0
        calls.append(list(dst))
        for s, d in zip(sources, dst):
            out[d].copy_(s)
        return out
    return gather


def test_scheduler_fills_every_tuple_and_moves_the_walk_once(monkeypatch):
    """two sessions, B = 4, a 3-frame custom video for type 2 on session 0; the step of the third round fails once and is retried"""
    from mere_fusion_amd import ops
    fake_cuda_events(monkeypatch)
    calls = []
    monkeypatch.setattr(ops, "gather_frames", _host_gather(calls))
    B = 4
    ci = {2: 0}
    cyc = _Cycles({2: _frames(3, 100)}, ci)
    bat = _IdleBatcher([_Session(_frames(20, 0), cyc), _Session(_frames(20, 50))], B, fail_steps={3})     # (the fake batcher's indices count up: 20 cached frames)
    rings = [FakeRing(8 * B), FakeRing(8 * B)]
    script = [[0] * 8, [1] * 8, [2] * 8, [0, 0, 0, 0, 1, 1, 1, 1], [2, 1, 1, 2, 0, 2, 2, 2]]
    refs = [RefConsumer({2: 3}, {2: 0}), RefConsumer({}, {})]
    want = [[], []]
    with S.PipelinedScheduler(bat, rings=rings, clock=lambda: 1.0, hold_s=0.0, single_stream=True, idle_frames=True) as sch:
        with pytest.raises(RuntimeError, match="0 pairs for 4 frames"):
            sch.submit(0, "mel", 0.1)                                       # no pairs: nothing to choose from
        for j, types in enumerate(script):
            for k in range(2):
                speech = any(t == 0 for t in types)
                sch.submit(k, "mel" if speech and not (j == 0 and k == 1) else None, 0.1 * j + 0.01 * k, pairs=typed(types, chunk=j))
                idx = list(range(j * B, j * B + B))
                for i, c in enumerate(refs[k].batch(idx, typed(types))):
                    if c[0] == "custom":
                        want[k].append(100 + c[2])
                    elif c[0] == "idle" or (j == 0 and k == 1):            # session 1's first batch: typed speech, nothing generated (a context still filling)
                        want[k].append(50 * k + c[1])
                    else:
                        want[k].append(200 + k)
            if j == 2:
                before = dict(ci)
                with pytest.raises(RuntimeError, match="step failed"):
                    sch.run_once()
                assert ci == before and all(not r.open and not r.msgs[2 * B:] for r in rings)      # nothing moved, nothing published, no place left open
            done = sch.run_once() + sch.drain()
            assert sorted(k for k, *_ in done) == [0, 1] and all(fr is not None and tuple(fr.shape) == (B, 4, 4, 3) for _, fr, _, _ in done)
    assert ci == refs[0].custom_index == {2: 4 + 2}
    for k, ring in enumerate(rings):
        assert len(ring.msgs) == len(script) * B and not ring.open and not ring.aborted
        got = []
        for f, i, audio in ring.msgs:
            assert f is not None and len(set(f.reshape(-1).tolist())) == 1 and len(audio) == 2
            got.append(int(f[0, 0, 0]))
        assert got == want[k], (k, got, want[k])
        assert [i for _, i, _ in ring.msgs] == list(range(len(script) * B))
    # an all-speech batch with every frame generated asks for no gather: 2 sessions x 5 rounds, less session 0's first
    assert len(calls) == 9 and calls[0] == [0, 1, 2, 3]


def test_option_off_is_todays_scheduler(monkeypatch):
    fake_cuda_events(monkeypatch)
    B = 2

    def run(**kw):
        bat = _IdleBatcher([_Session(_frames(5, 10)), _Session(_frames(5, 20))], B)
        rings = [FakeRing(8 * B), FakeRing(8 * B)]
        with S.PipelinedScheduler(bat, rings=rings, clock=lambda: 1.0, hold_s=0.0, single_stream=True, **kw) as sch:
            for j, types in enumerate(([0] * 4, [1] * 4, [0, 0, 1, 1])):
                for k in range(2):
                    sch.submit(k, "mel" if 0 in types else None, 0.1 * j, pairs=typed(types, chunk=j))
                sch.run_once()
                sch.drain()
        return [[(None if f is None else f.tolist(), i, a) for f, i, a in r.msgs] for r in rings]

    off, default = run(idle_frames=False), run()
    assert off == default
    assert [f is None for f, _, _ in off[0]] == [False, False, True, True, False, False]
