"""CPU: the bookkeeping of the multi-session Wav2Lip stack (lip_driver.LipBatcher / LipSessionScheduler / LipEndToEndScheduler) with a fake generator and
CPU tensors -- pool offsets, the ping-pong walk, silence, `only=`, validation before any index moves, scheduling on an injected clock, ring deferral -- and the
C ABI of the two entry points underneath (header, exports, ctypes table, argument checks that need no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mere_fusion_amd import lip_driver as D
from serving_fakes import FakeBatcher, FakeRing, fake_cuda_events

B = 2
COUNTS = (3, 4, 5)


class FakeModel:
    """stands where the generator stands: the 'frames' it returns are the pool faces it was asked for, so a test sees which rows a step read"""

    def __init__(self):
        self.calls = []

    def parameters(self):
        yield torch.zeros(1)

    def forward_u8_rows(self, mel, pool, rows):
        assert mel.shape[0] == len(rows)
        self.calls.append(list(rows))
        return pool[torch.tensor(rows)].float()


class FakeAvatar:
    def __init__(self, n):
        self.n, self.calls = n, []

    def paste(self, res, indices):
        self.calls.append(list(indices))
        return res.to(torch.uint8)


def _faces(s, n):
    """face i of session s is filled with the value 16 * s + i"""
    return torch.stack([torch.full((96, 96, 3), 16 * s + i, dtype=torch.uint8) for i in range(n)])


def _batcher(paste=False, max_sessions_per_step=None):
    m = FakeModel()
    sessions = [D.LipSession(m, _faces(s, n), avatar_frames=FakeAvatar(n) if paste else None) for s, n in enumerate(COUNTS)]
    return m, sessions, D.LipBatcher(m, sessions, batch_size=B, paste=paste, device="cpu", max_sessions_per_step=max_sessions_per_step)


def _mel(v=0.0):
    return torch.full((B, 1, 80, 16), v)


def test_pool_offsets_and_ping_pong_walk_across_steps():
    m, sessions, bat = _batcher()
    assert [s.pool_offset for s in sessions] == [0, 3, 7] and bat.pool.shape == (12, 96, 96, 3) and bat.max_sessions_per_step == 3
    for step in range(6):                                                # 12 frames: every walk turns round at least once (3, 4 and 5 faces)
        out = bat.step([_mel(), _mel(), _mel()])
        want_rows = []
        for s, n in enumerate(COUNTS):
            idx = [D.mirror_index(n, step * B + i) for i in range(B)]
            assert out[s][1] == idx
            assert [int(f[0, 0, 0]) for f in out[s][0]] == [16 * s + i for i in idx]      # the frames of session s come from ITS faces
            want_rows += [sessions[s].pool_offset + i for i in idx]
        assert m.calls[-1] == want_rows                                  # one generator call for all three
    assert len(m.calls) == 6 and [s.index for s in sessions] == [12, 12, 12]


def test_silent_sessions_advance_and_only_leaves_the_rest_untouched():
    m, sessions, bat = _batcher()
    out = bat.step([_mel(), None, _mel()])
    assert out[1] == (None, [0, 1]) and sessions[1].index == B and m.calls[-1] == [0, 1, 7, 8]
    out = bat.step([None, None, None])                                   # everybody silent: no generator call, every walk moves
    assert len(m.calls) == 1 and [o[0] for o in out] == [None] * 3 and [o[1] for o in out] == [[2, 2], [2, 3], [2, 3]]
    out = bat.step([_mel(), _mel(), _mel()], only=[2, 0])
    assert out[1] is None and sessions[1].index == 2 * B                 # absent: untouched, no entry
    assert out[0][1] == [1, 0] and out[2][1] == [4, 4] and m.calls[-1] == [1, 0, 7 + 4, 7 + 4]
    out = bat.step([_mel(), _mel(), None], only=[1])                     # entries of sessions outside `only` are not looked at
    assert out[0] is None and out[2] is None and out[1][1] == [3, 2] and m.calls[-1] == [3 + 3, 3 + 2]


def test_paste_is_one_call_per_active_session():
    m, sessions, bat = _batcher(paste=True)
    out = bat.step([_mel(), None, _mel()])
    assert sessions[0].avatar_frames.calls == [[0, 1]] and sessions[1].avatar_frames.calls == [] and sessions[2].avatar_frames.calls == [[0, 1]]
    assert out[0][0].dtype == torch.uint8 and out[1] == (None, [0, 1])


def test_every_validation_error_is_raised_before_any_index_moves():
    m, sessions, bat = _batcher(max_sessions_per_step=2)
    bad = [
        dict(mel_chunks=[_mel(), _mel()]),                                                  # one entry per session
        dict(mel_chunks=[_mel(), _mel(), _mel()]),                                          # more active sessions than a step holds
        dict(mel_chunks=[_mel(), None, torch.zeros(B + 1, 1, 80, 16)]),                     # wrong batch
        dict(mel_chunks=[_mel(), None, torch.zeros(B, 80, 16)]),                            # wrong rank
        dict(mel_chunks=[_mel(), None, np.zeros((B, 1, 80, 16), np.float32)]),              # not a tensor
        dict(mel_chunks=[_mel(), None, _mel().to("meta")]),                                 # wrong device
        dict(mel_chunks=[_mel(), None, None], only=[0, 3]),                                 # no such session
        dict(mel_chunks=[_mel(), None, None], only=[-1]),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            bat.step(**kw)
        assert [s.index for s in sessions] == [0, 0, 0] and not m.calls, kw
    # more sessions than the step holds is fine as long as the ACTIVE ones fit
    out = bat.step([_mel(), None, _mel()])
    assert [o[1] for o in out] == [[0, 1]] * 3
    # paste without AvatarFrames: refused up front as well
    m2 = FakeModel()
    ss = [D.LipSession(m2, _faces(0, 3), avatar_frames=FakeAvatar(3)), D.LipSession(m2, _faces(1, 4))]
    bat2 = D.LipBatcher(m2, ss, batch_size=B, paste=True, device="cpu")
    with pytest.raises(RuntimeError, match="AvatarFrames"):
        bat2.step([_mel(), _mel()])
    assert [s.index for s in ss] == [0, 0] and not m2.calls
    with pytest.raises(RuntimeError, match="one cached full frame"):
        D.LipBatcher(m2, [D.LipSession(m2, _faces(0, 3), avatar_frames=FakeAvatar(4))], batch_size=B, device="cpu")
    with pytest.raises(RuntimeError, match="uint8"):
        D.LipBatcher(m2, [D.LipSession(m2, _faces(0, 3).float())], batch_size=B, device="cpu")


def test_prewarm_sizes_the_handle_with_the_largest_step_first():
    """a Wav2Lip handle's workspace grows with the largest batch it has seen and growing drops its captured graphs: the first forward of prewarm is the
    largest step, then every k * B twice (eager, capture); no session's walk moves"""
    m, sessions, bat = _batcher()
    bat.prewarm()
    sizes = [len(r) for r in m.calls]
    assert sizes == [3 * B, B, B, 2 * B, 2 * B, 3 * B, 3 * B]
    assert [s.index for s in sessions] == [0, 0, 0]


def test_end_to_end_scheduler_refuses_other_frontends_before_it_builds_anything():
    m, sessions, bat = _batcher()
    for fes in ([D.LipASRFrontend(B, device="cpu")] * 3, list(reversed(bat.frontends())), bat.frontends()[:2]):
        with pytest.raises(RuntimeError):
            D.LipEndToEndScheduler(bat, fes)


def test_window_pool_slides_like_the_host_frontend():
    """LipWindowPool.push == lipasr.py:17-21 + :36 as LipASRFrontend keeps them on the host (warm-up: l + r silent chunks), for one session and for several
    at once, whole pool and subset; the chunk starts are mel_chunk_starts of the full window."""
    l, r = 3, 2
    pool = D.LipWindowPool(3, B, fps=50, stride_left=l, stride_right=r, device="cpu")
    assert pool.n == (2 * B + l + r) * 320 and pool.starts == D.mel_chunk_starts(2 * B + l + r, l, r, 50, 1 + pool.n // 200) and len(pool.starts) == B
    rng = np.random.default_rng(0)
    host = [[np.zeros(320, np.float32) for _ in range(l + r)] for _ in range(3)]
    for ks in ([0, 1, 2], [1], [2, 0], [0, 1, 2], [0, 2]):
        blocks = []
        for k in ks:
            new = [rng.standard_normal(320).astype(np.float32) for _ in range(2 * B)]
            host[k] = (host[k] + new)[-(2 * B + l + r):]
            blocks.append(pool.host_block(new))
        pool.push(ks, blocks)
        for k in range(3):
            want = np.concatenate(host[k])
            want = np.concatenate([np.zeros(pool.n - len(want), np.float32), want])
            assert np.array_equal(pool.buf[k].numpy(), want), (ks, k)
        assert np.array_equal(pool.rows(ks).numpy(), pool.buf.numpy()[ks])
    fe = D.LipASRDeviceFrontend(pool, 1)
    fe.warm_up()
    assert not pool.buf[1].any() and pool.buf[0].any() and pool.buf[2].any()
    for bad in ([np.zeros(320, np.float32)] * (2 * B - 1), [np.zeros(160, np.float32)] * (2 * B)):
        with pytest.raises(RuntimeError):
            pool.host_block(bad)
    with pytest.raises(RuntimeError, match="twice"):
        pool.push([0, 0], [pool.host_block([np.zeros(320, np.float32)] * (2 * B))] * 2)


def test_session_scheduler_serves_in_arrival_order_on_an_injected_clock():
    now = [0.0]
    bat = FakeBatcher(3, 2)
    sch = D.LipSessionScheduler(bat, clock=lambda: now[0], sync=lambda: None)
    assert abs(sch.period - B * 0.040) < 1e-12 and abs(sch.hold - sch.period / 4) < 1e-12 and sch.next_due() is None
    assert sch.run_once() == []
    sch.submit(2, "m2", 0.010)
    assert abs(sch.next_due() - (0.010 + sch.hold)) < 1e-12             # one session waits: the step goes out after the hold ...
    now[0] = 0.015
    assert sch.run_once() == []
    sch.submit(0, "m0", 0.012)
    sch.submit(1, None, 0.011)                                           # (a silent batch)
    sch.submit(2, "m2b", 0.013)
    assert sch.next_due() == 0.011                                       # ... or at once when `capacity` sessions wait (the 2nd-oldest arrival)
    done = sch.run_once()
    assert [d[0] for d in done] == [2, 1] and bat.steps[-1] == ([1, 2], [None, None, "mel"])      # oldest first; session 0 waits for the next step
    assert done[1][1] is None and done[1][2] == [0, 1] and abs(done[0][3] - 0.005) < 1e-12
    done = sch.run_once()
    assert [d[0] for d in done] == [0, 2] and done[1][2] == [2, 3]       # session 2's second batch: its own arrival order, consecutive indices
    assert sch.steps == 2 and sch.sessions_served == 4 and sch.backlog() == 0 and sch.next_due() is None


def test_end_to_end_scheduler_defers_a_full_ring_and_offers_it_again(monkeypatch):
    """Host logic of LipEndToEndScheduler with fake rings and a fake batcher: a session whose ring reports no room is deferred (one episode in `ring_full`) while
    the other is served, its window does NOT slide for the deferred batch, and it is served -- in order -- once its consumer has read.  Silent batches deliver B
    (None, idx, audio) tuples; the waiter thread exists only after the first step."""
    fake_cuda_events(monkeypatch)
    now = [0.0]
    bat = FakeBatcher(2, 2)
    pool = D.LipWindowPool(2, B, stride_left=1, stride_right=1, device="cpu")
    melled = []
    pool.mel = lambda wav: (melled.append(wav.clone()), torch.zeros(len(wav) * B, 1, 80, 16))[1]
    rings = [FakeRing(2 * B), FakeRing(2 * B)]
    fes = [D.LipASRDeviceFrontend(pool, k) for k in range(2)]
    with D.LipEndToEndScheduler(bat, fes, rings=rings, clock=lambda: now[0], hold_s=0.0, single_stream=True) as sch:
        assert sch._waiter is None and abs(sch.period - B * 0.040) < 1e-12
        pcm = lambda s, j: [np.full(320, 10 * s + j + 1, np.float32) for _ in range(2 * B)]
        for j in range(3):
            sch.submit(0, pcm(0, j), 0.001 * j)                                             # session 0's consumer never reads
            sch.submit(1, pcm(1, j) if j != 1 else [(c, 1) for c in pcm(1, j)], 0.001 * j + 0.0005)
        with pytest.raises(RuntimeError):
            sch.submit(0, pcm(0, 0)[:-1])                                                   # a malformed batch is refused before it is queued
        served, got1 = [], []
        for _ in range(12):
            now[0] += 0.05
            done = sch.run_once() + sch.drain()
            served += [k for k, *_ in done]
            for k, fr, idx, lat in done:
                if k == 1:
                    got1 += [rings[1].get() for _ in range(B)]
        assert sch._waiter is not None
        assert served.count(1) == 3 and served.count(0) == 2 and len(sch.queues[0]) == 1 and sch.ring_full >= 1
        assert [g[1] for g in got1] == list(range(3 * B))
        assert all(g[0] is not None for g in got1[:B] + got1[2 * B:]) and all(g[0] is None and g[2][0][1] == 1 for g in got1[B:2 * B])
        assert all(np.array_equal(g[2][0][0], pcm(1, i // B)[0]) and len(g[2]) == 2 for i, g in enumerate(got1))
        # the deferred batch has not entered session 0's window: it ends with batch 1's samples, and session 1's silent batch DID enter its window
        assert float(pool.buf[0, -1]) == 2.0 and float(pool.buf[1, -1]) == 13.0
        assert bat.steps[0] == ([0, 1], ["mel", "mel"]) and bat.steps[1] == ([0, 1], ["mel", None])
        assert [tuple(w.shape) for w in melled[:2]] == [(2, pool.n), (1, pool.n)]            # one mel call per step, for the speaking sessions only
        episodes = sch.ring_full
        first = [rings[0].get() for _ in range(2 * B)]                                       # the consumer catches up ...
        assert [g[1] for g in first] == list(range(2 * B))
        for _ in range(4):
            now[0] += 0.05
            served += [k for k, *_ in sch.run_once() + sch.drain()]
        assert served.count(0) == 3 and not sch.pending() and sch.ring_full == episodes      # ... and the batch is served, with the indices that follow
        assert [rings[0].get()[1] for _ in range(B)] == [2 * B, 2 * B + 1] and float(pool.buf[0, -1]) == 3.0
    assert sch._waiter is None                                                               # close() via the context manager


def test_a_failed_step_does_not_slide_the_window_twice(monkeypatch):
    fake_cuda_events(monkeypatch)
    bat = FakeBatcher(1, 1)
    pool = D.LipWindowPool(1, B, stride_left=1, stride_right=1, device="cpu")
    pool.mel = lambda wav: torch.zeros(len(wav) * B, 1, 80, 16)
    good_step, fail = bat.step, [True]

    def step(chunks, only=None):
        if fail[0]:
            raise RuntimeError("step failed")
        return good_step(chunks, only=only)

    bat.step = step
    sch = D.LipEndToEndScheduler(bat, [D.LipASRDeviceFrontend(pool, 0)], rings=[FakeRing(2 * B)], clock=lambda: 1.0, hold_s=0.0, single_stream=True)
    sch.submit(0, [np.full(320, 7.0, np.float32)] * (2 * B), 0.5)
    with pytest.raises(RuntimeError, match="step failed"):
        sch.run_once()
    assert len(sch.queues[0]) == 1 and sch.rings[0].taken == 0
    after_first = pool.buf.clone()
    fail[0] = False
    sch.run_once()
    sch.drain()
    assert torch.equal(pool.buf, after_first) and float(pool.buf[0, 0]) == 0.0 and float(pool.buf[0, -1]) == 7.0     # slid once: the l chunk of silence is still there
    sch.close()


# ---- the C ABI of the two entry points ------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("mf_melspec_windows", "mf_wav2lip_forward_u8_rows")


def test_header_exports_and_ctypes_table_agree_for_the_new_symbols(lib_built):
    from mere_fusion_amd import _lib
    declared = _lib.HEADER.functions
    names = sorted(declared)
    lib = C.CDLL(lib_built)
    for n in NEW_SYMBOLS:
        assert n in names, f"{n} is not declared in merefusion.h"
        assert hasattr(lib, n), f"{n} declared but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names
    # argument counts of the ctypes rows against the declarations
    for n in NEW_SYMBOLS:
        assert len(declared[n][1]) == len(_lib.SIGNATURES[n][1]) == 8, n
    text = open(_lib.HEADER_PATH).read()
    assert "lipasr.py:24-35" in text[text.index("mf_melspec_frames(int n);"):text.index("mf_melspec_windows(")]
    assert _lib.lib().mf_abi_version() == 4


def test_argument_checks_that_need_no_device(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    starts = (C.c_int * 2)(16, 19)
    one = C.c_void_p(64)                                                # a non-null pointer that is never dereferenced: every call below is refused first
    n = 24 * 320
    assert l.mf_melspec_windows(one, 0, 1, starts, 2, one, 0, None) == -1 and b"empty signal" in l.mf_last_error()
    assert l.mf_melspec_windows(one, -5, 1, starts, 2, one, 0, None) == -1
    assert l.mf_melspec_windows(one, n, 0, starts, 2, one, 0, None) == -1 and b"n_windows" in l.mf_last_error()
    assert l.mf_melspec_windows(None, n, 1, starts, 2, one, 0, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_melspec_windows(one, n, 1, None, 2, one, 0, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_melspec_windows(one, n, 1, starts, 2, None, 0, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_melspec_windows(one, n, 1, starts, 0, one, 0, None) == -1
    assert l.mf_melspec_windows(one, n, 1, starts, 2, one, 2, None) == -1 and b"pad_mode" in l.mf_last_error()
    assert l.mf_melspec_windows(one, 400, 1, (C.c_int * 1)(0), 1, one, 1, None) == -1 and b"reflect" in l.mf_last_error()
    T = 1 + n // 200
    for bad in (-1, T - 15, T):
        assert l.mf_melspec_windows(one, n, 1, (C.c_int * 2)(16, bad), 2, one, 0, None) == -1 and b"outside" in l.mf_last_error(), bad
    rows = (C.c_int * 2)(0, 1)
    assert l.mf_wav2lip_forward_u8_rows(None, one, one, 12, rows, one, 2, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_wav2lip_forward_u8_rows(one, one, one, 12, None, one, 2, None) == -1 and b"null" in l.mf_last_error()
    assert l.mf_wav2lip_forward_u8_rows(one, one, None, 12, rows, one, 2, None) == -1
    assert l.mf_wav2lip_forward_u8_rows(one, one, one, 12, rows, one, 0, None) == -1 and b"batch" in l.mf_last_error()
    assert l.mf_wav2lip_forward_u8_rows(one, one, one, 0, rows, one, 2, None) == -1
    for bad in (-1, 12):
        assert l.mf_wav2lip_forward_u8_rows(one, one, one, 12, (C.c_int * 2)(3, bad), one, 2, None) == -1 and b"out of range" in l.mf_last_error(), bad
