"""GPU: many Wav2Lip sessions through one generator handle -- mf_melspec_windows (every session's mel chunks in one launch), mf_wav2lip_forward_u8_rows
(faces straight from a pool), lip_driver.LipBatcher and LipEndToEndScheduler.

Bars:
  mel windows, pooled faces, a step with ONE active session   bit-equal to the single-session route (same arithmetic, same launch configurations)
  mixed steps (another batch size, other launch configurations) the committed CPU oracle, at the tolerance of test_wav2lip_gpu.py::test_forward_u8_matches_glue_oracle
  pasted uint8 frames of mixed steps                            oracle frames through oracle/blend_ref.lip_paste: at most 1 level, differing share < 1 %
"""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT
from mere_fusion_amd import weights as W
from oracle import blend_ref, glue_ref
from oracle import wav2lip_ref as R

pytestmark = pytest.mark.gpu

TOL_X3 = 1.5e-4            # test_wav2lip_gpu.py:23, as test_forward_u8_matches_glue_oracle applies it (:213): |frames - oracle| <= 255 * TOL_X3
TOL_U8_SHARE = 0.01        # test_muse_driver.py:303: pasted frames against the reference route differ by <= 1 level in < 1 % of the pixels
B = 2
COUNTS = (3, 4, 5)


# ---- 1. mel windows ------------------------------------------------------------------------------------------------------------
def _windows(n):
    """three windows of different seeded noise and an all-zero one between two loud ones (a read across a row boundary would show in it)"""
    rng = np.random.default_rng(11)
    w = np.stack([0.5 * rng.standard_normal(n), np.zeros(n), 0.5 * rng.standard_normal(n), 0.05 * rng.standard_normal(n)]).astype(np.float32)
    return torch.from_numpy(w).cuda()


def _mel_reference(wav, starts, pad):
    from mere_fusion_amd import ops
    out = []
    for row in wav:
        mel = ops.melspec(row, pad)                                    # [80, T]
        out += [mel[:, s:s + 16] for s in starts]
    return torch.stack(out)[:, None]


# (l, r): 10, 10 is the serving configuration: n = 24 x 320 = 7680 samples, T = 39.  (10, 6) is there for the tail clamp (s + 16 > T): at 10, 10 no start of
# either fps reaches the tail
@pytest.mark.parametrize("l,r", [(10, 10), (10, 6)])
@pytest.mark.parametrize("fps", [50, 25])
@pytest.mark.parametrize("pad", [0, 1])
def test_mel_windows_bit_equal_to_melspec_per_row(lib_built, pad, fps, l, r):
    from mere_fusion_amd import ops
    from mere_fusion_amd.lip_driver import mel_chunk_starts
    n = (2 * B + l + r) * 320
    T = 1 + n // 200
    starts = mel_chunk_starts(2 * B + l + r, l, r, fps, T)
    if (l, r) == (10, 10):
        assert n == 7680 and T == 39 and starts == ([16, 19] if fps == 50 else [16, 22])
    else:
        assert T == 33 and starts == [16, 17]                          # 19 (fps 50) and 22 (fps 25) clamped to the tail T - 16 (lipasr.py:31-32)
    wav = _windows(n)
    want = _mel_reference(wav, starts, pad)
    got = ops.melspec_windows(wav, starts, pad)
    assert got.shape == (4 * B, 1, 80, 16) and torch.equal(got, want)
    assert (want[B:2 * B] == -4.0).all() and not (want[:B] == -4.0).all()      # the silent window is silent, its neighbours are not
    one = ops.melspec_windows(wav[2:3], starts, pad)                  # n_windows = 1
    assert torch.equal(one, want[2 * B:3 * B])


def test_mel_windows_bad_arguments_launch_nothing(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    _lib.init_device(0)
    n, T = 7680, 39
    wav = _windows(n)
    out = torch.full((4 * B, 1, 80, 16), 7.0, device="cuda")
    ok = (C.c_int * 2)(16, 19)
    call = lambda wav_p, n_, nw, st, ns, out_p, pad: l.mf_melspec_windows(wav_p, n_, nw, st, ns, out_p, pad, None)
    wp, op = wav.data_ptr(), out.data_ptr()
    bad = [(wp, 0, 4, ok, 2, op, 0), (wp, n, 0, ok, 2, op, 0), (None, n, 4, ok, 2, op, 0), (wp, n, 4, None, 2, op, 0), (wp, n, 4, ok, 2, None, 0),
           (wp, n, 4, (C.c_int * 2)(16, T - 15), 2, op, 0), (wp, n, 4, (C.c_int * 2)(-1, 19), 2, op, 0), (wp, 400, 4, (C.c_int * 1)(0), 1, op, 1),
           (wp, n, 4, ok, 2, op, 3), (wp, n, 4, ok, 0, op, 0)]
    for args in bad:
        assert call(*args) == -1 and l.mf_last_error(), args
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                          # nothing was launched
    assert call(wp, n, 4, ok, 2, op, 0) == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any()


# ---- 2. pooled faces -----------------------------------------------------------------------------------------------------------
def _pool():
    rng = np.random.default_rng(21)
    return torch.from_numpy(rng.integers(0, 256, (sum(COUNTS), 96, 96, 3), dtype=np.uint8))


def _check_pooled_faces(m):
    """forward_u8_rows(mel, pool, rows) == forward_u8(mel, pool[rows]), call after call on one handle at one batch size (eager, capture, replays), each call with
    its own rows: a graph that replayed stale rows, or a reference that did, would differ"""
    pool = _pool().cuda()
    mel = W.make_lip_inputs(6, 31)[0].cuda()
    seen = []
    with torch.no_grad():
        for rows in ([11, 0, 0, 7, 3, 11], [5, 4, 3, 2, 1, 0], [11, 0, 0, 7, 3, 11], [8, 8, 9, 10, 6, 2]):
            want = m.forward_u8(mel, pool[torch.tensor(rows, device="cuda")])
            got = m.forward_u8_rows(mel, pool, rows)
            assert got.shape == (6, 96, 96, 3) and torch.equal(got, want), rows
            seen.append(got.clone())
        assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])
        with pytest.raises(RuntimeError, match="out of range"):
            m.forward_u8_rows(mel, pool, [0, 1, 2, 3, 4, 12])
        with pytest.raises(RuntimeError):
            m.forward_u8_rows(mel, pool, [0, 1, 2])
        with pytest.raises(RuntimeError, match="no CPU"):
            m.forward_u8_rows(mel, pool.cpu(), [0] * 6)


def _new_model():
    from mere_fusion_amd.wav2lip.models import Wav2Lip
    m = Wav2Lip(precision="bf16x3")
    m.load_state_dict(W.make_wav2lip_state_dict(0))
    return m.to("cuda").eval()


def test_pooled_faces_bit_equal_to_the_gathered_route(gpu_model_factory):
    _check_pooled_faces(gpu_model_factory("bf16x3"))


def test_pooled_faces_without_the_graph_in_a_child_process(lib_built):
    """MF_NO_GRAPH is read when a handle is created and the library is loaded once per process: a fresh child, every forward an eager launch chain"""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_lip_batcher as T; T._check_pooled_faces(T._new_model()); print('pooled-ok')"
            % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MF_NO_GRAPH="1"), timeout=300)
    assert out.returncode == 0 and "pooled-ok" in out.stdout, out.stderr[-2000:]


# ---- 3. the batcher against the single-session route ------------------------------------------------------------------------------
SIZES = ((40, 56), (64, 48), (40, 56))                                 # full frames H x W
# (y1, y2, x1, x2) per cached frame, lipreal.py:208; session 1's boxes touch the frame's right and bottom edges
def _boxes(s, n):
    H, Wd = SIZES[s]
    if s == 1:
        return [(H - 30 - i, H, Wd - 25 - i, Wd) for i in range(n)]
    return [(4 + i + 3 * s, 30 + i + 2 * s, 6 + 2 * i, 40 + i + s) for i in range(n)]


def _avatar_data(s, n):
    rng = np.random.default_rng(40 + s)
    H, Wd = SIZES[s]
    return rng.integers(0, 256, (n, H, Wd, 3), dtype=np.uint8), _boxes(s, n)


# step -> per session: "mel" (spoken), None (silent) or "absent" (left out through only=)
PLAN = [("mel", "mel", "mel"), ("mel", "mel", "mel"), ("mel", None, "mel"), ("mel", "absent", "mel"), (None, "mel", None)]


@pytest.fixture(scope="module")
def lip_case(sd0):
    """faces, mel chunks and the CPU oracle's frames for every spoken (step, session) of PLAN: ONE oracle forward, shared and left unchanged"""
    pool = _pool().numpy()
    offs = np.cumsum((0,) + COUNTS[:-1])
    faces = [pool[offs[s]:offs[s] + n] for s, n in enumerate(COUNTS)]
    mels, idxs, index = {}, {}, [0, 0, 0]
    for t, plan in enumerate(PLAN):
        for s, what in enumerate(plan):
            if what == "absent":
                continue
            idxs[t, s] = [glue_ref.mirror_index(COUNTS[s], index[s] + i) for i in range(B)]
            index[s] += B
            if what == "mel":
                mels[t, s] = W.make_lip_inputs(B, 100 + 10 * t + s)[0]
    keys = sorted(mels)
    img = np.concatenate([glue_ref.face_batch(faces[s][idxs[t, s]], [np.zeros((80, 16))] * B)[0] for t, s in keys])
    pred = R.wav2lip_forward(sd0, torch.cat([mels[k] for k in keys]), torch.from_numpy(img)).numpy()
    fr = glue_ref.frames_from_pred(pred)
    oracle = {k: fr[i * B:(i + 1) * B] for i, k in enumerate(keys)}
    return dict(faces=faces, mels=mels, idxs=idxs, oracle=oracle, avatars=[_avatar_data(s, n) for s, n in enumerate(COUNTS)])


def _sessions(m, case, D):
    from mere_fusion_amd.paste import AvatarFrames
    return [D.LipSession(m, case["faces"][s], avatar_frames=AvatarFrames(*case["avatars"][s], lip_order=True)) for s in range(3)]


@pytest.mark.parametrize("paste", [False, True])
def test_batcher_three_sessions_against_the_single_session_route(gpu_model_factory, lip_case, paste):
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    bat = D.LipBatcher(m, _sessions(m, lip_case, D), batch_size=B, paste=paste)
    alone = _sessions(m, lip_case, D)                                  # three independent LipSessions walk beside the batcher
    assert [s.pool_offset for s in bat.sessions] == [0, 3, 7]
    bat.prewarm()
    assert [s.index for s in bat.sessions] == [0, 0, 0]
    worst, share = 0.0, 0.0
    for t, plan in enumerate(PLAN):
        only = None if "absent" not in plan else [s for s in range(3) if plan[s] != "absent"]
        out = bat.step([lip_case["mels"][t, s].cuda() if plan[s] == "mel" else None for s in range(3)], only=only)
        active = [s for s in range(3) if plan[s] == "mel"]
        for s in range(3):
            if plan[s] == "absent":
                assert out[s] is None
                continue
            fr, idx = out[s]
            assert idx == lip_case["idxs"][t, s]
            if plan[s] is None:
                assert fr is None and alone[s].next_indices(B) == idx
                continue
            mel = lip_case["mels"][t, s].cuda()
            ref, ref_idx = alone[s].step_pasted(mel) if paste else alone[s].step(mel)
            assert ref_idx == idx
            if len(active) == 1:                                       # the same batch size, the same launches: bit for bit
                assert torch.equal(fr, ref), (t, s)
            want = lip_case["oracle"][t, s]
            if not paste:
                assert fr.shape == (B, 96, 96, 3) and fr.dtype == torch.float32
                err = float(np.abs(fr.cpu().numpy() - want).max())
                worst = max(worst, err)
                assert err <= 255 * TOL_X3, (t, s, err)
            else:
                H, Wd = SIZES[s]
                frames, boxes = lip_case["avatars"][s]
                assert fr.shape == (B, H, Wd, 3) and fr.dtype == torch.uint8
                got = fr.cpu().numpy()
                for i, fi in enumerate(idx):
                    d = np.abs(got[i].astype(int) - blend_ref.lip_paste(frames[fi], want[i], boxes[fi]).astype(int))
                    share = max(share, float((d > 0).mean()))
                    assert d.max() <= 1 and (d > 0).mean() < TOL_U8_SHARE, \
                        f"step {t} session {s} frame {i}: max difference {d.max()} levels, {100 * (d > 0).mean():.3f} % of the pixels differ (bound {100 * TOL_U8_SHARE} %)"
    print(f"LipBatcher paste={paste}: worst |frames - oracle| {worst:.3e} (gate {255 * TOL_X3:.3e}), largest share of differing pasted pixels {100 * share:.3f} %")
    assert [s.index for s in bat.sessions] == [s.index for s in alone] == [10, 8, 10]


@pytest.mark.parametrize("tune", [False, True])
def test_prewarm_leaves_a_captured_graph_for_every_step_size(lib_built, lip_case, tune):
    """A Wav2Lip handle's workspace grows with the largest batch it has seen, and growing drops every captured graph: a prewarm that walked the sizes upwards
    would leave only the largest one captured.  On a FRESH handle, after prewarm every k * B holds a graph (tune=True: the one captured AFTER the measurement,
    which dropped the earlier one), and a serving step at any size replays: no graph appears or disappears."""
    from mere_fusion_amd import lip_driver as D
    m = _new_model()
    sessions = [D.LipSession(m, lip_case["faces"][s]) for s in range(2 if tune else 3)]
    bat = D.LipBatcher(m, sessions, batch_size=B)
    sizes = [k * B for k in range(1, len(sessions) + 1)]
    bat.prewarm(tune=tune)
    assert [m.graph_captured(n) for n in sizes] == [True] * len(sizes)
    assert not m.graph_captured(B + 1)
    mel = W.make_lip_inputs(B, 5)[0].cuda()
    for active in ([0], list(range(len(sessions))), [0], [len(sessions) - 1]):
        out = bat.step([mel if k in active else None for k in range(len(sessions))])
        assert out[active[0]][0].shape == (B, 96, 96, 3)
        assert [m.graph_captured(n) for n in sizes] == [True] * len(sizes), active


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def _pcm(s, j):
    return [W.make_speech_like_wav(320, 70 * s + 9 * j + i) for i in range(2 * B)]


def _e2e(m, lip_case, single_stream, read=(True, True), NB=3):
    """two sessions, three batches each (session 1's second one typed silent), rings of 2B places; a consumer thread per reading session.  Returns per session the
    tuples its consumer got, the batcher's device results as run_once reported them, and the scheduler."""
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.transport import FrameRing
    sessions = _sessions(m, lip_case, D)[:2]
    bat = D.LipBatcher(m, sessions, batch_size=B, paste=True)
    rings = [FrameRing(2 * B, SIZES[s] + (3,)) for s in range(2)]
    got, dev = [[], []], [[], []]
    want_n = [NB * B if read[s] else 0 for s in range(2)]
    cond = threading.Condition()

    def consume(s):
        while len(got[s]) < want_n[s]:
            item = rings[s].get(timeout=20)
            with cond:
                got[s].append(item)
                cond.notify_all()

    threads = [threading.Thread(target=consume, args=(s,), daemon=True) for s in range(2) if read[s]]
    for th in threads:
        th.start()
    now = [0.0]
    with D.LipEndToEndScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, single_stream=single_stream) as sch:
        assert sch._waiter is None
        for j in range(NB):
            sch.submit(0, _pcm(0, j), 0.001 * j)
            sch.submit(1, [(c, 1) for c in _pcm(1, j)] if j == 1 else _pcm(1, j), 0.001 * j + 0.0005)
        served = []
        for _ in range(8):
            now[0] += 0.001
            done = sch.run_once() + sch.drain()
            for k, fr, idx, lat in done:
                served.append(k)
                dev[k].append((None if fr is None else fr.cpu().numpy(), idx))
                if read[k]:                                            # the reading consumers keep up: every run sees the same rings, hence the same steps
                    with cond:
                        assert cond.wait_for(lambda: len(got[k]) >= B * len(dev[k]), timeout=20)
            if all(read) and not sch.pending():
                break
        assert sch._waiter is not None
        for th in threads:
            th.join(timeout=30)
            assert not th.is_alive()
        stats = dict(served=served, ring_full=sch.ring_full, queued=[len(q) for q in sch.queues])
    for r in rings:
        r.close()
    return got, dev, stats


def test_end_to_end_scheduler_delivers_through_rings(gpu_model_factory, lip_case):
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    got, dev, stats = _e2e(m, lip_case, single_stream=False)
    assert sorted(stats["served"]) == [0, 0, 0, 1, 1, 1] and stats["ring_full"] == 0
    for s in range(2):
        assert [g[1] for g in got[s]] == [D.mirror_index(COUNTS[s], i) for i in range(3 * B)]          # per session, in index order
        for i, (f, idx, audio) in enumerate(got[s]):
            j, silent = i // B, s == 1 and i // B == 1
            pcm = _pcm(s, j)
            assert len(audio) == 2 and all(a[1] == (1 if silent else 0) for a in audio)
            assert np.array_equal(audio[0][0], pcm[2 * (i % B)]) and np.array_equal(audio[1][0], pcm[2 * (i % B) + 1])   # the submitted chunks
            fr, didx = dev[s][j]
            assert didx[i % B] == idx
            if silent:
                assert f is None and fr is None
            else:
                assert f.shape == SIZES[s] + (3,) and np.array_equal(f, fr[i % B])                       # the batcher's device result
    # the same frames as the step-by-step route of this library: LipASRDeviceFrontend.run_step + LipBatcher.step, same step compositions
    sessions = _sessions(m, lip_case, D)[:2]
    bat = D.LipBatcher(m, sessions, batch_size=B, paste=True)
    fes = bat.frontends()
    for j in range(3):
        mels = [fes[s].run_step(_pcm(s, j)) for s in range(2)]
        out = bat.step([mels[0], None if j == 1 else mels[1]])
        for s in range(2):
            if out[s][0] is not None:
                assert np.array_equal(out[s][0].cpu().numpy(), dev[s][j][0]), (s, j)
    # and the device window gives the host frontend's chunks (a single window per call both ways: bit-equal)
    host = D.LipASRFrontend(B)
    host.warm_up()
    devfe = D.LipBatcher(m, sessions[:1], batch_size=B).frontends()[0]
    for j in range(2):
        assert torch.equal(devfe.run_step(_pcm(0, j)), host.run_step(_pcm(0, j)))
    # single_stream=True: the same frames
    got1, dev1, stats1 = _e2e(m, lip_case, single_stream=True)
    assert stats1["served"] == stats["served"]
    for s in range(2):
        for a, b in zip(got[s], got1[s]):
            assert a[1] == b[1] and ((a[0] is None and b[0] is None) or np.array_equal(a[0], b[0]))


def test_end_to_end_scheduler_stalled_consumer(gpu_model_factory, lip_case):
    """session 0's consumer never reads: its ring (2B places) takes two batches, the third is deferred -- ONE episode in `ring_full` -- and session 1 completes"""
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    got, dev, stats = _e2e(m, lip_case, single_stream=False, read=(False, True))
    assert stats["served"].count(1) == 3 and stats["served"].count(0) == 2 and stats["queued"] == [1, 0]
    assert stats["ring_full"] == 1
    assert [g[1] for g in got[1]] == [D.mirror_index(COUNTS[1], i) for i in range(3 * B)] and all(g[0] is None for g in got[1][B:2 * B])
