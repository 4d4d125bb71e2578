"""GPU: the multi-session ER-NeRF stack (mere_fusion_amd/nerf_serving.py) and the two launches under it (csrc/mf_nerf_featpool.hip).  Everything new only moves
fp32 values or calls code that already ran one session at a time, so every comparison is for equal bits: the pool against one `NerfASRFrontend` per session
stepped the reference's way, the batcher against each session alone through `NerfSession.step`, the end-to-end scheduler against both in sequence.  Only the
real wav2vec2 net is held to a tolerance: the one tests/test_wav2vec2.py already sets for a window inside a batch against the window alone (2e-5)."""
import numpy as np
import pytest
import torch

import nerf_serving_util as U

pytestmark = pytest.mark.gpu

B = 4


def _block(k, first, n):
    return sum((U.pcm(k, first + b) for b in range(n)), [])


# ---- 1. the pool against NerfASRFrontend -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("att", [2, 0])
@pytest.mark.parametrize("dim", [29, 44, 1024])
def test_pool_equals_one_frontend_per_session(lib_built, dim, att):
    """12 frames of 3 sessions right after warm_up, as three steps of B = 4: the four windows of the first call, windows that wrap round the ring's end
    (front > tail), three scatters, and windows that are views of rows a later scatter rewrites.  dim 29 and 44 leave one partly filled tile, 1024 is 16 tiles."""
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    net = U.StubNet(dim, "cuda", hidden=dim == 1024)
    pool = NerfFeaturePool(3, net, dim, att=att)
    pool.warm_up()
    fes = [U.warmed_frontend(U.StubNet(dim, "cuda", hidden=dim == 1024), dim, att, "cuda") for _ in range(3)]
    l0, wrapped = pool.launches, False
    for step in range(3):
        got = pool.step([0, 1, 2], [_block(k, B * step, B) for k in range(3)], B)
        assert tuple(got.shape) == (3, B, 8 if att else 1, dim, 16) and got.dtype == torch.float32
        for k in range(3):
            for b in range(B):
                wrapped |= fes[k].front > fes[k].tail
                want = U.reference_frame(fes[k], U.pcm(k, B * step + b))
                assert got[k, b].is_contiguous() and torch.equal(got[k, b], want), (step, k, b, float((got[k, b] - want).abs().max()))
            assert U.pool_counters(pool, k) == U.counters(fes[k])
    assert wrapped and net.calls == [3] * 5 and pool.launches - l0 == 3 * (B + 1)          # B window launches + one scatter per step, for any number of sessions
    assert float(got.abs().max()) > 0.5


def test_pool_with_sessions_out_of_phase_and_a_restart(lib_built):
    """Steps of one frame: sessions {0, 2} alone for three frames, so that session 1's net window completes in another frame than theirs and `ks` is a subset of
    the rows; then session 1 is warmed up again mid-run while the others go on."""
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    dim = 44
    pool = NerfFeaturePool(3, U.StubNet(dim, "cuda"), dim)
    pool.warm_up()
    fes = [U.warmed_frontend(U.StubNet(dim, "cuda"), dim, 2, "cuda") for _ in range(3)]
    done = [0, 0, 0]
    for f in range(16):
        if f == 9:
            pool.warm_up(1)
            fes[1] = U.warmed_frontend(U.StubNet(dim, "cuda"), dim, 2, "cuda")
        ks = [2, 0] if f in (2, 3, 4) else [0, 1, 2]
        got = pool.step(ks, [U.pcm(k, done[k]) for k in ks], 1)
        for i, k in enumerate(ks):
            want = U.reference_frame(fes[k], U.pcm(k, done[k]))
            done[k] += 1
            assert torch.equal(got[i, 0], want), (f, k)
            assert U.pool_counters(pool, k) == U.counters(fes[k])
    assert done == [16, 13, 16]


def test_pool_with_the_real_net_equals_single_window_frontends(lib_built):
    """The smallest wav2vec2 configuration of tests/test_wav2vec2.py: one call of three windows against three calls of one, at that file's tolerance for a window
    inside a batch against the window alone."""
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    cfg = W.WAV2VEC2_SMALL
    sd = W.make_wav2vec2_state_dict(cfg, 0)
    pool = NerfFeaturePool(3, HipWav2Vec2ForCTC(cfg, sd, max_windows=3), 44)
    pool.warm_up()
    single = HipWav2Vec2ForCTC(cfg, sd, max_windows=1)
    fes = [U.warmed_frontend(single, 44, 2, "cuda") for _ in range(3)]
    speech = [W.make_speech_like_wav(2 * B * 2 * U.CHUNK, s) * (0.3 + 0.3 * s) for s in range(3)]
    chunks = lambda k, f: [speech[k][(2 * f + i) * U.CHUNK:(2 * f + i + 1) * U.CHUNK] for i in range(2)]
    worst = 0.0
    for step in range(2):
        got = pool.step([0, 1, 2], [sum((chunks(k, B * step + b) for b in range(B)), []) for k in range(3)], B)
        for k in range(3):
            for b in range(B):
                want = U.reference_frame(fes[k], chunks(k, B * step + b))
                worst = max(worst, float((got[k, b] - want).abs().max()))
    print(f"[nerf pool, wav2vec2 small] three windows per call against one: L-inf {worst:.3e} (|feature| max {float(got.abs().max()):.2f})")
    assert float(got.abs().max()) > 0.1 and worst <= 2e-5


# ---- 2. the batcher ----------------------------------------------------------------------------------------------------------------------------
def _sessions(model, inp):
    """four sessions over ONE model: two plain ones on different poses, one with body frames, one with a custom-video cycle of its output size"""
    from mere_fusion_amd.nerf_driver import NerfSession
    import test_nerf_session as T
    flip = {k: v.flip(0) for k, v in inp.items()}
    common = dict(gui_size=(T.GH, T.GW), render_kw=T.RENDER_KW)
    mk = lambda i, **kw: NerfSession(model, i["poses"].cuda(), T.INTR, T.S, T.S, T._ref_get_rays, eye_area=i["eye"].cuda(), bg=i["bg"].cuda(),
                                     torso_imgs=i["torso"].cuda(), **common, **kw)
    custom = torch.randint(0, 256, (3, T.GH, T.GW, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).cuda()
    return [lambda: mk(inp), lambda: mk(flip), lambda: mk(inp, fullbody_frames=inp["body"].cuda(), fullbody_offset=(T.X0, T.Y0)),
            lambda: mk(flip, custom_img_cycle={2: custom})]


TYPES = [[(0, 0)] * B, [(0, 0), (1, 1), (0, 1), (0, 0)], [(0, 0)] * B, [(2, 2), (0, 0), (2, 0), (2, 2)]]


def _auds(g, k, step):
    base = torch.from_numpy(np.ascontiguousarray(g["auds"])).cuda()
    return torch.stack([base * (1.0 + 0.05 * (B * step + b) + 0.01 * k) for b in range(B)])


@pytest.fixture(scope="module")
def scene():
    import test_nerf_session as T
    m_bat, g = T._make_model()
    m_ref, _ = T._make_model()
    m_bat.smooth_lips = m_ref.smooth_lips = True
    return m_bat, m_ref, g, T._session_inputs()


def test_batcher_equals_every_session_alone(lib_built, scene):
    import test_nerf_session as T
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m_bat, m_ref, g, inp = scene
    m_bat.enc_a = m_ref.enc_a = None
    ss = [f() for f in _sessions(m_bat, inp)]
    bat = NerfBatcher(ss)
    assert bat.out_shape == [(T.GH, T.GW, 3), (T.GH, T.GW, 3), (T.FH, T.FW, 3), (T.GH, T.GW, 3)]
    bat.prewarm(_auds(g, 0, 0)[0])
    assert [s.index for s in ss] == [0] * 4 and m_bat.enc_a is None and bat.enc_a == [None] * 4
    outs = [bat.step([(_auds(g, k, step), TYPES[k]) for k in range(4)]) for step in range(2)]
    # `only=`: sessions 0 and 2 sit a step out; their indices and EMAs do not move
    keep = [ss[0].index, ss[2].index, bat.enc_a[0], bat.enc_a[2]]
    third = bat.step([None, (_auds(g, 1, 2), TYPES[1]), "not looked at", (_auds(g, 3, 2), TYPES[3])], only=[3, 1])
    assert third[0] is None and third[2] is None and [ss[0].index, ss[2].index] == keep[:2] and bat.enc_a[0] is keep[2] and bat.enc_a[2] is keep[3]
    outs.append(third)
    for k, make in enumerate(_sessions(m_ref, inp)):                  # each session alone, the route of one session per model: a fresh EMA
        m_ref.enc_a = None
        s = make()
        for step in range(3):
            if outs[step][k] is None:
                assert step == 2 and k in (0, 2)
                continue
            frames, idx = outs[step][k]
            assert frames.dtype == torch.uint8 and tuple(frames.shape) == (B,) + bat.out_shape[k] and len(idx) == B
            a = _auds(g, k, step)
            for b in range(B):
                want = s.step(a[b], TYPES[k][b])
                assert idx[b] == s.last_index and torch.equal(frames[b], want), (k, step, b)
        assert torch.equal(bat.enc_a[k], m_ref.enc_a) and s.custom_index == ss[k].custom_index
    assert ss[3].custom_index[2] == 6 and float(outs[1][0][0].float().std()) > 1.0
    assert not torch.equal(bat.enc_a[0], bat.enc_a[1])                # one EMA per session, although the model is shared
    with pytest.raises(RuntimeError, match=r"custom_img_cycle\[2\]"):   # the 30 x 26 cycle of tests/test_nerf_session.py under 52 x 44 body frames
        NerfBatcher([T._make_session(m_bat, inp)])


# ---- 3. the end-to-end scheduler ---------------------------------------------------------------------------------------------------------------
N_BATCH = 3
PCM_TYPES = [[0] * 8, [0, 0, 1, 1, 2, 2, 0, 1], [2, 2, 2, 2, 0, 0, 1, 1]]               # per session: the types of a batch's 2B chunks


def _pairs(k, j):
    return list(zip(_block(k, B * j, B), PCM_TYPES[k]))


@pytest.fixture(scope="module")
def sequential(scene):
    """the parent commit's route: each session on its own, one NerfASRFrontend and NerfSession.step per frame -> per session the (frame, idx, audio) tuples"""
    m_bat, m_ref, g, inp = scene
    want = []
    for k, make in enumerate(_sessions(m_ref, inp)[1:]):              # (flip, body frames, custom-video cycle)
        m_ref.enc_a = None
        s, fe = make(), U.warmed_frontend(U.StubNet(44, "cuda"), 44, 2, "cuda")
        rows = []
        for j in range(N_BATCH):
            pairs = _pairs(k, j)
            for b in range(B):
                two = pairs[2 * b:2 * b + 2]
                auds = U.reference_frame(fe, [c for c, _ in two])
                frame = s.step(auds, (two[0][1], two[1][1]))
                rows.append((frame.cpu().numpy(), s.last_index, two))
        want.append(rows)
    return want


@pytest.mark.parametrize("single_stream", [False, True])
def test_end_to_end_scheduler_equals_the_sequential_route(lib_built, scene, sequential, single_stream):
    """Three sessions, PCM pairs of mixed types in, what reaches each FrameRing out.  Session 2's ring holds one batch and its consumer reads late: the session is
    deferred and later served with nothing lost.  An injected clock drives the picks."""
    import test_nerf_session as T
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfEndToEndScheduler, NerfFeaturePool
    from mere_fusion_amd.transport import FrameRing
    m_bat, m_ref, g, inp = scene
    m_bat.enc_a = None
    ss = [f() for f in _sessions(m_bat, inp)[1:]]
    pool = NerfFeaturePool(3, U.StubNet(44, "cuda"), 44)
    pool.warm_up()
    bat = NerfBatcher(ss, pool=pool)
    bat.prewarm()
    shapes = bat.out_shape
    rings = [FrameRing(3 * B, shapes[0]), FrameRing(3 * B, shapes[1]), FrameRing(B, shapes[2])]
    now = [0.0]
    got = [[], [], []]
    try:
        with NerfEndToEndScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, single_stream=single_stream) as sch:
            for j in range(N_BATCH):
                for k in range(3):
                    sch.submit(k, _pairs(k, j), 0.001 * j + 0.0001 * k)
            served, unread = [], [0, 0, 0]
            for it in range(12):
                now[0] += 0.05
                done = sch.run_once() + sch.drain()
                served += [k for k, *_ in done]
                for k, *_ in done:
                    unread[k] += 1
                for k in (0, 1) if it < 6 else (0, 1, 2):               # session 2's consumer starts reading late
                    for _ in range(B * unread[k]):                        # (a published batch is B descriptors in one message: read exactly what was served)
                        got[k].append(rings[k].get(timeout=10))
                    unread[k] = 0
            assert sorted(served) == [0] * N_BATCH + [1] * N_BATCH + [2] * N_BATCH and sch.ring_full >= 1 and not sch.pending(), (served, sch.ring_full, unread)
    finally:
        for r in rings:
            r.close()
    for k in range(3):
        assert len(got[k]) == len(sequential[k]) == N_BATCH * B
        for i, ((frame, idx, audio), (w_frame, w_idx, w_audio)) in enumerate(zip(got[k], sequential[k])):
            assert idx == w_idx and frame.dtype == np.uint8 and np.array_equal(frame, w_frame), (k, i)
            assert len(audio) == 2 and all(a[1] == w[1] and np.array_equal(a[0], w[0]) for a, w in zip(audio, w_audio)), (k, i)
    # nerfreal.py:98: a custom-video frame needs both types non-zero AND a cycle registered for the first: (2, 2), not (1, 1)
    assert ss[2].custom_index[2] == N_BATCH * sum(1 for b in range(B) if PCM_TYPES[2][2 * b] == 2 and PCM_TYPES[2][2 * b + 1] == 2) == 6
