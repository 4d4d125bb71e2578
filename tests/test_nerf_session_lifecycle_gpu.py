"""GPU: ER-NeRF sessions that join and leave a running batcher -- mf_nerf_feat_rows_load against torch indexing, `NerfFeaturePool.join` against `warm_up` with
the real (small) wav2vec2 net, a `NerfBatcher` whose sessions come and go against one built with everybody, and `NerfEndToEndScheduler` with a joiner and a
leaver against one built with the full list.  Everything new only moves fp32 values or runs code that ran before, so every comparison is for equal bits.  The
small scene and the sessions are those of tests/test_nerf_serving.py."""
import numpy as np
import pytest
import torch

import nerf_serving_util as U
from test_nerf_serving import B, TYPES, _auds, _block, _sessions, scene  # noqa: F401  (scene: the module-scoped fixture, one instance for this file)

pytestmark = pytest.mark.gpu


# ---- 1. the launch ------------------------------------------------------------------------------------------------------------------------------
def _picked(N, n_rows):
    """n_rows distinct rows of N in an order of their own; in the 66-row pool 65 rows (two launches: 64 + 1), which leaves one row unnamed"""
    order = [int(k) for k in torch.randperm(N, generator=torch.Generator().manual_seed(N + n_rows))]
    return order[:n_rows]


@pytest.mark.parametrize("N, R, dim", [(3, 32, 29), (3, 20, 44), (2, 32, 1024), (66, 32, 29)])
def test_rows_load_equals_torch_indexing(lib_built, N, R, dim):
    """The pool is one allocation of N + 1 rows filled with a sentinel (seeded noise); the source is its last row, the scratch row of a NerfFeaturePool.  After
    the call the whole buffers are compared, so every row that was not named -- the source included -- is shown untouched."""
    from mere_fusion_amd import ops
    g = torch.Generator().manual_seed(1000 * N + dim)
    rings0 = torch.randn((N + 1, R, dim), generator=g).cuda()
    hist0 = torch.randn((N + 1, 8, dim, 16), generator=g).cuda()
    for n_rows in (1, 2) + ((65,) if N == 66 else ()):
        rows = _picked(N, n_rows)
        for from_snapshot in (True, False):
            for with_hist in (True, False):
                rings, hist = rings0.clone(), hist0.clone() if with_hist else None
                ops.nerf_feat_rows_load(rings, hist, rows, rings[N] if from_snapshot else None, hist[N] if from_snapshot and with_hist else None)
                want = rings0.clone()
                want[rows] = rings0[N] if from_snapshot else 0.0
                assert torch.equal(rings, want), (n_rows, from_snapshot, with_hist)
                if with_hist:
                    want = hist0.clone()
                    want[rows] = hist0[N] if from_snapshot else 0.0
                    assert torch.equal(hist, want), (n_rows, from_snapshot, with_hist)
    # a ring snapshot with a zeroed history (a source per buffer), and a source of its own allocation
    rings, hist, own = rings0.clone(), hist0.clone(), torch.randn((R, dim), generator=g).cuda()
    ops.nerf_feat_rows_load(rings, hist, [0], own, None)
    assert torch.equal(rings[0], own) and torch.equal(rings[1:], rings0[1:]) and float(hist[0].abs().max()) == 0.0 and torch.equal(hist[1:], hist0[1:])


def test_rows_load_refusals(lib_built):
    from mere_fusion_amd import ops
    rings, hist = torch.ones((3, 32, 8)).cuda(), torch.ones((3, 8, 8, 16)).cuda()
    for kw, text in ((dict(rings=rings.cpu()), "no CPU fallback"), (dict(src_ring=rings[2].cpu()), "no CPU fallback"), (dict(rows=[0, 0]), "twice"),
                     (dict(rows=[3]), "out of range"), (dict(rows=[]), "picked"), (dict(rows=[2, 0]), "ring source overlaps session row 2"),
                     (dict(src_hist=hist[1]), "history source overlaps session row 1"), (dict(hist=None), "without a history"),
                     (dict(src_ring=rings[2, :16]), "src_ring must be"), (dict(rings=rings.double()), "fp32"), (dict(hist=hist[:2]), "2 histories for 3 rings")):
        with pytest.raises(RuntimeError, match=text):
            ops.nerf_feat_rows_load(**{**dict(rings=rings, hist=hist, rows=[0, 1], src_ring=rings[2], src_hist=hist[2]), **kw})
    torch.cuda.synchronize()
    assert float(rings.min()) == 1.0 and float(hist.min()) == 1.0         # nothing was launched


# ---- 2. join against warm_up, with the real net ----------------------------------------------------------------------------------------------------
def test_join_leaves_what_warm_up_leaves_with_the_real_net(lib_built):
    """The smallest wav2vec2 configuration of tests/test_wav2vec2.py.  warm_state() runs what warm_up([k]) runs -- single-window net calls on silence -- so the
    joined row is warm_up's bit for bit (the handle gives the same bits run to run), and one step of speech after it too."""
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC
    from mere_fusion_amd.nerf_serving import NerfFeaturePool
    cfg = W.WAV2VEC2_SMALL
    net = HipWav2Vec2ForCTC(cfg, W.make_wav2vec2_state_dict(cfg, 0), max_windows=3)
    pool = NerfFeaturePool(1, net, 44, max_sessions=3)
    fresh = NerfFeaturePool(3, net, 44)
    k = 2
    fresh.warm_up([k])
    pool.warm_state()
    calls, launches = pool.net_calls, pool.launches
    pool.join([k])
    assert pool.net_calls == calls and pool.launches == launches + 1 and pool.live() == [0, 2]
    assert float(pool.rings[k].abs().max()) > 1e-3                       # (the net's answer to silence is not zeros: the snapshot carries values)

    def same():
        assert torch.equal(pool.rings[k], fresh.rings[k]) and torch.equal(pool.hist[k], fresh.hist[k])
        assert U.pool_counters(pool, k) == U.pool_counters(fresh, k) and (pool.head[k], pool.first[k], pool.win_fronts[k]) == (fresh.head[k], fresh.first[k], fresh.win_fronts[k])
        assert np.array_equal(pool.pcm[k], fresh.pcm[k])

    same()
    assert U.pool_counters(pool, k) == (22, 2, 24, 8) and pool.first[k]
    speech = W.make_speech_like_wav(2 * B * U.CHUNK, 1) * 0.5
    chunks = [speech[i * U.CHUNK:(i + 1) * U.CHUNK] for i in range(2 * B)]
    assert torch.equal(pool.step([k], [chunks], B), fresh.step([k], [chunks], B))
    same()
    # a second joiner, after the first has moved on, gets the snapshot and not the first one's state
    pool.join([1])
    again = NerfFeaturePool(2, net, 44)
    again.warm_up([1])
    assert torch.equal(pool.rings[1], again.rings[1]) and torch.equal(pool.hist[1], again.hist[1]) and U.pool_counters(pool, 1) == (22, 2, 24, 8)
    assert not torch.equal(pool.rings[1], pool.rings[k])


# ---- 3. the batcher -----------------------------------------------------------------------------------------------------------------------------------
def _five(m_shared, m_own, inp):
    """the four sessions of tests/test_nerf_serving.py over ONE model, and a fifth with a model object of its own"""
    return _sessions(m_shared, inp) + [_sessions(m_own, inp)[0]]


# who is present in which step (session numbers of _five): 2 and 4 join before step 1; 1 leaves and 3 joins -- into 1's slot -- before step 2
PRESENT = [[0, 1], [0, 1, 2, 4], [0, 3, 2, 4], [0, 3, 2, 4]]


def _inputs_for(g, j, n):
    return (_auds(g, j, n), TYPES[j % 4])


def test_batcher_with_joiners_and_leavers_equals_one_built_with_everybody(lib_built, scene):
    """Every frame and index of every session, bit for bit.  A step's head calls see the same sessions either way (`only=` in the full batcher), so the frames
    are the same by construction as long as a join moves nothing it should not: the slot's EMA, the custom-video counters, the loader's position."""
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m_bat, m_ref, g, inp = scene
    m_bat.enc_a = m_ref.enc_a = None
    warm = _auds(g, 0, 0)[0]
    # the batcher built with everybody: session j in slot j
    full_s = [f() for f in _five(m_bat, m_ref, inp)]
    full = NerfBatcher(full_s)
    full.prewarm(warm)
    done, want = [0] * 5, []
    for present in PRESENT:
        out = full.step([_inputs_for(g, j, done[j]) if j in present else None for j in range(5)], only=present)
        want.append({j: out[j] for j in present})
        for j in present:
            done[j] += 1
    # the one whose sessions come and go
    m_bat.enc_a = m_ref.enc_a = None
    make = _five(m_bat, m_ref, inp)
    ss = {j: make[j]() for j in range(5)}
    bat = NerfBatcher([ss[0], ss[1]], max_sessions=4)
    assert bat.sessions == [ss[0], ss[1], None, None] and bat.max_pixels == ss[0].H * ss[0].W
    bat.prewarm(warm)
    most = bat._most_frames(m_bat)
    slot, done = {0: 0, 1: 1}, [0] * 5
    for n, present in enumerate(PRESENT):
        if n == 1:
            slot[2] = bat.add_session(ss[2])
            keep = (ss[4].index, ss[4].last_index, dict(ss[4].custom_index), m_ref.enc_a)
            bat.prewarm_session(ss[4], warm)                             # a new model object: its first-time costs, before it joins
            assert (ss[4].index, ss[4].last_index, dict(ss[4].custom_index), m_ref.enc_a) == keep
            slot[4] = bat.add_session(ss[4])
            assert (slot[2], slot[4]) == (2, 3)
        if n == 2:
            assert bat.remove_session(slot.pop(1)) is ss[1] and bat.enc_a[1] is None
            slot[3] = bat.add_session(ss[3])
            assert slot[3] == 1 and bat.enc_a[1] is None                 # the leaver's slot, without the leaver's EMA
        assert sorted(slot) == sorted(present) and bat._most_frames(m_bat) == bat._most_frames(m_ref) == most
        inputs = [None] * 4
        for j in present:
            inputs[slot[j]] = _inputs_for(g, j, done[j])
            done[j] += 1
        out = bat.step(inputs)
        for j in present:
            (frames, idx), (w_frames, w_idx) = out[slot[j]], want[n][j]
            assert idx == w_idx and frames.dtype == torch.uint8 and torch.equal(frames, w_frames), (n, j)
        assert [o is None for o in out] == [s is None for s in bat.sessions]
    for j, k in slot.items():
        assert torch.equal(bat.enc_a[k], full.enc_a[j]) and ss[j].custom_index == full_s[j].custom_index, j
    assert ss[3].custom_index[2] == full_s[3].custom_index[2] > 0 and float(want[1][0][0][0].float().std()) > 1.0
    big = _sessions(m_bat, inp)[0]()
    big.H, big.W = big.H + 1, big.W
    with pytest.raises(RuntimeError, match=f"{big.H * big.W} pixels; the frame batch was sized for {bat.max_pixels}"):
        (bat.remove_session(0), bat.add_session(big))


# ---- 4. the end-to-end scheduler ------------------------------------------------------------------------------------------------------------------
PCM_TYPES = [[0] * 8, [0, 0, 1, 1, 2, 2, 0, 1], [2, 2, 2, 2, 0, 0, 1, 1]]
# rounds of (sessions that submit their next batch): session 2 joins before round 1, session 1 leaves before round 2
ROUNDS = [[0, 1], [0, 1, 2], [0, 2], [0, 2]]


def _pairs(j, n):
    return list(zip(_block(j, B * n, B), PCM_TYPES[j]))


def _run(sch, rings, slot_of, events=()):
    """drives ROUNDS through a scheduler; events: {round: callable} run before the round's submits.  Returns per session the tuples its ring delivered"""
    now, got, done = [0.0], {0: [], 1: [], 2: []}, [0, 0, 0]
    sch.clock = lambda: now[0]
    for n, who in enumerate(ROUNDS):
        if n in events:
            events[n]()
        for j in who:
            sch.submit(slot_of[j], _pairs(j, done[j]), now[0] + 0.0001 * j)
            done[j] += 1
        now[0] += 0.05
        served = sch.run_once() + sch.drain()
        assert sorted(k for k, *_ in served) == sorted(slot_of[j] for j in who), (n, served)
        for j in who:
            got[j] += [rings[j].get(timeout=10) for _ in range(B)]
    return got


@pytest.mark.parametrize("single_stream, frame_format", [(False, "packed"), (True, "packed"), (False, "i420")])
def test_scheduler_with_a_joiner_and_a_leaver_equals_one_built_with_the_full_list(lib_built, scene, single_stream, frame_format):
    """What each session's ring delivers: frames, indices and audio pairs, bit for bit.  The net is nerf_serving_util.StubNet, a callable whose output row
    depends only on its input row through elementwise, fixed-order ops, so net calls of S = 1 (the joiner's warm state), S = 2 and S = 3 windows agree by
    construction and the comparison is about the life cycle alone."""
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfEndToEndScheduler, NerfFeaturePool
    from mere_fusion_amd.transport import FrameRing, i420_shape
    m_bat, m_ref, g, inp = scene
    make = _sessions(m_bat, inp)[1:]                                      # (flip, body frames, custom-video cycle)
    slots = lambda s: i420_shape(*s[:2]) if frame_format == "i420" else s
    kw = dict(hold_s=0.0, single_stream=single_stream, frame_format=frame_format)

    def through(build):
        m_bat.enc_a = None
        ss = [f() for f in make]
        shapes = NerfBatcher(ss).out_shape
        rings = [FrameRing(2 * B, slots(s)) for s in shapes]
        try:
            return build(ss, rings)
        finally:
            for r in rings:
                r.close()

    def full(ss, rings):
        pool = NerfFeaturePool(3, U.StubNet(44, "cuda"), 44)
        pool.warm_up()
        bat = NerfBatcher(ss, pool=pool)
        bat.prewarm()
        with NerfEndToEndScheduler(bat, rings=rings, **kw) as sch:
            return _run(sch, rings, {0: 0, 1: 1, 2: 2})

    def dynamic(ss, rings):
        net = U.StubNet(44, "cuda")
        pool = NerfFeaturePool(2, net, 44, max_sessions=3)
        pool.warm_up()
        bat = NerfBatcher(ss[:2], pool=pool, max_sessions=3)
        bat.prewarm()                                                    # (computes the pool's warm state too)
        slot_of = {0: 0, 1: 1}
        with NerfEndToEndScheduler(bat, rings=rings[:2] + [None], **kw) as sch:
            def join():
                calls = len(net.calls)
                slot_of[2] = sch.add_session(ss[2], ring=rings[2])
                assert slot_of[2] == 2 and len(net.calls) == calls and pool.live() == [0, 1, 2]

            def leave():
                sch.remove_session(slot_of.pop(1))
                assert pool.live() == [0, 2] and bat.live() == [0, 2] and sch.rings[1] is None      # nothing was in flight: released at once

            with pytest.raises(RuntimeError, match="ring 2 has slots of shape"):
                sch.add_session(ss[2], ring=rings[1])                    # session 1's ring: the size of its body frames
            assert pool.live() == [0, 1] and bat.live() == [0, 1]
            got = _run(sch, rings, slot_of, {1: join, 2: leave})
            late = make[1]()                                             # a joiner into the leaver's slot and pool row
            assert sch.add_session(late, ring=FrameRing(B, slots(bat.session_hw(late) + (3,)))) == 1 and U.pool_counters(pool, 1) == (22, 2, 24, 8)
            sch.rings[1].close()
            return got

    want, got = through(full), through(dynamic)
    for j in range(3):
        assert len(got[j]) == len(want[j]) == B * sum(j in who for who in ROUNDS)
        for i, ((frame, idx, audio), (w_frame, w_idx, w_audio)) in enumerate(zip(got[j], want[j])):
            assert idx == w_idx and frame.dtype == np.uint8 and np.array_equal(frame, w_frame), (j, i)
            assert len(audio) == 2 and all(a[1] == w[1] and np.array_equal(a[0], w[0]) for a, w in zip(audio, w_audio)), (j, i)
    assert float(np.std(got[0][0][0].astype(np.float32))) > 1.0
