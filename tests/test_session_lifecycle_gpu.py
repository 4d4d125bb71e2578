"""GPU: sessions that join and leave a running LipBatcher / MuseBatcher (max_sessions=, pool_rows=; add_session, remove_session) and the schedulers over them.

The reference of every comparison is the EXISTING static route -- a batcher (or scheduler) built with the full session list -- given the same inputs at the same
walk positions: the same sessions in the same slot order make the same batch through the same handle, so every frame is compared bit for bit."""
import numpy as np
import pytest
import torch

from mere_fusion_amd import weights as W

pytestmark = pytest.mark.gpu

B = 2
# avatar -> (cached crops, full frame H x W); D has A's length, so it fits the rows A leaves
AVATARS = {"A": (3, (40, 56)), "B": (5, (64, 48)), "C": (5, (40, 56)), "D": (3, (64, 48))}


@pytest.fixture(scope="module")
def avatar_data():
    data = {}
    for s, (name, (n, (H, Wd))) in enumerate(AVATARS.items()):
        rng = np.random.default_rng(300 + s)
        boxes = [(4 + i + s, 30 + i + s, 6 + 2 * i, 40 + i) for i in range(n)]                   # (y1, y2, x1, x2), lipreal.py:208
        data[name] = (rng.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8), rng.integers(0, 256, (n, H, Wd, 3), dtype=np.uint8), boxes)
    return data


def _session(m, data, name, index=0):
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.paste import AvatarFrames
    faces, frames, boxes = data[name]
    s = D.LipSession(m, faces, avatar_frames=AvatarFrames(frames, boxes, lip_order=True))
    s.index = index
    return s


def _mel(step, name):
    return W.make_lip_inputs(B, 500 + 10 * step + ord(name))[0].cuda()


def test_lip_batcher_sessions_join_and_leave_bit_equal_to_static_batchers(gpu_model_factory, avatar_data):
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    dyn = D.LipBatcher(m, [_session(m, avatar_data, "A"), _session(m, avatar_data, "B")], batch_size=B, paste=True, max_sessions=4, pool_rows=13,
                       max_sessions_per_step=3)
    dyn.prewarm()
    ptr, sizes = dyn.pool.data_ptr(), [B, 2 * B, 3 * B]
    assert [m.graph_captured(n) for n in sizes] == [True] * 3
    walk, step_no = {}, [0]

    def step_and_compare(silent=()):
        """one step of every live session of `dyn` against a LipBatcher built from the same sessions, in slot order, at the same walk positions"""
        t = step_no[0]
        step_no[0] += 1
        names = [None if s is None else s.name for s in dyn.sessions]
        live = [nm for nm in names if nm is not None]
        ref = D.LipBatcher(m, [_session(m, avatar_data, nm, walk.get(nm, 0)) for nm in live], batch_size=B, paste=True)
        got = dyn.step([None if nm is None or nm in silent else _mel(t, nm) for nm in names])
        want = ref.step([None if nm in silent else _mel(t, nm) for nm in live])
        for j, nm in enumerate(live):
            fr, idx = got[names.index(nm)]
            assert idx == want[j][1], (t, nm)
            assert (fr is None and want[j][0] is None) if nm in silent else torch.equal(fr, want[j][0]), (t, nm)
            walk[nm] = walk.get(nm, 0) + B
        assert all(got[k] is None for k, nm in enumerate(names) if nm is None)

    for k, nm in enumerate("AB"):
        dyn.sessions[k].name = nm
    step_and_compare()
    step_and_compare()
    c = _session(m, avatar_data, "C")
    c.name = "C"
    captured = [m.graph_captured(n) for n in range(1, 17)]               # (the handle is shared with other tests: whatever it holds, a join leaves it as it is)
    assert dyn.add_session(c) == 2 and c.pool_offset == 8
    assert [m.graph_captured(n) for n in range(1, 17)] == captured and [m.graph_captured(n) for n in sizes] == [True] * 3       # a join captures and drops nothing
    step_and_compare()
    step_and_compare(silent=("B",))
    assert dyn.remove_session(0).name == "A" and dyn.live() == [1, 2]
    step_and_compare()
    d = _session(m, avatar_data, "D")
    d.name = "D"
    assert dyn.add_session(d) == 0 and d.pool_offset == 0                                           # A's slot and A's rows
    step_and_compare()
    step_and_compare()                                                                              # D walks past its 3 crops: mirrored
    assert dyn.pool.data_ptr() == ptr and [m.graph_captured(n) for n in sizes] == [True] * 3
    assert torch.equal(dyn.pool[0:3].cpu(), torch.from_numpy(avatar_data["D"][0])) and torch.equal(dyn.pool[8:13].cpu(), torch.from_numpy(avatar_data["C"][0]))
    with pytest.raises(RuntimeError, match="no gap of 5 rows: the largest free gap has 0 of 13 rows"):
        dyn.add_session(_session(m, avatar_data, "B"))


def _pcm(name, j, silent=False):
    chunks = [W.make_speech_like_wav(320, 1000 * ord(name) + 9 * j + i) for i in range(2 * B)]
    return [(c, 1) for c in chunks] if silent else chunks


def _rings(names, fmt):
    from mere_fusion_amd.transport import FrameRing, i420_shape
    return [FrameRing(8 * B, i420_shape(*AVATARS[nm][1]) if fmt == "i420" else AVATARS[nm][1] + (3,)) for nm in names]


def _drain_ring(ring):
    out = []
    while True:
        try:
            out.append(ring.get(timeout=0.2))
        except Exception:
            return out


def _same_tuples(got, want):
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        assert a[1] == b[1] and np.array_equal(a[0], b[0]) and len(a[2]) == len(b[2]) == 2
        assert all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("fmt", ["packed", "i420"])
def test_lip_end_to_end_scheduler_with_a_joiner_equals_a_scheduler_built_with_everybody(gpu_model_factory, avatar_data, fmt):
    """A and B run two batches, C joins, all three run three more (one of B's typed silent: idle frames); the reference scheduler holds A, B and C from the start
    and C simply submits nothing before the join.  Same picks, same steps: every tuple of every ring is the same."""
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    rounds = [("AB", ()), ("AB", ()), ("ABC", ()), ("ABC", ("B",)), ("ABC", ())]

    def run(dynamic):
        names = "AB" if dynamic else "ABC"
        kw = dict(max_sessions=4, pool_rows=16, max_sessions_per_step=3) if dynamic else {}
        bat = D.LipBatcher(m, [_session(m, avatar_data, nm) for nm in names], batch_size=B, paste=True, **kw)
        rings = _rings("ABC", fmt)
        now = [0.0]
        with D.LipEndToEndScheduler(bat, rings=rings[:2] + [None, None] if dynamic else rings, clock=lambda: now[0], hold_s=0.0, frame_format=fmt,
                                    idle_frames=True) as sch:
            if dynamic:
                assert sch.windows.staging is not None and sch.windows.buf.shape[0] == 4
            for j, (who, silent) in enumerate(rounds):
                if dynamic and j == 2:
                    assert sch.add_session(_session(m, avatar_data, "C"), ring=rings[2]) == 2
                for nm in who:
                    sch.submit("ABC".index(nm), _pcm(nm, j, nm in silent), 0.001 * j)
                now[0] += 0.01
                done = sch.run_once() + sch.drain()
                assert sorted(k for k, *_ in done) == ["ABC".index(nm) for nm in who]
            if dynamic:
                with pytest.raises(RuntimeError, match="frontend=None"):
                    sch.add_session(_session(m, avatar_data, "D"), ring=rings[2], frontend=sch.frontends[0])
                windows = sch.windows.buf[:3].clone()
            else:
                windows = sch.windows.buf.clone()
        got = [_drain_ring(r) for r in rings]
        for r in rings:
            r.close()
        return got, windows

    want, want_win = run(dynamic=False)
    got, got_win = run(dynamic=True)
    assert [len(g) for g in got] == [5 * B, 5 * B, 3 * B]
    for s in range(3):
        _same_tuples(got[s], want[s])
    assert torch.equal(got_win, want_win)                                                           # the windows slid the same way by either route


def test_lip_scheduler_remove_session_with_batches_in_flight(gpu_model_factory, avatar_data):
    """two batches of A go out back to back (depth 2), A is removed and D joins at once: both batches reach A's ring with the frames a static batcher gives, and
    while A is leaving D gets another slot and other rows"""
    from mere_fusion_amd import lip_driver as D
    m = gpu_model_factory("bf16x3")
    bat = D.LipBatcher(m, [_session(m, avatar_data, "A"), _session(m, avatar_data, "B")], batch_size=B, paste=True, max_sessions=4, pool_rows=16,
                       max_sessions_per_step=3)
    rings = _rings("ABD", "packed")
    now = [0.0]
    with D.LipEndToEndScheduler(bat, rings=rings[:2] + [None, None], clock=lambda: now[0], hold_s=0.0, depth=2) as sch:
        for j in range(3):
            sch.submit(0, _pcm("A", j), 0.001 * j)
        now[0] = 0.01
        early = sch.run_once() + sch.run_once()                          # two steps launched; the third batch stays queued
        sch.remove_session(0)
        assert len(sch.queues[0] or ()) == 0
        k = sch.add_session(_session(m, avatar_data, "D"), ring=rings[2])
        if 0 in sch.leaving:                                             # (the usual case: the steps are still running)
            assert k == 2 and bat.sessions[0] is not None and bat.sessions[0].pool_offset == 0 and bat.sessions[2].pool_offset == 8
        done = early + sch.drain()
        assert [kk for kk, *_ in done] == [0, 0] and not sch.leaving and (bat.sessions[0] is None or k == 0)
        with pytest.raises(RuntimeError, match="submit\\(0\\)" if k != 0 else "submit\\(2\\)"):
            sch.submit(0 if k != 0 else 2, _pcm("A", 3))
        sch.submit(k, _pcm("D", 0), 0.02)
        now[0] = 0.03
        assert [kk for kk, *_ in sch.run_once() + sch.drain()] == [k]
    got_a, got_d = _drain_ring(rings[0]), _drain_ring(rings[2])
    # the reference: a static batcher per avatar, its own frontend, the same PCM
    for name, got, nb in (("A", got_a, 2), ("D", got_d, 1)):
        ref = D.LipBatcher(m, [_session(m, avatar_data, name)], batch_size=B, paste=True)
        fe = ref.frontends()[0]
        assert len(got) == nb * B
        for j in range(nb):
            (fr, idx), = ref.step([fe.run_step(_pcm(name, j))])
            for i in range(B):
                f, fi, audio = got[j * B + i]
                assert fi == idx[i] and np.array_equal(f, fr[i].cpu().numpy()), (name, j, i)
    for r in rings:
        r.close()


def test_muse_batcher_sessions_join_and_leave_bit_equal_to_static_batchers(lib_built):
    from mere_fusion_amd import muse_driver as D
    from mere_fusion_amd.musetalk.config import unet_config_json, vae_config_json
    from mere_fusion_amd.musetalk.models.unet import UNet
    from mere_fusion_amd.musetalk.models.vae import VAE
    from oracle import musetalk_ref as R
    cfg = R.MUSETALK_SMALL
    usd, vsd = W.make_musetalk_unet_state_dict(cfg, 0), W.make_musetalk_vae_state_dict(cfg, 0)
    unet = UNet(unet_config_json(cfg["unet"]), usd, max_batch=3 * B)
    vae = VAE(config=vae_config_json(cfg["vae"]), state_dict=vsd, max_batch=3 * B)
    lats = {nm: [W.make_musetalk_inputs(1, 700 + 10 * s + i)[0] for i in range(n)] for s, (nm, n) in enumerate((("A", 3), ("B", 5), ("C", 5), ("D", 3)))}
    dyn = D.MuseBatcher(unet, vae, [D.MuseSession(lats["A"]), D.MuseSession(lats["B"])], batch_size=B, max_sessions=4, pool_rows=13, max_sessions_per_step=3)
    ptr, names, walk = dyn.pool.data_ptr(), ["A", "B", None, None], {}

    def step_and_compare(t):
        live = [nm for nm in names if nm is not None]
        chunk = {nm: W.make_musetalk_inputs(B, 900 + 10 * t + ord(nm))[1].cuda() for nm in live}
        ref_sessions = [D.MuseSession(lats[nm]) for nm in live]
        for s, nm in zip(ref_sessions, live):
            s.index = walk.get(nm, 0)
        ref = D.MuseBatcher(unet, vae, ref_sessions, batch_size=B)
        got = dyn.step([None if nm is None else chunk[nm] for nm in names])
        want = ref.step([chunk[nm] for nm in live])
        for j, nm in enumerate(live):
            fr, idx = got[names.index(nm)]
            assert idx == want[j][1] and torch.equal(fr, want[j][0]), (t, nm)
            walk[nm] = walk.get(nm, 0) + B

    step_and_compare(0)
    with pytest.raises(RuntimeError, match="session 2: cached latents of shape"):
        dyn.add_session(D.MuseSession([torch.zeros(1, 8, 16, 64)] * 2))
    assert dyn.add_session(D.MuseSession(lats["C"])) == 2 and dyn.sessions[2].pool_offset == 8      # (host latents: copied into the pool on the stream)
    names[2] = "C"
    step_and_compare(1)
    dyn.remove_session(0)
    names[0] = None
    step_and_compare(2)
    assert dyn.add_session(D.MuseSession(torch.cat(lats["D"]).cuda())) == 0 and dyn.sessions[0].pool_offset == 0       # (device latents)
    names[0] = "D"
    step_and_compare(3)
    step_and_compare(4)
    assert dyn.pool.data_ptr() == ptr
