"""CPU: the three stages of `NerfBatcher.step` (mere_fusion_amd/nerf_serving.py) -- begin, group and render, end -- with stand-in sessions and models in the style
of tests/test_nerf_serving_host.py: which frames reach which `render_frames` call, in which order and with which keywords; what never reaches a renderer; who
keeps the one-step-per-frame route; and that a refused input moves nothing.  The stand-in model's "render" is an EMA over the frames' audio, as the real
renderers keep one, so the routes can be compared value for value."""
import pytest
import torch

B = 4


class FakeModel:
    """render_frames records (the frames' tags, the keywords) and the frame slots asked for per call; a frame's image is filled with its session's EMA after the frame"""

    def __init__(self):
        self.enc_a, self.calls, self.reserved = None, [], []

    def render_frames(self, jobs, reserve_frames=0, **kw):
        self.calls.append(([j["tag"] for j in jobs], dict(kw)))
        self.reserved.append(reserve_frames)
        res = []
        for j in jobs:
            box = j.get("ema")
            if box is not None:
                self.enc_a = box[0]
            m = float(j["auds"].mean())
            self.enc_a = m if self.enc_a is None else 0.5 * self.enc_a + m
            if box is not None:
                box[0] = self.enc_a
            res.append({"image": torch.full((j["rays_o"].shape[0], 3), self.enc_a)})
        return res


class _SessionState:
    def __init__(self, model, value, rays=24, render_kw=None, size=5, hw=(6, 4), cycle=None):
        self.model, self.value, self.rays, self.size, self.GH, self.GW = model, value, rays, size, hw[0], hw[1]
        self.render_kw = dict(dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4) if render_kw is None else dict(render_kw)
        self.fullbody_frames, self.aabb_infer = None, None
        self.custom_img_cycle = dict(cycle or {})
        self.custom_index = {k: 0 for k in self.custom_img_cycle}
        self.index, self.last_index, self.last_audio_index, self.begun, self.stepped, self.bound = 0, None, None, 0, 0, 0


class FakeSession(_SessionState):
    """the surface of NerfSession the batcher uses: begin / end / bind_aabb / step over a loader of `size` poses; a frame is filled with value + its image's value"""

    def begin(self, auds, audiotype=(0, 0), out=None):
        from mere_fusion_amd.nerf_driver import loader_indices
        from mere_fusion_amd.serving import mirror_index
        self.begun += 1
        self.last_audio_index, self.last_index = loader_indices(self.size, self.index)
        self.index += 1
        t1, t2 = audiotype
        if t1 != 0 and t2 != 0 and self.custom_index.get(t1) is not None:
            cycle = self.custom_img_cycle[t1]
            frame = cycle[mirror_index(len(cycle), self.custom_index[t1])]
            self.custom_index[t1] += 1
            if out is not None:
                out.copy_(frame)
            return frame if out is None else out
        return {"rays_o": torch.zeros(self.rays, 3), "auds": auds, "tag": (self.value, self.index - 1), "body": None}

    def bind_aabb(self):
        self.bound += 1

    def end(self, job, image, out=None):
        frame = torch.full((self.GH, self.GW, 3), int(self.value + float(image[0, 0])) % 256, dtype=torch.uint8)
        if out is not None:
            out.copy_(frame)
        return frame if out is None else out

    def step(self, auds, audiotype=(0, 0), out=None):
        self.stepped += 1
        job = self.begin(auds, audiotype, out=out)
        if not isinstance(job, dict):
            return job
        return self.end(job, self.model.render_frames([job], **self.render_kw)[0]["image"], out=out)


class StepOnlySession(_SessionState):
    """a session of before the two halves existed (the stand-ins of tests/test_nerf_serving_host.py): `step` alone"""

    def step(self, auds, audiotype=(0, 0), out=None):
        from mere_fusion_amd.nerf_driver import loader_indices
        self.stepped += 1
        self.last_audio_index, self.last_index = loader_indices(self.size, self.index)
        self.index += 1
        frame = torch.full((self.GH, self.GW, 3), self.value, dtype=torch.uint8)
        if out is not None:
            out.copy_(frame)
        return frame if out is None else out


def _inp(v, types=None, dim=3):
    auds = torch.stack([torch.full((8, dim, 16), float(v) + 0.25 * b) for b in range(B)])
    return auds, list(types or [(0, 0)] * B)


def _tags(value, first, n):
    return [(value, first + i) for i in range(n)]


def test_groups_by_model_ray_count_and_render_kw_in_session_then_frame_order():
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m1, m2 = FakeModel(), FakeModel()
    other_kw = dict(dt_gamma=1 / 128, max_steps=16, T_thresh=1e-4)
    ss = [FakeSession(m1, 10), FakeSession(m1, 20), FakeSession(m1, 30, rays=12), FakeSession(m1, 40, render_kw=other_kw), FakeSession(m2, 50)]
    bat = NerfBatcher(ss, device="cpu")
    assert bat.frames_per_render == 32
    out = bat.step([_inp(k) for k in range(5)])
    # sessions 0 and 1 share a model, a ray count and the keywords: one call of their 8 frames, session order then frame order; the others render on their own
    assert m1.calls == [(_tags(10, 0, B) + _tags(20, 0, B), ss[0].render_kw), (_tags(30, 0, B), ss[2].render_kw), (_tags(40, 0, B), other_kw)]
    assert m2.calls == [(_tags(50, 0, B), ss[4].render_kw)]
    assert [s.begun for s in ss] == [B] * 5 and [s.stepped for s in ss] == [0] * 5 and [s.bound for s in ss] == [1, 0, 1, 1, 1]
    assert all(o[1] == [0, 1, 2, 3] and tuple(o[0].shape) == (B, 6, 4, 3) and o[0].dtype == torch.uint8 for o in out)
    # ... and every session kept its own EMA although four of them share a model: the values of each session alone
    for k, s in enumerate(ss):
        alone = FakeSession(FakeModel(), s.value, rays=s.rays)
        a = _inp(k)[0]
        want = torch.stack([alone.step(a[b]) for b in range(B)])
        assert torch.equal(out[k][0], want) and bat.enc_a[k] == alone.model.enc_a, k
    assert len({bat.enc_a[k] for k in range(4)}) == 4


@pytest.mark.parametrize("per_render,want", [(3, [3, 3, 2]), (8, [8]), (5, [5, 3]), (1000, [8])])
def test_chunks_of_frames_per_render(per_render, want):
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m = FakeModel()
    ss = [FakeSession(m, 10), FakeSession(m, 20)]
    bat = NerfBatcher(ss, device="cpu", frames_per_render=per_render)
    assert bat.frames_per_render == min(per_render, 64)                  # capped by the head's frame slots
    bat.step([_inp(1), _inp(2)])
    assert [len(tags) for tags, _ in m.calls] == want
    assert sum((tags for tags, _ in m.calls), []) == _tags(10, 0, B) + _tags(20, 0, B)      # an uneven split keeps the order
    with pytest.raises(RuntimeError, match="frames_per_render"):
        NerfBatcher(ss, device="cpu", frames_per_render=0)


def test_custom_video_frames_never_reach_the_renderer():
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m = FakeModel()
    cycle = [torch.full((6, 4, 3), 200 + i, dtype=torch.uint8) for i in range(3)]
    ss = [FakeSession(m, 10, cycle={2: cycle}), FakeSession(m, 20)]
    bat = NerfBatcher(ss, device="cpu")
    out = bat.step([_inp(1, [(2, 2), (0, 0), (2, 0), (2, 2)]), _inp(2)])
    assert m.calls == [([(10, 1), (10, 2)] + _tags(20, 0, B), ss[0].render_kw)]           # (2, 0) is a rendered frame (nerfreal.py:98)
    assert out[0][1] == [0, 1, 2, 3] and ss[0].custom_index[2] == 2
    assert int(out[0][0][0, 0, 0, 0]) == 200 and int(out[0][0][3, 0, 0, 0]) == 201 and int(out[0][0][1, 0, 0, 0]) not in (200, 201)
    # a step of custom-video frames only renders nothing
    m.calls.clear()
    bat.step([_inp(1, [(2, 2)] * B), None], only=[0])
    assert m.calls == [] and ss[0].index == 2 * B


def test_step_only_sessions_and_the_switch_keep_one_step_per_frame(monkeypatch):
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m = FakeModel()
    ss = [FakeSession(m, 10), StepOnlySession(m, 20), FakeSession(m, 30)]
    bat = NerfBatcher(ss, device="cpu")
    out = bat.step([_inp(1), _inp(2), _inp(3)])
    assert [s.stepped for s in ss] == [0, B, 0] and m.calls == [(_tags(10, 0, B) + _tags(30, 0, B), ss[0].render_kw)]
    assert int(out[1][0][0, 0, 0, 0]) == 20 and out[1][1] == [0, 1, 2, 3]
    # a model without render_frames: its sessions step frame by frame as well
    class OldModel:
        enc_a = None

    class HalvesOverAnOldModel(FakeSession):
        step = StepOnlySession.step
    lone = HalvesOverAnOldModel(OldModel(), 40)
    NerfBatcher([lone], device="cpu").step([_inp(4)])
    assert lone.stepped == B and lone.begun == 0
    # MF_NERF_BATCH=0, read per step: everyone steps frame by frame, and the frames and EMAs are those of the batched route
    twin_m = FakeModel()
    twins = [FakeSession(twin_m, 10), StepOnlySession(twin_m, 20), FakeSession(twin_m, 30)]
    tb = NerfBatcher(twins, device="cpu")
    monkeypatch.setenv("MF_NERF_BATCH", "0")
    got = tb.step([_inp(1), _inp(2), _inp(3)])
    assert [s.stepped for s in twins] == [B, B, B] and all(len(tags) == 1 for tags, _ in twin_m.calls)
    assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(got, out)) and tb.enc_a == bat.enc_a
    monkeypatch.setenv("MF_NERF_BATCH", "1")
    n = len(twin_m.calls)
    tb.step([_inp(1), _inp(2), _inp(3)])
    assert len(twin_m.calls) == n + 1 and len(twin_m.calls[-1][0]) == 2 * B


def test_only_leaves_the_others_untouched_and_a_refused_input_moves_nothing():
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m = FakeModel()
    ss = [FakeSession(m, 10), FakeSession(m, 20), FakeSession(m, 30)]
    bat = NerfBatcher(ss, device="cpu")
    bat.step([_inp(1), _inp(2), _inp(3)])
    keep = [(s.index, s.begun, dict(s.custom_index)) for s in ss], list(bat.enc_a)
    m.calls.clear()
    out = bat.step([None, _inp(5), "not looked at"], only=[1])
    assert out[0] is None and out[2] is None and out[1][1] == [4, 4, 3, 2]
    assert m.calls == [(_tags(20, B, B), ss[1].render_kw)]
    assert [(s.index, s.begun, dict(s.custom_index)) for s in (ss[0], ss[2])] == [keep[0][0], keep[0][2]] and (bat.enc_a[0], bat.enc_a[2]) == (keep[1][0], keep[1][2])
    # every input is checked BEFORE any session moves: a later session's bad input is refused with no `begin` run for the earlier ones and nothing rendered
    state = [(s.index, s.begun) for s in ss], list(bat.enc_a)
    m.calls.clear()
    for bad in ((torch.zeros(B + 1, 8, 3, 16), [(0, 0)] * B), (_inp(1)[0], [(0, 0)] * (B - 1)), None):
        with pytest.raises(RuntimeError, match="NerfBatcher"):
            bat.step([_inp(1), _inp(2), bad])
        assert ([(s.index, s.begun) for s in ss], list(bat.enc_a)) == state and m.calls == []
    # a `begin` that fails for a later session: the earlier sessions' EMAs are what they were (nothing was rendered), and the error is the session's own
    def broken(*a, **k):
        raise ValueError("loader")
    ss[2].begin = broken
    with pytest.raises(ValueError, match="loader"):
        bat.step([_inp(1), _inp(2), _inp(3)])
    assert m.calls == [] and list(bat.enc_a) == state[1]


def test_prewarm_with_more_sessions_than_a_step_holds_and_the_slots_asked_for():
    """The serving set-up: more sessions than share a step.  prewarm warms the batched route in slices of at most max_sessions_per_step sessions, the fullest first,
    and moves nothing; every head call asks for the slots of the largest call this batcher can make, so the handle is sized at its first call."""
    from mere_fusion_amd.nerf_serving import NerfBatcher
    m, lone = FakeModel(), FakeModel()
    ss = [FakeSession(m, 10 * (k + 1)) for k in range(5)] + [FakeSession(lone, 60)]
    bat = NerfBatcher(ss, device="cpu", max_sessions_per_step=2)
    state = [(s.index, s.last_index, dict(s.custom_index)) for s in ss], list(bat.enc_a), [s.model.enc_a for s in ss]
    bat.prewarm(torch.ones(8, 3, 16))
    assert ([(s.index, s.last_index, dict(s.custom_index)) for s in ss], list(bat.enc_a), [s.model.enc_a for s in ss]) == state
    batched = [tags for tags, _ in m.calls if len(tags) > 1]
    assert [len(t) for t in batched] == [2 * B, 2 * B, B] and [t[0][0] for t in batched] == [10, 30, 50]      # sessions (0, 1), (2, 3), then 4 with the other model's
    assert [len(tags) for tags, _ in lone.calls] == [1, B]
    assert set(m.reserved) == {0, 2 * B} and set(lone.reserved) == {0, B}          # (0: the one-frame `step`s of the fakes)
    # a serving step of two sessions asks for the same slots; frames_per_render caps them
    m.reserved.clear()
    bat.step([_inp(1), None, None, _inp(4), None, None], only=[0, 3])
    assert m.reserved == [2 * B]
    small = NerfBatcher(ss, device="cpu", frames_per_render=3)
    m.reserved.clear()
    small.step([_inp(k) for k in range(6)])
    assert set(m.reserved) == {3}
    # under MF_NERF_BATCH=0 prewarm is one step per session, as before
    mp = pytest.MonkeyPatch()
    mp.setenv("MF_NERF_BATCH", "0")
    try:
        m.calls.clear()
        bat.prewarm(torch.ones(8, 3, 16))
        assert [len(tags) for tags, _ in m.calls] == [1] * 5
    finally:
        mp.undo()
