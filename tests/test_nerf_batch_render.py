"""GPU: several ER-NeRF head frames in one device loop (mf_nerf_head_batch_render, csrc/mf_nerf_head_batch.hip and the frame-indexed kernels of mf_nerf.hip /
mf_nerf_fused.hip).  Every frame keeps its own round control, so nothing is held to a tolerance: a frame rendered in a batch is `torch.equal` to the same frame
rendered alone by mf_nerf_head_render -- image, depth, weights_sum, the uint8 frame, the three per-ray sums and the round count -- wherever the launch chain
hands over to the tail, at ragged ray counts, and through `NerfBatcher`."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("image", "depth", "weights_sum", "frame_u8", "ambient_aud", "ambient_eye", "uncertainty")


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def runner(lib_built):
    import bench
    return bench.ErNeRFRunner("bf16x3", 33, torch.device("cuda:0"), seed=3)        # 1 089 rays: no multiple of 64, 256 or 512


def _frame(r, shift=(0.0, 0.0, 0.0), enc=1.0, eye=0.4, eye_on_device=True, per_ray_bg=False):
    """one frame of the runner's scene: the camera origin moved by `shift`, the audio feature scaled, another eye value, constant or per-ray background"""
    N = r.ro.shape[0]
    e = torch.tensor([[eye]])
    bg = torch.rand(N, 3, generator=torch.Generator().manual_seed(17)).cuda() if per_ray_bg else 1.0
    return dict(rays_o=(r.ro + torch.tensor(shift, device=r.ro.device)).contiguous(), rays_d=r.rd, enc_a=r.d_enc_a * enc, eye=e.cuda() if eye_on_device else e, bg_color=bg)


def _five(r):
    """distinct origins / enc_a / eye; [3] equals [0] input for input; [2] in the middle misses the box (moved sideways by five bounds); [4] has the per-ray background"""
    return [_frame(r), _frame(r, (0.25, -0.1, 0.6), 0.7, 0.1, eye_on_device=False), _frame(r, (5.0, 0.0, 0.0), 1.3, 0.2), _frame(r),
            _frame(r, (-0.2, 0.15, -0.4), 1.2, 0.3, per_ray_bg=True)]


def _alone(r, frames, **kw):
    """every frame through mf_nerf_head_render on the single-frame head: per frame the seven tensors of KEYS and the round count"""
    from mere_fusion_amd import _lib
    lib, res = _lib.lib(), []
    for f in frames:
        out = r.r.run_cuda_device(f["rays_o"], f["rays_d"], f["enc_a"], r.d_ind, f["eye"], bg_color=f["bg_color"], want_u8=True, **kw)
        N = f["rays_o"].shape[0]
        sums = [torch.empty(N, device="cuda") for _ in range(3)]
        _lib.check(lib.mf_nerf_head_sums(r.r._head, N, *[C.c_void_p(t.data_ptr()) for t in sums], _stream()))
        torch.cuda.synchronize()
        rounds, err = C.c_int(), C.c_int()
        _lib.check(lib.mf_nerf_head_last_rounds(r.r._head, C.byref(rounds), C.byref(err)))
        assert err.value == 0
        res.append(([out[k].clone() for k in KEYS[:4]] + sums, rounds.value))
    return res


def _batched(r, frames, **kw):
    from mere_fusion_amd import _lib
    lib = _lib.lib()
    outs = r.r.run_cuda_device_batch(frames, want_u8=True, **kw)
    N, res = frames[0]["rays_o"].shape[0], []
    for i, out in enumerate(outs):
        sums = [torch.empty(N, device="cuda") for _ in range(3)]
        _lib.check(lib.mf_nerf_head_batch_sums(r.r._batch, i, N, *[C.c_void_p(t.data_ptr()) for t in sums], _stream()))
        res.append([out[k] for k in KEYS[:4]] + sums)
    torch.cuda.synchronize()
    cap = r.r._batch_cap[1]
    rounds, errs = (C.c_int * cap)(), (C.c_int * cap)()
    _lib.check(lib.mf_nerf_head_batch_last_rounds(r.r._batch, rounds, errs))
    assert list(errs)[:len(frames)] == [0] * len(frames)
    return [(t, rounds[i]) for i, t in enumerate(res)]


def _eq(a, b):
    """equal bits (a ray that misses the box has a NaN depth: 0 / 0 in renderer.py:280)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for i, ((g, gr), (w, wr)) in enumerate(zip(got, want)):
        assert gr == wr, (what, i, "rounds", gr, wr)
        for a, b, name in zip(g, w, KEYS):
            assert _eq(a, b), (what, i, name, float((a.float() - b.float()).abs().nan_to_num().max()))


@pytest.fixture(scope="module")
def five_alone(runner):
    """the F = 5 batch one frame at a time, launches only (computed once, shared, never changed)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("MF_NERF_TAIL_AFTER", "off")
    try:
        return _alone(runner, _five(runner))
    finally:
        mp.undo()


# ---- 1. same bits as one frame at a time -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 5])
def test_batch_is_the_same_bits_as_one_frame_at_a_time(runner, five_alone, monkeypatch, F):
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", "off")
    frames = _five(runner)[:F]
    got = _batched(runner, frames)
    _same_bits(got, five_alone[:F], f"F={F}")
    print(f"[nerf batch] F = {F}: rounds per frame {[n for _, n in got]}, image std {[round(float(t[0].std()), 3) for t, _ in got]}")
    assert all(float(t[0].std()) > 0.05 for i, (t, _) in enumerate(got) if i != 2)                 # pictures, not constants
    if F == 5:
        # frames that hit the head run different numbers of rounds (5, 7, 5 and 4 with these cameras: frame 1 is moved towards the head, frame 4 away from it), so
        # one frame's loop ends while others still march and composite in the same launches; the frame that misses ends after its first round
        assert len({n for i, (_, n) in enumerate(got) if i != 2}) >= 2, [n for _, n in got]
        assert got[2][1] == 1 and all(n >= 2 for i, (_, n) in enumerate(got) if i != 2)
        for a, b in zip(got[0][0], got[3][0]):                                                    # the duplicate pair
            assert _eq(a, b)
        img, _, wsum = got[2][0][:3]                                                              # every ray misses: the background, untouched
        assert torch.equal(img, torch.ones_like(img)) and float(wsum.abs().max()) == 0.0
        assert not torch.equal(got[0][0][0], got[1][0][0]) and not torch.equal(got[0][0][0], got[4][0][0])


# ---- 2. hand-over to the per-frame tail launches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after", ["0", "1", "2", "max"])
def test_hand_over_to_the_tail_wherever_the_chain_ends(runner, five_alone, monkeypatch, after):
    most = max(n for _, n in five_alone)
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", str(most) if after == "max" else after)
    _same_bits(_batched(runner, _five(runner)), five_alone, f"tail after {after}")                 # (_batched asserts every frame's error flag 0)


# ---- 3. other shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,width,max_steps,generic", [("bf16", 20, 64, False), ("bf16x3", 40, 1, False), ("bf16x3", 20, 16, True)])
def test_other_shapes(lib_built, monkeypatch, precision, width, max_steps, generic):
    """400 and 1 600 rays, the one-pass bf16 field, a long loop and the shortest one (rays still alive when `step >= max_steps` ends it), F = 3; once with the
    reference-shaped march (MF_NERF_MARCH=generic reaches the batch too); launches only, then handed to the tail after one round"""
    import bench
    r = bench.ErNeRFRunner(precision, width, torch.device("cuda:0"), seed=7)
    if generic:
        monkeypatch.setenv("MF_NERF_MARCH", "generic")
    frames = [_frame(r), _frame(r, (0.2, 0.1, 0.5), 0.8, 0.1), _frame(r, (-0.1, 0.0, -0.3), 1.1, 0.3, per_ray_bg=True)]
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", "off")
    want = _alone(r, frames, max_steps=max_steps)
    assert all(1 <= n <= max_steps for _, n in want)
    _same_bits(_batched(r, frames, max_steps=max_steps), want, "launches only")
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", "1")
    _same_bits(_batched(r, frames, max_steps=max_steps), want, "tail after 1")


# ---- 4. slots and outputs are not shared -----------------------------------------------------------------------------------------------------
GUARD, POISON = 64, 0x5A5A5A5A


def _raw_render(r, h, frames, n_frames=None, n_rays=None, null=None, max_steps=16):
    """mf_nerf_head_batch_render called by hand: the outputs of all frames carved from ONE poisoned int32 allocation with GUARD words between them.
    Returns (rc, per-frame [image, depth, weights_sum, frame_u8], the allocation, the guards' offsets)."""
    from mere_fusion_amd import _lib
    N = frames[0]["rays_o"].shape[0]
    sizes = (3 * N, N, N, (3 * N + 3) // 4)
    per = sum(s + GUARD for s in sizes)
    block = torch.full((GUARD + per * len(frames),), POISON, dtype=torch.int32, device="cuda")
    descs, keep, outs, guards, o = (_lib.MfNerfFrameDesc * len(frames))(), [], [], [(0, GUARD)], GUARD
    for i, f in enumerate(frames):
        t = []
        for s in sizes:
            t.append(block[o:o + s])
            guards.append((o + s, o + s + GUARD))
            o += s + GUARD
        out = [t[0].view(torch.float32).view(N, 3), t[1].view(torch.float32), t[2].view(torch.float32), t[3].view(torch.uint8)[:3 * N].view(N, 3)]
        ea, ic = f["enc_a"].float().reshape(-1).contiguous(), r.d_ind.float().reshape(-1).contiguous()
        bg = f["bg_color"] if torch.is_tensor(f["bg_color"]) else None
        eye = f["eye"].float().reshape(-1)[:1].contiguous()
        keep.append((ea, ic, bg, eye))
        d = descs[i]
        d.rays_o, d.rays_d, d.enc_a, d.ind_code = _p(f["rays_o"]), _p(f["rays_d"]), _p(ea), _p(ic)
        d.eye_dev, d.eye = (_p(eye), 0.0) if eye.is_cuda else (None, float(eye[0]))
        d.bg_color, d.bg_per_ray, d.bg_const = _p(bg), int(bg is not None), 0.0 if bg is not None else float(f["bg_color"])
        d.image, d.depth, d.weights_sum, d.frame_u8 = (_p(x) for x in out)
        if null and null[0] == i:
            setattr(d, null[1], None)
        outs.append(out)
    rr = r.r
    rc = _lib.lib().mf_nerf_head_batch_render(h, descs, len(frames) if n_frames is None else n_frames, N if n_rays is None else n_rays, C.c_void_p(rr.bitfield.data_ptr()),
                                              rr.cascade, rr.grid_size, rr.min_near, 1 / 256, max_steps, 1e-4, rr.density_scale, None, _stream())
    torch.cuda.synchronize()
    return rc, outs, block, guards


@pytest.fixture()
def handle5(runner):
    from mere_fusion_amd import _lib
    h = C.c_void_p()
    _lib.check(_lib.lib().mf_nerf_head_batch_create(runner.field._h, runner.ro.shape[0], 5, C.byref(h)), "mf_nerf_head_batch_create")
    yield h
    torch.cuda.synchronize()
    _lib.lib().mf_nerf_head_batch_destroy(h)


def test_slots_and_outputs_are_not_shared(runner, five_alone, handle5, monkeypatch):
    """F = 2 on a handle created for 5; batch A, a different batch B (other frames in the same slots, one of them the frame that misses), then A again: A's bits
    again -- a stale control block or alive list would show -- and every guard word between the outputs is intact"""
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", "off")
    five = _five(runner)
    for name, pick in (("A", (0, 1)), ("B", (2, 4)), ("A again", (0, 1))):
        rc, outs, block, guards = _raw_render(runner, handle5, [five[i] for i in pick])
        assert rc == 0, name
        for out, i in zip(outs, pick):
            for a, b, key in zip(out, five_alone[i][0], KEYS[:4]):
                assert _eq(a, b), (name, i, key)
        assert all(bool((block[a:b] == POISON).all()) for a, b in guards), name
    # ... and with the default plan (the rounds the batches before needed, then one tail launch per frame)
    monkeypatch.delenv("MF_NERF_TAIL_AFTER")
    rc, outs, block, guards = _raw_render(runner, handle5, [five[4], five[0], five[1]])
    assert rc == 0 and all(_eq(a, b) for out, i in zip(outs, (4, 0, 1)) for a, b in zip(out, five_alone[i][0]))
    assert all(bool((block[a:b] == POISON).all()) for a, b in guards)


# ---- 5. refusals by name ----------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(runner, handle5):
    from mere_fusion_amd import _lib
    lib, five = _lib.lib(), _five(runner)
    N = runner.ro.shape[0]
    for kw, msg in ((dict(n_frames=0), b"n_frames=0"), (dict(n_frames=6), b"n_frames=6 (the handle holds 1..5)"), (dict(n_rays=N + 1), b"n_rays=%d (capacity %d)" % (N + 1, N)),
                    (dict(null=(1, "rays_o")), b"frame 1: null rays_o"), (dict(null=(0, "ind_code")), b"frame 0: the field was built with an individual code")):
        rc, outs, block, _ = _raw_render(runner, handle5, five[:2], **kw)
        assert rc == -1 and msg in lib.mf_last_error(), (kw, lib.mf_last_error())
        assert bool((block == POISON).all()), kw                         # refused before any launch
    h = C.c_void_p()
    for frames in (0, 65):
        assert lib.mf_nerf_head_batch_create(runner.field._h, N, frames, C.byref(h)) == -1 and b"max_frames" in lib.mf_last_error()
    with pytest.raises(RuntimeError, match="one ray count per call"):
        runner.r.run_cuda_device_batch([five[0], dict(five[1], rays_o=five[1]["rays_o"][:100], rays_d=five[1]["rays_d"][:100])])


# ---- 6. the batcher ---------------------------------------------------------------------------------------------------------------------------
def _serve(monkeypatch, switch, g, inp, **kw):
    """three steps (the third with only=) of the four sessions of tests/test_nerf_serving.py over a fresh model; MF_NERF_BATCH as `switch` says"""
    import test_nerf_serving as TS
    import test_nerf_session as T
    from mere_fusion_amd.nerf_serving import NerfBatcher
    if switch is None:
        monkeypatch.delenv("MF_NERF_BATCH", raising=False)
    else:
        monkeypatch.setenv("MF_NERF_BATCH", switch)
    m, _ = T._make_model()
    m.smooth_lips, m.enc_a = True, None
    ss = [f() for f in TS._sessions(m, inp)]
    bat = NerfBatcher(ss, **kw)
    bat.prewarm(TS._auds(g, 0, 0)[0])
    assert [s.index for s in ss] == [0] * 4 and m.enc_a is None and bat.enc_a == [None] * 4
    outs = [bat.step([(TS._auds(g, k, step), TS.TYPES[k]) for k in range(4)]) for step in range(2)]
    outs.append(bat.step([None, (TS._auds(g, 1, 2), TS.TYPES[1]), "not looked at", (TS._auds(g, 3, 2), TS.TYPES[3])], only=[3, 1]))
    torch.cuda.synchronize()
    return outs, bat.enc_a, [dict(s.custom_index) for s in ss], [s.index for s in ss], m


def test_batcher_batched_route_equals_one_step_per_frame(lib_built, monkeypatch):
    import numpy as np
    import test_nerf_session as T
    from conftest import ROOT
    import os
    g, inp = np.load(os.path.join(ROOT, "tests", "golden", "ernerf_golden.npz")), T._session_inputs()
    want, want_ema, want_custom, want_index, m0 = _serve(monkeypatch, "0", g, inp)
    assert getattr(m0._mf["renderer"], "_batch", None) is None           # the switch kept everyone on NerfSession.step
    for kw in ({}, {"frames_per_render": 3}):
        got, ema, custom, index, m = _serve(monkeypatch, None, g, inp, **kw)
        assert m._mf["renderer"]._batch_cap[1] == kw.get("frames_per_render", 16)              # sized once, for the largest call of this batcher: never regrown
        assert m._mf["renderer"]._batch is not None and m.mf_frames == m0.mf_frames + 16      # (prewarm's batched step: four frames of each of the four sessions)
        for step in range(3):
            for k in range(4):
                if want[step][k] is None:
                    assert got[step][k] is None and step == 2 and k in (0, 2)
                    continue
                assert got[step][k][1] == want[step][k][1] and torch.equal(got[step][k][0], want[step][k][0]), (kw, step, k)
        assert all(torch.equal(a, b) for a, b in zip(ema, want_ema)) and custom == want_custom and index == want_index
    assert float(want[1][0][0].float().std()) > 1.0


# ---- 7. more calls in flight than a table ring holds -------------------------------------------------------------------------------------------
def _hold_the_stream():
    """10 to 200 ms of device time on the current stream (the counter runs at 0.1 to 2 GHz): what is enqueued behind it in the next few milliseconds is all in
    flight at once, and the call that comes round to a used ring entry has to wait for it"""
    torch.cuda._sleep(20_000_000)


def test_nine_batched_calls_in_flight_are_each_the_frames_rendered_alone(runner, monkeypatch):
    """2 * 4 + 1 calls of F = 2 back to back with no synchronise between them, twice round the head batch's ring of four frame tables and once more; every call
    has its own enc_a and bg_color (a constant for frame 0, a per-ray image for frame 1).  Outputs start as NaN / 0x5A, so a frame a call never wrote shows; the
    default round plan, so the calls hand over to the tail wherever the feedback words of the moment say."""
    r, N = runner, runner.ro.shape[0]
    calls = [[dict(_frame(r, enc=0.6 + 0.05 * (2 * c + j), eye=0.1 + 0.04 * c),
                   bg_color=torch.rand(N, 3, generator=torch.Generator().manual_seed(50 + c)).cuda() if j else c / 8) for j in range(2)] for c in range(9)]
    want = [_alone(r, frames) for frames in calls]
    r.r.run_cuda_device_batch(calls[0])                                  # the handle exists: no allocation among the nine
    torch.cuda.synchronize()
    empty = torch.empty

    def poisoned(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float("nan") if t.is_floating_point() else 0x5A)
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", poisoned)
        _hold_the_stream()
        got = [r.r.run_cuda_device_batch(frames, want_u8=True) for frames in calls]
    torch.cuda.synchronize()
    for c, (outs, alone) in enumerate(zip(got, want)):
        for j, (out, (w, _)) in enumerate(zip(outs, alone)):
            for key, b in zip(KEYS[:4], w):
                assert _eq(out[key], b), (c, j, key)
    assert not _eq(got[0][0]["image"], got[1][0]["image"]) and not _eq(got[0][1]["image"], got[8][1]["image"])      # the calls differ: nothing compares a frame with itself


def test_thirty_three_frame_out_calls_in_flight_are_each_the_single_frame_bytes(lib_built):
    """2 * 16 + 1 mf_nerf_frame_batch_out calls of F = 2 at 8 x 8 pixels with no synchronise between them, twice round the frame batch's ring of sixteen tables and
    once more, each with its own renders, against mf_nerf_frame_out; the output blocks start as 0x5A"""
    from mere_fusion_amd import _lib
    _lib.init_device(0)
    lib, S, CALLS = _lib.lib(), 8, 33
    renders = torch.rand(CALLS, 2, S, S, 3, generator=torch.Generator().manual_seed(43)).cuda()
    want = torch.empty(CALLS, 2, S, S, 3, dtype=torch.uint8, device="cuda")
    for c in range(CALLS):
        for j in range(2):
            _lib.check(lib.mf_nerf_frame_out(_p(renders[c, j]), S, S, S, S, None, S, S, 0, 0, 1, _p(want[c, j]), _stream()), "mf_nerf_frame_out")
    torch.cuda.synchronize()
    h = C.c_void_p()
    _lib.check(lib.mf_nerf_frame_batch_create(2, S * S, C.byref(h)), "mf_nerf_frame_batch_create")
    try:
        got = torch.full((CALLS, 2, S, S, 3), 0x5A, dtype=torch.uint8, device="cuda")
        scratch, d0 = torch.empty(2, S, S, 3, dtype=torch.uint8, device="cuda"), (_lib.MfNerfOutDesc * 2)()
        d0[0].render = d0[1].render = _p(renders[0, 0])
        _lib.check(lib.mf_nerf_frame_batch_out(h, d0, 2, S, S, S, S, S, S, 1, _p(scratch), _stream()), "mf_nerf_frame_batch_out")      # the ring exists: no allocation among the 33
        torch.cuda.synchronize()
        _hold_the_stream()
        for c in range(CALLS):
            descs = (_lib.MfNerfOutDesc * 2)()
            for j in range(2):
                descs[j].render, descs[j].body_bgr, descs[j].x0, descs[j].y0 = _p(renders[c, j]), None, 0, 0
            _lib.check(lib.mf_nerf_frame_batch_out(h, descs, 2, S, S, S, S, S, S, 1, _p(got[c]), _stream()), "mf_nerf_frame_batch_out")
        torch.cuda.synchronize()
    finally:
        lib.mf_nerf_frame_batch_destroy(h)
    assert torch.equal(got, want)
    assert not torch.equal(want[0, 0], want[0, 1]) and not torch.equal(want[0], want[32]) and float(want.float().std()) > 10
