"""GPU: idle and custom-video frames from the device -- mf_frames_gather / ops.gather_frames byte for byte against its sources (packed) and against
ops.frames_to_i420 and the numpy integer model (I420) on every path, and the Wav2Lip scheduler with idle_frames=True against the reference consumer's branch
(tests/idle_frames_ref.py) frame for frame, in both ring formats.  Everything is integer: the bar is equality."""
import numpy as np
import pytest
import torch

import i420_ref as R
from idle_frames_ref import RefConsumer, mirror, typed
from mere_fusion_amd import weights as W

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64


def _sources(n, H, Wd, seed, odd=None):
    """n frames [H, W, 3] as rows of one buffer (numpy, device views).  odd: that source lives one byte into a buffer of its own"""
    frames = np.random.default_rng(seed).integers(0, 256, (n, H, Wd, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    views = [dev[i] for i in range(n)]
    if odd is not None:
        buf = torch.zeros(H * Wd * 3 + 8, dtype=torch.uint8, device="cuda")
        v = buf[1:1 + H * Wd * 3].view(H, Wd, 3)
        v.copy_(dev[odd])
        assert v.data_ptr() % 4 == 1 and v.is_contiguous()
        views[odd] = v
    return frames, views


def _dst_with_holes(n, seed):
    """n distinct frame numbers out of n + n // 2 + 2, in a shuffled order: (dst, out_frames)"""
    N = n + n // 2 + 2
    return [int(d) for d in np.random.default_rng(seed).permutation(N)[:n]], N


def _guarded(N, frame_shape):
    """(out [N, *frame_shape] filled with the sentinel, the whole buffer with GUARD more bytes behind it)"""
    per = int(np.prod(frame_shape))
    buf = torch.full((N * per + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf[:N * per].view((N,) + tuple(frame_shape)), buf


def _check(out, buf, dst, want):
    """frames dst of `out` equal `want`, every other byte of the buffer is the sentinel"""
    got = out.cpu().numpy()
    exp = np.full_like(got, SENTINEL)
    exp[dst] = want
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert (buf[out.numel():].cpu().numpy() == SENTINEL).all()


# (H, W): 3-byte frames at odd offsets; odd sizes; 16-byte units exactly; the same; a dword tail behind two units; a tail only; two workgroups on either path
PACKED_SHAPES = [(1, 1), (3, 5), (2, 8), (4, 16), (2, 6), (2, 2), (24, 64), (19, 21)]


@pytest.mark.parametrize("n", [1, 3, 64, 65])
@pytest.mark.parametrize("H,Wd", PACKED_SHAPES)
def test_gather_packed_copies_each_source_to_its_frame(lib_built, H, Wd, n):
    from mere_fusion_amd import ops
    frames, views = _sources(n, H, Wd, 1000 * H + 10 * Wd + n)
    dst, N = _dst_with_holes(n, n + H)
    out, buf = _guarded(N, (H, Wd, 3))
    assert ops.gather_frames(views, dst, out) is out
    _check(out, buf, dst, frames)


def test_gather_packed_with_one_misaligned_source_takes_the_byte_path(lib_built):
    from mere_fusion_amd import ops
    frames, views = _sources(5, 2, 8, 28, odd=3)
    dst, N = _dst_with_holes(5, 7)
    out, buf = _guarded(N, (2, 8, 3))
    ops.gather_frames(views, dst, out, fmt="packed")
    _check(out, buf, dst, frames)
    obuf = torch.full((3 * 48 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")           # ... and so does a misaligned `out`
    out = obuf[1:1 + 3 * 48].view(3, 2, 8, 3)
    ops.gather_frames(views[:2], [2, 0], out)
    got = out.cpu().numpy()
    assert np.array_equal(got[2], frames[0]) and np.array_equal(got[0], frames[1]) and (got[1] == SENTINEL).all()
    assert int(obuf[0]) == SENTINEL and (obuf[-7:].cpu().numpy() == SENTINEL).all()


# (H, W, n, odd): strip path; strip path, more than one launch; byte path x 3; (2, 8) with one source at an odd byte offset: byte path; two workgroups on either path
I420_CASES = [(2, 8, 3, None), (4, 16, 65, None), (2, 2, 3, None), (2, 6, 64, None), (4, 10, 3, None), (2, 8, 3, 1), (32, 136, 2, None), (20, 54, 2, None)]


@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("H,Wd,n,odd", I420_CASES)
def test_gather_i420_equals_the_converter(lib_built, H, Wd, n, odd, order):
    from mere_fusion_amd import ops
    frames, views = _sources(n, H, Wd, 2000 * H + 10 * Wd + n, odd=odd)
    if n == 3:
        frames[2] = R.primaries_frame(H, Wd, order)
        views[2].copy_(torch.from_numpy(frames[2]))
    dst, N = _dst_with_holes(n, n + Wd)
    out, buf = _guarded(N, (H * 3 // 2, Wd))
    assert ops.gather_frames(views, dst, out, fmt="i420", order=order) is out
    want = ops.frames_to_i420(torch.from_numpy(frames).cuda(), order=order).cpu().numpy()
    _check(out, buf, dst, want)
    assert np.array_equal(want, R.i420_model(frames, order))                                # the converter's own bar, restated: the numpy integer model


def test_gather_from_different_allocations_and_the_wrappers_refusals(lib_built):
    """a row of an avatar's frame cache and a frame of a custom cycle in one call"""
    from mere_fusion_amd import ops, paste
    rng = np.random.default_rng(5)
    full = rng.integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)
    cyc = rng.integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    av = paste.AvatarFrames(full, [(2, 2, 10, 10)] * 3)
    ci = {2: 0}
    cv = paste.CustomVideos({2: cyc}, ci)
    assert cv.lengths == {2: 5} and cv.custom_index is ci and paste.gather_frames is ops.gather_frames
    srcs = [av.source(2), cv.source(2, 4), av.source(0)]
    assert srcs[0].data_ptr() == av.frames[2].data_ptr() and srcs[1].data_ptr() == cv.cycles[2][4].data_ptr()          # views, not copies
    for fmt, shape in (("packed", (16, 24, 3)), ("i420", (24, 24))):
        out, buf = _guarded(4, shape)
        ops.gather_frames(srcs, [3, 0, 1], out, fmt=fmt)
        want = np.stack([full[2], cyc[4], full[0]])
        _check(out, buf, [3, 0, 1], want if fmt == "packed" else R.i420_model(want, "bgr"))
    cv.check_size(16, 24)
    with pytest.raises(RuntimeError, match=r"custom video 2 holds 16 x 24 frames \(H x W\), the avatar's frames are 16 x 32"):
        cv.check_size(16, 32)
    with pytest.raises(RuntimeError, match="frame 5 of custom video 2"):
        cv.source(2, 5)
    with pytest.raises(RuntimeError, match="frame 3 of 3"):
        av.source(3)
    out = torch.zeros((4, 16, 24, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="must name distinct frames of out, 0 to 3"):
        ops.gather_frames(srcs, [0, 1, 0], out)
    with pytest.raises(RuntimeError, match="must name distinct frames of out, 0 to 3"):
        ops.gather_frames(srcs, [0, 1, 4], out)
    with pytest.raises(RuntimeError, match="3 sources for 2 destination frames"):
        ops.gather_frames(srcs, [0, 1], out)
    with pytest.raises(RuntimeError, match=r"out must be a contiguous uint8 tensor \[N, 24, 24\]"):
        ops.gather_frames(srcs, [0, 1, 2], out, fmt="i420")
    with pytest.raises(RuntimeError, match="fmt must be 'packed' or 'i420'"):
        ops.gather_frames(srcs, [0, 1, 2], out, fmt="nv12")
    with pytest.raises(RuntimeError, match="source 1 must be contiguous uint8"):
        ops.gather_frames([srcs[0], srcs[1][:, :12]], [0, 1], out)
    with pytest.raises(RuntimeError, match="tensor is on cpu.*no CPU fallback"):
        ops.gather_frames([srcs[0].cpu()], [0], out)
    with pytest.raises(RuntimeError, match=r"frame size 3 x 5 \(H x W\) is odd"):
        ops.gather_frames([torch.zeros((3, 5, 3), dtype=torch.uint8, device="cuda")], [0], torch.zeros((1, 4, 5), dtype=torch.uint8, device="cuda"), fmt="i420")
    assert not out.any()


# ---- end to end: Wav2Lip ---------------------------------------------------------------------------------------------------------------
EB, EH, EW, COUNTS, NCYC = 4, 16, 24, (3, 4), 5
SCRIPT = [[0] * 8, [1] * 8, [2] * 8, [0, 0, 0, 0, 1, 1, 1, 1], [2] * 8]           # per batch the 2B audio types; the shared dict is reset before the last
REINIT_BEFORE = 4
_RUNS = {}


def _avatars():
    rng = np.random.default_rng(1624)
    faces = [rng.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8) for n in COUNTS]
    full = [rng.integers(0, 256, (n, EH, EW, 3), dtype=np.uint8) for n in COUNTS]
    boxes = [[(2 + i + s, 12 + i, 3 + s, 15 + i) for i in range(n)] for s, n in enumerate(COUNTS)]      # (y1, y2, x1, x2), lipreal.py:208
    cyc = rng.integers(0, 256, (NCYC, EH, EW, 3), dtype=np.uint8)
    return faces, full, boxes, cyc


def _lip_run(m, frame_format, idle, script=SCRIPT, fail_first_step=False):
    """two sessions, the script's batches for both, both sessions in every step: (per session the tuples its ring delivered, session 0's custom_index at the end)"""
    key = (frame_format, idle, fail_first_step, len(script))
    if key in _RUNS:
        return _RUNS[key]
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.paste import AvatarFrames, CustomVideos
    from mere_fusion_amd.transport import FrameRing, i420_shape
    faces, full, boxes, cyc = _avatars()
    ci = {2: 0}
    sessions = [D.LipSession(m, faces[s], avatar_frames=AvatarFrames(full[s], boxes[s], lip_order=True), custom_videos=CustomVideos({2: cyc}, ci) if s == 0 else None)
                for s in range(2)]

    class FailsOnce(D.LipBatcher):
        failed = False

        def step(self, mel_chunks, only=None):
            if fail_first_step and not self.failed:
                self.failed = True
                raise RuntimeError("step failed")
            return super().step(mel_chunks, only)

    bat = FailsOnce(m, sessions, batch_size=EB, paste=True)
    shape = i420_shape(EH, EW) if frame_format == "i420" else (EH, EW, 3)
    rings = [FrameRing(2 * EB, shape) for _ in range(2)]
    pcm = lambda s, j: [W.make_speech_like_wav(320, 50 * s + 7 * j + i) for i in range(2 * EB)]      # noqa: E731
    got, now = [[], []], [0.0]
    kw = {} if idle is None else {"idle_frames": idle}                                     # None: a scheduler built without the argument
    try:
        with D.LipEndToEndScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, frame_format=frame_format, **kw) as sch:
            for j, types in enumerate(script):
                if j == REINIT_BEFORE:
                    ci[2] = 0                                                              # set_curr_state(2, reinit=True) on the deployment's side
                for s in range(2):
                    sch.submit(s, [(c, t) for c, t in zip(pcm(s, j), types)], 0.001 * j)
                now[0] += 0.001
                if fail_first_step and j == 0:
                    before = dict(ci)
                    with pytest.raises(RuntimeError, match="step failed"):
                        sch.run_once()
                    assert ci == before and all(r.qsize() == 0 for r in rings)
                done = sch.run_once() + sch.drain()
                assert sorted(k for k, *_ in done) == [0, 1]
                for k, fr, idx, _ in done:
                    for i in range(EB):
                        f, fi, audio = rings[k].get(timeout=20)
                        assert fi == idx[i] and (f is None) == (fr is None)
                        if f is not None:
                            assert np.array_equal(f, fr[i].cpu().numpy())              # what run_once reports is what the ring carried
                        got[k].append((f, fi, audio))
            assert sch.ring_full == 0 and not sch.pending() and all(r.qsize() == 0 for r in rings)
    finally:
        for r in rings:
            r.close()
    _RUNS[key] = (got, dict(ci))
    return _RUNS[key]


def _expected(frame_format, base):
    """per session the frames the reference consumer would show for SCRIPT, from the option-off run `base` (speech frames) and the avatars"""
    _, full, _, cyc = _avatars()
    conv = (lambda f: R.i420_model(f[None], "bgr")[0]) if frame_format == "i420" else (lambda f: f)
    refs = [RefConsumer({2: NCYC}, {2: 0}), RefConsumer({}, {})]
    want = [[], []]
    for s in range(2):
        for j, types in enumerate(SCRIPT):
            if j == REINIT_BEFORE and 2 in refs[s].custom_index:
                refs[s].custom_index[2] = 0
            for i in range(EB):
                f0, idx, audio = base[s][j * EB + i]
                assert [a[1] for a in audio] == types[2 * i:2 * i + 2]
                c = refs[s].show(idx, audio)
                if c[0] == "speech":
                    assert f0 is not None
                    want[s].append(f0)
                elif c[0] == "idle":
                    want[s].append(conv(full[s][idx]))
                else:
                    want[s].append(conv(cyc[c[2]]))
    return want, refs[0].custom_index


@pytest.mark.parametrize("frame_format", ["packed", "i420"])
def test_lip_scheduler_delivers_idle_and_custom_frames(gpu_model_factory, frame_format):
    m = gpu_model_factory("bf16x3")
    base, ci_off = _lip_run(m, frame_format, False)
    got, ci_on = _lip_run(m, frame_format, True)
    want, ci_ref = _expected(frame_format, base)
    assert ci_off == {2: 0}                                                                # option off: the walk is the consumer's, the scheduler leaves it alone
    assert ci_on == ci_ref == {2: EB}                                                      # reset before the last batch, then its B custom frames
    shape = (EH * 3 // 2, EW) if frame_format == "i420" else (EH, EW, 3)
    kinds = set()
    for s in range(2):
        assert len(got[s]) == len(base[s]) == len(SCRIPT) * EB
        for n, ((f1, i1, a1), (f0, i0, a0), w) in enumerate(zip(got[s], base[s], want[s])):
            assert f1 is not None and f1.shape == shape and f1.dtype == np.uint8           # no tuple carries None
            assert i1 == i0 and all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a1, a0))
            assert np.array_equal(f1, w), (s, n)
            kinds.add((f0 is None, bool(np.array_equal(f1, f0)) if f0 is not None else None))
    # the script met all three: a silent batch filled (None before), a generated frame kept, a generated frame of a mixed batch overwritten
    assert kinds == {(True, None), (False, True), (False, False)}
    # session 0's third batch walked the custom video 0 1 2 3, its fifth again after the reset; session 1 showed its idle frames there
    _, full, _, cyc = _avatars()
    conv = (lambda f: R.i420_model(f[None], "bgr")[0]) if frame_format == "i420" else (lambda f: f)
    for j in (2, 4):
        assert all(np.array_equal(got[0][j * EB + i][0], conv(cyc[mirror(NCYC, i)])) for i in range(EB))
        assert all(np.array_equal(got[1][j * EB + i][0], conv(full[1][got[1][j * EB + i][1]])) for i in range(EB))


def test_a_retried_step_moves_the_custom_walk_once(gpu_model_factory):
    m = gpu_model_factory("bf16x3")
    got, ci = _lip_run(m, "packed", True, script=[[2] * 8], fail_first_step=True)
    _, full, _, cyc = _avatars()
    assert ci == {2: EB}
    assert len(got[0]) == len(got[1]) == EB                                                # each frame once
    assert all(np.array_equal(got[0][i][0], cyc[mirror(NCYC, i)]) for i in range(EB))
    assert all(np.array_equal(f, full[1][idx]) for f, idx, _ in got[1])


@pytest.mark.parametrize("frame_format", ["packed", "i420"])
def test_option_off_is_todays_scheduler(gpu_model_factory, frame_format):
    m = gpu_model_factory("bf16x3")
    off, ci_off = _lip_run(m, frame_format, False)
    plain, ci_plain = _lip_run(m, frame_format, None)
    assert ci_off == ci_plain == {2: 0}
    nones = 0
    for s in range(2):
        assert len(off[s]) == len(plain[s]) == len(SCRIPT) * EB
        for (f0, i0, a0), (f1, i1, a1) in zip(off[s], plain[s]):
            assert i0 == i1 and (f0 is None) == (f1 is None) and all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a0, a1))
            nones += f0 is None
            assert f0 is None or np.array_equal(f0, f1)
    assert nones == 2 * 3 * EB                                                             # the three silent batches of either session travel as None


def test_sessions_refuse_a_custom_video_of_another_size(gpu_model_factory):
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.muse_driver import MuseSession
    from mere_fusion_amd.paste import AvatarFrames, CustomVideos
    m = gpu_model_factory("bf16x3")
    av = AvatarFrames(np.zeros((2, EH, EW, 3), np.uint8), [(2, 12, 3, 15)] * 2, lip_order=True)
    cv = CustomVideos({3: np.zeros((2, EH, EW + 2, 3), np.uint8)}, {3: 0})
    with pytest.raises(RuntimeError, match=r"LipSession: custom video 3 holds 16 x 26 frames \(H x W\), the avatar's frames are 16 x 24"):
        D.LipSession(m, np.zeros((2, 96, 96, 3), np.uint8), avatar_frames=av, custom_videos=cv)
    with pytest.raises(RuntimeError, match=r"MuseSession: custom video 3 holds 16 x 26 frames"):
        MuseSession(torch.zeros(2, 8, 32, 32), avatar_frames=av, custom_videos=cv)
    assert MuseSession(torch.zeros(2, 8, 32, 32), avatar_frames=av, custom_videos=CustomVideos({3: np.zeros((2, EH, EW, 3), np.uint8)}, {3: 0})).custom_videos is not None
