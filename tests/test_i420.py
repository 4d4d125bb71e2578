"""GPU: finished frames as planar YUV 4:2:0 -- mf_frames_to_i420 / ops.frames_to_i420 byte for byte against the numpy integer model (tests/i420_ref.py) on both
kernel paths and both channel orders, AvatarFrames.paste_i420, and the I420 route of the Wav2Lip scheduler and of NerfSession.step_to_ring against the packed
frames the default route delivers on identical inputs.  Everything is integer: the bar is equality."""
import numpy as np
import pytest
import torch

import i420_ref as R
from mere_fusion_amd import weights as W

pytestmark = pytest.mark.gpu

GUARD = 64
# [B, H, W]: one block; scalar path with H no multiple of 4; vector path; more than one workgroup; vector path with H / 2 odd
SHAPES = [(1, 2, 2), (3, 6, 10), (2, 16, 24), (2, 64, 72), (1, 30, 40)]


def _inputs(B, H, Wd, order, kind):
    if kind == "random":
        return np.random.default_rng(1000 * B + 10 * H + Wd).integers(0, 256, (B, H, Wd, 3), dtype=np.uint8)
    if kind == "primaries":
        return np.stack([R.primaries_frame(H, Wd, order)] * B)
    return np.stack([np.full((H, Wd, 3), 255 * ((b + 1) % 2), np.uint8) for b in range(B)])       # "flat": all-255 and all-0 frames in turn


def _convert_guarded(frames_dev, order):
    """ops.frames_to_i420 into the front of a buffer that is GUARD bytes longer: (the planes, the bytes behind them)"""
    from mere_fusion_amd import ops
    B, H, Wd = frames_dev.shape[:3]
    n = B * H * Wd * 3 // 2
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:n].view(B, H * 3 // 2, Wd)
    got = ops.frames_to_i420(frames_dev, order=order, out=out)
    assert got is out
    return out.cpu().numpy(), buf[n:].cpu().numpy()


@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("B,H,Wd", SHAPES)
def test_frames_to_i420_equals_the_integer_model(lib_built, B, H, Wd, order):
    from mere_fusion_amd import ops
    for kind in ("random", "primaries", "flat"):
        frames = _inputs(B, H, Wd, order, kind)
        want = R.i420_model(frames, order)
        dev = torch.from_numpy(frames).cuda()
        assert dev.data_ptr() % 4 == 0                                   # W % 8 == 0 then takes the strip path
        got, guard = _convert_guarded(dev, order)
        assert got.shape == (B, H * 3 // 2, Wd) and np.array_equal(got, want), (kind, int((got != want).sum()))
        assert (guard == 0xA5).all(), kind                                # nothing behind the last plane is written
        fresh = ops.frames_to_i420(dev, order=order)                      # out=None
        assert fresh.dtype == torch.uint8 and fresh.is_cuda and np.array_equal(fresh.cpu().numpy(), want), kind
    one = ops.frames_to_i420(dev[0], order=order)                         # [H, W, 3] -> [H * 3 / 2, W]
    assert tuple(one.shape) == (H * 3 // 2, Wd) and np.array_equal(one.cpu().numpy(), want[0])
    if kind == "flat" and order == "rgb":                                 # the known answers, on the device: white is (235, 128, 128)
        y, cb, cr = R.planes(want[:1], H, Wd)
        assert set(y.ravel().tolist()) == {235} and set(cb.ravel().tolist()) == set(cr.ravel().tolist()) == {128}


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_a_misaligned_view_takes_the_scalar_path_and_matches(lib_built, order):
    """[1, 18, 16]: W % 8 == 0, but the frames start one byte into a buffer, so the dword loads of the strip path would be misaligned; the host picks the byte path.
    The same bytes from an aligned copy (strip path) close the loop: both paths agree."""
    from mere_fusion_amd import ops
    B, H, Wd = 1, 18, 16
    frames = _inputs(B, H, Wd, order, "random")
    n = frames.size
    buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + n].view(B, H, Wd, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    want = R.i420_model(frames, order)
    got, guard = _convert_guarded(view, order)
    assert np.array_equal(got, want) and (guard == 0xA5).all()
    aligned = ops.frames_to_i420(torch.from_numpy(frames).cuda(), order=order)
    assert np.array_equal(aligned.cpu().numpy(), got)
    # ... and a misaligned `out` alone does the same
    obuf = torch.full((B * H * Wd * 3 // 2 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    out = obuf[1:1 + B * H * Wd * 3 // 2].view(B, H * 3 // 2, Wd)
    ops.frames_to_i420(torch.from_numpy(frames).cuda(), order=order, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and int(obuf[0]) == 0xA5 and (obuf[-7:].cpu().numpy() == 0xA5).all()


def test_refusals(lib_built):
    from mere_fusion_amd import ops
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.uint8), device=k.get("device", "cuda"))      # noqa: E731
    with pytest.raises(RuntimeError, match=r"frame size 5 x 4 \(H x W\) is odd"):
        ops.frames_to_i420(z(1, 5, 4, 3))
    with pytest.raises(RuntimeError, match=r"frame size 4 x 7 \(H x W\) is odd"):
        ops.frames_to_i420(z(4, 7, 3))
    with pytest.raises(RuntimeError, match="tensor is on cpu.*no CPU fallback"):
        ops.frames_to_i420(z(1, 4, 4, 3, device="cpu"))
    with pytest.raises(RuntimeError, match=r"must be contiguous uint8 \[B, H, W, 3\] or \[H, W, 3\], got torch.float32"):
        ops.frames_to_i420(z(1, 4, 4, 3, dtype=torch.float32))
    with pytest.raises(RuntimeError, match=r"got torch.uint8 \(1, 4, 4, 4\)"):
        ops.frames_to_i420(z(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="not contiguous"):
        ops.frames_to_i420(z(1, 4, 8, 3)[:, :, ::2])
    with pytest.raises(RuntimeError, match="order must be 'bgr' or 'rgb'"):
        ops.frames_to_i420(z(1, 4, 4, 3), order="yuv")
    with pytest.raises(RuntimeError, match=r"out must be a contiguous uint8 tensor \(1, 6, 4\)"):
        ops.frames_to_i420(z(1, 4, 4, 3), out=z(1, 4, 4))


def test_paste_i420_equals_convert_after_paste(lib_built):
    """a 3-frame 48 x 64 avatar: one blended job (mask + crop box, uint8 faces) and one rectangle job (Wav2Lip's fp32 faces)"""
    from mere_fusion_amd import ops, paste
    rng = np.random.default_rng(48)
    frames = rng.integers(0, 256, (3, 48, 64, 3), dtype=np.uint8)
    bboxes = [(10 + i, 8 + i, 40 + i, 36 + i) for i in range(3)]                       # (x1, y1, x2, y2)
    crops = [(6, 4, 50, 44)] * 3
    masks = [rng.integers(0, 256, (40, 44, 3), dtype=np.uint8) for _ in range(3)]
    for av, res in ((paste.AvatarFrames(frames, bboxes, masks=masks, crop_boxes=crops), torch.from_numpy(rng.integers(0, 256, (1, 32, 32, 3), dtype=np.uint8)).cuda()),
                    (paste.AvatarFrames(frames, bboxes), torch.from_numpy((rng.random((1, 96, 96, 3)) * 255).astype(np.float32)).cuda())):
        packed = av.paste(res, [1])
        assert not torch.equal(packed[0], av.frames[1])                                    # the paste did something
        want = ops.frames_to_i420(packed, order="bgr")
        got = av.paste_i420(res, [1])
        assert tuple(got.shape) == (1, 72, 64) and torch.equal(got, want)
        assert np.array_equal(got.cpu().numpy(), R.i420_model(packed.cpu().numpy(), "bgr"))
        out = torch.empty_like(want)
        assert av.paste_i420(res, [1], out=out) is out and torch.equal(out, want)
    assert paste.frames_to_i420 is ops.frames_to_i420                                      # re-exported next to resize_linear_u8


# ---- end to end: Wav2Lip ---------------------------------------------------------------------------------------------------------------
LB, LH, LW, COUNTS = 2, 64, 48, (3, 4)


def _lip_run(m, frame_format):
    """two sessions, two batches each (session 1's second typed silent), both sessions in every step: per session the tuples its ring delivered"""
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.paste import AvatarFrames
    from mere_fusion_amd.transport import FrameRing, i420_shape
    rng = np.random.default_rng(64)
    sessions = []
    for s, n in enumerate(COUNTS):
        faces = rng.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8)
        full = rng.integers(0, 256, (n, LH, LW, 3), dtype=np.uint8)
        boxes = [(6 + i + s, 50 + i, 4 + s, 40 + i) for i in range(n)]                     # (y1, y2, x1, x2), lipreal.py:208
        sessions.append(D.LipSession(m, faces, avatar_frames=AvatarFrames(full, boxes, lip_order=True)))
    bat = D.LipBatcher(m, sessions, batch_size=LB, paste=True)
    shape = i420_shape(LH, LW) if frame_format == "i420" else (LH, LW, 3)
    rings = [FrameRing(2 * LB, shape) for _ in range(2)]
    pcm = lambda s, j: [W.make_speech_like_wav(320, 50 * s + 7 * j + i) for i in range(2 * LB)]      # noqa: E731
    got, now = [[], []], [0.0]
    try:
        with D.LipEndToEndScheduler(bat, rings=rings, clock=lambda: now[0], hold_s=0.0, frame_format=frame_format) as sch:
            for j in range(2):
                sch.submit(0, pcm(0, j), 0.001 * j)
                sch.submit(1, [(c, 1) for c in pcm(1, j)] if j == 1 else pcm(1, j), 0.001 * j)
                now[0] += 0.001
                done = sch.run_once() + sch.drain()
                assert sorted(k for k, *_ in done) == [0, 1]
                for k, fr, idx, _ in done:
                    for i in range(LB):
                        f, fi, audio = rings[k].get(timeout=20)
                        assert fi == idx[i] and (f is None) == (fr is None)
                        if f is not None:
                            assert np.array_equal(f, fr[i].cpu().numpy())              # what run_once reports is what the ring carried
                        got[k].append((f, fi, audio))
            assert sch.ring_full == 0 and not sch.pending()
    finally:
        for r in rings:
            r.close()
    return got


def test_lip_scheduler_delivers_i420_of_the_packed_frames(gpu_model_factory):
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd.transport import FrameRing
    m = gpu_model_factory("bf16x3")
    packed, planar = _lip_run(m, "packed"), _lip_run(m, "i420")
    spoken = 0
    for s in range(2):
        assert len(packed[s]) == len(planar[s]) == 2 * LB
        for (f0, i0, a0), (f1, i1, a1) in zip(packed[s], planar[s]):
            assert i0 == i1 and len(a0) == len(a1) == 2
            assert all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a0, a1))
            if f0 is None:
                assert f1 is None
                continue
            spoken += 1
            assert f0.shape == (LH, LW, 3) and f1.shape == (LH * 3 // 2, LW) and f1.dtype == np.uint8
            assert np.array_equal(f1, R.i420_model(f0[None], "bgr")[0])
    assert spoken == 3 * LB                                                                # session 1's second batch is silent: None both ways
    # a ring of packed slots is refused when the scheduler is built, and so is a batcher that does not paste
    bat = D.LipBatcher(m, [D.LipSession(m, np.zeros((2, 96, 96, 3), np.uint8))], batch_size=LB)
    ring = FrameRing(2 * LB, (LH, LW, 3))
    try:
        with pytest.raises(RuntimeError, match="paste=False"):
            D.LipEndToEndScheduler(bat, rings=[ring], frame_format="i420")
    finally:
        ring.close()


# ---- end to end: ER-NeRF ---------------------------------------------------------------------------------------------------------------
def test_nerf_session_step_to_ring_i420(lib_built):
    from mere_fusion_amd.nerf_driver import NerfSession
    from mere_fusion_amd.transport import FrameRing, i420_shape
    from test_nerf_session import INTR, RENDER_KW, S, _make_model, _ref_get_rays, _session_inputs
    inp = _session_inputs()
    m, g = _make_model()
    auds = torch.from_numpy(np.ascontiguousarray(g["auds"])).cuda()
    rings = {False: FrameRing(4, (S, S, 3)), True: FrameRing(4, i420_shape(S, S))}
    got = {}
    try:
        for i420 in (False, True):
            s = NerfSession(m, inp["poses"].cuda(), INTR, S, S, _ref_get_rays, eye_area=inp["eye"].cuda(), bg=inp["bg"].cuda(), torso_imgs=inp["torso"].cuda(),
                            render_kw=RENDER_KW)
            if i420:
                with pytest.raises(RuntimeError, match=r"slots of shape \(32, 32, 3\)"):
                    s.step_to_ring(rings[False], auds, [], i420=True)
                assert s.index == 0                                                          # refused before the session moved
            got[i420] = []
            for k in range(3):
                audio = [(np.full(320, k, np.float32), 0), (np.full(320, -k, np.float32), 0)]
                frame, idx = s.step_to_ring(rings[i420], auds * (1.0 + 0.05 * k), audio, i420=i420)
                f, fi, fa = rings[i420].get(timeout=10)
                assert fi == idx and np.array_equal(f, frame.cpu().numpy())
                got[i420].append((f, fi, fa))
        for (f0, i0, a0), (f1, i1, a1) in zip(got[False], got[True]):
            assert i0 == i1 and all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(a0, a1))
            assert f0.shape == (S, S, 3) and f1.shape == (S * 3 // 2, S) and float(f0.astype(np.float64).std()) > 1.0
            assert np.array_equal(f1, R.i420_model(f0[None], "rgb")[0])
        # frame_out(i420=True): the same launch pair on a render of its own
        image = torch.rand(S, S, 3, generator=torch.Generator().manual_seed(5)).cuda()
        planar = s.frame_out(image, i420=True)
        assert np.array_equal(planar.cpu().numpy(), R.i420_model(s.frame_out(image).cpu().numpy()[None], "rgb")[0])
    finally:
        for r in rings.values():
            r.close()
