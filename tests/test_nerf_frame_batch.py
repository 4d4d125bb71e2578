"""GPU: the three stages around the batched ER-NeRF head render with a frame index in the grid (csrc/mf_nerf_frame_batch.hip; the kernels stand beside the
single-frame ones in mf_nerf_frame.hip and mf_nerf_torso.hip).  The oracle of every kernel is the project's own single-frame entry point, which
tests/test_nerf_session.py and tests/test_ernerf.py pin to the reference; nothing is held to a tolerance: frame i of a batched call is the same bytes as
mf_nerf_frame_background / mf_nerf_torso_forward / mf_nerf_frame_out give for the same inputs, through `NerfBatcher` too."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def lib(lib_built):
    from mere_fusion_amd import _lib
    _lib.init_device(0)
    return _lib.lib()


def _handle(lib, max_frames, max_pixels):
    from mere_fusion_amd import _lib
    h = C.c_void_p()
    _lib.check(lib.mf_nerf_frame_batch_create(max_frames, max_pixels, C.byref(h)), "mf_nerf_frame_batch_create")
    return h


@pytest.fixture(scope="module")
def handle5(lib):
    h = _handle(lib, 5, 480)
    yield h
    torch.cuda.synchronize()
    lib.mf_nerf_frame_batch_destroy(h)


# ---- 1. background ------------------------------------------------------------------------------------------------------------------------------
BH, BW = 20, 24                                     # 480 pixels: one full workgroup of 256 and a partial one per frame


@pytest.fixture(scope="module")
def bg_scene(lib):
    """five different torso images, one background image, and every frame through mf_nerf_frame_background: [image or constant][half_mode][frame]"""
    from mere_fusion_amd import _lib
    g = torch.Generator().manual_seed(31)
    torso = torch.randint(0, 256, (5, BH, BW, 4), generator=g, dtype=torch.uint8).cuda()
    torso[0, 0, :4, 3] = torch.tensor([0, 255, 1, 254], dtype=torch.uint8)
    image = torch.rand(BH, BW, 3, generator=g).cuda()
    want = {}
    for with_image in (True, False):
        for half in (0, 1):
            rows = []
            for i in range(5):
                out = torch.empty(BH * BW, 3, device="cuda")
                _lib.check(lib.mf_nerf_frame_background(_p(torso[i]), _p(image) if with_image else None, 0.25 + 0.125 * i, BH, BW, half, _p(out), _stream()))
                rows.append(out)
            want[(with_image, half)] = rows
    torch.cuda.synchronize()
    return torso, image, want


@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("with_image", [True, False])
def test_background_batch_is_the_same_bytes_per_frame(lib, handle5, bg_scene, F, with_image):
    from mere_fusion_amd import _lib
    torso, image, want = bg_scene
    for halves in ([0] * F, [1] * F, [i & 1 for i in range(F)]):              # both modes, and both in one call
        block = torch.full((F + 1, BH * BW * 3), POISON, dtype=torch.int32, device="cuda")
        descs = (_lib.MfNerfBgDesc * F)()
        for i in range(F):
            d = descs[i]
            d.torso_rgba, d.bg_image, d.bg_const, d.half_mode, d.bg_color = _p(torso[i]), (_p(image) if with_image else None), 0.25 + 0.125 * i, halves[i], _p(block[i])
        _lib.check(lib.mf_nerf_frame_batch_background(handle5, descs, F, BH, BW, _stream()), "mf_nerf_frame_batch_background")
        torch.cuda.synchronize()
        for i in range(F):
            assert torch.equal(block[i], _bits(want[(with_image, halves[i])][i]).reshape(-1)), (F, with_image, halves, i)
        assert bool((block[F] == POISON).all())
    assert not _same(want[(with_image, 0)][0], want[(with_image, 0)][1]) and not _same(want[(with_image, 0)][0], want[(with_image, 1)][0])


# ---- 2. torso -----------------------------------------------------------------------------------------------------------------------------------
G, TORSO_FRAMES = 32, 4                              # the torso handle's grid; max_frames of the batch handle the torso tests use
POSE = torch.tensor([[0.98, 0.05, -0.19, 0.05], [-0.03, 0.995, 0.09, -0.02], [0.195, -0.083, 0.977, 0.9], [0.0, 0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def torso(lib):
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.field import grid_geometry
    from mere_fusion_amd.ernerf.torso import HipTorso
    offs, _ = grid_geometry(num_levels=16, base_resolution=16, log2_hashmap_size=16, desired_resolution=2048)
    sd = W.make_ernerf_torso_state_dict(int(offs[-1]), 4, 8, G)
    t = HipTorso(sd, torso_shrink=1.0, individual_dim=8, grid_size=G, max_pixels=1024)
    u = torch.linspace(-1, 1, G, dtype=torch.float64)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    grids = {"mixed": (0.6 + 0.5 * torch.sin(3 * xx + 1) * torch.cos(2 * yy - 0.5)).float().reshape(-1).cuda(),      # 0.1 .. 1.1, crosses 0.6 all over the image
             "zero": torch.zeros(G * G, device="cuda")}
    h = _handle(lib, TORSO_FRAMES, 480)
    yield t, grids, h
    torch.cuda.synchronize()
    lib.mf_nerf_frame_batch_destroy(h)


def _torso_frames(t, N, F):
    """F frames of N pixels: own coordinates (corners and edges included), own pose -> own frame constants, own background form, and a threshold that leaves the
    frame's mask full (0: the mixed grid is nowhere below 0.1), empty (2) or mixed (0.6) -- in that order, so that F = 1 is a full one and F >= 3 has all three"""
    from mere_fusion_amd.ernerf.torso import wrapped_anchor_code
    frames = []
    for i in range(F):
        g = torch.Generator().manual_seed(100 + 7 * i + N)
        xy = torch.rand(N, 2, generator=g) * 2 - 1
        xy[:4] = torch.tensor([[-1.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, 0.3]])
        pose = POSE.clone()
        pose[:3, 3] += 0.03 * i
        consts = wrapped_anchor_code(t.anchor_points, pose[None], t.ind_code)
        bg = (torch.rand(N, 3, generator=g).cuda(), 1, 0.0) if i % 3 == 0 else ((torch.rand(3, generator=g).cuda(), 0, 0.0) if i % 3 == 1 else (None, 0, 0.75))
        frames.append(dict(xy=xy.cuda().contiguous(), consts=consts, bg=bg, thresh=(0.0, 2.0, 0.6)[i % 3]))
    return frames


def _torso_alone(lib, t, grid, frames):
    from mere_fusion_amd import _lib
    res = []
    _lib.check(lib.mf_nerf_torso_set_grid(t._h, _p(grid)))
    for f in frames:
        N = f["xy"].shape[0]
        out, alpha, deform = torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, 2, device="cuda")
        cbuf = (C.c_float * len(f["consts"]))(*f["consts"].tolist())
        _lib.check(lib.mf_nerf_torso_forward(t._h, _p(f["xy"]), cbuf, _p(f["bg"][0]), f["bg"][1], f["bg"][2], f["thresh"], N, _p(out), _p(alpha), _p(deform), _stream()),
                   "mf_nerf_torso_forward")
        res.append((out, alpha, deform))
    torch.cuda.synchronize()
    return res


def _torso_batch(lib, t, h, grid, frames, slots=None):
    """mf_nerf_torso_forward_batch with every output carved from one poisoned block of `slots` frame slots -> (per frame (bg_out, alpha, deform), the block)"""
    from mere_fusion_amd import _lib
    F, N = len(frames), frames[0]["xy"].shape[0]
    block = torch.full((slots or F + 1, 6 * N), POISON, dtype=torch.int32, device="cuda")
    descs, res = (_lib.MfNerfTorsoDesc * F)(), []
    for i, f in enumerate(frames):
        row = block[i].view(torch.float32)
        out, alpha, deform = row[:3 * N].view(N, 3), row[3 * N:4 * N], row[4 * N:].view(N, 2)
        d = descs[i]
        d.frame_consts[:len(f["consts"])] = f["consts"].tolist()
        d.bg_coords, d.bg_color, d.bg_per_ray, d.bg_const, d.density_thresh = _p(f["xy"]), _p(f["bg"][0]), f["bg"][1], f["bg"][2], f["thresh"]
        d.bg_out, d.torso_alpha, d.deform = _p(out), _p(alpha), _p(deform)
        res.append((out, alpha, deform))
    _lib.check(lib.mf_nerf_torso_set_grid(t._h, _p(grid)))
    _lib.check(lib.mf_nerf_torso_forward_batch(t._h, h, descs, F, N, _stream()), "mf_nerf_torso_forward_batch")
    torch.cuda.synchronize()
    return res, block


@pytest.fixture(scope="module")
def torso_alone(lib, torso):
    """the single-frame results, computed once and never changed: [grid][N] -> TORSO_FRAMES frames"""
    t, grids, _ = torso
    return {(name, N): _torso_alone(lib, t, grids[name], _torso_frames(t, N, TORSO_FRAMES)) for name in grids for N in (480, 64)}


@pytest.mark.parametrize("F", [1, 3, TORSO_FRAMES])
@pytest.mark.parametrize("N", [480, 64])            # 480: a full tile and a partial one per frame; 64: one wave of one tile
@pytest.mark.parametrize("grid", ["mixed", "zero"])
def test_torso_batch_is_the_same_bits_per_frame(lib, torso, torso_alone, grid, N, F):
    t, grids, h = torso
    want = torso_alone[(grid, N)][:F]
    got, block = _torso_batch(lib, t, h, grids[grid], _torso_frames(t, N, F))
    for i, (g3, w3) in enumerate(zip(got, want)):
        for a, b, name in zip(g3, w3, ("bg_out", "torso_alpha", "deform")):
            assert _same(a, b), (grid, N, F, i, name, float((a - b).abs().max()))
    assert bool((block[F] == POISON).all())
    # the masks are what the cases say: full, empty, mixed (and every frame empty over the zero grid); frames differ
    alphas = [w[1] for w in want]
    if grid == "zero":
        assert all(bool((a == 0).all()) for a in alphas)
    else:
        assert bool((alphas[0] != 0).all())
        if F >= 3:
            assert bool((alphas[1] == 0).all()) and 0 < int((alphas[2] != 0).sum()) < N
            assert not _same(want[0][2], want[1][2]) and not _same(want[0][2], want[2][2])        # the deform follows the frame constants


def test_torso_second_call_with_fewer_frames_and_run_to_run(lib, torso, torso_alone):
    t, grids, h = torso
    frames = _torso_frames(t, 480, TORSO_FRAMES)
    first, _ = _torso_batch(lib, t, h, grids["mixed"], frames)
    # other frames in slots 0 and 1 of the same handle, outputs in a fresh poisoned block of four slots: slots 2 and 3 stay untouched
    got, block = _torso_batch(lib, t, h, grids["mixed"], [frames[2], frames[0]], slots=TORSO_FRAMES)
    for g3, i in zip(got, (2, 0)):
        assert all(_same(a, b) for a, b in zip(g3, torso_alone[("mixed", 480)][i])), i
    assert bool((block[2:] == POISON).all())
    again, _ = _torso_batch(lib, t, h, grids["mixed"], frames)
    assert all(_same(a, b) for x, y in zip(first, again) for a, b in zip(x, y))


def test_run_torso_batch_equals_run_torso(lib, torso):
    """the Python entry the renderer uses: HipTorso.run_torso_batch against run_torso, frame by frame"""
    t, grids, _ = torso
    t.density_grid, t.thresh = grids["mixed"], 0.6
    frames = []
    for i, f in enumerate(_torso_frames(t, 480, 3)):
        pose = POSE.clone()
        pose[:3, 3] += 0.03 * i
        frames.append((f["xy"], pose[None], f["bg"][0] if f["bg"][0] is not None else 0.75))
    want = [t.run_torso(*f) for f in frames]
    got = t.run_torso_batch(frames)
    torch.cuda.synchronize()
    assert all(_same(g[k], w[k]) for g, w in zip(got, want) for k in ("bg_color", "torso_alpha", "deform"))
    assert 0 < int((want[0]["torso_alpha"] != 0).sum()) < 480


# ---- 3. frame-out -------------------------------------------------------------------------------------------------------------------------------
RH, RW, GH, GW, FH, FW = 16, 12, 26, 30, 36, 40     # 16 x 12 -> 26 x 30: 1.625 and 2.5, no integer ratio in either axis


def _out_alone(lib, render, body, x0, y0, srgb):
    from mere_fusion_amd import _lib
    fh, fw = (GH, GW) if body is None else (int(body.shape[0]), int(body.shape[1]))
    out = torch.empty(fh, fw, 3, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mf_nerf_frame_out(_p(render), RH, RW, GH, GW, _p(body), fh, fw, x0, y0, srgb, _p(out), _stream()), "mf_nerf_frame_out")
    return out


@pytest.fixture(scope="module")
def out_scene():
    g = torch.Generator().manual_seed(41)
    renders = torch.rand(5, RH, RW, 3, generator=g).cuda()
    renders[0, 0, 0] = torch.tensor([0.0, 1.0, 0.0031308])
    bodies = torch.randint(0, 256, (5, FH, FW, 3), generator=g, dtype=torch.uint8).cuda()
    custom = torch.randint(0, 256, (GH, GW, 3), generator=g, dtype=torch.uint8).cuda()
    return renders, bodies, custom


@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("case", ["no body", "body at (0, 0)", "body at the last legal corner", "a custom-video frame in the middle"])
def test_frame_out_batch_is_the_same_bytes_per_frame(lib, handle5, out_scene, case, srgb):
    from mere_fusion_amd import _lib, ops
    renders, bodies, custom = out_scene
    F = 5
    if case == "no body":
        frames = [(renders[i], None, 0, 0) for i in range(F)]
    elif case == "body at (0, 0)":
        frames = [(renders[i], bodies[i], 0, 0) for i in range(F)]
    elif case == "body at the last legal corner":
        frames = [(renders[i], bodies[i], FW - GW, FH - GH) for i in range(F)]
    else:                                                               # the custom image alone in slot 2; once among body-less frames, once (a body-sized one) among pasted ones
        frames = [(renders[i], None, 0, 0) for i in range(F)]
        frames[2] = (None, custom, 0, 0)
    fh, fw = (GH, GW) if frames[0][1] is None else (FH, FW)
    want = torch.stack([_out_alone(lib, *f, srgb) for f in frames])
    block = torch.full((F + 1, fh, fw, 3), 0x5A, dtype=torch.uint8, device="cuda")
    descs = (_lib.MfNerfOutDesc * F)()
    for i, (render, body, x0, y0) in enumerate(frames):
        descs[i].render, descs[i].body_bgr, descs[i].x0, descs[i].y0 = _p(render), _p(body), x0, y0
    _lib.check(lib.mf_nerf_frame_batch_out(handle5, descs, F, RH, RW, GH, GW, fh, fw, srgb, _p(block), _stream()), "mf_nerf_frame_batch_out")
    torch.cuda.synchronize()
    for i in range(F):
        assert torch.equal(block[i], want[i]), (case, srgb, i, int((block[i].int() - want[i].int()).abs().max()))
    assert bool((block[F] == 0x5A).all())
    assert not torch.equal(want[0], want[1]) and float(want[0].float().std()) > 10
    if case.startswith("a custom"):
        assert torch.equal(block[2], custom.flip(-1))
        # ... and a body-sized custom-video frame between pasted ones
        frames = [(renders[0], bodies[0], 3, 5), (None, bodies[3], 0, 0), (renders[1], bodies[1], 3, 5)]
        want3 = torch.stack([_out_alone(lib, *f, srgb) for f in frames])
        block3 = torch.empty(3, FH, FW, 3, dtype=torch.uint8, device="cuda")
        d3 = (_lib.MfNerfOutDesc * 3)()
        for i, (render, body, x0, y0) in enumerate(frames):
            d3[i].render, d3[i].body_bgr, d3[i].x0, d3[i].y0 = _p(render), _p(body), x0, y0
        _lib.check(lib.mf_nerf_frame_batch_out(handle5, d3, 3, RH, RW, GH, GW, FH, FW, srgb, _p(block3), _stream()), "mf_nerf_frame_batch_out")
        assert torch.equal(block3, want3)
    # the batched block through the I420 converter equals the per-frame route
    assert torch.equal(ops.frames_to_i420(block[:F], order="rgb"), torch.stack([ops.frames_to_i420(w, order="rgb") for w in want]))


# ---- 4. end to end: NerfBatcher ------------------------------------------------------------------------------------------------------------------
def _serve(monkeypatch, switch, g, inp, **kw):
    """two steps of three sessions x two frames at 32 x 32 over a fresh model: a plain session, one with body frames, one with a custom-video cycle"""
    import test_nerf_session as T
    from mere_fusion_amd.nerf_driver import NerfSession
    from mere_fusion_amd.nerf_serving import NerfBatcher
    if switch is None:
        monkeypatch.delenv("MF_NERF_BATCH", raising=False)
    else:
        monkeypatch.setenv("MF_NERF_BATCH", switch)
    m, _ = T._make_model()
    m.smooth_lips, m.enc_a = True, None
    flip = {k: v.flip(0) for k, v in inp.items()}
    mk = lambda i, **kw: NerfSession(m, i["poses"].cuda(), T.INTR, T.S, T.S, T._ref_get_rays, eye_area=i["eye"].cuda(), bg=i["bg"].cuda(), torso_imgs=i["torso"].cuda(),
                                     gui_size=(T.GH, T.GW), render_kw=T.RENDER_KW, **kw)
    custom = torch.randint(0, 256, (3, T.GH, T.GW, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).cuda()
    ss = [mk(inp), mk(flip, fullbody_frames=inp["body"].cuda(), fullbody_offset=(T.X0, T.Y0)), mk(flip, custom_img_cycle={2: custom})]
    bat = NerfBatcher(ss, batch_size=2, **kw)
    base = torch.from_numpy(np.ascontiguousarray(g["auds"])).cuda()
    types = [[(0, 0), (0, 0)], [(0, 0), (0, 0)], [(2, 2), (0, 0)]]
    outs = []
    for step in range(2):
        outs.append(bat.step([(torch.stack([base * (1.0 + 0.05 * (2 * step + b) + 0.01 * k) for b in range(2)]), types[k]) for k in range(3)]))
    torch.cuda.synchronize()
    return outs, [s.index for s in ss], [dict(s.custom_index) for s in ss], bat


def test_batcher_default_equals_the_per_frame_route(lib, monkeypatch):
    import os
    import test_nerf_session as T
    from conftest import ROOT
    g, inp = np.load(os.path.join(ROOT, "tests", "golden", "ernerf_golden.npz")), T._session_inputs()
    want, want_index, want_custom, bat0 = _serve(monkeypatch, "0", g, inp)
    got, index, custom, bat = _serve(monkeypatch, None, g, inp)
    assert bat0._fb is None
    print(f"[nerf frame batch] NerfBatcher.frame_batch = {bat.frame_batch}; the frame-batch handle was {'used' if bat._fb is not None else 'not used'}")
    assert (bat._fb is not None) == bat.frame_batch                     # the default route is what the batcher says it is
    for step in range(2):
        for k in range(3):
            assert got[step][k][1] == want[step][k][1] and torch.equal(got[step][k][0], want[step][k][0]), (step, k)
    assert index == want_index == [4, 4, 4] and custom == want_custom and custom[2] == {2: 2}
    assert float(want[1][0][0].float().std()) > 1.0 and tuple(want[0][1][0].shape) == (2, T.FH, T.FW, 3)
    # ... and with the frame batch switched on by hand, whatever the default is
    got2, _, _, bat2 = _serve(monkeypatch, None, g, inp, frame_batch=True)
    assert bat2._fb is not None and all(torch.equal(got2[s][k][0], want[s][k][0]) for s in range(2) for k in range(3))
