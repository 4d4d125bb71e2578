"""GPU: the ER-NeRF session driver (mere_fusion_amd/nerf_driver.py) and the kernels under it (csrc/mf_nerf_frame.hip, mf_nerf_head_set_aabb), on the 32 x 32
synthetic scene the other ER-NeRF tests render (tests/golden/ernerf_golden.npz and the seeded builders of mere_fusion_amd.weights) and on seeded images.
The yardsticks are torch on the CPU, the existing `mf_nerf_resize_frame`, float64, and the existing route (`model.render` through the drop-in mixin);
tests/nerf_session_ref.py restates the reference's lines."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import nerf_session_ref as ref

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _frame_out(render, H, W, body=None, x0=0, y0=0, srgb=0):
    from mere_fusion_amd import _lib
    h, w = (int(render.shape[0]), int(render.shape[1])) if render is not None else (0, 0)
    FH, FW = (int(body.shape[0]), int(body.shape[1])) if body is not None else (H, W)
    out = torch.zeros(FH, FW, 3, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mf_nerf_frame_out(_p(render), h, w, H, W, _p(body), FH, FW, x0, y0, srgb, _p(out), _stream()), "mf_nerf_frame_out")
    return out


def _resize_u8(render, H, W):
    from mere_fusion_amd import _lib
    h, w = int(render.shape[0]), int(render.shape[1])
    out = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mf_nerf_resize_frame(_p(render), None, h, w, H, W, None, None, _p(out), _stream()), "mf_nerf_resize_frame")
    return out


def _seeded_render(seed=3, h=32, w=32):
    return torch.rand(h, w, 3, generator=torch.Generator().manual_seed(seed))


RESIZES = [(40, 36), (24, 20), (32, 32)]          # up at a non-integer ratio, down, identity


# ---- 1. background ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(32, 32), (37, 29)])
def test_background_is_bit_equal_to_the_torch_expression(lib_built, H, W):
    """provider.py:323 in both arithmetic modes, against the torch expression on the CPU.  The alpha plane holds 0, 255 and every value between; 37 x 29 = 1073
    pixels leaves a partly filled last block."""
    from mere_fusion_amd import _lib
    g = torch.Generator().manual_seed(11)
    rgba = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8)
    alpha = (torch.arange(H * W) % 256).to(torch.uint8)[torch.randperm(H * W, generator=g)]
    rgba[..., 3] = alpha.view(H, W)
    assert set(range(256)) <= set(rgba[..., 3].reshape(-1).tolist())
    image = torch.rand(H, W, 3, generator=g)
    d_rgba = rgba.cuda()
    for name, bg_img, bg_const in (("image", image, 0.0), ("white", None, 1.0), ("black", None, 0.0)):
        bg_cpu = image if bg_img is not None else ref.constant_background(name, H, W)
        d_bg = bg_img.cuda() if bg_img is not None else None
        for preload in (0, 2):
            want = ref.collate_background(rgba.numpy(), bg_cpu, preload)
            assert want.dtype == (torch.half if preload == 2 else torch.float32)
            got = torch.full((H * W, 3), -1.0, device="cuda")
            _lib.check(_lib.lib().mf_nerf_frame_background(_p(d_rgba), _p(d_bg), bg_const, H, W, int(preload == 2), _p(got), _stream()), "mf_nerf_frame_background")
            assert torch.equal(got.cpu(), want.float()), (name, preload, float((got.cpu() - want.float()).abs().max()))


# ---- 2. / 3. frame out --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", RESIZES)
def test_frame_out_equals_the_existing_resize_kernel(lib_built, H, W):
    render = _seeded_render().cuda()
    want = _resize_u8(render, H, W)
    assert torch.equal(_frame_out(render, H, W), want)
    # ... and as the pasted rectangle of a body frame
    body = torch.randint(0, 256, (H + 9, W + 5, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    got = _frame_out(render, H, W, body, x0=2, y0=7)
    assert torch.equal(got[7:7 + H, 2:2 + W], want)
    if (H, W) == (32, 32):                          # the identity: no blend error at all
        assert torch.equal(want.cpu(), torch.from_numpy(ref.to_frame(render.cpu().numpy())))


def _assert_matches_float64(got, exact255, what):
    """got: uint8 from the kernel; exact255: the float64 restatement's image * 255.  A pixel may differ, by one level, only where exact255 lies within 1e-3 of an
    integer (fp32 sampling error x 255 stays below that); such pixels are under 1 % of the frame for the seeded input, so the allowance cannot hide an error."""
    want = exact255.astype(np.uint8)
    near = np.abs(exact255 - np.rint(exact255)) <= 1e-3
    share = float(near.mean())
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: near-integer values {share:.4%} of the frame, differing values {int((diff > 0).sum())}, max difference {int(diff.max())}")
    assert share < 0.01
    assert diff.max() <= 1 and not (diff > 0)[~near].any(), (what, int(diff.max()), int((diff > 0)[~near].sum()))


@pytest.mark.parametrize("H,W", RESIZES)
def test_frame_out_against_float64(lib_built, H, W):
    render = _seeded_render()
    exact = ref.gui_image(render.double()[None], H, W) * 255.0
    _assert_matches_float64(_frame_out(render.cuda(), H, W).cpu().numpy(), exact, f"32 x 32 -> {H} x {W}")


def test_frame_out_linear_to_srgb_against_float64(lib_built):
    """utils.py:78-81 applied to the render before the resize (utils.py:1208-1212).  The values span both branches of the formula."""
    render = _seeded_render(seed=4)
    render[:4] *= 0.004                                # the linear branch, x < 0.0031308, and its neighbourhood
    exact = ref.gui_image(render.double()[None], 40, 36, color_space="linear") * 255.0
    _assert_matches_float64(_frame_out(render.cuda(), 40, 36, srgb=1).cpu().numpy(), exact, "linear -> srgb, 32 x 32 -> 40 x 36")


# ---- 4. paste geometry --------------------------------------------------------------------------------------------------------------
def test_paste_geometry(lib_built):
    FH, FW, H, W = 64, 48, 24, 20
    body = torch.randint(0, 256, (FH, FW, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    render = _seeded_render().cuda()
    d_body = body.cuda()
    small = _resize_u8(render, H, W).cpu().numpy()
    for x0, y0 in ((5, 7), (FW - W, FH - H)):         # inside; touching the right and bottom edges
        want = ref.fullbody_paste(small, body.numpy(), x0, y0)
        assert np.array_equal(_frame_out(render, H, W, d_body, x0, y0).cpu().numpy(), want), (x0, y0)
    whole = _resize_u8(render, FH, FW).cpu().numpy()    # covering the whole frame
    assert np.array_equal(_frame_out(render, FH, FW, d_body).cpu().numpy(), ref.fullbody_paste(whole, body.numpy(), 0, 0))
    for x0, y0 in ((FW - W + 1, 0), (0, FH - H + 1), (-1, 0)):   # one pixel past an edge: refused with both sizes, as the slice assignment raises
        with pytest.raises(RuntimeError, match=rf"a {W} x {H} frame at \({x0}, {y0}\) leaves the {FW} x {FH} body frame"):
            _frame_out(render, H, W, d_body, x0, y0)
    with pytest.raises(ValueError):
        ref.fullbody_paste(small, body.numpy(), FW - W + 1, 0)
    # no render: the custom-video frame of nerfreal.py:100-101
    assert np.array_equal(_frame_out(None, H, W, d_body).cpu().numpy(), ref.bgr2rgb(body.numpy()))


# ---- 5. / 6. the session -------------------------------------------------------------------------------------------------------------
def _ref_get_rays(poses, intrinsics, H, W, N=-1, patch_size=1, rect=None):
    """utils.py:274-336, whole-frame branch (as tests/test_dropin_ernerf.py restates it)"""
    device, B = poses.device, poses.shape[0]
    fx, fy, cx, cy = intrinsics
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device), indexing="ij")
    i = i.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    j = j.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    inds = torch.arange(H * W, device=device).expand([B, H * W])
    zs = torch.ones_like(i)
    directions = torch.stack(((i - cx) / fx * zs, (j - cy) / fy * zs, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions @ poses[:, :3, :3].transpose(-1, -2)
    return {"i": i, "j": j, "inds": inds, "rays_o": poses[..., :3, 3][..., None, :].expand_as(rays_d), "rays_d": rays_d}


def _make_model():
    """The golden scene's field behind the drop-in mixin, as tests/test_dropin_ernerf.py builds it."""
    from mere_fusion_amd import weights as Wt
    from mere_fusion_amd.ernerf.network import HipRenderMixin
    from test_dropin_ernerf import _ReferenceShapedBase
    g = np.load(os.path.join(ROOT, "tests", "golden", "ernerf_golden.npz"))
    sd = Wt.make_ernerf_field_state_dict(int(g["offsets"][-1]), 0)
    sd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in sd.items()}
    sd.update({k[len("audio_sd/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("audio_sd/")})
    opt = argparse.Namespace(asr_model="esperanto", emb=False, att=2, bound=1, min_near=0.05, exp_eye=True, smooth_lips=False, ind_num=16, ind_dim=4)

    class Net(HipRenderMixin, _ReferenceShapedBase):
        pass

    m = Net(opt, sd)
    with torch.no_grad():
        m.individual_codes[0].copy_(torch.from_numpy(g["render_ind_code"]))
        m.density_bitfield.copy_(torch.from_numpy(Wt.make_ernerf_sphere_bitfield()))
    m = m.cuda().eval()
    m.density_scale = 40.0
    return m, g


SIZE, S, GH, GW, FH, FW, X0, Y0 = 5, 32, 40, 36, 52, 44, 3, 6
RENDER_KW = dict(dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)
INTR = np.array([S / 0.7, S / 0.7, S / 2, S / 2])            # the camera of weights.make_ernerf_camera_rays (bench.py's whole_frame_loop uses the same)


def _session_inputs():
    g = torch.Generator().manual_seed(21)
    poses = torch.eye(4).repeat(SIZE, 1, 1)
    poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2]) + 0.05 * torch.randn(SIZE, 3, generator=g)
    return dict(poses=poses, eye=torch.rand(SIZE, 1, generator=g) * 0.5,
                torso=torch.randint(0, 256, (SIZE, S, S, 4), generator=g, dtype=torch.uint8), bg=torch.rand(S, S, 3, generator=g),
                body=torch.randint(0, 256, (SIZE, FH, FW, 3), generator=g, dtype=torch.uint8),
                custom=torch.randint(0, 256, (3, 30, 26, 3), generator=g, dtype=torch.uint8))


def _make_session(model, inp, **kw):
    from mere_fusion_amd.nerf_driver import NerfSession
    return NerfSession(model, inp["poses"].cuda(), INTR, S, S, _ref_get_rays, eye_area=inp["eye"].cuda(), bg=inp["bg"].cuda(), torso_imgs=inp["torso"].cuda(),
                       preload=kw.pop("preload", 0), fullbody_frames=inp["body"].cuda(), fullbody_offset=(X0, Y0), custom_img_cycle={2: inp["custom"].cuda()},
                       gui_size=(GH, GW), render_kw=RENDER_KW, **kw)


AUDIOTYPES = [(0, 0)] * 12
AUDIOTYPES[3], AUDIOTYPES[7], AUDIOTYPES[5] = (2, 2), (2, 2), (2, 0)        # two custom-video frames; (2, 0) is a rendered one


@pytest.mark.parametrize("preload", [0, 2])
def test_session_frame_by_frame_against_the_existing_route(lib_built, preload):
    """12 steps over 5 poses cross the mirror point and one wrap.  The yardstick per frame: collate's background in torch on the CPU, `model.render` through
    the drop-in mixin on a second, identically built model, `mf_nerf_resize_frame`, then the host paste of nerfreal.py:117-122 -- the same kernels on the same
    inputs, so the frames are bit-equal."""
    from mere_fusion_amd.ernerf import frontend
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    inp = _session_inputs()
    m_session, g = _make_model()
    m_ref, _ = _make_model()
    auds = torch.from_numpy(np.ascontiguousarray(g["auds"])).cuda()
    s = _make_session(m_session, inp, preload=preload)
    resizer = HipHeadRenderer(None, m_ref.density_bitfield)
    custom_index = {2: 0}
    cycle = {2: [f.numpy() for f in inp["custom"]]}
    seen, rendered = [], 0
    for k in range(12):
        a = auds * (1.0 + 0.05 * k)
        got = s.step(a, audiotype=AUDIOTYPES[k])
        seen.append((s.last_audio_index, s.last_index))
        mi = ref.loader_sequence(SIZE, 12)[k][1]
        if ref.is_custom(*AUDIOTYPES[k], custom_index):
            want = ref.custom_frame(cycle, custom_index, AUDIOTYPES[k][0])
        else:
            rendered += 1
            pose = inp["poses"][mi:mi + 1].cuda()
            rays = frontend.get_rays(_ref_get_rays, pose, INTR, S, S)
            bg = ref.collate_background(inp["torso"][mi].numpy(), inp["bg"], preload).view(1, -1, 3).cuda()
            out = m_ref.render(rays["rays_o"], rays["rays_d"], a, torch.zeros(1, S * S, 2, device="cuda"), pose, eye=inp["eye"][mi:mi + 1].cuda(), index=[mi],
                               staged=True, bg_color=bg, perturb=False, **RENDER_KW)
            small = resizer.resize({"image": out["image"].reshape(S, S, 3), "depth": out["depth"].reshape(S, S)}, S, S, GH, GW)["frame_u8"]
            want = ref.fullbody_paste(small.cpu().numpy(), inp["body"][mi].numpy(), X0, Y0)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape, (k, tuple(got.shape), want.shape)
        assert np.array_equal(got.cpu().numpy(), want), k
    assert seen == list(zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 1], [0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 0, 1]))
    assert rendered == 10 and m_session.mf_frames == 10 and s.custom_index[2] == 2
    assert float(got.float().std()) > 1.0                       # the last frame is a picture, not a constant


def test_session_frames_through_the_ring(lib_built):
    from mere_fusion_amd.transport import FrameRing
    inp = _session_inputs()
    m, g = _make_model()
    auds = torch.from_numpy(np.ascontiguousarray(g["auds"])).cuda()
    s = _make_session(m, inp)
    ring = FrameRing(4, (FH, FW, 3))
    try:
        for k in range(6):                                       # more frames than slots: the consumer frees them as it reads
            audio = [(np.full(320, k, np.float32), AUDIOTYPES[k][0]), (np.full(320, -k, np.float32), AUDIOTYPES[k][1])]
            frame, idx = s.step_to_ring(ring, auds, audio, audiotype=AUDIOTYPES[k])
            assert idx == s.last_index == ref.loader_sequence(SIZE, 6)[k][1]
            got, got_idx, got_audio = ring.get(timeout=10)
            assert got_idx == idx and got.dtype == np.uint8 and np.array_equal(got, frame.cpu().numpy()), k
            assert len(got_audio) == 2 and got_audio[0][1] == AUDIOTYPES[k][0] and np.array_equal(got_audio[1][0], audio[1][0])
            assert tuple(got.shape) == ((30, 26, 3) if k == 3 else (FH, FW, 3))
        assert ring.empty()
    finally:
        ring.close()


def _bare_renderer():
    """smoke()'s head-only scene: a `HipHeadRenderer` without audio or torso nets (enc_a goes in as `auds`)"""
    from mere_fusion_amd import weights as Wt
    from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    offsets, _ = grid_geometry()
    fsd = Wt.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    fsd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in fsd.items()}
    g = torch.Generator().manual_seed(0)
    enc_a, ind, eye = torch.randn(1, 32, generator=g).cuda(), (torch.randn(1, 4, generator=g) * 0.1).cuda(), torch.tensor([[0.4]]).cuda()
    rend = HipHeadRenderer(HipNeRFField(fsd, max_samples=32 * 32), torch.from_numpy(Wt.make_ernerf_sphere_bitfield()).cuda(), density_scale=40.0, ind_code=ind)
    return rend, enc_a, ind, eye


def test_session_hands_a_bare_renderer_its_aabb(lib_built):
    """A bare `HipHeadRenderer` has no module buffer: the session takes `aabb_infer` and binds it every frame.  The frame equals the renderer's own frame with
    that box bound by hand, and differs from the default box's."""
    from mere_fusion_amd.ernerf import frontend
    from mere_fusion_amd.nerf_driver import NerfSession
    half_box = torch.tensor([-0.5, -0.25, -0.5, 0.5, 0.25, 0.5], device="cuda")
    poses = torch.eye(4).repeat(2, 1, 1)
    poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2])
    poses = poses.cuda()
    frames = {}
    for name, box in (("default", None), ("half", half_box)):
        rend, enc_a, _, eye = _bare_renderer()
        s = NerfSession(rend, poses, INTR, S, S, _ref_get_rays, eye_area=eye.expand(2, 1).contiguous(), bg="white", gui_size=(GH, GW), render_kw=RENDER_KW,
                        aabb_infer=box)
        frames[name] = s.step(enc_a)
        assert (rend.aabb_infer is rend._aabb_default) == (box is None)
    rend, enc_a, _, eye = _bare_renderer()
    rend.aabb_infer = half_box
    rays = frontend.get_rays(_ref_get_rays, poses[:1], INTR, S, S)
    bg = torch.ones(S * S, 3, device="cuda")
    out = rend.render(rays["rays_o"], rays["rays_d"], enc_a, None, poses[:1], eye, bg_color=bg, loop="device", **RENDER_KW)
    assert torch.equal(frames["half"], _resize_u8(out["image"].reshape(S, S, 3), GH, GW))
    assert int((frames["half"].int() - frames["default"].int()).abs().max()) > 2
    with pytest.raises(RuntimeError, match="aabb_infer is for a bare HipHeadRenderer"):
        NerfSession(_make_model()[0], poses, INTR, S, S, _ref_get_rays, aabb_infer=half_box)


# ---- 7. aabb ------------------------------------------------------------------------------------------------------------------------
def test_head_reads_the_aabb_the_setter_stores(lib_built):
    """The head's near / far are not an output; they are read through its outputs: a render left unfinished returns the raw depth, the finished one
    clamp(depth - near, 0) / (far - near) (renderer.py:275-280, three fp32 operations, restated on the host bit for bit) -- with near / far from
    `mf_near_far_from_aabb` fed the same six floats.  A ray that misses the box has near = far = FLT_MAX and 0 / 0 in both.  The whole image is also held to the
    host loop, which takes near / far from `mf_near_far_from_aabb` itself, at twice smoke()'s gate (each loop is within 1e-5 of the CPU restatement)."""
    from mere_fusion_amd import weights as Wt
    from mere_fusion_amd.ernerf import _raymarching_face as rm
    from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    rend, enc_a, ind, eye = _bare_renderer()
    ro, rd = (torch.from_numpy(a).cuda() for a in Wt.make_ernerf_camera_rays(32))
    N = ro.shape[0]

    def render(finish=True):
        out = rend.run_cuda_device(ro, rd, enc_a, ind, eye, bg_color=1.0, finish=finish)
        return {k: v.clone() for k, v in out.items() if v is not None}
    same_bits = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))       # (a ray that misses the box has a NaN depth)
    default = render()
    b = rend.bound
    half_box = torch.tensor([-b / 2, -b / 4, -b / 2, b / 2, b / 4, b / 2], dtype=torch.float32, device="cuda")
    rend.aabb_infer = half_box
    raw = render(finish=False)
    got = render()
    nears, fars = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    rm.near_far_from_aabb(ro.contiguous(), rd.contiguous(), half_box, N, rend.min_near, nears, fars)
    nr, fr, dr = nears.cpu().numpy(), fars.cpu().numpy(), raw["depth"].cpu().numpy()
    with np.errstate(invalid="ignore"):
        want_depth = np.maximum(dr - nr, np.float32(0)) / (fr - nr)
    hit = nr < np.float32(3e38)
    assert 0.05 < hit.mean() < 1.0                              # the half box is hit by some rays of this camera and missed by others
    assert np.array_equal(got["depth"].cpu().numpy(), want_depth, equal_nan=True)
    assert float((dr[hit] > nr[hit]).mean()) > 0.05             # ... and for these rays the finished depth depends on near AND far
    host = rend.run_cuda(ro, rd, enc_a, ind, eye, bg_color=1.0)  # the host loop reads self.aabb_infer through mf_near_far_from_aabb
    assert float((got["image"] - host["image"]).abs().max()) <= 2e-5
    assert float((got["image"] - default["image"]).abs().max()) > 1e-2      # another box, another picture
    # the default box handed over explicitly gives the default's bits, and so does going back to the built-in box
    rend.aabb_infer = torch.tensor([-b, -b / 2, -b, b, b / 2, b], dtype=torch.float32, device="cuda")
    again = render()
    assert same_bits(again["image"], default["image"]) and same_bits(again["depth"], default["depth"])
    rend.aabb_infer = rend._aabb_default
    again = render()
    assert same_bits(again["image"], default["image"]) and same_bits(again["depth"], default["depth"])
    with pytest.raises(RuntimeError, match="aabb_infer must be a contiguous float32 CUDA tensor of 6 values"):
        rend.aabb_infer = torch.zeros(6)
        render()


def test_mixin_passes_the_modules_aabb_infer(lib_built):
    """`HipRenderMixin.run_cuda` hands the module's `aabb_infer` buffer over every frame; a module without one (the stand-in of the other drop-in tests) renders as
    before -- the golden frame."""
    m, g = _make_model()
    Wd = int(g["render_W"])
    from mere_fusion_amd import weights as Wt
    ro, rd = Wt.make_ernerf_camera_rays(Wd)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bg = torch.tensor([0.1, 0.2, 0.3]).expand(Wd * Wd, 3).contiguous().cuda()
    args = (cu(ro)[None], cu(rd)[None], cu(g["auds"]), torch.zeros(1, Wd * Wd, 2, device="cuda"), torch.eye(4, device="cuda")[None])
    kw = dict(eye=cu(g["field_e"]), index=[0], staged=True, bg_color=bg, perturb=False, **RENDER_KW)
    first = m.render(*args, **kw)["image"].clone()
    assert np.abs(first.reshape(-1, 3).cpu().numpy() - g["render_image"]).max() <= 1e-3       # the bound of tests/test_dropin_ernerf.py
    m.register_buffer("aabb_infer", torch.tensor([-0.5, -0.25, -0.5, 0.5, 0.25, 0.5], device="cuda"))
    boxed = m.render(*args, **kw)["image"].clone()
    assert float((boxed - first).abs().max()) > 1e-2
    m.aabb_infer.copy_(torch.tensor([-1.0, -0.5, -1.0, 1.0, 0.5, 1.0]))                        # the buffer is read where it lives, every frame
    assert torch.equal(m.render(*args, **kw)["image"], first)
    assert m._mf["renderer"].aabb_infer.data_ptr() == m.aabb_infer.data_ptr()
    # a buffer that is not fp32 (a `.half()`ed module): its values go into one fp32 copy whose address stays, frame after frame
    m.aabb_infer = torch.tensor([-0.5, -0.25, -0.5, 0.5, 0.25, 0.5], device="cuda").half()
    ptrs = []
    for _ in range(2):
        assert torch.equal(m.render(*args, **kw)["image"], boxed)
        ptrs.append(m._mf["renderer"].aabb_infer.data_ptr())
    assert ptrs[0] == ptrs[1] and m._mf["renderer"].aabb_infer.dtype == torch.float32
