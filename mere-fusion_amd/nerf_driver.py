"""One ER-NeRF session, frame by frame, with the frame in HBM until the last copy: the counterpart of `MuseSession` (muse_driver.py) and
`LipSession.step_pasted` (lip_driver.py) for the third model the reference serves.

The reference runs one frame as `NeRFReal.test_step` (nerfreal.py:70-127): the loader's `collate` (provider.py:285-341: mirrored index, pose, `get_rays`, eye
feature, the torso image over the background), `Trainer.test_gui_with_data` (utils.py:1190-1223: `model.render`, resize, `.cpu().numpy()`), then numpy and cv2 on
the host (`(image * 255).astype(np.uint8)`, the --fullbody paste, or a custom-video frame instead of a render).  `NerfSession.step` is the same frame as one
enqueue on the caller's stream that ends in the uint8 RGB frame a `VideoFrame` takes:

    frontend.get_rays                      rays of the frame's pose (directions cached per (H, W, intrinsics))
    mf_nerf_frame_background               provider.py:323, when torso images are given (a head-only model)
    model.render / HipHeadRenderer.render  the device loop (mf_nerf_head_render), as the drop-in runs it
    mf_nerf_frame_out                      utils.py:1208-1212 + nerfreal.py:110-122 (or :98-107 for a custom-video frame)

`NerfFrameBatch` is the first and the last of these for the frames of many sessions in one launch each (mf_nerf_frame_batch_background / _out), the same bits per
frame; `nerf_serving.NerfBatcher` uses it around its batched head call.

No synchronisation, no graph of its own, no side stream.  `step_to_ring` hands the frame to a `transport.FrameRing` as the other two drivers do."""
import ctypes as C

import torch

from . import _lib, ops
from .ernerf import frontend
from .serving import mirror_index, refuse
from .transport import is_i420_shape


def loader_indices(size, index):
    """(index the audio uses, index pose / eye / torso image / body frame use) of the `index`-th frame of a session over `size` poses: the live loader runs over
    2 * size indices and starts again (provider.py:351, nerfreal.py:72-76); `collate` mirrors what is not audio (provider.py:292-298, 276-283)."""
    i = index % (2 * size)
    return i, mirror_index(size, i)


def _refuse(msg):
    refuse("NerfSession", msg)


class NerfFrameBatch:
    """mf_nerf_frame_batch: `NerfSession.background` and `.frame_out` for a list of frames in ONE launch each.  The sessions of a call have the same sizes (`bg_key` /
    `out_key`); a call takes at most `max_frames` frames of at most `max_pixels` rendered pixels each.  Nothing synchronises."""

    MAX_FRAMES = 64                     # the library's limit per call

    def __init__(self, max_frames, max_pixels):
        self._lib = _lib.lib()
        self.max_frames, self.max_pixels = int(max_frames), int(max_pixels)
        self._h = C.c_void_p()
        _lib.check(self._lib.mf_nerf_frame_batch_create(self.max_frames, self.max_pixels, C.byref(self._h)), "mf_nerf_frame_batch_create")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.mf_nerf_frame_batch_destroy(h)
            self._h = None

    def background(self, sessions, mis):
        """bg_color [F, H * W, 3] fp32: row i is `sessions[i].background(mis[i])` (sessions with torso images, of one `bg_key`)"""
        s0, F = sessions[0], len(sessions)
        if any(s.torso_imgs is None or s.bg_key() != s0.bg_key() for s in sessions):
            refuse("NerfFrameBatch", "background: the sessions of a call have torso images and one render size")
        out = torch.empty(F, s0.H * s0.W, 3, dtype=torch.float32, device=s0.poses.device)
        descs = (_lib.MfNerfBgDesc * F)()
        for i, (s, mi) in enumerate(zip(sessions, mis)):
            d = descs[i]
            d.torso_rgba, d.bg_image = s.torso_imgs[mi].data_ptr(), (s.bg_image.data_ptr() if s.bg_image is not None else None)
            d.bg_const, d.half_mode, d.bg_color = s.bg_const, int(s.half), out[i].data_ptr()
        _lib.check(self._lib.mf_nerf_frame_batch_background(self._h, descs, F, s0.H, s0.W, _lib.stream_ptr(s0.poses.device)), "mf_nerf_frame_batch_background")
        return out

    def frame_out(self, sessions, images, bodies, out):
        """`sessions[i].frame_out(images[i], bodies[i])` into out[i]: out is a contiguous uint8 block [F, FH, FW, 3] (sessions of one `out_key`).  images[i] None:
        the custom-video frame bodies[i]."""
        s0, F = sessions[0], len(sessions)
        key = s0.out_key()
        FH, FW = key[4], key[5]
        if any(s.out_key() != key for s in sessions):
            refuse("NerfFrameBatch", "frame_out: the sessions of a call have one render size, GUI size, frame size and colour space")
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (F, FH, FW, 3)):
            refuse("NerfFrameBatch", f"frame_out: out must be a contiguous uint8 CUDA tensor [{F}, {FH}, {FW}, 3]")
        descs = (_lib.MfNerfOutDesc * F)()
        keep = []
        for i, (s, image, body) in enumerate(zip(sessions, images, bodies)):
            if image is not None:
                image = image.reshape(s.H, s.W, 3)
                if image.dtype != torch.float32 or not image.is_contiguous():
                    image = image.float().contiguous()
            if body is not None and tuple(body.shape) != (FH, FW, 3):
                refuse("NerfFrameBatch", f"frame_out: frame {i} is {tuple(body.shape)}, the block's frames are ({FH}, {FW}, 3)")
            keep.append(image)
            d = descs[i]
            d.render, d.body_bgr = (image.data_ptr() if image is not None else None), (body.data_ptr() if body is not None else None)
            d.x0, d.y0 = (s.x0, s.y0) if (image is not None and body is not None) else (0, 0)
        _lib.check(self._lib.mf_nerf_frame_batch_out(self._h, descs, F, s0.H, s0.W, s0.GH, s0.GW, FH, FW, int(s0.linear_to_srgb), C.c_void_p(out.data_ptr()),
                                                     _lib.stream_ptr(s0.poses.device)), "mf_nerf_frame_batch_out")
        del keep
        return out


class NerfSession:
    """model: the reference's NeRFNetwork behind `HipRenderMixin` (the drop-in class), or a bare `HipHeadRenderer`.  poses [N, 4, 4]; intrinsics (fx, fy, cx, cy);
    (H, W) the render size; get_rays: the reference's `get_rays` (ernerf/nerf_triplane/utils.py:255), called once per (H, W, intrinsics) by `frontend.get_rays`;
    eye_area [N, 1] or None; bg: an image [H, W, 3] in [0, 1], 'white' or 'black' (provider.py:203-212); torso_imgs: uint8 RGBA [N, H, W, 4] with `preload` 0 / 1
    (fp32 arithmetic) or 2 (half), as `--preload` chooses in the reference; fullbody_frames: uint8 BGR [N, FH, FW, 3] with fullbody_offset (x, y);
    custom_img_cycle {audiotype: uint8 BGR [M, h, w, 3]} and custom_index {audiotype: int} as `BaseReal` holds them (basereal.py:52-68); gui_size (H, W) of
    `test_gui_with_data`, default the render size; linear_to_srgb: `opt.color_space == 'linear'`; render_kw: what `Trainer.test_step` passes on from `opt`
    (dt_gamma, max_steps, T_thresh); aabb_infer: fp32 [6], the checkpoint's box for a bare `HipHeadRenderer`, handed to it every frame (a module behind the mixin
    carries its own buffer, which the mixin hands over).  Every tensor lives on the device and is uploaded by the caller once: there is no CPU path."""

    def __init__(self, model, poses, intrinsics, H, W, get_rays, eye_area=None, bg="white", torso_imgs=None, preload=0, fullbody_frames=None,
                 fullbody_offset=(0, 0), custom_img_cycle=None, custom_index=None, gui_size=None, bg_coords=None, linear_to_srgb=False, render_kw=None, aabb_infer=None):
        H, W = int(H), int(W)
        GH, GW = (H, W) if gui_size is None else (int(gui_size[0]), int(gui_size[1]))
        if not (torch.is_tensor(poses) and poses.dim() == 3 and tuple(poses.shape[1:]) == (4, 4) and poses.shape[0] >= 1):
            _refuse("poses must be a tensor [N, 4, 4] with N >= 1")
        N = int(poses.shape[0])
        if eye_area is not None and not (torch.is_tensor(eye_area) and eye_area.numel() == N):
            _refuse(f"eye_area holds {eye_area.numel() if torch.is_tensor(eye_area) else '?'} values for {N} poses")
        if torso_imgs is not None:
            if not (torch.is_tensor(torso_imgs) and torso_imgs.dtype == torch.uint8 and torso_imgs.dim() == 4 and tuple(torso_imgs.shape[1:]) == (H, W, 4)):
                _refuse(f"torso_imgs must be uint8 RGBA [N, {H}, {W}, 4]")
            if torso_imgs.shape[0] != N:
                _refuse(f"{torso_imgs.shape[0]} torso images for {N} poses (the loader indexes both with the same mirrored index, provider.py:300, 317)")
            if preload not in (0, 1, 2):
                _refuse(f"preload {preload} (0, 1: fp32 arithmetic; 2: half)")
        x0, y0 = int(fullbody_offset[0]), int(fullbody_offset[1])
        if fullbody_frames is not None:
            if not (torch.is_tensor(fullbody_frames) and fullbody_frames.dtype == torch.uint8 and fullbody_frames.dim() == 4 and fullbody_frames.shape[3] == 3):
                _refuse("fullbody_frames must be uint8 BGR [N, FH, FW, 3]")
            if fullbody_frames.shape[0] != N:
                _refuse(f"{fullbody_frames.shape[0]} body frames for {N} poses (nerfreal.py:118 indexes them with the loader's mirrored index)")
            FH, FW = int(fullbody_frames.shape[1]), int(fullbody_frames.shape[2])
            if x0 < 0 or y0 < 0 or x0 + GW > FW or y0 + GH > FH:
                _refuse(f"a {GW} x {GH} frame at ({x0}, {y0}) leaves the {FW} x {FH} body frame (nerfreal.py:122 raises there; nothing is clipped)")
        elif (x0, y0) != (0, 0):
            _refuse(f"fullbody_offset ({x0}, {y0}) without fullbody_frames")
        if torch.is_tensor(bg):
            if tuple(bg.shape) != (H, W, 3):
                _refuse(f"the background image must be [{H}, {W}, 3] (got {tuple(bg.shape)})")
        elif bg not in ("white", "black"):
            _refuse(f"bg must be an image, 'white' or 'black' (got {bg!r})")
        custom_img_cycle = dict(custom_img_cycle or {})
        if aabb_infer is not None:
            if isinstance(model, torch.nn.Module):
                _refuse("aabb_infer is for a bare HipHeadRenderer; a module's own `aabb_infer` buffer is read every frame")
            if not (torch.is_tensor(aabb_infer) and aabb_infer.numel() == 6):
                _refuse("aabb_infer must be a tensor of 6 values")
        for name, t in (("poses", poses), ("eye_area", eye_area), ("bg", bg), ("torso_imgs", torso_imgs), ("fullbody_frames", fullbody_frames), ("bg_coords", bg_coords),
                        ("aabb_infer", aabb_infer),
                        *((f"custom_img_cycle[{k}]", f) for k, v in custom_img_cycle.items() for f in v)):
            if torch.is_tensor(t) and not t.is_cuda:
                _refuse(f"{name} must be a CUDA tensor (there is no CPU path)")
        for k, v in custom_img_cycle.items():
            if len(v) == 0 or any(not (torch.is_tensor(f) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3) for f in v):
                _refuse(f"custom_img_cycle[{k}] must hold uint8 BGR frames [h, w, 3]")
        dev = poses.device
        self.model, self.H, self.W, self.GH, self.GW, self.size = model, H, W, GH, GW, N
        self._is_module = hasattr(model, "run_cuda") and isinstance(model, torch.nn.Module)      # behind HipRenderMixin; else a bare HipHeadRenderer
        has_torso = bool(getattr(model, "torso", None))
        self.poses = poses.to(torch.float32).contiguous()
        self.intrinsics, self._ref_get_rays = intrinsics, get_rays
        self.eye_area = None if eye_area is None else eye_area.to(torch.float32).reshape(N, 1).contiguous()
        self.half = preload == 2
        # a model with a torso net takes the plain background, whatever torso images were given (provider.py:325-328)
        self.torso_imgs = None if (torso_imgs is None or has_torso) else torso_imgs.contiguous()
        if torch.is_tensor(bg):
            self.bg_image, self.bg_const = bg.to(torch.float32).contiguous(), 0.0
        else:
            self.bg_image, self.bg_const = None, (1.0 if bg == "white" else 0.0)
        if self.torso_imgs is None:
            # the loader's own bg_color (provider.py:328-330); bg_img is a half tensor when no torso images are given or with preload 2 (provider.py:237-238)
            full = self.bg_image if self.bg_image is not None else torch.full((H, W, 3), self.bg_const, dtype=torch.float32, device=dev)
            self.bg_color = (full.half().float() if (torso_imgs is None or self.half) else full).reshape(H * W, 3).contiguous()
        if bg_coords is None:
            if has_torso:
                _refuse("a model with a torso net needs bg_coords (provider.py:274)")
            bg_coords = torch.zeros(1, H * W, 2, dtype=torch.float32, device=dev)             # read by run_torso only
        self.bg_coords = bg_coords
        self.fullbody_frames = None if fullbody_frames is None else fullbody_frames.contiguous()
        self.x0, self.y0 = x0, y0
        self.custom_img_cycle = custom_img_cycle
        self.custom_index = {k: 0 for k in custom_img_cycle} if custom_index is None else custom_index
        self.linear_to_srgb = bool(linear_to_srgb)
        self.render_kw = dict(dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4) if render_kw is None else dict(render_kw)
        self.aabb_infer = None if aabb_infer is None else aabb_infer.to(torch.float32).reshape(6).contiguous()
        self.index = 0                    # frames stepped: the loader's position
        self.last_index = None            # the mirrored index of the frame step() returned last
        self.last_audio_index = None      # ... and its unmirrored one (what indexes precomputed audio features, provider.py:292-295)
        self._lib = _lib.lib()

    # ---- the two launches around the render ------------------------------------------------------------------------------------------
    def background(self, mi):
        """bg_color [H * W, 3] fp32 of the frame (provider.py:316-330)"""
        if self.torso_imgs is None:
            return self.bg_color
        out = torch.empty(self.H * self.W, 3, dtype=torch.float32, device=self.poses.device)
        _lib.check(self._lib.mf_nerf_frame_background(C.c_void_p(self.torso_imgs[mi].data_ptr()), C.c_void_p(self.bg_image.data_ptr()) if self.bg_image is not None else None,
                                                      self.bg_const, self.H, self.W, int(self.half), C.c_void_p(out.data_ptr()), _lib.stream_ptr(self.poses.device)),
                   "mf_nerf_frame_background")
        return out

    # ---- what the frames of one NerfFrameBatch call share ----------------------------------------------------------------------------
    def bg_key(self):
        return (self.H, self.W)

    def out_key(self):
        """(render size, GUI size, frame size, colour space): the sizes one mf_nerf_frame_batch_out call shares"""
        FH, FW = (int(self.fullbody_frames.shape[1]), int(self.fullbody_frames.shape[2])) if self.fullbody_frames is not None else (self.GH, self.GW)
        return (self.H, self.W, self.GH, self.GW, FH, FW, self.linear_to_srgb)

    def frame_out(self, image, body=None, out=None, i420=False):
        """The uint8 RGB frame: `image` [H, W, 3] fp32 (or None: `body` alone, channels reversed) resized to the GUI size, over `body` at the offset.
        out: the contiguous uint8 device tensor of the frame's size to write instead of a new one (nerf_serving.NerfBatcher: one block per step).
        i420: the frame as planar YUV 4:2:0 instead, uint8 [FH * 3 / 2, FW] (ops.frames_to_i420 behind the same launch; `out` then has that shape)."""
        if i420:
            return ops.frames_to_i420(self.frame_out(image, body), order="rgb", out=out)
        dev = self.poses.device
        FH, FW = (self.GH, self.GW) if body is None else (int(body.shape[0]), int(body.shape[1]))
        if out is None:
            out = torch.empty(FH, FW, 3, dtype=torch.uint8, device=dev)
        elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (FH, FW, 3)):
            _refuse(f"out must be a contiguous uint8 CUDA tensor [{FH}, {FW}, 3]")
        x0, y0 = (self.x0, self.y0) if (image is not None and body is not None) else (0, 0)
        _lib.check(self._lib.mf_nerf_frame_out(C.c_void_p(image.data_ptr()) if image is not None else None, self.H, self.W, self.GH, self.GW,
                                               C.c_void_p(body.data_ptr()) if body is not None else None, FH, FW, x0, y0, int(self.linear_to_srgb),
                                               C.c_void_p(out.data_ptr()), _lib.stream_ptr(self.poses.device)), "mf_nerf_frame_out")
        return out

    def next_custom(self, audiotype):
        """nerfreal.py:98-102: the custom-video image (uint8 BGR) that stands in for this frame's render -- both audio types non-zero and a cycle registered for the
        first; the cycle ping-pongs on its own counter -- or None for a rendered frame."""
        t1, t2 = audiotype
        if t1 != 0 and t2 != 0 and self.custom_index.get(t1) is not None:
            cycle = self.custom_img_cycle[t1]
            ci = mirror_index(len(cycle), self.custom_index[t1])
            self.custom_index[t1] += 1
            return cycle[ci].contiguous()
        return None

    # ---- one frame ---------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, auds, audiotype=(0, 0), out=None):
        """One `NeRFReal.test_step`: the uint8 RGB frame as a device tensor -- [GH, GW, 3], [FH, FW, 3] with body frames, or the custom image's size.
        auds: `NerfASRFrontend.get_next_feat()`; audiotype: the types of the frame's two audio chunks (nerfreal.py:81-88); out: see frame_out."""
        job = self.begin(auds, audiotype, out=out)
        if not isinstance(job, dict):                           # the finished custom-video frame
            return job
        if self._is_module:                                                                      # utils.py:949-950
            res = self.model.render(job["rays_o"], job["rays_d"], auds, self.bg_coords, job["poses"], eye=job["eye"], index=[job["mi"]], staged=True,
                                    bg_color=job["bg_color"], perturb=False, **self.render_kw)
        else:
            self.bind_aabb()
            res = self.model.render(job["rays_o"], job["rays_d"], auds, self.bg_coords, job["poses"], job["eye"], bg_color=job["bg_color"], loop="device",
                                    **self.render_kw)
        return self.end(job, res["image"], out=out)

    # ---- the same frame in two halves, so that a batcher can render the frames of many sessions in one call between them (nerf_serving.NerfBatcher) ----------
    @torch.no_grad()
    def begin(self, auds, audiotype=(0, 0), out=None, defer=False):
        """The part of step() in front of the render: advances the loader and returns either the finished custom-video frame (`out` as in step) or the
        frame's render job -- a dict of what `model.render` / `render_frames` take (rays_o, rays_d, auds, bg_coords, poses, eye, bg_color) plus `mi`, the mirrored
        index, and `body`, the body frame or None.
        defer: nothing is launched for the two ends of the frame, a NerfFrameBatch call does them for many frames later: a custom-video frame comes back as
        {"custom": image}, and a job whose background is the torso image over the background carries bg_color None until `set_background`."""
        ai, mi = loader_indices(self.size, self.index)          # the loader advances on every frame, a custom-video one included (nerfreal.py:72-76)
        self.index += 1
        self.last_audio_index, self.last_index = ai, mi
        custom = self.next_custom(audiotype)
        if custom is not None:
            if defer:
                return {"custom": custom, "mi": mi}
            return self.frame_out(None, custom, **({} if out is None else {"out": out}))
        pose = self.poses[mi:mi + 1]
        rays = frontend.get_rays(self._ref_get_rays, pose, self.intrinsics, self.H, self.W)
        eye = None if self.eye_area is None else self.eye_area[mi:mi + 1]
        bg = None if (defer and self.torso_imgs is not None) else self.background(mi)
        return {"rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "auds": auds, "bg_coords": self.bg_coords, "poses": pose, "eye": eye,
                "bg_color": None if bg is None else (bg[None] if self._is_module else bg), "mi": mi, "body": None if self.fullbody_frames is None else self.fullbody_frames[mi],
                "bg_pending": bg is None}

    def set_background(self, job, bg):
        """the deferred background of `job`: bg [H * W, 3] fp32, a row of NerfFrameBatch.background"""
        job["bg_color"], job["bg_pending"] = (bg[None] if self._is_module else bg), False

    def bind_aabb(self):
        """a bare HipHeadRenderer reads the session's box (renderer.py:226 reads the buffer every frame)"""
        if not self._is_module and self.aabb_infer is not None:
            self.model.aabb_infer = self.aabb_infer

    def end(self, job, image, out=None):
        """The part of step() behind the render: the rendered `image` of `job` -> the uint8 RGB frame (`out` as in step)."""
        image = image.reshape(self.H, self.W, 3)
        if image.dtype != torch.float32 or not image.is_contiguous():
            image = image.float().contiguous()
        return self.frame_out(image, job["body"], **({} if out is None else {"out": out}))

    def step_to_ring(self, ring, auds, audio_frames, audiotype=(0, 0), i420=False):
        """step() and the frame into `ring` (transport.FrameRing): one DMA into the slot behind the frame's kernels, one stream fence, then the consumer's
        `(frame, idx, audio_frames)` tuple is published -- idx the frame's mirrored index, audio_frames its two (pcm, type) pairs.  A custom-video frame
        takes the same way.  i420: the frame is converted to planar YUV 4:2:0 on the same stream and travels as uint8 [h * 3 / 2, w] (ops.frames_to_i420, RGB
        order; the consumer's line is `VideoFrame.from_ndarray(frame, format="yuv420p")`); a ring whose slots are no such block (transport.i420_shape) is
        refused before the session moves.  Returns (the device frame as it entered the ring, idx)."""
        if i420 and not is_i420_shape(tuple(getattr(ring, "frame_shape", ()))):
            _refuse(f"step_to_ring(i420=True): the ring has slots of shape {tuple(getattr(ring, 'frame_shape', ()))}, which is no [H * 3 / 2, W] plane block "
                    f"(FrameRing(slots, transport.i420_shape(H, W)))")
        frame = self.step(auds, audiotype)
        if i420:
            frame = ops.frames_to_i420(frame, order="rgb")
        idx = self.last_index
        tok = ring.begin_batch(frame[None], [idx])
        try:
            _lib.check(self._lib.mf_stream_synchronize(tok["stream"]), "stream_synchronize")
        except BaseException:
            ring.abort_batch(tok)
            raise
        ring.commit_batch(tok, list(audio_frames))
        return frame, idx
