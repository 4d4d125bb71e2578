"""The head render loop of ER-NeRF on MI355X: the inference branch of `NeRFRenderer.run_cuda`
(ernerf/nerf_triplane/renderer.py:158-291) over the HIP kernels, one frame per call.

The reference's own renderer keeps working unchanged on top of the extension shims (dropin/_raymarching_face.py ...) and a
`model.forward = HipNeRFField(...).forward` hook; this module is the same loop without the torch.autograd wrappers, used by
bench.py / smoke() / the tests, and it is what `nerfreal.py:render` amounts to per frame once torso and audio nets are fixed.
The compaction `rays_alive[rays_alive >= 0]` (renderer.py:266) and its host sync are kept as in the reference."""
import ctypes as C
import os

import torch

from .. import _lib
from . import _raymarching_face as rm


class HipHeadRenderer:
    def __init__(self, field, density_bitfield, bound=1.0, min_near=0.05, density_scale=1.0, grid_size=128, torso=None, audio=None,
                 ind_code=None, smooth_lips=False):
        import math
        self.field = field
        self.torso, self.audio, self.ind_code, self.smooth_lips, self.enc_a = torso, audio, ind_code, bool(smooth_lips), None
        self.bound, self.min_near, self.density_scale, self.grid_size = float(bound), float(min_near), float(density_scale), int(grid_size)
        self.cascade = 1 + math.ceil(math.log2(bound))                                   # renderer.py:69
        self.bitfield = density_bitfield.contiguous()
        b = self.bound
        self.aabb_infer = torch.tensor([-b, -b / 2, -b, b, b / 2, b], dtype=torch.float32, device=density_bitfield.device)   # renderer.py:86-89
        self._aabb_default = self.aabb_infer        # rebinding `aabb_infer` (a checkpoint's buffer: HipRenderMixin does, and NerfSession for a bare renderer) makes the device loop read it too
        self._lib = _lib.lib()
        self._head, self._side, self._batch = None, None, None

    def _audio_part(self, auds):
        """audio window -> enc_a with the lip-smoothing EMA of renderer.py:190-194 (state: self.enc_a)"""
        if self.audio is not None and self.smooth_lips and hasattr(self.audio, "encode_audio_smooth"):
            # the EMA of renderer.py:190-194 inside the encoder's launch (three torch elementwise launches per frame otherwise; same bits)
            enc_a = self.audio.encode_audio_smooth(auds, self.enc_a)
            if enc_a is not None:
                self.enc_a = enc_a
            return enc_a
        enc_a = self.audio.encode_audio(auds) if self.audio is not None else auds
        if enc_a is not None and self.smooth_lips:
            if self.enc_a is not None:
                enc_a = 0.35 * self.enc_a + (1 - 0.35) * enc_a
            self.enc_a = enc_a
        return enc_a

    @torch.no_grad()
    def render(self, rays_o, rays_d, auds, bg_coords, poses, eye, bg_color=None, **kw):
        """One frame as `NeRFRenderer.render` -> `run_cuda` does it (renderer.py:657-677, 158-291): audio window -> enc_a (+ the lip
        smoothing EMA of :190-194), fixed individual code 0 (:197-202), head loop, torso / background mix (:272-277).
        loop="device" runs the head with device-side round control."""
        device_loop = kw.pop("loop", "host") == "device"
        # (the torso on a second stream beside the head paid while it was a ~0.3 ms launch chain; as one 71 us kernel the cross-stream dependency cost more
        # than the overlap returned, 0.737 vs 0.711 ms per frame: the path left in round 5)
        enc_a = self._audio_part(auds)
        if device_loop and self.torso is not None and not kw.get("graph"):
            # the head loop is enqueued FIRST and left unfinished; the torso's per-frame host work (the wrapped anchors: a 4 x 4 inverse and 42 sines, ~90 us, and the
            # device -> host copy of the pose when it lives on the device as the reference's does) then runs while the GPU marches, and the background mix closes the
            # frame.  Same kernels, same bits; a caller that syncs every frame (the reference's loop, through the drop-in) no longer pays that host time on top
            out = self.run_cuda_device(rays_o, rays_d, enc_a, self.ind_code, eye, bg_color=None, finish=False, **kw)
            return self.finish_device(out, self.torso.run_torso(bg_coords, poses, bg_color)["bg_color"])
        if self.torso is not None:
            bg_color = self.torso.run_torso(bg_coords, poses, bg_color)["bg_color"]
        if device_loop:
            return self.run_cuda_device(rays_o, rays_d, enc_a, self.ind_code, eye, bg_color=bg_color, **kw)
        return self.run_cuda(rays_o, rays_d, enc_a, self.ind_code, eye, bg_color=bg_color, **kw)

    @torch.no_grad()
    def resize(self, out, h, w, H, W, want_u8=True):
        """`test_gui_with_data`'s resize to the GUI size (utils.py:1208-1216): image bilinear, depth nearest, uint8 frame of nerfreal.py:111."""
        dev = out["image"].device
        img, dep = out["image"].contiguous(), out["depth"].contiguous()
        assert img.numel() == 3 * h * w and dep.numel() == h * w
        res = {"image": torch.empty(H, W, 3, device=dev), "depth": torch.empty(H, W, device=dev),
               "frame_u8": torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if want_u8 else None}
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.mf_nerf_resize_frame(p(img), p(dep), h, w, H, W, p(res["image"]), p(res["depth"]), p(res["frame_u8"]),
                                                  _lib.stream_ptr()), "mf_nerf_resize_frame")
        return res

    @staticmethod
    def _bg_args(bg_color, N):
        """`bg_color` (None: white, a number, a [3] or a per-ray [N, 3] tensor) as the finish kernels take it: (tensor or None, per_ray, constant)"""
        bg = bg_color.float().contiguous() if torch.is_tensor(bg_color) else None
        return bg, bg is not None and bg.numel() == 3 * N, float(1.0 if bg_color is None else (0.0 if bg is not None else bg_color))

    @staticmethod
    def _frame_args(rays_o, rays_d, enc_a, ind_code, eye, want_u8):
        """One frame's inputs as the device loops take them -> (rays_o, rays_d, enc_a, ind_code or None, eye_dev or None, eye value, fresh); fresh() allocates
        the frame's dict of output tensors."""
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N, dev = rays_o.shape[0], rays_o.device
        ea = enc_a.float().reshape(-1).contiguous()
        ic = ind_code.float().reshape(-1).contiguous() if ind_code is not None else None
        # the eye feature: a device tensor (the reference's loader hands one over, provider.py) is read by the kernels where it lives -- no device -> host copy, no
        # sync in front of the frame; a host tensor / None goes by value as before
        eye_dev = eye.float().reshape(-1)[:1].contiguous() if (torch.is_tensor(eye) and eye.is_cuda) else None
        ev = 0.0 if (eye is None or eye_dev is not None) else float(eye.reshape(-1)[0])

        def fresh():
            return {"image": torch.empty(N, 3, device=dev), "depth": torch.empty(N, device=dev), "weights_sum": torch.empty(N, device=dev),
                    "frame_u8": torch.empty(N, 3, dtype=torch.uint8, device=dev) if want_u8 else None}
        return rays_o, rays_d, ea, ic, eye_dev, ev, fresh

    def finish_device(self, out, bg_color):
        """Background mix / depth normalisation / uint8 frame for a run_cuda_device(finish=False) result."""
        N = out["image"].shape[0]
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        bg, per_ray, bgc = self._bg_args(bg_color, N)
        _lib.check(self._lib.mf_nerf_head_finish(self._head, N, p(bg), int(per_ray), bgc, p(out["image"]), p(out["depth"]), p(out["weights_sum"]),
                                                 p(out["frame_u8"]), _lib.stream_ptr()), "mf_nerf_head_finish")
        return out

    def __del__(self):
        h = getattr(self, "_head", None)
        if h:
            self._lib.mf_nerf_head_destroy(h)
            self._head = None
        b = getattr(self, "_batch", None)
        if b:
            self._lib.mf_nerf_head_batch_destroy(b)
            self._batch = None

    @torch.no_grad()
    def run_cuda_device(self, rays_o, rays_d, enc_a, ind_code, eye, bg_color=None, dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4, want_u8=False,
                        graph=False, finish=True):
        """The same frame as run_cuda with the round control on the device (mf_nerf_head_render): one enqueue, no host sync between
        rounds.  graph=True captures the enqueue once per (ray count, tensors, launched rounds) into a CUDA graph and replays it."""
        rays_o, rays_d, ea, ic, eye_dev, ev, fresh = self._frame_args(rays_o, rays_d, enc_a, ind_code, eye, want_u8)
        N = rays_o.shape[0]
        if getattr(self, "_head", None) is None or self._head_cap < N:
            if getattr(self, "_head", None):
                self._lib.mf_nerf_head_destroy(self._head)
            self._head = C.c_void_p()
            _lib.check(self._lib.mf_nerf_head_create(self.field._h, N, C.byref(self._head)), "mf_nerf_head_create")
            self._head_cap, self._graphs = N, {}
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        bg, per_ray, bgc = self._bg_args(bg_color, N)
        self._eye_keep = eye_dev
        _lib.check(self._lib.mf_nerf_head_set_eye(self._head, p(eye_dev)), "mf_nerf_head_set_eye")
        # the box of near / far: the reference reads its persistent buffer `self.aabb_infer` every frame (renderer.py:226); the head reads a rebound one where it
        # lives (mf_nerf_head_set_aabb).  Never rebound: the head's own box from `bound`, as before
        aabb = self._aabb_arg()
        _lib.check(self._lib.mf_nerf_head_set_aabb(self._head, p(aabb)), "mf_nerf_head_set_aabb")

        def enqueue(out):
            _lib.check(self._lib.mf_nerf_head_render(self._head, p(rays_o), p(rays_d), N, p(self.bitfield), self.cascade, self.grid_size, self.min_near,
                                                     float(dt_gamma), int(max_steps), float(T_thresh), self.density_scale, p(ea), p(ic), ev, p(bg), int(per_ray) if finish else -1,
                                                     bgc, p(out["image"]), p(out["depth"]), p(out["weights_sum"]), p(out["frame_u8"]),
                                                     _lib.stream_ptr()), "mf_nerf_head_render")

        if not graph:
            out = fresh()
            enqueue(out)
            return out
        # graph mode: static input / output buffers per (ray count, scalar arguments); inputs are copied in unless they already live there.  The number of rounds
        # enqueued as launches (the tail launch stands for the rest) follows the frames before: a graph is captured per count -- two or three in a session
        planned = C.c_int(0)
        _lib.check(self._lib.mf_nerf_head_plan_rounds(self._head, int(max_steps), C.byref(planned)), "mf_nerf_head_plan_rounds")
        key = (N, ev, eye_dev is not None, bool(want_u8), bgc, bool(finish), None if bg is None else bg.numel(), float(dt_gamma), int(max_steps), float(T_thresh),
               None if aabb is None else aabb.data_ptr(), planned.value)
        hit = self._graphs.get(key)
        live = (rays_o, rays_d, ea, ic, bg, eye_dev)
        if hit is None:
            static = tuple(None if t is None else t.clone() for t in live)
            rays_o, rays_d, ea, ic, bg, eye_dev = static
            _lib.check(self._lib.mf_nerf_head_set_eye(self._head, p(eye_dev)), "mf_nerf_head_set_eye")
            out = fresh()
            _lib.check(self._lib.mf_nerf_head_set_rounds(self._head, planned.value), "mf_nerf_head_set_rounds")
            try:
                enqueue(out)                               # warm-up outside the capture
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    enqueue(out)
            finally:
                _lib.check(self._lib.mf_nerf_head_set_rounds(self._head, -1), "mf_nerf_head_set_rounds")
            hit = (g, out, static)
            self._graphs[key] = hit
        else:
            for dst, src in zip(hit[2], live):
                if dst is not None and dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
        hit[0].replay()
        return hit[1]

    # ---- several frames in one device loop (mf_nerf_head_batch_render) ----------------------------------------------------------------
    MAX_BATCH_FRAMES = 64               # the library's limit per call

    def _aabb_arg(self):
        """the box the device loops read: None for the built-in one from `bound`, else the rebound `aabb_infer` (checked)"""
        aabb = None if self.aabb_infer is self._aabb_default else self.aabb_infer
        if aabb is not None and not (torch.is_tensor(aabb) and aabb.is_cuda and aabb.dtype == torch.float32 and aabb.is_contiguous() and aabb.numel() == 6):
            raise RuntimeError("HipHeadRenderer: aabb_infer must be a contiguous float32 CUDA tensor of 6 values (there is no CPU path)")
        return aabb

    def _batch_handle(self, n_rays, n_frames):
        """the batch handle, created or grown (rays or frame slots) on demand"""
        if getattr(self, "_batch", None) is None or self._batch_cap[0] < n_rays or self._batch_cap[1] < n_frames:
            cap = (n_rays, n_frames)
            if getattr(self, "_batch", None):
                cap = (max(n_rays, self._batch_cap[0]), max(n_frames, self._batch_cap[1]))
                self._lib.mf_nerf_head_batch_destroy(self._batch)
                self._batch = None
            h = C.c_void_p()
            _lib.check(self._lib.mf_nerf_head_batch_create(self.field._h, cap[0], cap[1], C.byref(h)), "mf_nerf_head_batch_create")
            self._batch, self._batch_cap = h, cap
        return self._batch

    @torch.no_grad()
    def run_cuda_device_batch(self, frames, dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4, want_u8=False, finish=True, reserve_frames=0):
        """`run_cuda_device` for several frames of one ray count in ONE chain of launches: frames is a list of dicts (rays_o, rays_d, enc_a, eye, bg_color and
        optionally ind_code, default the renderer's); returns the list of the dicts run_cuda_device returns.  Every frame is the same bits as rendered alone.
        reserve_frames: frame slots the batch handle is created with when that is more than this call needs -- a caller that knows its largest call says so once,
        because growing the handle later frees and reallocates every slot (a synchronising free)."""
        F = len(frames)
        if not 1 <= F <= self.MAX_BATCH_FRAMES:
            raise RuntimeError(f"HipHeadRenderer.run_cuda_device_batch: {F} frames (1..{self.MAX_BATCH_FRAMES} per call)")
        p = lambda t: t.data_ptr() if t is not None else None
        descs = (_lib.MfNerfFrameDesc * F)()
        keep, outs, N = [], [], None
        for i, fr in enumerate(frames):
            rays_o, rays_d, ea, ic, eye_dev, ev, fresh = self._frame_args(fr["rays_o"], fr["rays_d"], fr["enc_a"], fr.get("ind_code", self.ind_code), fr.get("eye"), want_u8)
            if N is None:
                N = rays_o.shape[0]
            elif rays_o.shape[0] != N:
                raise RuntimeError(f"HipHeadRenderer.run_cuda_device_batch: frame {i} has {rays_o.shape[0]} rays, frame 0 has {N} (one ray count per call)")
            bg, per_ray, bgc = self._bg_args(fr.get("bg_color"), N)
            out = fresh()
            d = descs[i]
            d.rays_o, d.rays_d, d.enc_a, d.ind_code, d.eye_dev, d.eye = p(rays_o), p(rays_d), p(ea), p(ic), p(eye_dev), ev
            d.bg_color, d.bg_per_ray, d.bg_const = p(bg), (int(per_ray) if finish else -1), bgc
            d.image, d.depth, d.weights_sum, d.frame_u8 = p(out["image"]), p(out["depth"]), p(out["weights_sum"]), p(out["frame_u8"])
            keep.append((rays_o, rays_d, ea, ic, eye_dev, bg))         # what the descriptors point at lives until the call is enqueued
            outs.append(out)
        aabb = self._aabb_arg()
        h = self._batch_handle(N, max(F, min(int(reserve_frames), self.MAX_BATCH_FRAMES)))
        _lib.check(self._lib.mf_nerf_head_batch_render(h, descs, F, N, C.c_void_p(self.bitfield.data_ptr()), self.cascade, self.grid_size, self.min_near,
                                                       float(dt_gamma), int(max_steps), float(T_thresh), self.density_scale,
                                                       C.c_void_p(aabb.data_ptr()) if aabb is not None else None,
                                                       _lib.stream_ptr()), "mf_nerf_head_batch_render")
        del keep
        return outs

    def finish_device_batch(self, outs, bg_colors):
        """finish_device for the results of a run_cuda_device_batch(finish=False): frame i with bg_colors[i]"""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        for i, (out, bg_color) in enumerate(zip(outs, bg_colors)):
            N = out["image"].shape[0]
            bg, per_ray, bgc = self._bg_args(bg_color, N)
            _lib.check(self._lib.mf_nerf_head_batch_finish(self._batch, i, N, p(bg), int(per_ray), bgc, p(out["image"]), p(out["depth"]), p(out["weights_sum"]),
                                                           p(out["frame_u8"]), _lib.stream_ptr()), "mf_nerf_head_batch_finish")
        return outs

    FRAME_BATCH = True                  # render_frames takes torso_batch (nerf_serving.NerfBatcher asks before it passes it)

    @torch.no_grad()
    def render_frames(self, jobs, reserve_frames=0, torso_batch=False, **kw):
        """`render(..., loop="device")` for several frames with ONE head call: jobs is a list of dicts (rays_o, rays_d, auds, bg_coords, poses, eye, bg_color), kw
        the render keywords they share (dt_gamma, max_steps, T_thresh, want_u8).  Per frame and in order: audio window -> enc_a with the lip-smoothing EMA; then the
        batched head, left unfinished when there is a torso net; then per frame the torso and the finish.  Same kernels per frame, same bits.
        A job may carry `ema`, a one-element list: the EMA value its frame continues (installed before the frame's audio, written back after it), so that frames of
        several sessions -- each with its own lip-smoothing state -- share one call (nerf_serving.NerfBatcher).
        torso_batch: the frames' torso branches go out as one launch too (HipTorso.run_torso_batch: mf_nerf_torso_forward_batch), the same bits per frame."""
        frames = []
        for j in jobs:
            box = j.get("ema")
            if box is not None:
                self.enc_a = box[0]
            enc_a = self._audio_part(j["auds"])
            if box is not None:
                box[0] = self.enc_a
            frames.append(dict(rays_o=j["rays_o"], rays_d=j["rays_d"], enc_a=enc_a, eye=j.get("eye"), bg_color=j.get("bg_color")))
        if self.torso is None:
            return self.run_cuda_device_batch(frames, reserve_frames=reserve_frames, **kw)
        outs = self.run_cuda_device_batch(frames, finish=False, reserve_frames=reserve_frames, **kw)
        if torso_batch and os.environ.get("MF_TORSO") != "gemm":
            bgs = [t["bg_color"] for t in self.torso.run_torso_batch([(j["bg_coords"], j["poses"], j.get("bg_color")) for j in jobs])]
        else:
            bgs = [self.torso.run_torso(j["bg_coords"], j["poses"], j.get("bg_color"))["bg_color"] for j in jobs]
        return self.finish_device_batch(outs, bgs)

    GRID_SIZES = (32, 64, 128)          # what the grid-maintenance entry points serve (the reference always uses 128); the library's rule: mf_nerf_occupancy_shape

    @classmethod
    def check_grid_size(cls, grid_size, who):
        """The one statement of the served sizes on the Python side: head rebuild, torso rebuild and mark_untrained all ask here."""
        if grid_size not in cls.GRID_SIZES:
            raise RuntimeError(f"{who}: grid_size {grid_size} is not served (32, 64 or 128)")

    @torch.no_grad()
    def update_density_grid(self, density_grid, enc_a, eye=None, decay=0.95, density_thresh=10.0, noise=None, cascades=None, tmp_grid=None, xyzs_out=None):
        """The head branch of `NeRFRenderer.update_extra_state` (renderer.py:437-485) on the device, three launches and no host sync
        (mf_nerf_density_grid_update): the density field swept over the cascades x grid_size^3 cell centres, six-neighbour dilation, the
        masked EMA with `decay`, mean density, bit pack with min(mean, density_thresh) (opt.density_thresh, default 10).

        density_grid [cascades, grid_size^3] fp32 is updated in place and so is `self.bitfield` (same tensor, same data_ptr: a captured
        graph stays valid).  enc_a: [1, 32] / [32] device tensor; eye: the scalar eye feature (a host number or tensor; a device tensor
        is read back, which syncs) or None; noise: [cascades, grid_size^3, 3] uniform numbers in the reference's meshgrid order (what its
        `torch.rand_like` calls draw, :467), None samples the cell centres.  tmp_grid / xyzs_out: optional [cascades, grid_size^3] /
        [cascades, grid_size^3, 3] fp32 buffers that keep the sweep's raw values and positions (Morton order).
        Returns mean_density as a 0-d float64 device tensor."""
        H = self.grid_size
        self.check_grid_size(H, "HipHeadRenderer.update_density_grid")
        cascades = self.cascade if cascades is None else int(cascades)
        if not 1 <= cascades <= 8:
            raise RuntimeError(f"HipHeadRenderer.update_density_grid: cascades {cascades} outside 1..8")
        cells = cascades * H ** 3

        def dev_f32(t, name, numel):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise RuntimeError(f"HipHeadRenderer.update_density_grid: {name} must be a CUDA tensor (there is no CPU path)")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
                raise RuntimeError(f"HipHeadRenderer.update_density_grid: {name} must be contiguous float32 with {numel} elements "
                                   f"(got {t.dtype}, {tuple(t.shape)})")
            return t
        dev_f32(density_grid, "density_grid", cells)
        if not (torch.is_tensor(enc_a) and enc_a.is_cuda):
            raise RuntimeError("HipHeadRenderer.update_density_grid: enc_a must be a CUDA tensor (there is no CPU path)")
        if not self.bitfield.is_cuda or self.bitfield.dtype != torch.uint8 or self.bitfield.numel() != cells // 8:
            raise RuntimeError(f"HipHeadRenderer.update_density_grid: the bitfield must be a CUDA uint8 tensor of {cells // 8} bytes")
        dev = density_grid.device
        ea = dev_f32(enc_a.float().reshape(-1).contiguous(), "enc_a", 32)
        if noise is not None:
            dev_f32(noise, "noise", cells * 3)
        tmp_grid = torch.empty(cascades, H ** 3, device=dev) if tmp_grid is None else dev_f32(tmp_grid, "tmp_grid", cells)
        if xyzs_out is not None:
            dev_f32(xyzs_out, "xyzs_out", cells * 3)
        use_eye = eye is not None and self.field.exp_eye
        ev = float(eye.reshape(-1)[0]) if torch.is_tensor(eye) else (float(eye) if eye is not None else 0.0)
        mean = torch.empty((), dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.mf_nerf_density_grid_update(self.field._h, p(density_grid), p(self.bitfield), cascades, H, self.bound, p(ea), ev, int(use_eye),
                                                         self.density_scale, float(decay), float(density_thresh), p(noise), p(tmp_grid), p(xyzs_out), p(mean),
                                                         _lib.stream_ptr()), "mf_nerf_density_grid_update")
        return mean

    @torch.no_grad()
    def mark_untrained(self, density_grid, poses, intrinsic, cascades=None):
        """`NeRFRenderer.mark_untrained_grid` (renderer.py:356-416) as one launch (mf_nerf_mark_untrained): a cell of the Morton-ordered
        density_grid [cascades, grid_size^3] (CUDA fp32, in place) whose centre no camera sees inside its frustum, widened by a cell, becomes -1;
        every other cell keeps its bits.  poses: [B, 4, 4] camera-to-world CUDA fp32, B >= 1; intrinsic: (fx, fy, cx, cy)."""
        H = self.grid_size
        self.check_grid_size(H, "HipHeadRenderer.mark_untrained")
        cascades = self.cascade if cascades is None else int(cascades)
        if not 1 <= cascades <= 8:
            raise RuntimeError(f"HipHeadRenderer.mark_untrained: cascades {cascades} outside 1..8")
        cells = cascades * H ** 3
        if not (torch.is_tensor(density_grid) and density_grid.is_cuda and density_grid.dtype == torch.float32 and density_grid.is_contiguous()
                and density_grid.numel() == cells):
            raise RuntimeError(f"HipHeadRenderer.mark_untrained: density_grid must be a contiguous float32 CUDA tensor with {cells} elements (there is no CPU path)")
        if not (torch.is_tensor(poses) and poses.is_cuda and poses.dtype == torch.float32 and poses.dim() == 3 and tuple(poses.shape[1:]) == (4, 4)):
            raise RuntimeError("HipHeadRenderer.mark_untrained: poses must be a float32 CUDA tensor [B, 4, 4] (there is no CPU path)")
        if poses.shape[0] < 1:
            raise RuntimeError("HipHeadRenderer.mark_untrained: no poses: with none every cell would be marked untrained")
        poses = poses.contiguous()
        fx, fy, cx, cy = (float(v) for v in intrinsic)
        _lib.check(self._lib.mf_nerf_mark_untrained(C.c_void_p(poses.data_ptr()), int(poses.shape[0]), fx, fy, cx, cy, self.bound, cascades, H,
                                                    C.c_void_p(density_grid.data_ptr()), _lib.stream_ptr()),
                   "mf_nerf_mark_untrained")

    @torch.no_grad()
    def run_cuda(self, rays_o, rays_d, enc_a, ind_code, eye, bg_color=None, dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4, perturb=False,
                 want_u8=False):
        """rays_o / rays_d: [N, 3] (or [1, N, 3]) CUDA fp32.  Returns image [N, 3] in [0, 1], depth [N], the ambient / weight sums and,
        with want_u8, the uint8 frame of nerfreal.py:111."""
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N, dev = rays_o.shape[0], rays_o.device
        nears, fars = torch.empty(N, device=dev), torch.empty(N, device=dev)
        rm.near_far_from_aabb(rays_o, rays_d, self.aabb_infer, N, self.min_near, nears, fars)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        weights_sum, depth, image = z(N), z(N), z(N, 3)
        amb_aud_sum, amb_eye_sum, unc_sum = z(N), z(N), z(N)
        rays_alive = torch.arange(N, dtype=torch.int32, device=dev)
        rays_t = nears.clone()
        step = 0
        trace = []
        while step < max_steps:
            n_alive = rays_alive.shape[0]
            if n_alive <= 0:
                break
            n_step = max(min(N // n_alive, 8), 1)                                        # renderer.py:256
            M = n_alive * n_step
            xyzs, dirs, deltas = z(M, 3), z(M, 3), z(M, 2)                                # raymarching.py:383-385
            noises = torch.rand(n_alive, device=dev) if (perturb and step == 0) else z(n_alive)
            rm.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound, dt_gamma, max_steps, self.cascade, self.grid_size,
                          self.bitfield, nears, fars, xyzs, dirs, deltas, noises)
            sigmas, rgbs, amb_aud, amb_eye, unc = self.field.forward(xyzs, dirs, enc_a, ind_code, eye)
            if self.density_scale != 1.0:
                sigmas = self.density_scale * sigmas
            rm.composite_rays_triplane(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, amb_aud.view(-1), amb_eye.view(-1),
                                       unc.view(-1), weights_sum, depth, image, amb_aud_sum, amb_eye_sum, unc_sum)
            rays_alive = rays_alive[rays_alive >= 0]                                     # renderer.py:266
            trace.append((n_alive, n_step))
            step += n_step
        frame = torch.empty(N, 3, dtype=torch.uint8, device=dev) if want_u8 else None
        bg, per_ray, bgc = self._bg_args(bg_color, N)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.mf_nerf_finish(p(image), p(depth), p(weights_sum), p(nears), p(fars), p(bg), int(per_ray), bgc, N, p(frame), _lib.stream_ptr()),
                   "mf_nerf_finish")
        return {"image": image, "depth": depth, "ambient_aud": amb_aud_sum, "ambient_eye": amb_eye_sum, "uncertainty": unc_sum,
                "weights_sum": weights_sum, "frame_u8": frame, "trace": trace}
