"""The ER-NeRF torso branch on MI355X: `NeRFRenderer.run_torso` (ernerf/nerf_triplane/renderer.py:294-352) with
`NeRFNetwork.forward_torso` (network.py:166-201) underneath, backed by mf_nerf_torso_* of libmerefusion_hip.so.

    torso = HipTorso(model.state_dict(), torso_shrink=opt.torso_shrink, individual_dim=opt.ind_dim_torso)
    bg = torso.run_torso(bg_coords, poses, bg_color)["bg_color"]         # what run_cuda mixes the head over, renderer.py:272-275

Every pixel runs through the two small MLPs and the occupancy mask is applied in the final mix (no boolean-mask gather/scatter, no
host sync); the frequency-encoded wrapped anchors and the individual code are per-frame constants folded into first-layer biases.

The occupancy grid `density_grid_torso` is not copied: `run_torso` samples the device tensor it is handed for the frame (`self.density_grid`
by default), because the reference rebinds that attribute at every torso `update_extra_state` (renderer.py:527).  `update_density_grid`
is that update on the device (mf_nerf_torso_grid_update)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .field import grid_geometry
from .renderer import HipHeadRenderer


def freq_encode_host(x, degree):
    """FreqEncoder.forward (freq.py:66-78 -> kernel_freq, freqencoder.cu:30-58) for a handful of values, in float32 like the kernel: output c >= D is
    sin(x[c % D] * 2^(col // 2) + (col % 2) * pi / 2) with col = c // D - 1.  (Vectorised: this runs on the host once per frame.)"""
    x = np.asarray(x, np.float32).reshape(-1)
    D = x.shape[0]
    c = np.arange(D, D + 2 * D * degree)
    col, d = c // D - 1, c % D
    arg = np.ldexp(x[d], col // 2).astype(np.float32) + ((col % 2).astype(np.float32) * np.float32(np.float32(np.pi) / 2)).astype(np.float32)
    return np.concatenate([x, np.sin(arg.astype(np.float32), dtype=np.float32)])


def wrapped_anchor_code(anchor_points, poses, ind_code):
    """network.py:175-178: anchors through the inverse pose, perspective-divided, FreqEncoder(6, 3), then the individual code."""
    a = anchor_points.numpy() if torch.is_tensor(anchor_points) else np.asarray(anchor_points, np.float32)
    p = (poses.detach().float().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses, np.float32)).reshape(4, 4)
    w = torch.from_numpy(a)[None, ...] @ torch.from_numpy(p)[None].permute(0, 2, 1).inverse()          # (torch's own 4 x 4 inverse: the reference's arithmetic)
    w = (w[:, :, :2] / w[:, :, 3, None] / w[:, :, 2, None]).reshape(-1)
    enc = freq_encode_host(w.numpy(), 3)
    code = np.zeros(0, np.float32) if ind_code is None else (ind_code.numpy() if torch.is_tensor(ind_code) and not ind_code.is_cuda else torch.as_tensor(ind_code).detach().float().cpu().numpy()).reshape(-1)
    return np.concatenate([enc, code]).astype(np.float32)


class HipTorso:
    def __init__(self, state_dict, torso_shrink=0.8, individual_dim=8, density_thresh_torso=0.01, mean_density_torso=0.0, grid_size=128,
                 precision="bf16x3", max_pixels=512 * 512, device="cuda"):
        self.device = torch.device(device)
        _lib.init_device(self.device.index or 0)
        self._lib = _lib.lib()
        offsets, pls = grid_geometry(num_levels=16, base_resolution=16, log2_hashmap_size=16, desired_resolution=2048)   # network.py:158
        cfg = _lib.MfNerfTorsoConfig(torso_shrink=float(torso_shrink), num_levels=16, level_dim=2, base_resolution=16,
                                     log2_per_level_scale=float(np.log2(pls)), individual_dim=int(individual_dim), grid_size=int(grid_size))
        for i, o in enumerate(offsets):
            cfg.offsets[i] = int(o)
        keep = {k: v for k, v in state_dict.items() if k.startswith(("torso_deform_net.", "torso_net.", "torso_encoder.embeddings", "density_grid_torso"))}
        arr, self._keep = _lib.tensor_array(keep)
        self._h = C.c_void_p()
        _lib.check(self._lib.mf_nerf_torso_create(C.byref(cfg), arr, len(arr), _lib.PRECISIONS[precision], int(max_pixels), C.byref(self._h)),
                   "mf_nerf_torso_create")
        self.anchor_points = state_dict["anchor_points"].detach().float().cpu()
        codes = state_dict.get("individual_codes_torso")
        self.ind_code = codes[0].detach().float().cpu() if (codes is not None and individual_dim > 0) else None      # renderer.py:318-319
        self.thresh = float(min(density_thresh_torso, mean_density_torso))                                           # renderer.py:325
        self.grid_size = int(grid_size)
        # the grid the frames sample: the caller's own tensor when it already lives on the device (borrowed, never copied), an upload of it otherwise
        g = state_dict["density_grid_torso"].detach()
        self.density_grid = g if self._is_grid(g) else g.to(self.device, torch.float32).contiguous()

    def _is_grid(self, g):
        return torch.is_tensor(g) and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.numel() == self.grid_size ** 2

    def _grid(self, g, who):
        if not self._is_grid(g):
            raise RuntimeError(f"HipTorso.{who}: density_grid must be a contiguous float32 CUDA tensor with {self.grid_size ** 2} elements "
                               f"(got {getattr(g, 'dtype', type(g))}, {tuple(getattr(g, 'shape', ()))}, {getattr(g, 'device', None)}); there is no CPU path")
        return g

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.mf_nerf_torso_destroy(h)
            self._h = None
        fb = getattr(self, "_fb", None)
        if fb:
            self._lib.mf_nerf_frame_batch_destroy(fb)
            self._fb = None

    @torch.no_grad()
    def run_torso(self, bg_coords, poses, bg_color=None, density_grid=None):
        """bg_coords: [N, 2] (or [1, N, 2]) CUDA fp32 in [-1, 1]; poses: [1, 4, 4]; bg_color: [N, 3] / [3] tensor, scalar or None (= 1);
        density_grid: the [grid_size^2] CUDA fp32 occupancy grid this frame samples (renderer.py:326), None = self.density_grid."""
        if not (torch.is_tensor(bg_coords) and bg_coords.is_cuda):
            raise RuntimeError("HipTorso.run_torso: bg_coords must be a CUDA tensor (there is no CPU path)")
        xy = bg_coords.contiguous().view(-1, 2).float()
        N = xy.shape[0]
        consts = wrapped_anchor_code(self.anchor_points, poses, self.ind_code)
        cbuf = (C.c_float * len(consts))(*consts.tolist())
        out = torch.empty(N, 3, device=xy.device)
        alpha = torch.empty(N, device=xy.device)
        deform = torch.empty(N, 2, device=xy.device)
        bg = bg_color.float().contiguous() if torch.is_tensor(bg_color) else None
        per_ray = bg is not None and bg.numel() == 3 * N
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        grid = self._grid(self.density_grid if density_grid is None else density_grid, "run_torso")
        _lib.check(self._lib.mf_nerf_torso_set_grid(self._h, p(grid)), "mf_nerf_torso_set_grid")
        _lib.check(self._lib.mf_nerf_torso_forward(self._h, p(xy), cbuf, p(bg), int(per_ray), float(1.0 if bg_color is None else (0.0 if bg is not None else bg_color)),
                                                   self.thresh, N, p(out), p(alpha), p(deform), _lib.stream_ptr()),
                   "mf_nerf_torso_forward")
        return {"bg_color": out, "torso_alpha": alpha.view(N, 1), "deform": deform}

    MAX_BATCH_FRAMES = 64               # the library's limit per call

    @torch.no_grad()
    def run_torso_batch(self, frames, density_grid=None):
        """`run_torso` for several frames of one pixel count in ONE launch (mf_nerf_torso_forward_batch): frames is a list of (bg_coords, poses, bg_color) as
        run_torso takes them; returns the list of the dicts run_torso returns, each the same bits as run_torso gives for that frame alone.  The frame constants
        travel in the call's descriptor table.  All frames sample one grid."""
        F = len(frames)
        if not 1 <= F <= self.MAX_BATCH_FRAMES:
            raise RuntimeError(f"HipTorso.run_torso_batch: {F} frames (1..{self.MAX_BATCH_FRAMES} per call)")
        p = lambda t: t.data_ptr() if t is not None else None
        descs = (_lib.MfNerfTorsoDesc * F)()
        keep, outs, N = [], [], None
        for i, (bg_coords, poses, bg_color) in enumerate(frames):
            if not (torch.is_tensor(bg_coords) and bg_coords.is_cuda):
                raise RuntimeError("HipTorso.run_torso_batch: bg_coords must be a CUDA tensor (there is no CPU path)")
            xy = bg_coords.contiguous().view(-1, 2).float()
            if N is None:
                N = xy.shape[0]
            elif xy.shape[0] != N:
                raise RuntimeError(f"HipTorso.run_torso_batch: frame {i} has {xy.shape[0]} pixels, frame 0 has {N} (one pixel count per call)")
            consts = wrapped_anchor_code(self.anchor_points, poses, self.ind_code)
            out, alpha, deform = torch.empty(N, 3, device=xy.device), torch.empty(N, device=xy.device), torch.empty(N, 2, device=xy.device)
            bg = bg_color.float().contiguous() if torch.is_tensor(bg_color) else None
            d = descs[i]
            d.frame_consts[:len(consts)] = consts.tolist()
            d.bg_coords, d.bg_color, d.bg_per_ray = p(xy), p(bg), int(bg is not None and bg.numel() == 3 * N)
            d.bg_const, d.density_thresh = float(1.0 if bg_color is None else (0.0 if bg is not None else bg_color)), self.thresh
            d.bg_out, d.torso_alpha, d.deform = p(out), p(alpha), p(deform)
            keep.append((xy, bg))
            outs.append({"bg_color": out, "torso_alpha": alpha.view(N, 1), "deform": deform})
        fb = getattr(self, "_fb", None)
        if fb is None or self._fb_pixels < N:
            if fb:
                self._lib.mf_nerf_frame_batch_destroy(fb)
                self._fb = None
            fb = C.c_void_p()
            _lib.check(self._lib.mf_nerf_frame_batch_create(self.MAX_BATCH_FRAMES, N, C.byref(fb)), "mf_nerf_frame_batch_create")
            self._fb, self._fb_pixels = fb, N
        grid = self._grid(self.density_grid if density_grid is None else density_grid, "run_torso_batch")
        _lib.check(self._lib.mf_nerf_torso_set_grid(self._h, C.c_void_p(grid.data_ptr())), "mf_nerf_torso_set_grid")
        _lib.check(self._lib.mf_nerf_torso_forward_batch(self._h, fb, descs, F, N, _lib.stream_ptr()),
                   "mf_nerf_torso_forward_batch")
        del keep
        return outs

    @torch.no_grad()
    def update_density_grid(self, grid, poses, ind_code, noise, decay=0.95, raw_out=None, xys_out=None):
        """The torso branch of `NeRFRenderer.update_extra_state` (renderer.py:488-528) on the device, three launches and no host sync
        (mf_nerf_torso_grid_update): `forward_torso`'s alpha swept over the grid_size^2 jittered cell centres of :511-514, the 5 x 5 max pool,
        grid = max(grid * decay, pooled), the mean.

        grid: `density_grid_torso`, [grid_size^2] CUDA fp32, updated in place; it is also the grid later `run_torso` calls sample.  poses: the
        [1, 4, 4] pose of :494; ind_code: the [1, ind_dim_torso] row of :497 (None without a code); noise: [grid_size^2, 2] uniform numbers in
        the reference's meshgrid order (row x * grid_size + y: what its `torch.rand_like` draws, :514), None samples the cell centres.
        raw_out / xys_out: optional [grid_size^2] / [grid_size^2, 2] fp32 buffers that keep the sweep's raw alpha (row y * grid_size + x, as the
        grid) and its positions (meshgrid order).  Returns mean_density_torso as a 0-d float32 device tensor."""
        G = self.grid_size
        HipHeadRenderer.check_grid_size(G, "HipTorso.update_density_grid")
        self._grid(grid, "update_density_grid")

        def dev_f32(t, name, numel):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
                raise RuntimeError(f"HipTorso.update_density_grid: {name} must be a contiguous float32 CUDA tensor with {numel} elements")
            return t
        if noise is not None:
            dev_f32(noise, "noise", 2 * G * G)
        raw = torch.empty(G * G, device=grid.device) if raw_out is None else dev_f32(raw_out, "raw_out", G * G)
        if xys_out is not None:
            dev_f32(xys_out, "xys_out", 2 * G * G)
        code = ind_code if self.ind_code is not None else None
        if self.ind_code is not None and (code is None or torch.as_tensor(code).numel() != self.ind_code.numel()):
            raise RuntimeError(f"HipTorso.update_density_grid: ind_code must have {self.ind_code.numel()} elements (the torso nets were built with a code)")
        consts = wrapped_anchor_code(self.anchor_points, poses, code)
        cbuf = (C.c_float * len(consts))(*consts.tolist())
        mean = torch.empty((), dtype=torch.float32, device=grid.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self._lib.mf_nerf_torso_grid_update(self._h, cbuf, p(noise), float(decay), p(grid), p(raw), p(xys_out), p(mean),
                                                       _lib.stream_ptr()), "mf_nerf_torso_grid_update")
        self.density_grid = grid
        return mean
