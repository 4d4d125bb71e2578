"""`ernerf.nerf_triplane.network.NeRFNetwork` as app.py:17 imports it, with the inference branch of its render path on MI355X (VERDICT r05 missing #1).

The reference builds the model (`NeRFNetwork(opt)`, app.py:379), lets its `Trainer` load the checkpoint into it (utils.py `load_checkpoint` ->
`model.load_state_dict`), and then calls `model.render(...)` once per frame from `Trainer.test_gui_with_data` (utils.py:1190-1223 -> `test_step` :926-956).
None of those files change.  `HipRenderMixin` goes IN FRONT of the reference's class (`dropin/ernerf/nerf_triplane/network.py`):

    class NeRFNetwork(HipRenderMixin, <the reference's NeRFNetwork>): pass

so the object is the reference's module in every respect -- same parameters, state-dict keys, `opt`, training methods -- except that `run_cuda`
(renderer.py:158-291), when called the way inference calls it, runs as one enqueue of HIP kernels:

    encode_audio + the lip-smoothing EMA (network.py:222-237, renderer.py:187-194)   mf_audio_encoder_forward_smooth
    run_torso (renderer.py:294-352, network.py:166-201)                              mf_nerf_torso_forward
    near/far, <= max_steps rounds of march -> field -> composite, background mix     mf_nerf_head_render (round control on the device, no host sync)

The device objects are built from `self.state_dict()` at the first frame AFTER the checkpoint is in (and again after any later `load_state_dict` / `.to()` /
`.half()`), i.e. with the weights the reference would have used for that frame (an EMA shadow copied in by `test_gui_with_data` included).  Training mode,
camera optimisation at test time, `perturb`, a missing audio window or eye feature, CPU tensors: the reference's own `run_cuda` runs, over the extension
shims (`dropin/_raymarching_face.py` ...), exactly as before."""
import os
import random
import sys

import torch

from .. import _lib, placement


class _Results(dict):
    """`run_cuda`'s result dict.  `image` and `depth` are what `test_step` reads (utils.py:953-954); the three per-ray sums the reference also returns
    (renderer.py:286-288) are copied out of the head's buffers only if somebody asks for them -- before the next frame is rendered."""

    def __init__(self, owner, frame_id, prefix, n, slot=None, *a, **k):
        super().__init__(*a, **k)
        self._owner, self._frame_id, self._prefix, self._n, self._slot = owner, frame_id, prefix, n, slot      # slot: the frame's place in a render_frames batch

    def __missing__(self, key):
        if key not in ("ambient_aud", "ambient_eye", "uncertainty"):
            raise KeyError(key)
        o = self._owner
        if o._mf_frame_id != self._frame_id:
            raise KeyError(f"{key}: the sums of this frame are gone (a later frame has been rendered); read them before the next render()")
        dev = self["image"].device
        aa, ae, un = (torch.empty(self._n, device=dev) for _ in range(3))
        import ctypes as C
        ptrs = (C.c_void_p(aa.data_ptr()), C.c_void_p(ae.data_ptr()), C.c_void_p(un.data_ptr()), _lib.stream_ptr(dev))
        if self._slot is None:
            _lib.check(_lib.lib().mf_nerf_head_sums(o._mf["renderer"]._head, self._n, *ptrs), "mf_nerf_head_sums")
        else:
            _lib.check(_lib.lib().mf_nerf_head_batch_sums(o._mf["renderer"]._batch, self._slot, self._n, *ptrs), "mf_nerf_head_batch_sums")
        self["ambient_aud"], self["ambient_eye"], self["uncertainty"] = aa.view(*self._prefix), ae.view(*self._prefix), un
        return self[key]


class HipRenderMixin:
    _mf = None
    _mf_frame_id = 0
    mf_frames = 0                      # frames rendered by the device loop (tests assert the fast route ran)
    mf_grid_updates = 0                # occupancy grids rebuilt by the device route
    mf_torso_grid_updates = 0          # torso occupancy grids rebuilt by the device route
    mf_marks = 0                       # mark_untrained_grid calls served by the device route

    def __init__(self, *args, **kwargs):
        # on a multi-GPU node the process takes its GPU here, before the reference's Trainer says `.to('cuda')` (placement.py)
        placement.charge_session(self)
        super().__init__(*args, **kwargs)

    # ---- anything that changes the weights (or where they live) drops the device objects ------------------------------------------
    def _mf_drop(self):
        self.__dict__["_mf"] = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._mf_drop()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._mf_drop()
        return out

    def _mf_build(self, n_rays, device):
        from .audio import HipAudioEncoder
        from .field import HipNeRFField
        from .renderer import HipHeadRenderer
        from .torso import HipTorso
        opt = self.opt
        with torch.no_grad():
            sd = {k: v.detach() for k, v in self.state_dict().items()}
        cap = max(int(n_rays), 1)
        field = HipNeRFField(sd, bound=self.bound, individual_dim=self.individual_dim, exp_eye=self.exp_eye, max_samples=cap, device=device)
        torso = None
        if self.torso:
            torso = HipTorso(sd, torso_shrink=getattr(opt, "torso_shrink", 0.8), individual_dim=self.individual_dim_torso,
                             density_thresh_torso=self.density_thresh_torso, mean_density_torso=self.mean_density_torso, grid_size=self.grid_size,
                             max_pixels=cap, device=device)
        audio = None if self.emb else HipAudioEncoder(sd, att=self.att, device=device)
        rend = HipHeadRenderer(field, self.density_bitfield, bound=self.bound, min_near=self.min_near, density_scale=self.density_scale,
                               grid_size=self.grid_size, torso=torso, audio=audio, ind_code=None, smooth_lips=self.smooth_lips)
        self.__dict__["_mf"] = {"renderer": rend, "cap": cap, "device": device, "bitfield_ptr": self.density_bitfield.data_ptr()}
        return self._mf

    def _mf_fast_path(self, rays_o, auds, eye, perturb):
        if os.environ.get("MF_NERF_DROPIN", "1") == "0" or self.training or perturb:
            return False
        if self.train_camera and self.test_train:                     # renderer.py:170-175: a per-index camera offset, training-time machinery
            return False
        if auds is None or (self.exp_eye and eye is None):             # the reference's own error / None handling applies
            return False
        return True

    def run_cuda(self, rays_o, rays_d, auds, bg_coords, poses, eye=None, index=0, dt_gamma=0, bg_color=None, perturb=False, force_all_rays=False,
                 max_steps=1024, T_thresh=1e-4, **kwargs):
        if not self._mf_fast_path(rays_o, auds, eye, perturb):
            return super().run_cuda(rays_o, rays_d, auds, bg_coords, poses, eye=eye, index=index, dt_gamma=dt_gamma, bg_color=bg_color, perturb=perturb,
                                    force_all_rays=force_all_rays, max_steps=max_steps, T_thresh=T_thresh, **kwargs)
        if not (torch.is_tensor(rays_o) and rays_o.is_cuda):
            raise RuntimeError("NeRFNetwork.run_cuda (MI355X drop-in): rays must be HIP device tensors; there is no CPU path (MF_NERF_DROPIN=0 runs the "
                               "reference's loop over the extension shims, which need a device too)")
        prefix = rays_o.shape[:-1]
        n = int(prefix.numel())
        r = self._mf_refresh(n, rays_o.device)
        with torch.no_grad():
            auds_in = self._mf_audio_in(r, auds)
            out = r.render(rays_o, rays_d, auds_in, bg_coords, poses, eye, bg_color=bg_color, loop="device", dt_gamma=float(dt_gamma),
                           max_steps=int(max_steps), T_thresh=float(T_thresh))
            if self.smooth_lips and not self.emb:
                self.enc_a = r.enc_a                                    # the EMA state lives where the reference keeps it (renderer.py:128-129, 190-194)
        self.__dict__["_mf_frame_id"] = self._mf_frame_id + 1
        self.__dict__["mf_frames"] = self.mf_frames + 1
        return self._mf_results(out, prefix, n)

    def _mf_results(self, out, prefix, n, slot=None):
        res = _Results(self, self._mf_frame_id, prefix, n, slot)
        res["depth"] = out["depth"].view(*prefix)
        res["image"] = out["image"].view(*prefix, 3)
        res["weights_sum"] = out["weights_sum"]
        return res

    def _mf_audio_in(self, r, auds):
        """what the renderer takes as one frame's `auds`, and who applies the lip-smoothing EMA to it (the state is `self.enc_a` either way)"""
        if self.emb:                                                # network.py:229-230: an embedding lookup in front of the audio net -- the reference's modules run it
            enc_a = super().encode_audio(auds)
            if enc_a is not None and self.smooth_lips:
                if self.enc_a is not None:
                    enc_a = 0.35 * self.enc_a + (1 - 0.35) * enc_a
                self.enc_a = enc_a
            r.smooth_lips = False
            return enc_a
        r.smooth_lips = bool(self.smooth_lips)
        r.enc_a = self.enc_a if self.smooth_lips else None
        return auds

    FRAME_BATCH = True                 # render_frames takes torso_batch (nerf_serving.NerfBatcher asks before it passes it)

    def render_frames(self, jobs, dt_gamma=0, max_steps=1024, T_thresh=1e-4, reserve_frames=0, torso_batch=False, **kwargs):
        """`run_cuda` for several frames of one ray count with ONE head call (HipHeadRenderer.render_frames): jobs is a list of dicts (rays_o, rays_d, auds,
        bg_coords, poses, eye, bg_color).  The per-frame refreshes of run_cuda happen once for the group; the audio windows, the EMA and the torso are taken per
        frame, in order.  Returns one result dict per frame, each the same bits as run_cuda gives for that frame alone.  Frames the device loop does not serve
        (see _mf_fast_path) go through run_cuda one by one.  reserve_frames: see HipHeadRenderer.run_cuda_device_batch; torso_batch: see HipHeadRenderer.render_frames."""
        kw = dict(dt_gamma=dt_gamma, max_steps=max_steps, T_thresh=T_thresh)
        if not jobs:
            return []
        if not all(self._mf_fast_path(j["rays_o"], j["auds"], j.get("eye"), False) and torch.is_tensor(j["rays_o"]) and j["rays_o"].is_cuda for j in jobs):
            outs = []
            for j in jobs:
                box = j.get("ema")
                if box is not None:
                    self.enc_a = box[0]
                outs.append(self.run_cuda(j["rays_o"], j["rays_d"], j["auds"], j["bg_coords"], j["poses"], eye=j.get("eye"), bg_color=j.get("bg_color"), **kw))
                if box is not None:
                    box[0] = self.enc_a
            return outs
        prefix = jobs[0]["rays_o"].shape[:-1]
        n = int(prefix.numel())
        r = self._mf_refresh(n, jobs[0]["rays_o"].device)
        with torch.no_grad():
            if self.emb:
                feed = []
                for j in jobs:                                          # (`ema`: see HipHeadRenderer.render_frames; here the state is the module's own)
                    box = j.get("ema")
                    if box is not None:
                        self.enc_a = box[0]
                    feed.append(dict(j, auds=self._mf_audio_in(r, j["auds"]), ema=None))
                    if box is not None:
                        box[0] = self.enc_a
            else:
                self._mf_audio_in(r, None)                              # the renderer applies the EMA frame by frame from the module's state
                feed = jobs
            outs = r.render_frames(feed, reserve_frames=reserve_frames, torso_batch=torso_batch, dt_gamma=float(dt_gamma), max_steps=int(max_steps), T_thresh=float(T_thresh))
            if self.smooth_lips and not self.emb:
                self.enc_a = r.enc_a
        self.__dict__["_mf_frame_id"] = self._mf_frame_id + 1
        self.__dict__["mf_frames"] = self.mf_frames + len(jobs)
        return [self._mf_results(out, prefix, n, slot=i) for i, out in enumerate(outs)]

    def _mf_refresh(self, n, dev):
        """the device objects for n rays on dev, with the per-frame attributes the reference reads at call time handed over; returns the renderer"""
        st = self._mf
        if st is None or st["cap"] < n or st["device"] != dev or st["bitfield_ptr"] != self.density_bitfield.data_ptr():
            st = self._mf_build(n, dev)
        r = st["renderer"]
        # per-frame attributes the reference reads at call time (renderer.py:197-202, 259, 325): they may have been set after construction (`load_checkpoint`
        # assigns mean_density_torso, the GUI density_scale)
        r.bitfield, r.density_scale = self.density_bitfield, float(self.density_scale)
        r.ind_code = self.individual_codes[0].detach() if self.individual_dim > 0 else None
        # the box of near / far is a persistent buffer a checkpoint may carry (renderer.py:86-89, read at :226): the head reads the module's own tensor
        ab = getattr(self, "aabb_infer", None)
        if torch.is_tensor(ab):
            ab = ab.detach()
            if not (ab.dtype == torch.float32 and ab.device == dev and ab.is_contiguous()):
                # (a `.half()`ed module, a host buffer) the values of the frame go into ONE fp32 copy kept with the device objects: its address does not change from
                # frame to frame, so a captured graph keyed on it stays one graph
                if st.get("aabb") is None:
                    st["aabb"] = torch.empty(6, dtype=torch.float32, device=dev)
                st["aabb"].copy_(ab.reshape(6))
                ab = st["aabb"]
            r.aabb_infer = ab
        if r.torso is not None:
            r.torso.thresh = float(min(self.density_thresh_torso, self.mean_density_torso))
            # the grid too: the reference's torso update rebinds `self.density_grid_torso` (renderer.py:527), so the frame samples the tensor of the frame.  A module
            # that carries the grid only in its state dict keeps the one the torso was built from
            g = getattr(self, "density_grid_torso", None)
            if torch.is_tensor(g):
                r.torso.density_grid = g if r.torso._is_grid(g) else g.detach().to(dev, torch.float32).contiguous()
        return r


    # ---- occupancy-grid maintenance (renderer.py:355-539) ---------------------------------------------------------------------------
    def _mf_sizes_served(self):
        from .renderer import HipHeadRenderer
        return self.grid_size in HipHeadRenderer.GRID_SIZES and 1 <= self.cascade <= 8      # (the library checks the same rule: mf_nerf_occupancy_shape)

    def _mf_grid_fast_path(self):
        if os.environ.get("MF_NERF_DROPIN", "1") == "0" or not self.cuda_ray or not self._mf_sizes_served():
            return False
        if not (torch.is_tensor(self.density_grid) and self.density_grid.is_cuda and self.density_bitfield.is_cuda):
            return False
        # what the two rebuilds do not serve goes the reference's way too: a field / torso without the fused kernel
        if self.torso:
            g = getattr(self, "density_grid_torso", None)
            return os.environ.get("MF_TORSO") != "gemm" and torch.is_tensor(g) and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()
        return os.environ.get("MF_NERF_FIELD") != "gemm"

    def _mf_state(self, dev):
        st = self._mf
        if st is None or st["device"] != dev or st["bitfield_ptr"] != self.density_bitfield.data_ptr():
            st = self._mf_build(st["cap"] if st is not None else 1, dev)
        return st

    def mark_untrained_grid(self, poses, intrinsic, S=64):
        """`NeRFRenderer.mark_untrained_grid` (renderer.py:356-416) as one launch (mf_nerf_mark_untrained) instead of the reference's five nested loops of batched
        matmuls: cells no training camera sees become -1 in `self.density_grid`, in place.  Another grid size, CPU tensors, MF_NERF_DROPIN=0: the reference's method."""
        if not self.cuda_ray:
            return
        import numpy as np
        from .renderer import HipHeadRenderer
        served = (os.environ.get("MF_NERF_DROPIN", "1") != "0" and self._mf_sizes_served() and torch.is_tensor(self.density_grid) and self.density_grid.is_cuda
                  and self.density_grid.dtype == torch.float32 and self.density_grid.is_contiguous())
        if not served:
            return super().mark_untrained_grid(poses, intrinsic, S=S)
        if isinstance(poses, np.ndarray):
            poses = torch.from_numpy(poses)
        with torch.no_grad():
            dev = self.density_grid.device
            # (no device objects are needed: the renderer is a holder of bound / grid_size here, as cheap as the call)
            r = HipHeadRenderer(None, self.density_bitfield, bound=self.bound, grid_size=self.grid_size)
            r.mark_untrained(self.density_grid, poses.to(dev, torch.float32), intrinsic, cascades=self.cascade)
        self.__dict__["mf_marks"] = self.mf_marks + 1

    def update_extra_state(self, decay=0.95, S=128):
        """`NeRFRenderer.update_extra_state` with the grid rebuilt on the device: the head grid (mf_nerf_density_grid_update: sweep, dilate + EMA, reduce + pack) or,
        for a torso model, the torso grid (mf_nerf_torso_grid_update: sweep, 5 x 5 dilate + EMA, mean) -- three kernels each, after the jitter's `torch.rand` draws.
        The selection statements are the reference's own and consume the same Python / torch random streams, so both routes rebuild from the same audio window, eye
        value, pose, code row and jitter.  CPU tensors, another grid size, MF_TORSO=gemm / MF_NERF_FIELD=gemm, MF_NERF_DROPIN=0: the reference's method runs, over
        the extension shims (`morton3D`, `morton3D_dilation`, `packbits`)."""
        if not self.cuda_ray:
            return
        if not self._mf_grid_fast_path():
            return super().update_extra_state(decay=decay, S=S)
        dev = self.density_bitfield.device
        # the reference's helper (ernerf/nerf_triplane/utils.py:43), as the module that defines the method this one stands in front of imported it (renderer.py:11)
        mro = type(self).__mro__
        owner = next(c for c in mro[mro.index(HipRenderMixin) + 1:] if "update_extra_state" in vars(c))
        get_audio_features = getattr(sys.modules[owner.__module__], "get_audio_features")
        H, Cn = self.grid_size, self.cascade
        steps = [(i, min(i + S, H)) for i in range(0, H, S)]
        with torch.no_grad():
            rand_idx = random.randint(0, self.aud_features.shape[0] - 1)                              # renderer.py:428-432
            auds = get_audio_features(self.aud_features, self.att, rand_idx).to(dev)
            enc_a = self.encode_audio(auds)
            if self.torso:
                rand_idx = random.randint(0, self.poses.shape[0] - 1)                                 # :492-499
                pose = self.poses[[rand_idx]]
                ind_code = self.individual_codes_torso[[rand_idx]].detach() if self.opt.ind_dim_torso > 0 else None
                # the jitter of :514, drawn block by block as the reference's two loops draw it
                noise = torch.empty(H, H, 2, device=dev)
                if len(steps) == 1:                                                                   # S >= grid_size (the reference's default): one draw, in place
                    torch.rand(H ** 2, 2, out=noise.view(H ** 2, 2))
                else:
                    for x0, x1 in steps:
                        for y0, y1 in steps:
                            noise[x0:x1, y0:y1] = torch.rand((x1 - x0) * (y1 - y0), 2, device=dev).view(x1 - x0, y1 - y0, 2)
                torso = self._mf_state(dev)["renderer"].torso
                mean = torso.update_density_grid(self.density_grid_torso, pose, ind_code, noise.view(H ** 2, 2), decay=decay)
            else:
                eye = float(self.eye_area[[rand_idx]].reshape(-1)[0]) if self.exp_eye else None       # :440-443 (eye_area lives on the host)
                # the jitter of :467, drawn block by block and cascade by cascade as the reference's loops draw it
                noise = torch.empty(Cn, H, H, H, 3, device=dev)
                if len(steps) == 1:                                                                   # S >= grid_size (the reference's default): one draw per cascade, in place
                    for cas in range(Cn):
                        torch.rand(H ** 3, 3, out=noise[cas].view(H ** 3, 3))
                else:
                    for x0, x1 in steps:
                        for y0, y1 in steps:
                            for z0, z1 in steps:
                                for cas in range(Cn):
                                    noise[cas, x0:x1, y0:y1, z0:z1] = torch.rand((x1 - x0) * (y1 - y0) * (z1 - z0), 3, device=dev).view(x1 - x0, y1 - y0, z1 - z0, 3)
                r = self._mf_state(dev)["renderer"]
                r.bitfield, r.density_scale = self.density_bitfield, float(self.density_scale)
                mean = r.update_density_grid(self.density_grid, enc_a, eye=eye, decay=decay, density_thresh=float(self.density_thresh), noise=noise.view(Cn, H ** 3, 3),
                                             cascades=Cn)
        if self.torso:
            self.mean_density_torso = mean.item()                                                     # :528, the one sync the reference has too
            self.__dict__["mf_torso_grid_updates"] = self.mf_torso_grid_updates + 1
        else:
            self.mean_density = mean.item()                                                           # :480, the one sync the reference has too
            self.iter_density += 1
            self.__dict__["mf_grid_updates"] = self.mf_grid_updates + 1
        total_step = min(16, self.local_step)                                                         # :533-537
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0


def load_reference_module(shadow_name, shadow_file, package):
    """The module the drop-in shadows, loaded from the NEXT directory of its package path under a private name, with the package set so that its relative
    imports (`from .renderer import NeRFRenderer`, `from ..encoding import get_encoder`) resolve through the same (extended) package."""
    import importlib
    import importlib.util
    import sys
    pkg = importlib.import_module(package)
    base = os.path.basename(shadow_file)
    for d in pkg.__path__:
        f = os.path.join(d, base)
        if os.path.exists(f) and os.path.abspath(f) != os.path.abspath(shadow_file):
            name = package + "._reference_" + os.path.splitext(base)[0]
            if name in sys.modules:
                return sys.modules[name]
            spec = importlib.util.spec_from_file_location(name, f)
            mod = importlib.util.module_from_spec(spec)
            mod.__package__ = package
            sys.modules[name] = mod
            try:
                spec.loader.exec_module(mod)
            except BaseException:
                sys.modules.pop(name, None)
                raise
            return mod
    raise ImportError(f"{shadow_name}: the reference's own {package.replace('.', '/')}/{base} was not found behind the drop-in -- put the mere-fusion checkout on "
                      "PYTHONPATH after mere-fusion_amd/dropin (INTEGRATION.md section 5)")
