"""Times one ER-NeRF frame, 512 x 512 rays -> a 450 x 450 GUI frame, through two routes, in one run on one scene:

  session   NerfSession.step (get_rays, mf_nerf_frame_background, the device render loop, mf_nerf_frame_out) + ONE device -> host copy of the uint8 frame
  existing  the `whole_frame_loop` sequence of bench.py as nerfreal.py:70-127 runs it with the drop-in's utils: get_rays, collate's background as torch
            half ops (provider.py:323, preload 2), the same render, `TrainerMixin.test_gui_with_data` (resize launch, fp32 image + depth to pinned memory,
            one sync), `(image * 255).astype(np.uint8)` and, with a body frame, the channel reversal and slice assignment on the host

each without and with a 580 x 1080 body frame.  Seeded weights (the scene of bench.py's ER-NeRF leg, head only), one stream; every frame sits between two
events recorded on that stream -- the second after the frame's last host step, so host work counts -- warm-up first, then the median of 60 frames.
Both routes must give the same frame; the tool checks that before it times anything.

    python tools/nerf_session_timing.py
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from mere_fusion_amd import weights as W                        # noqa: E402
from mere_fusion_amd.ernerf import frontend as fe               # noqa: E402
from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry   # noqa: E402
from mere_fusion_amd.ernerf.renderer import HipHeadRenderer     # noqa: E402
from mere_fusion_amd.nerf_driver import NerfSession             # noqa: E402

S, GUI, FH, FW, X0, Y0, POSES = 512, 450, 1080, 580, 60, 40, 8
KW = dict(dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)


def ref_get_rays(poses, intrinsics, H, Wd, N=-1, patch_size=1, rect=None):
    """utils.py:274-336, whole-frame branch (restated as in bench.py: no reference checkout is needed to run the tool)"""
    device, B = poses.device, poses.shape[0]
    fx, fy, cx, cy = intrinsics
    i, j = torch.meshgrid(torch.linspace(0, Wd - 1, Wd, device=device), torch.linspace(0, H - 1, H, device=device), indexing="ij")
    i = i.t().reshape([1, H * Wd]).expand([B, H * Wd]) + 0.5
    j = j.t().reshape([1, H * Wd]).expand([B, H * Wd]) + 0.5
    inds = torch.arange(H * Wd, device=device).expand([B, H * Wd])
    zs = torch.ones_like(i)
    directions = torch.stack(((i - cx) / fx * zs, (j - cy) / fy * zs, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions @ poses[:, :3, :3].transpose(-1, -2)
    return {"i": i, "j": j, "inds": inds, "rays_o": poses[..., :3, 3][..., None, :].expand_as(rays_d), "rays_d": rays_d}


def median_ms(frame, warmup=10, runs=60):
    for k in range(warmup):
        frame(k)
    torch.cuda.synchronize()
    ts = []
    for k in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame(warmup + k)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    offsets, _ = grid_geometry()
    fsd = W.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    fsd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in fsd.items()}
    g = torch.Generator().manual_seed(0)
    enc_a, ind = torch.randn(1, 32, generator=g).cuda(), (torch.randn(1, 4, generator=g) * 0.1).cuda()
    rend = HipHeadRenderer(HipNeRFField(fsd, max_samples=S * S), torch.from_numpy(W.make_ernerf_sphere_bitfield()).cuda(), density_scale=40.0, ind_code=ind)
    poses = torch.eye(4).repeat(POSES, 1, 1)
    poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2]) + 0.02 * torch.randn(POSES, 3, generator=g)
    poses = poses.cuda()
    intr = np.array([S / 0.7, S / 0.7, S / 2, S / 2])
    eye = (torch.rand(POSES, 1, generator=g) * 0.5).cuda()
    torso = torch.randint(0, 256, (POSES, S, S, 4), generator=g, dtype=torch.uint8).cuda()
    bg = torch.rand(S, S, 3, generator=g).cuda()
    body = torch.randint(0, 256, (POSES, FH, FW, 3), generator=g, dtype=torch.uint8)
    torso_half, bg_half = (torso.float() / 255).half(), bg.half()          # provider.py:186, 198, 238: what preload 2 keeps on the device
    body_host = [b.numpy() for b in body]
    bg_coords = torch.zeros(1, S * S, 2, device="cuda")

    class _Model:
        def eval(self):
            pass

    class _Trainer(fe.TrainerMixin):
        def __init__(self):
            self.model, self.ema, self.fp16, self.opt = _Model(), None, True, argparse.Namespace(color_space="srgb")

        def test_step(self, data, perturb=False):
            o = rend.render(data["rays_o"], data["rays_d"], enc_a, bg_coords, data["poses"], data["eye"], bg_color=data["bg_color"], loop="device", **KW)
            return o["image"].reshape(-1, S, S, 3), o["depth"].reshape(-1, S, S)
    tr = _Trainer()

    def existing(k, with_body):
        mi = k % POSES
        pose = poses[mi:mi + 1]
        rays = fe.get_rays(ref_get_rays, pose, intr, S, S)
        t = torso_half[mi:mi + 1]
        bg_color = (t[..., :3] * t[..., 3:] + bg_half * (1 - t[..., 3:])).view(1, -1, 3)
        out = tr.test_gui_with_data({"rays_o": rays["rays_o"], "rays_d": rays["rays_d"], "poses": pose, "eye": eye[mi:mi + 1], "bg_color": bg_color}, GUI, GUI)
        image = (out["image"] * 255).astype(np.uint8)
        if not with_body:
            return image
        full = np.ascontiguousarray(body_host[mi][..., ::-1])
        full[Y0:Y0 + GUI, X0:X0 + GUI] = image
        return full

    sessions, pins = {}, {}
    for with_body in (False, True):
        sessions[with_body] = NerfSession(rend, poses, intr, S, S, ref_get_rays, eye_area=eye, bg=bg, torso_imgs=torso, preload=2,
                                          fullbody_frames=body.cuda() if with_body else None, fullbody_offset=(X0, Y0) if with_body else (0, 0),
                                          gui_size=(GUI, GUI), render_kw=KW)
        pins[with_body] = torch.empty((FH, FW, 3) if with_body else (GUI, GUI, 3), dtype=torch.uint8).pin_memory()

    def session(k, with_body):
        s = sessions[with_body]
        s.index = k % POSES                                      # the same pose walk as the existing route (no mirroring: the comparison is per frame)
        pins[with_body].copy_(s.step(enc_a), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return pins[with_body].numpy()

    print(f"device: {torch.cuda.get_device_name(0)}; {S} x {S} rays -> {GUI} x {GUI}, body frame {FW} x {FH}")
    for with_body in (False, True):
        same = all(np.array_equal(session(k, with_body), existing(k, with_body)) for k in range(3))
        a = median_ms(lambda k: session(k, with_body))
        b = median_ms(lambda k: existing(k, with_body))
        print(f"{'with' if with_body else 'without'} body frame: NerfSession.step + D2H {a:.3f} ms, existing sequence {b:.3f} ms per frame (medians of 60), "
              f"ratio {b / a:.2f}; same frame: {same}")


if __name__ == "__main__":
    main()
