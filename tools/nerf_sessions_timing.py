"""One ER-NeRF step of N sessions x 4 frames, 64 x 64 rays (and one row at 512 x 512), three routes in one process (MI355X):

  (a) the sessions one after the other on one stream, each with its own NerfASRFrontend over a one-window wav2vec2 handle: per frame two run_steps (the
      third frame of each four runs the net), get_next_feat (torch.cat / permute / stack) and NerfSession.step
  (b) NerfEndToEndScheduler's stages over the same sessions: NerfFeaturePool.step (ONE net call for all N windows, one scatter, four window launches) and
      NerfBatcher.step with one NerfSession.step per frame (MF_NERF_BATCH=0), every session on one model object
  (c) the same as (b) with the render batched: the step's 4 N frames through one head call (mf_nerf_head_batch_render), MF_NERF_BATCH=1

All start from the same 8 PCM chunks per session and end with every session's uint8 frames on the device.  The net is XLSR-53 large with seeded weights (44
symbols), the head a seeded ER-NeRF field with its audio net.  hipEvents around the step, warm-up first, median of the repeats.  The audio stage of (b) is also
timed alone.  (b) and (c) run on the same batcher and alternate repeat by repeat, so that they see the same machine; the comparison that matters is (c) against
(b) of the same run.  Prints a table and one JSON line.

    python tools/nerf_sessions_timing.py [--sessions 1 4 8] [--repeats 30] [--warmup 5] [--rays 64] [--big-rays 512] [--big-sessions 8]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, DIM, POSES = 4, 44, 8
KW = dict(dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)


def ref_get_rays(poses, intrinsics, H, Wd, N=-1, patch_size=1, rect=None):
    """utils.py:274-336, whole-frame branch (restated as in bench.py: no reference checkout is needed to run the tool)"""
    device, n = poses.device, poses.shape[0]
    fx, fy, cx, cy = intrinsics
    i, j = torch.meshgrid(torch.linspace(0, Wd - 1, Wd, device=device), torch.linspace(0, H - 1, H, device=device), indexing="ij")
    i = i.t().reshape([1, H * Wd]).expand([n, H * Wd]) + 0.5
    j = j.t().reshape([1, H * Wd]).expand([n, H * Wd]) + 0.5
    inds = torch.arange(H * Wd, device=device).expand([n, H * Wd])
    zs = torch.ones_like(i)
    directions = torch.stack(((i - cx) / fx * zs, (j - cy) / fy * zs, zs), dim=-1)
    directions = directions / torch.norm(directions, dim=-1, keepdim=True)
    rays_d = directions @ poses[:, :3, :3].transpose(-1, -2)
    return {"i": i, "j": j, "inds": inds, "rays_o": poses[..., :3, 3][..., None, :].expand_as(rays_d), "rays_d": rays_d}


def audio_state_dict(W, in_dim):
    shapes = {"audio_net.encoder_conv.0": (32, in_dim, 3), "audio_net.encoder_conv.2": (32, 32, 3), "audio_net.encoder_conv.4": (64, 32, 3),
              "audio_net.encoder_conv.6": (64, 64, 3), "audio_net.encoder_fc1.0": (64, 64), "audio_net.encoder_fc1.2": (32, 64),
              "audio_att_net.attentionConvNet.0": (16, 32, 3), "audio_att_net.attentionConvNet.2": (8, 16, 3), "audio_att_net.attentionConvNet.4": (4, 8, 3),
              "audio_att_net.attentionConvNet.6": (2, 4, 3), "audio_att_net.attentionConvNet.8": (1, 2, 3), "audio_att_net.attentionNet.0": (8, 8)}
    template = {}
    for k, s in shapes.items():
        template[k + ".weight"], template[k + ".bias"] = torch.empty(s), torch.empty(s[0])
    return W.make_ernerf_audio_state_dict(template, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--big-rays", type=int, default=512, help="one more row at this frame size (0: none)")
    ap.add_argument("--big-sessions", type=int, default=8)
    args = ap.parse_args()

    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC, NerfASRFrontend
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    from mere_fusion_amd.nerf_driver import NerfSession
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfEndToEndScheduler, NerfFeaturePool

    offsets, _ = grid_geometry()
    fsd = W.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    fsd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in fsd.items()}
    g = torch.Generator().manual_seed(0)
    ind = (torch.randn(1, 4, generator=g) * 0.1).cuda()
    bitfield = torch.from_numpy(W.make_ernerf_sphere_bitfield()).cuda()
    asd = audio_state_dict(W, DIM)

    def renderer(S):
        return HipHeadRenderer(HipNeRFField(fsd, max_samples=S * S), bitfield, density_scale=40.0, ind_code=ind, audio=HipAudioEncoder(asd, att=2), smooth_lips=True)

    cfg = W.WAV2VEC2_XLSR_LARGE
    wsd = W.make_wav2vec2_state_dict(cfg, 0)
    single = HipWav2Vec2ForCTC(cfg, wsd, max_windows=1)
    batched = HipWav2Vec2ForCTC(cfg, wsd, max_windows=max(args.sessions + [args.big_sessions]))

    def sessions(N, S, rend):
        intr = np.array([S / 0.7, S / 0.7, S / 2, S / 2])
        out = []
        for s in range(N):
            gs = torch.Generator().manual_seed(100 + s)
            poses = torch.eye(4).repeat(POSES, 1, 1)
            poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2]) + 0.02 * torch.randn(POSES, 3, generator=gs)
            out.append(NerfSession(rend, poses.cuda(), intr, S, S, ref_get_rays, eye_area=(torch.rand(POSES, 1, generator=gs) * 0.5).cuda(),
                                   bg=torch.rand(S, S, 3, generator=gs).cuda(), torso_imgs=torch.randint(0, 256, (POSES, S, S, 4), generator=gs, dtype=torch.uint8).cuda(),
                                   render_kw=KW))
        return out

    def timed(step):
        with torch.no_grad():
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def timed_alternating(steps):
        """the routes of `steps` repeat by repeat in turn: (median, min, max) per route"""
        with torch.no_grad():
            for _ in range(args.warmup):
                for step in steps:
                    step()
            torch.cuda.synchronize()
            ms = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, step in enumerate(steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    e1.synchronize()
                    ms[i].append(e0.elapsed_time(e1))
        return [(statistics.median(m), min(m), max(m)) for m in ms]

    rows = []
    for S, N in [(args.rays, n) for n in args.sessions] + ([(args.big_rays, args.big_sessions)] if args.big_rays > 0 else []):
        rend = renderer(S)
        pcm = [[W.make_speech_like_wav(320, 1000 * s + i) for i in range(2 * B)] for s in range(N)]
        # route (a)
        sa = sessions(N, S, rend)
        fa = [NerfASRFrontend(single, audio_dim=DIM) for _ in range(N)]
        for f in fa:
            for _ in range(f.warm_up_steps):
                f.run_step()

        def step_a():
            out = []
            for s in range(N):
                for b in range(B):
                    fa[s].put_audio_frame(pcm[s][2 * b])
                    fa[s].put_audio_frame(pcm[s][2 * b + 1])
                    fa[s].run_step()
                    fa[s].run_step()
                    out.append(sa[s].step(fa[s].get_next_feat()))
            return out

        # route (b): the two stages NerfEndToEndScheduler.run_once runs between picking and the rings
        pool = NerfFeaturePool(N, batched, DIM)
        pool.warm_up()
        bat = NerfBatcher(sessions(N, S, rend), pool=pool)
        bat.prewarm()
        sch = NerfEndToEndScheduler(bat)
        ks = list(range(N))

        def queued():
            for k in ks:
                sch.submit(k, pcm[k], 0.0)
            return {k: sch.queues[k].popleft()[1][0] for k in ks}

        def step_b():
            os.environ["MF_NERF_BATCH"] = "0"
            return bat.step(sch._audio_stage(ks, queued(), bat.device), only=ks)

        def step_c():
            os.environ["MF_NERF_BATCH"] = "1"
            return bat.step(sch._audio_stage(ks, queued(), bat.device), only=ks)

        def audio_b():
            return pool.step(ks, pcm, B)

        a, (b, cc), c = timed(step_a), timed_alternating([step_b, step_c]), timed(audio_b)
        sch.close()
        os.environ.pop("MF_NERF_BATCH", None)
        rows.append(dict(rays=S, sessions=N, frames=N * B, c_ms=round(cc[0], 3), c_min=round(cc[1], 3), c_max=round(cc[2], 3), b_over_c=round(b[0] / cc[0], 2),
                         ms_per_frame_c=round(cc[0] / (N * B), 3), a_ms=round(a[0], 3), a_min=round(a[1], 3), a_max=round(a[2], 3), b_ms=round(b[0], 3), b_min=round(b[1], 3),
                         b_max=round(b[2], 3), b_audio_ms=round(c[0], 3), ratio=round(a[0] / b[0], 2), ms_per_frame_a=round(a[0] / (N * B), 3),
                         ms_per_frame_b=round(b[0] / (N * B), 3)))
    print(f"{'rays':>4} {'N':>2} {'frames':>6} {'(a) one by one ms':>26} {'(b) pooled ms':>26} {'(c) pooled, batched render ms':>30} {'audio of (b)':>13} {'a/b':>6} {'b/c':>6} "
          f"{'ms/frame b':>11} {'ms/frame c':>11}")
    for r in rows:
        print(f"{r['rays']:>4} {r['sessions']:>2} {r['frames']:>6} {r['a_ms']:>9.3f} [{r['a_min']:.3f}-{r['a_max']:.3f}] {r['b_ms']:>9.3f} [{r['b_min']:.3f}-{r['b_max']:.3f}] "
              f"{r['c_ms']:>13.3f} [{r['c_min']:.3f}-{r['c_max']:.3f}] {r['b_audio_ms']:>13.3f} {r['ratio']:>6.2f} {r['b_over_c']:>6.2f} {r['ms_per_frame_b']:>11.3f} "
              f"{r['ms_per_frame_c']:>11.3f}")
    print(json.dumps(dict(tool="nerf_sessions_timing", batch=B, repeats=args.repeats, device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
