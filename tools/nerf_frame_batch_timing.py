"""One NerfBatcher.step of 8 sessions x 4 frames with and without the frame-indexed launches around the head call (csrc/mf_nerf_frame_batch.hip), in one process
(MI355X), at 64 x 64 and at 512 x 512:

  (p)  frame_batch=False: one head call for the step's 32 frames, then mf_nerf_frame_background and mf_nerf_frame_out once per frame -- the launches the step
       made before the frame-indexed entry points existed
  (p') the same route on a second batcher: the same code twice, whose difference is the run-to-run spread a gain has to exceed
  (f)  frame_batch=True: ONE background launch, the head call, ONE frame-out launch

The three alternate repeat by repeat, so that they see the same machine.  Each repeat is timed twice over: hipEvents around the step (the device's view) and
the host clock from the call to the end of a device synchronise (what a serving loop waits for).  The sessions are head-only models with torso images, as
tools/nerf_sessions_timing.py builds them.  A second table times the torso branch of 32 frames alone: mf_nerf_torso_forward once per frame against ONE
mf_nerf_torso_forward_batch, same alternation.  Prints the tables and one JSON line.

    python tools/nerf_frame_batch_timing.py [--sessions 8] [--repeats 40] [--warmup 5] [--rays 64 512]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_sessions_timing as ST  # noqa: E402  (the scene: seeded field, audio net, sessions' inputs)

B, DIM, POSES, KW = ST.B, ST.DIM, ST.POSES, ST.KW


def alternating(steps, warmup, repeats):
    """the routes of `steps` repeat by repeat in turn -> per route {event: (median, min, max), wall: (median, min, max)} in ms"""
    with torch.no_grad():
        for _ in range(warmup):
            for step in steps:
                step()
        torch.cuda.synchronize()
        ev, wall = [[] for _ in steps], [[] for _ in steps]
        for _ in range(repeats):
            for i, step in enumerate(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize()
                wall[i].append((time.perf_counter() - t0) * 1e3)
                ev[i].append(e0.elapsed_time(e1))
    stat = lambda m: (round(statistics.median(m), 3), round(min(m), 3), round(max(m), 3))
    return [dict(event=stat(e), wall=stat(w)) for e, w in zip(ev, wall)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 512])
    args = ap.parse_args()

    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    from mere_fusion_amd.ernerf.torso import HipTorso
    from mere_fusion_amd.nerf_driver import NerfSession
    from mere_fusion_amd.nerf_serving import NerfBatcher

    offsets, _ = grid_geometry()
    fsd = W.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    fsd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in fsd.items()}
    g = torch.Generator().manual_seed(0)
    ind = (torch.randn(1, 4, generator=g) * 0.1).cuda()
    bitfield = torch.from_numpy(W.make_ernerf_sphere_bitfield()).cuda()
    asd = ST.audio_state_dict(W, DIM)
    N = args.sessions
    os.environ.pop("MF_NERF_BATCH", None)

    def sessions(S, rend):
        intr = np.array([S / 0.7, S / 0.7, S / 2, S / 2])
        out = []
        for s in range(N):
            gs = torch.Generator().manual_seed(100 + s)
            poses = torch.eye(4).repeat(POSES, 1, 1)
            poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2]) + 0.02 * torch.randn(POSES, 3, generator=gs)
            out.append(NerfSession(rend, poses.cuda(), intr, S, S, ST.ref_get_rays, eye_area=(torch.rand(POSES, 1, generator=gs) * 0.5).cuda(),
                                   bg=torch.rand(S, S, 3, generator=gs).cuda(), torso_imgs=torch.randint(0, 256, (POSES, S, S, 4), generator=gs, dtype=torch.uint8).cuda(),
                                   render_kw=KW))
        return out

    rows, torso_rows = [], []
    for S in args.rays:
        rend = HipHeadRenderer(HipNeRFField(fsd, max_samples=S * S), bitfield, density_scale=40.0, ind_code=ind, audio=HipAudioEncoder(asd, att=2), smooth_lips=True)
        auds = torch.randn(B, 8, DIM, 16, generator=torch.Generator().manual_seed(5)).cuda()
        inp = [(auds * (1.0 + 0.01 * k), [(0, 0)] * B) for k in range(N)]
        bats = [NerfBatcher(sessions(S, rend), frame_batch=fb) for fb in (False, False, True)]
        for bat in bats:
            bat.prewarm(auds[0])
        # the three routes give the same frames
        first = [[f.clone() for f, _ in bat.step(inp)] for bat in bats]
        assert all(torch.equal(a, b) for a, b in zip(first[0], first[2])) and all(torch.equal(a, b) for a, b in zip(first[0], first[1]))
        p, p2, f = alternating([lambda bat=bat: bat.step(inp) for bat in bats], args.warmup, args.repeats)
        rows.append(dict(rays=S, sessions=N, frames=N * B, per_frame=p, per_frame_again=p2, frame_batch=f,
                         spread_event_ms=round(abs(p["event"][0] - p2["event"][0]), 3), spread_wall_ms=round(abs(p["wall"][0] - p2["wall"][0]), 3),
                         gain_event_ms=round(min(p["event"][0], p2["event"][0]) - f["event"][0], 3), gain_wall_ms=round(min(p["wall"][0], p2["wall"][0]) - f["wall"][0], 3)))
        del bats, rend
        # ---- the torso branch of the step's frames alone
        toffs, _ = grid_geometry(num_levels=16, base_resolution=16, log2_hashmap_size=16, desired_resolution=2048)
        tsd = W.make_ernerf_torso_state_dict(int(toffs[-1]), 4, 8, 128)
        tsd["density_grid_torso"] = torch.full((128 * 128,), 0.5)
        torso = HipTorso(tsd, individual_dim=8, grid_size=128, max_pixels=S * S)
        torso.thresh = 0.01
        u = torch.linspace(-1, 1, S)
        xy = torch.stack(torch.meshgrid(u, u, indexing="xy"), -1).reshape(-1, 2).cuda().contiguous()
        pose = torch.eye(4)
        pose[2, 3] = 0.9
        frames = [(xy, pose[None], 1.0)] * (N * B)
        a, b = [t["bg_color"] for t in (torso.run_torso(*fr) for fr in frames)], [t["bg_color"] for t in torso.run_torso_batch(frames)]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        one, one2, bat = alternating([lambda: [torso.run_torso(*fr) for fr in frames], lambda: [torso.run_torso(*fr) for fr in frames], lambda: torso.run_torso_batch(frames)],
                                     args.warmup, args.repeats)
        torso_rows.append(dict(rays=S, frames=N * B, per_frame=one, per_frame_again=one2, batch=bat))
        del torso

    fmt = lambda t: f"{t[0]:>9.3f} [{t[1]:.3f}-{t[2]:.3f}]"
    for clock in ("event", "wall"):
        print(f"NerfBatcher.step, {clock} ms: median [min-max]")
        print(f"{'rays':>4} {'frames':>6} {'(p) per frame':>28} {'(p-again) the same again':>28} {'(f) frame batch':>28}")
        for r in rows:
            print(f"{r['rays']:>4} {r['frames']:>6} {fmt(r['per_frame'][clock]):>28} {fmt(r['per_frame_again'][clock]):>28} {fmt(r['frame_batch'][clock]):>28}")
    for clock in ("event", "wall"):
        print(f"torso of the step's frames alone, {clock} ms: median [min-max]")
        for r in torso_rows:
            print(f"{r['rays']:>4} {r['frames']:>6} {fmt(r['per_frame'][clock]):>28} {fmt(r['per_frame_again'][clock]):>28} {fmt(r['batch'][clock]):>28}")
    print(json.dumps(dict(tool="nerf_frame_batch_timing", batch=B, repeats=args.repeats, device=torch.cuda.get_device_name(0), rows=rows, torso_rows=torso_rows)))


if __name__ == "__main__":
    main()
