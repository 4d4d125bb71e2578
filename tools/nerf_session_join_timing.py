"""What an ER-NeRF session's joining and leaving costs the sessions that are running (one MI355X, one process), written as a markdown report:

  (i)   the step of 8 running sessions x 4 frames (NerfEndToEndScheduler's stages: NerfFeaturePool.step + NerfBatcher.step, 64 x 64 rays, every session on one
        model object) right after a ninth session has joined through add_session, and right after it has left, against the same steps with no join and no
        leave: same build, alternating repeats; and the host time of add_session / remove_session themselves
  (ii)  NerfFeaturePool.join([k]) (one mf_nerf_feat_rows_load launch) against warm_up([k]) (28 run_steps on silence: two single-window net forwards)
  (iii) the alternative that exists without add_session: a NEW pool, batcher and scheduler with the ninth session, plus prewarm() and warm_up([k])

The net is XLSR-53 large with seeded weights (44 symbols), the head a seeded ER-NeRF field with its audio net, as in tools/nerf_sessions_timing.py.

    python tools/nerf_session_join_timing.py [--out profiles/nerf_session_join_timing.md] [--repeats 20] [--rays 64] [--commit <id>]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from nerf_sessions_timing import B, DIM, KW, POSES, audio_state_dict, ref_get_rays  # noqa: E402


def spread(v):
    return f"**{statistics.median(v):.3f}** ({min(v):.3f} – {max(v):.3f})"


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_session_join_timing.md"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--commit", default=None, help="what the report names as the commit (default: git rev-parse of this checkout)")
    args = ap.parse_args()

    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.asr import HipWav2Vec2ForCTC
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    from mere_fusion_amd.ernerf.field import HipNeRFField, grid_geometry
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    from mere_fusion_amd.nerf_driver import NerfSession
    from mere_fusion_amd.nerf_serving import NerfBatcher, NerfEndToEndScheduler, NerfFeaturePool

    N, S = 8, args.rays
    offsets, _ = grid_geometry()
    fsd = W.make_ernerf_field_state_dict(int(offsets[-1]), 0)
    fsd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in fsd.items()}
    ind = (torch.randn(1, 4, generator=torch.Generator().manual_seed(0)) * 0.1).cuda()
    bitfield = torch.from_numpy(W.make_ernerf_sphere_bitfield()).cuda()
    rend = HipHeadRenderer(HipNeRFField(fsd, max_samples=S * S), bitfield, density_scale=40.0, ind_code=ind, audio=HipAudioEncoder(audio_state_dict(W, DIM), att=2),
                           smooth_lips=True)
    cfg = W.WAV2VEC2_XLSR_LARGE
    net = HipWav2Vec2ForCTC(cfg, W.make_wav2vec2_state_dict(cfg, 0), max_windows=N + 1)
    intr = np.array([S / 0.7, S / 0.7, S / 2, S / 2])

    def session(s):
        gs = torch.Generator().manual_seed(100 + s)
        poses = torch.eye(4).repeat(POSES, 1, 1)
        poses[:, :3, 3] = torch.tensor([0.02, -0.01, -2.2]) + 0.02 * torch.randn(POSES, 3, generator=gs)
        return NerfSession(rend, poses.cuda(), intr, S, S, ref_get_rays, eye_area=(torch.rand(POSES, 1, generator=gs) * 0.5).cuda(), bg=torch.rand(S, S, 3, generator=gs).cuda(),
                           torso_imgs=torch.randint(0, 256, (POSES, S, S, 4), generator=gs, dtype=torch.uint8).cuda(), render_kw=KW)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    pcm = [[W.make_speech_like_wav(320, 1000 * s + i) for i in range(2 * B)] for s in range(N + 1)]

    # ---- (i) -----------------------------------------------------------------------------------------------------------------------------------------
    pool = NerfFeaturePool(N, net, DIM, max_sessions=N + 1)
    pool.warm_up()
    bat = NerfBatcher([session(s) for s in range(N)], pool=pool, max_sessions=N + 1, max_sessions_per_step=N)
    bat.prewarm()
    sch = NerfEndToEndScheduler(bat)
    ks = list(range(N))
    joiner = session(N)

    def step():
        for k in ks:
            sch.submit(k, pcm[k], 0.0)
        wins = {k: sch.queues[k].popleft()[1][0] for k in ks}
        return bat.step(sch._audio_stage(ks, wins, bat.device), only=ks)

    names = ["2 before", "1 before", "join, then step", "1 after join", "leave, then step", "1 after leave"]
    times = {True: {n: [] for n in names}, False: {n: [] for n in names}}
    join_ms, leave_ms = [], []
    with torch.no_grad():
        for _ in range(5):
            step()
        for rep in range(2 * args.repeats):
            event = rep % 2 == 0                                         # alternating: with the join and the leave, without
            for name in names:
                def one():
                    if event and name.startswith("join"):
                        t0 = time.perf_counter()
                        sch.add_session(joiner)
                        join_ms.append((time.perf_counter() - t0) * 1e3)
                    if event and name.startswith("leave"):
                        t0 = time.perf_counter()
                        sch.remove_session(N)
                        leave_ms.append((time.perf_counter() - t0) * 1e3)
                    step()
                times[event][name].append(wall(one)[0])
    sch.close()

    # ---- (ii) ----------------------------------------------------------------------------------------------------------------------------------------
    join_only, warm_only = [], []
    with torch.no_grad():
        for _ in range(3):
            pool.join([N]), pool.leave(N)
        for _ in range(args.repeats):
            join_only.append(wall(lambda: pool.join([N]))[0])
            warm_only.append(wall(lambda: pool.warm_up([N]))[0])
            pool.leave(N)

    # ---- (iii) ---------------------------------------------------------------------------------------------------------------------------------------
    nine = [session(s) for s in range(N + 1)]

    def rebuild():
        p = NerfFeaturePool(N + 1, net, DIM)
        b = NerfBatcher(nine, pool=p)
        return p, b, NerfEndToEndScheduler(b)

    with torch.no_grad():
        build_ms, (p9, b9, s9) = wall(rebuild)
        prewarm_ms, _ = wall(b9.prewarm)
        warm_ms, _ = wall(lambda: p9.warm_up([N]))
    s9.close()

    inside = {n: min(times[False][n]) <= statistics.median(times[True][n]) <= max(times[False][n]) for n in ("join, then step", "leave, then step")}
    verdict = "lies inside" if all(inside.values()) else "does NOT lie inside"
    lines = [
        "# ER-NeRF sessions that come and go: what a join and a leave cost the running sessions",
        "",
        f"One box, one run ({torch.cuda.get_device_name(0)}; commit {args.commit or commit_id()}; `tools/nerf_session_join_timing.py --repeats {args.repeats}`): {N} running "
        f"sessions x {B} frames at {S} x {S} rays on one model object, XLSR-53 large (seeded) behind the feature pool.  Host wall time around a synchronised step, "
        "median (min – max), ms.  Nobody had measured any of this before; nothing here is a target.",
        "",
        f"## (i) The step of the {N} running sessions around a join and a leave",
        "",
        f"`NerfFeaturePool(max_sessions={N + 1})`, `NerfBatcher(max_sessions={N + 1}, max_sessions_per_step={N})`; a step is `NerfFeaturePool.step` + `NerfBatcher.step(only=the {N})`. "
        f"Repeats alternate between a sequence with `add_session` / `remove_session` of a ninth session in front of the marked steps and the same sequence without "
        f"({args.repeats} each).",
        "",
        "| step | with the join / leave | without |",
        "|---|---|---|",
    ] + [f"| {n} | {spread(times[True][n])} | {spread(times[False][n])} |" for n in names] + [
        "",
        f"The median of the step right after a join / a leave {verdict} the run's spread (min – max) of the same step without one "
        f"(join: {'inside' if inside['join, then step'] else 'outside'}, leave: {'inside' if inside['leave, then step'] else 'outside'}).",
        "",
        f"`add_session` itself (checks, one `mf_nerf_feat_rows_load` enqueued, the slot): {spread(join_ms)} ms of host time; `remove_session`: {spread(leave_ms)} ms.",
        "",
        "## (ii) Bringing one pool row into the joined state",
        "",
        "| route | ms |",
        "|---|---|",
        f"| `pool.join([k])`: one launch from the snapshot row | {spread(join_only)} |",
        f"| `pool.warm_up([k])`: 28 `run_step`s on silence, two single-window net forwards | {spread(warm_only)} |",
        "",
        "## (iii) The alternative without `add_session`: new objects with the ninth session",
        "",
        f"A new `NerfFeaturePool`, `NerfBatcher` and `NerfEndToEndScheduler` over {N + 1} sessions: **{build_ms:.1f}** ms; `prewarm()`: **{prewarm_ms:.1f}** ms; "
        f"`warm_up([{N}])` for the newcomer: **{warm_ms:.1f}** ms (one sample each).  Every running session waits for all three.",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
