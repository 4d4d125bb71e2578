"""What a session's joining and leaving costs the sessions that are running (Wav2Lip, one MI355X, one process), written as a markdown report:

  (i)   the step latency of 8 running sessions x B frames in the steps around a join and around a leave (LipBatcher(max_sessions=): add_session /
        remove_session between two steps), against the same steps with no join, same build, alternating repeats
  (ii)  a window push for 8 of 16 sessions: LipWindowPool.push + rows as they stand (index tensor, cat, indexed assignment, gather) against the pool built with
        max_sessions= (pinned staging block, one mf_windows_push launch)
  (iii) the alternative that exists without add_session: a NEW LipBatcher with one session more, and its prewarm()

    python tools/session_join_timing.py [--out profiles/session_join_timing.md] [--repeats 20] [--batch 16] [--frame 480 640]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(v):
    return f"**{statistics.median(v):.3f}** ({min(v):.3f} – {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_join_timing.md"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--frame", type=int, nargs=2, default=[480, 640], help="full frame H W")
    ap.add_argument("--faces", type=int, default=40, help="cached crops per session")
    args = ap.parse_args()

    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.paste import AvatarFrames
    from mere_fusion_amd.wav2lip.models import Wav2Lip

    B, (H, Wd), N = args.batch, args.frame, 8
    m = Wav2Lip(precision="bf16x3")
    m.load_state_dict(W.make_wav2lip_state_dict(0))
    m = m.to("cuda").eval()

    def session(s):
        r = np.random.default_rng(100 + s)
        n = args.faces
        boxes = [(H // 4 + i % 7, H // 4 + 200 + i % 5, Wd // 4 + i % 3, Wd // 4 + 180 + i % 9) for i in range(n)]           # (y1, y2, x1, x2)
        av = AvatarFrames(r.integers(0, 256, (n, H, Wd, 3), dtype=np.uint8), boxes, lip_order=True)
        return D.LipSession(m, r.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8), avatar_frames=av)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # ---- (i) -----------------------------------------------------------------------------------------------------------------------------------------
    bat = D.LipBatcher(m, [session(s) for s in range(N)], batch_size=B, paste=True, max_sessions=N + 1, pool_rows=(N + 1) * args.faces, max_sessions_per_step=N)
    bat.prewarm()
    pool = bat.frontends()[0].pool
    ks = list(range(N))
    pcm = [[W.make_speech_like_wav(320, 1000 * s + i) for i in range(2 * B)] for s in ks]
    joiner = session(N)

    def step():
        win = pool.push(ks, [pool.host_block(pcm[s]) for s in ks])
        mel = pool.mel(win)
        return bat.step([mel[s * B:(s + 1) * B] for s in ks] + [None], only=ks)

    with torch.no_grad():
        for _ in range(5):
            step()
        names = ["2 before", "1 before", "join, then step", "1 after join", "leave, then step", "1 after leave"]
        times = {True: {n: [] for n in names}, False: {n: [] for n in names}}
        join_ms, leave_ms = [], []
        for rep in range(2 * args.repeats):
            event = rep % 2 == 0                                         # alternating: with the join and the leave, without
            for name in names:
                def one():
                    if event and name.startswith("join"):
                        t0 = time.perf_counter()
                        bat.add_session(joiner)
                        join_ms.append((time.perf_counter() - t0) * 1e3)
                    if event and name.startswith("leave"):
                        t0 = time.perf_counter()
                        bat.remove_session(N)
                        leave_ms.append((time.perf_counter() - t0) * 1e3)
                    step()
                times[event][name].append(wall(one)[0])

    # ---- (ii) ----------------------------------------------------------------------------------------------------------------------------------------
    sub = [1, 2, 5, 7, 8, 11, 12, 15]
    static, dynamic = D.LipWindowPool(16, B), D.LipWindowPool(16, B, max_sessions=16)
    blocks = [static.host_block(pcm[i]) for i in range(8)]
    routes = {"today's route: `push` + `rows` (index tensor, `cat`, indexed assignment, gather)": lambda: (static.push(sub, blocks), static.rows(sub))[1],
              "`max_sessions=`: pinned staging block + one `mf_windows_push`": lambda: dynamic.push(sub, blocks)}
    push_ms = {k: [] for k in routes}
    for _ in range(5):
        for fn in routes.values():
            fn()
    for _ in range(3 * args.repeats):
        for k, fn in routes.items():
            push_ms[k].append(wall(fn)[0])
    assert torch.equal(static.buf, dynamic.buf)

    # ---- (iii) ---------------------------------------------------------------------------------------------------------------------------------------
    nine = [session(s) for s in range(N + 1)]
    build_ms, nb = wall(lambda: D.LipBatcher(m, nine, batch_size=B, paste=True))
    prewarm_ms, _ = wall(nb.prewarm)

    lines = [
        "# Sessions that come and go: what a join and a leave cost the running sessions",
        "",
        f"One box, one run ({torch.cuda.get_device_name(0)}; `tools/session_join_timing.py --repeats {args.repeats}`): Wav2Lip bf16x3, B = {B}, {N} running sessions of "
        f"{args.faces} cached crops and {H} x {Wd} frames, paste on.  Host wall time around a synchronised step, median (min – max), ms.",
        "",
        f"## (i) Step latency of the {N} running sessions around a join and a leave",
        "",
        f"`LipBatcher(max_sessions={N + 1})`; a step is `LipWindowPool.push` (`mf_windows_push`), one mel launch, `step(only=the {N})`.  Repeats alternate between a "
        f"sequence with `add_session` / `remove_session` of a ninth session before the marked steps and the same sequence without ({args.repeats} each).",
        "",
        "| step | with the join / leave | without |",
        "|---|---|---|",
    ] + [f"| {n} | {spread(times[True][n])} | {spread(times[False][n])} |" for n in names] + [
        "",
        f"`add_session` itself (slot, rows, the stream-ordered copy of {args.faces} crops enqueued): {spread(join_ms)} ms of host time; `remove_session`: {spread(leave_ms)} ms.",
        "",
        "## (ii) A window push for 8 of 16 sessions",
        "",
        "| route | ms |",
        "|---|---|",
    ] + [f"| {k} | {spread(v)} |" for k, v in push_ms.items()] + [
        "",
        "## (iii) The alternative without `add_session`: a new batcher with one session more",
        "",
        f"`LipBatcher(...)` with {N + 1} sessions on the same generator handle: **{build_ms:.1f}** ms; its `prewarm()` (the larger step grows the workspace, which drops every "
        f"captured graph; {N + 1} sizes, eager + capture each): **{prewarm_ms:.1f}** ms.  Every running session waits for both.",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
