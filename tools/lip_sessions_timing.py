"""One Wav2Lip step of N sessions x 16 frames, two routes in one process (MI355X):

  (a) per session, in sequence on one stream: LipASRFrontend.run_step (host window, full upload, mf_melspec, torch chunking) + LipSession.step_pasted
  (b) LipBatcher: one upload of the new chunks, the windows slide on the device, ONE mf_melspec_windows, ONE forward_u8_rows, one paste per session

Both start from the same 2B new PCM chunks per session and end with every session's pasted uint8 frames on the device.  hipEvents around the step, warm-up
first (hipGraph capture included), median of the repeats.  Prints a table and one JSON line.

    python tools/lip_sessions_timing.py [--sessions 1 2 4 8] [--repeats 30] [--warmup 5] [--frame 480 640]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frame", type=int, nargs=2, default=[480, 640], help="full frame H W")
    ap.add_argument("--faces", type=int, default=40, help="cached crops per session")
    args = ap.parse_args()

    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.paste import AvatarFrames
    from mere_fusion_amd.wav2lip.models import Wav2Lip

    B, (H, Wd) = args.batch, args.frame
    m = Wav2Lip(precision="bf16x3")
    m.load_state_dict(W.make_wav2lip_state_dict(0))
    m = m.to("cuda").eval()
    rows = []
    for N in args.sessions:
        def sessions():
            out = []
            for s in range(N):
                r = np.random.default_rng(100 + s)
                n = args.faces + s
                boxes = [(H // 4 + i % 7, H // 4 + 200 + i % 5, Wd // 4 + i % 3, Wd // 4 + 180 + i % 9) for i in range(n)]       # (y1, y2, x1, x2)
                av = AvatarFrames(r.integers(0, 256, (n, H, Wd, 3), dtype=np.uint8), boxes, lip_order=True)
                out.append(D.LipSession(m, r.integers(0, 256, (n, 96, 96, 3), dtype=np.uint8), avatar_frames=av))
            return out

        pcm = [[W.make_speech_like_wav(320, 1000 * s + i) for i in range(2 * B)] for s in range(N)]
        # route (a)
        sa = sessions()
        fa = [D.LipASRFrontend(B) for _ in range(N)]
        for f in fa:
            f.warm_up()

        def step_a():
            return [sa[s].step_pasted(fa[s].run_step(pcm[s]))[0] for s in range(N)]

        # route (b)
        bat = D.LipBatcher(m, sessions(), batch_size=B, paste=True)
        bat.prewarm()
        pool = bat.frontends()[0].pool
        ks = list(range(N))

        def step_b():
            pool.push(ks, [pool.host_block(pcm[s]) for s in ks])
            mel = pool.mel(pool.rows(ks))
            return [o[0] for o in bat.step([mel[s * B:(s + 1) * B] for s in ks])]

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

        a, b = timed(step_a), timed(step_b)
        rows.append(dict(sessions=N, frames=N * B, a_ms=round(a[0], 3), a_min=round(a[1], 3), a_max=round(a[2], 3), b_ms=round(b[0], 3), b_min=round(b[1], 3),
                         b_max=round(b[2], 3), speedup=round(a[0] / b[0], 2), fps_a=round(N * B / a[0] * 1e3), fps_b=round(N * B / b[0] * 1e3)))
    print(f"{'N':>2} {'frames':>6} {'(a) per-session ms':>20} {'(b) LipBatcher ms':>20} {'a/b':>6} {'frames/s a':>11} {'frames/s b':>11}")
    for r in rows:
        print(f"{r['sessions']:>2} {r['frames']:>6} {r['a_ms']:>9.3f} [{r['a_min']:.3f}-{r['a_max']:.3f}] {r['b_ms']:>9.3f} [{r['b_min']:.3f}-{r['b_max']:.3f}] "
              f"{r['speedup']:>6.2f} {r['fps_a']:>11} {r['fps_b']:>11}")
    print(json.dumps(dict(tool="lip_sessions_timing", batch=B, frame=[H, Wd], repeats=args.repeats, device=torch.cuda.get_device_name(0), rows=rows)))


if __name__ == "__main__":
    main()
