"""What showing idle and custom-video frames from the device costs (profiles/idle_frames_timing.md), in one run:

  1. mf_frames_gather of 8 frames of 720 x 1280 (every second one from a second allocation) into a block, packed and as I420, next to mf_frames_to_i420 on the
     same pixels: the gather moves the bytes the converter moves (I420: 3 in, 1.5 out per pixel; packed: 3 in, 3 out), so the converter is the yardstick.  A
     sample is one replay of a graph of `--inner` launches between one event pair, divided by their number, the three alternating in one loop.
  2. a SILENT step of 8 Wav2Lip sessions x 8 frames of 720 x 1280 through LipEndToEndScheduler with idle_frames=True against the same step with the option off
     (today's B (None, idx, audio) tuples: nothing is launched or copied for them), alternating in one loop, in both ring formats: host wall time from submit
     to the last descriptor published (run_once + drain), the consumer emptying the rings outside the timed part.  The difference is what the option costs per
     silent step: the gathers and the D2H of 64 frames.

5 warm-ups, then the median of 30 samples with min and max.  What the option SAVES -- the consumer's per-frame host pass over a packed frame -- is not measured
here: that needs libav / OpenCV.  Prints one JSON line per part.

    python tools/idle_frames_timing.py [--frames 8] [--sessions 8] [--samples 30] [--warmup 5] [--inner 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT]

H, W = 720, 1280


def stats(ms):
    return {"median_us": round(1e3 * float(np.median(ms)), 2), "min_us": round(1e3 * float(np.min(ms)), 2), "max_us": round(1e3 * float(np.max(ms)), 2)}


def timed(fn):
    """device time of fn between one event pair, in ms"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_part(a):
    from mere_fusion_amd import ops
    from mere_fusion_amd.transport import i420_shape
    B = a.frames
    rng = np.random.default_rng(720)
    pool = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()          # an avatar's frame cache
    cycle = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()         # a custom video, another allocation
    srcs = [(cycle if i % 2 else pool)[i] for i in range(B)]
    stacked = torch.stack(srcs)                                                                 # the same pixels as one block: what the converter takes
    dst = list(range(B))
    packed = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    planes, planes_ref = (torch.empty((B,) + i420_shape(H, W), dtype=torch.uint8, device="cuda") for _ in range(2))
    calls = {"gather_packed": lambda: ops.gather_frames(srcs, dst, packed, fmt="packed"),
             "gather_i420": lambda: ops.gather_frames(srcs, dst, planes, fmt="i420", order="bgr"),
             "frames_to_i420": lambda: ops.frames_to_i420(stacked, "bgr", out=planes_ref)}
    moved = {"gather_packed": B * H * W * 6, "gather_i420": B * H * W * 9 // 2, "frames_to_i420": B * H * W * 9 // 2}
    graphs = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(a.inner):
                fn()
    t = {name: [] for name in calls}
    for i in range(a.warmup + a.samples):
        for name in calls:
            ms = timed(graphs[name].replay) / a.inner
            if i >= a.warmup:
                t[name].append(ms)
    row = {"part": "kernel", "frames": B, "H": H, "W": W, "samples": a.samples, "warmup": a.warmup, "inner": a.inner,
           "bytes_equal": bool(torch.equal(planes, planes_ref) and torch.equal(packed, stacked))}
    for name in calls:
        row[name] = stats(t[name])
        row[name]["gb_s"] = round(moved[name] / (np.median(t[name]) * 1e-3) / 1e9, 1)
    print(json.dumps(row), flush=True)


def step_part(a):
    from mere_fusion_amd import lip_driver as D
    from mere_fusion_amd import weights
    from mere_fusion_amd.paste import AvatarFrames
    from mere_fusion_amd.transport import FrameRing, i420_shape
    from mere_fusion_amd.wav2lip.models import Wav2Lip
    B, N, n_cached = a.frames, a.sessions, 4
    m = Wav2Lip(precision="bf16x3")
    m.load_state_dict(weights.make_wav2lip_state_dict(0))
    m = m.to("cuda").eval()
    rng = np.random.default_rng(1280)
    avatars = [AvatarFrames(rng.integers(0, 256, (n_cached, H, W, 3), dtype=np.uint8), [(200, 400, 500, 700)] * n_cached, lip_order=True) for _ in range(N)]
    faces = rng.integers(0, 256, (n_cached, 96, 96, 3), dtype=np.uint8)
    silence = [(np.zeros(320, np.float32), 1)] * (2 * B)
    row = {"part": "silent_step", "sessions": N, "frames": B, "H": H, "W": W, "samples": a.samples, "warmup": a.warmup}
    for fmt in ("packed", "i420"):
        shape = i420_shape(H, W) if fmt == "i420" else (H, W, 3)
        runs = {}
        for idle in (False, True):
            bat = D.LipBatcher(m, [D.LipSession(m, faces, avatar_frames=av) for av in avatars], batch_size=B, paste=True)
            rings = [FrameRing(B, shape) for _ in range(N)]
            runs[idle] = (D.LipEndToEndScheduler(bat, rings=rings, hold_s=0.0, frame_format=fmt, idle_frames=idle), rings)
        t = {False: [], True: []}
        try:
            for i in range(a.warmup + a.samples):
                for idle in (False, True):
                    sch, rings = runs[idle]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(N):
                        sch.submit(k, silence, t0)
                    done = sch.run_once(t0 + 1.0) + sch.drain()
                    ms = (time.perf_counter() - t0) * 1e3
                    assert len(done) == N and all((fr is not None) == idle for _, fr, _, _ in done)
                    for r in rings:                                                      # the consumer, outside the timed part
                        for _ in range(B):
                            f, _, _ = r.get(timeout=10, copy=False)
                            if f is not None:
                                r.release()
                    if i >= a.warmup:
                        t[idle].append(ms)
        finally:
            for sch, rings in runs.values():
                sch.close()
                for r in rings:
                    r.close()
        row[fmt] = {"option_off": stats(t[False]), "option_on": stats(t[True]),
                    "difference_us": round(1e3 * float(np.median(t[True]) - np.median(t[False])), 2), "d2h_bytes_per_step": N * B * int(np.prod(shape))}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sessions", type=int, default=8)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("idle_frames_timing needs the GPU: a time taken anywhere else says nothing")
    kernel_part(a)
    step_part(a)


if __name__ == "__main__":
    main()
