"""What lip-sync scoring costs on the device (profiles/sync_score_timing.md), beside one Wav2Lip step measured in the same run:

  1. SyncScorer.score on 4 s of one session (100 frames of 96 x 96, 64000 samples: W = 96 windows, S = 15, max_batch 64, so two chunks of the face encoder) --
     host wall time of the call, which ends in its one read-back;
  2. the window-input kernel alone (mf_net_set_input_u8_windows, 64 windows of 5 x 48 x 96 x 3 from the same frames), per launch, from hipEvents around
     `--inner` launches;
  3. mf_sync_score alone at W = 96, S = 15, dim 512, likewise;
  4. one Wav2Lip generator step at B = 16 (bf16x3, the serving default), hipEvents around one forward.

The four alternate in one loop: `--warmup` rounds are dropped, then the median of `--samples` with min and max.  Seeded weights: the times depend on the shapes
alone.  Prints one JSON line.

    python tools/sync_score_timing.py [--samples 20] [--warmup 5] [--inner 20] [--precision bf16x3]
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


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def timed(fn, inner=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_score_timing needs the GPU: a time taken anywhere else says nothing")
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.sync_score import SyncScorer, sync_score
    from mere_fusion_amd.wav2lip.models import SyncNet_color, Wav2Lip
    seconds, fps, S = 4, 25, 15
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (seconds * fps, 96, 96, 3), dtype=np.uint8)).cuda()
    wav = torch.from_numpy(W.make_speech_like_wav(seconds * 16000, 0)).cuda()
    net = SyncNet_color(precision=a.precision, max_batch=64)
    net.load_state_dict(W.syncnet_state_dict(0))
    net = net.to("cuda").eval()
    scorer = SyncScorer(net, fps=fps, max_shift=S, max_batch=64)
    r = scorer.score(frames, wav)
    assert r.W == 96, r.W
    g = net._graphs["face_encoder"]
    starts = list(range(64))
    emb_f, emb_a = torch.randn(96, 512, device="cuda"), torch.randn(96, 512, device="cuda")
    out = (torch.empty((96, 2 * S + 1), device="cuda"), torch.empty(2 * (2 * S + 1), device="cuda"))
    lip = Wav2Lip(precision="bf16x3")
    lip.load_state_dict(W.make_wav2lip_state_dict(0))
    lip = lip.to("cuda").eval()
    mel, face, _ = W.make_lip_inputs(16, 0)
    mel, face = mel.cuda(), face.cuda()
    with torch.no_grad():
        lip(mel, face)
    torch.cuda.synchronize()
    t = {"score_4s_wall": [], "window_kernel_64": [], "sync_score_kernels": [], "wav2lip_b16_step": []}
    for i in range(a.warmup + a.samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scorer.score(frames, wav)
        ms = {"score_4s_wall": (time.perf_counter() - t0) * 1e3,
              "window_kernel_64": timed(lambda: g["net"].set_input_u8_windows(g["bufs"][0], frames, starts, 5, 48, 48), a.inner),
              "sync_score_kernels": timed(lambda: sync_score(emb_f, emb_a, S, out=out), a.inner)}
        with torch.no_grad():
            ms["wav2lip_b16_step"] = timed(lambda: lip(mel, face))
        if i >= a.warmup:
            for k, v in ms.items():
                t[k].append(v)
    res = {"precision": a.precision, "samples": a.samples, "warmup": a.warmup, "inner": a.inner, "W": r.W, "max_shift": S, "max_batch": 64}
    res.update({k: stats(v) for k, v in t.items()})
    res["score_over_wav2lip_step"] = round(res["score_4s_wall"]["median_ms"] / res["wav2lip_b16_step"]["median_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
