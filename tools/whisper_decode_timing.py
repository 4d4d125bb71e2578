"""Times the Whisper text decoder's decode step on the device (tiny geometry, seeded weights) and prints what profiles/whisper_decoder_timing.md holds.

    python tools/whisper_decode_timing.py [--steps 200] [--json out.json]

Per batch size (1 and 8): ms per decode step with the cache half full (events around `steps` consecutive steps, after a warm-up, the median of 5
repeats), the bytes a step must read (weight planes + the cross K | V of the batch + the self cache read so far) and the rate that makes;
then tokens/s of one 24-token utterance END TO END, the encoder call and the host's reads included (wall clock around Transcriber.transcribe).
The HBM rate the byte floor is stated against is measured here too: a device-to-device copy of 1 GiB."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

from mere_fusion_amd import weights as W                                   # noqa: E402
from mere_fusion_amd.musetalk.whisper import weights as DW                 # noqa: E402
from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature   # noqa: E402
from mere_fusion_amd.musetalk.whisper.decoder import WhisperDecoder        # noqa: E402
from mere_fusion_amd.transcribe import Transcriber                         # noqa: E402


def step_bytes(d, batch, cache_len, t_audio, x3=True):
    C, L, V = d["n_text_state"], d["n_text_layer"], d["n_vocab"]
    planes = 2 if x3 else 1
    weights = (L * 14 * C * C + V * C) * 2 * planes          # qkv 3, out 1, cross q 1, cross out 1, mlp 8 per layer; cross k|v is not read by a step
    cross = batch * L * t_audio * 2 * C * 4
    self_cache = batch * L * cache_len * 2 * C * 4
    return weights, cross, self_cache


def copy_rate():
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 10 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    d = DW.WHISPER_TINY_TEXT
    sd = DW.make_decoder_state_dict(1, d)
    esd = W.make_whisper_encoder_state_dict(0)
    sd.update({"encoder.ln_post." + k: esd["ln_post." + k] for k in ("weight", "bias")})
    res = {"hbm_copy_bytes_per_s": copy_rate(), "steps": args.steps}
    dec = WhisperDecoder(sd, n_head=6, max_batch=8)
    rng = np.random.default_rng(0)
    for B in (1, 8):
        enc = torch.from_numpy(rng.standard_normal((B, 1500, 384)).astype(np.float32)).cuda()
        toks = torch.from_numpy(rng.integers(0, 50000, (B, 1)).astype(np.int32)).cuda()
        start = 224 - args.steps // 2                        # the timed steps straddle a half-full cache
        reps = []
        for _ in range(5):
            dec.begin(enc)
            dec.logits(torch.from_numpy(rng.integers(0, 50000, (B, start)).astype(np.int32)))
            for _ in range(10):
                dec.logits(toks)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                dec.logits(toks)
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / args.steps)
        ms = float(np.median(reps))
        w, c, s = step_bytes(d, B, 224, 1500)
        res[f"B{B}"] = {"ms_per_step": ms, "ms_per_step_repeats": reps, "weight_bytes": w, "cross_kv_bytes": c, "self_cache_bytes": s,
                        "bytes_per_s": (w + c + s) / (ms * 1e-3), "weight_bytes_per_s": w / (ms * 1e-3),
                        "floor_ms_at_copy_rate": (w + c + s) / res["hbm_copy_bytes_per_s"] * 1e3}
    a2f = Audio2Feature(state_dict=esd, n_head=6)
    tr = Transcriber(a2f, dec, suppress=[50257])             # end-of-text suppressed: all 24 tokens are decoded
    wav = W.make_speech_like_wav(16000 * 5, 5)
    tr.transcribe(wav, max_new=24)
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = tr.transcribe(wav, max_new=24)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["utterance"] = {"tokens": len(ids), "seconds_median": float(np.median(times)), "seconds": times, "tokens_per_s": len(ids) / float(np.median(times))}
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
