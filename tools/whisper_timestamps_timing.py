"""Times a decode step under the logit rules (mf_whisper_decoder_decode) against mf_whisper_decoder_greedy, tiny geometry, seeded weights, and
prints what profiles/whisper_timestamps_timing.md holds.

    python tools/whisper_timestamps_timing.py [--short 8] [--long 136] [--json out.json]

End-of-text is suppressed, so a call with max_new = n decodes exactly n tokens: one prefill and n - 1 steps.  ms per step = (wall time of a
`long` call - wall time of a `short` call) / (long - short), which takes the prefill, the uploads and the final read-back out; median and
min..max of 7 repeats, both calls on one box in one run, B = 1 and B = 8, check_every = 8 for both.  No time is gated.  The launches of a step
are NOT measured: the figure printed is read from the one step loop both calls share (csrc/mf_whisper_dec.hip `decode`): 1 embedding + 8 per
layer + 1 head + 1 choose, the choose kernel being the only launch that differs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

from mere_fusion_amd.musetalk.whisper import weights as DW                                 # noqa: E402
from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules, WhisperDecoder           # noqa: E402
from mere_fusion_amd.transcribe import SpecialTokens                                       # noqa: E402


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return np.asarray(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=136)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sp = SpecialTokens.multilingual()
    d = DW.WHISPER_TINY_TEXT
    dec = WhisperDecoder(DW.make_decoder_state_dict(1, d, timestamp_begin=sp.timestamp_begin, timestamp_gain=1.25), n_head=6, max_batch=8)
    mask = dec.suppress_mask([sp.eot, sp.sot, sp.sot_prev, sp.sot_lm, sp.no_speech])
    rules = DecodeRules(sp.eot, timestamp_begin=sp.timestamp_begin, no_timestamps=sp.no_timestamps, max_initial_timestamp_index=50, blank=220, no_speech=sp.no_speech, sot=sp.sot)
    rng = np.random.default_rng(0)
    # not measured here: both calls run the ONE step loop of `mf_whisper_decoder::decode`, which differs only in which choose kernel it launches
    res = {"short": args.short, "long": args.long, "launches_per_step_read_from_the_shared_loop": 3 + 8 * dec.n_layer}
    for B in (1, 8):
        enc = torch.from_numpy(rng.standard_normal((B, 1500, 384)).astype(np.float32)).cuda()
        prompts = [[sp.sot, sp.language_tokens["en"], sp.transcribe]] * B

        def greedy(n):
            dec.begin(enc)
            ids, _ = dec.greedy([p + [sp.no_timestamps] for p in prompts], sp.eot, n, suppress=mask)
            assert all(len(i) == n for i in ids)

        def ruled(n):
            dec.begin(enc)
            ids, _, _ = dec.decode(prompts, rules, n, suppress=mask)
            assert all(len(i) == n for i in ids)

        row = {}
        for name, fn in (("greedy", greedy), ("rules", ruled)):
            fn(args.long)                                                                  # warm-up
            per = []
            for _ in range(7):
                per.append((wall(lambda: fn(args.long), 1)[0] - wall(lambda: fn(args.short), 1)[0]) / (args.long - args.short) * 1e3)
            row[name] = {"ms_per_step_median": float(np.median(per)), "ms_per_step_min": float(np.min(per)), "ms_per_step_max": float(np.max(per))}
        row["rules_over_greedy"] = row["rules"]["ms_per_step_median"] / row["greedy"]["ms_per_step_median"]
        res[f"B{B}"] = row
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
