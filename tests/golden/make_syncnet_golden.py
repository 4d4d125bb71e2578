"""Generates tests/golden/syncnet_golden.npz by running the REAL reference module (build container only).

    python tests/golden/make_syncnet_golden.py            # needs /root/reference

`wav2lip.models.syncnet.SyncNet_color` (wav2lip/models/syncnet.py:7-66) is loaded with weights.syncnet_state_dict(0), cast to float64 and run on the two windows the
seeded clip of tests/sync_ref.py gives (6 frames of 96 x 96, 3840 samples): 5 BGR frames on the channel axis, / 255., lower half; mel[:, int(80 i / 25) : + 16] of
the project's float64-checked mel (oracle/mel_ref.py).  Only data is stored: the clip, the windows, both embeddings raw and normalised, a strided sample of the
face encoder after each of its 6 stages (make_golden.py's sampling), the sim / curve the float64 formulas give, and the pairwise distances below.

Condition on the fixture: the smallest L2 distance between normalised embeddings of different windows, face and audio alike, is at least 10 x the embedding gate
of the GPU test (sync_ref.TOL_X3) -- a network that returned the same embedding for every window would otherwise pass."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), "/root/reference"]

from mere_fusion_amd import weights as W          # noqa: E402
import geometry_cases as G                        # noqa: E402
import sync_ref as SR                             # noqa: E402
from oracle import mel_ref                        # noqa: E402

MAX_SHIFT = 3
MIN_DISTANCE = 1e-2          # 10 x the project's bf16x3 bound: holds for any gate the GPU test may carry


def sample(t):
    return t.detach().reshape(-1).numpy()[:: G.TAP_STRIDE][: G.TAP_MAX].copy()


def generate():
    from wav2lip.models.syncnet import SyncNet_color  # (the reference)
    torch.manual_seed(0)
    torch.set_num_threads(4)
    model = SyncNet_color()
    model.load_state_dict(W.syncnet_state_dict(0))
    model = model.double().eval()
    frames, pcm = SR.golden_frames(), SR.golden_pcm()
    starts = SR.window_starts(len(frames), len(pcm))
    mel = mel_ref.melspectrogram(pcm)
    mel_windows = np.stack([mel[:, m:m + SR.MEL_STEP] for _, m in starts])[:, None].astype(np.float32)
    face = SR.face_windows(frames, [s for s, _ in starts])
    taps = {}
    hooks = [model.face_encoder[i].register_forward_hook(lambda m, a, o, k=i: taps.__setitem__(k, o)) for i in W.SYNCNET_FACE_STAGE_ENDS]
    with torch.no_grad():
        a_n, f_n = model(torch.from_numpy(mel_windows).double(), torch.from_numpy(face))
        a_raw = model.audio_encoder(torch.from_numpy(mel_windows).double()).reshape(len(starts), -1)
    for h in hooks:
        h.remove()
    f_raw = taps[W.SYNCNET_FACE_STAGE_ENDS[-1]].reshape(len(starts), -1)
    sim, curve, counts = SR.sync_score_ref(f_raw.numpy(), a_raw.numpy(), MAX_SHIFT)
    dist = lambda e: min(float((e[i] - e[j]).norm()) for i in range(len(e)) for j in range(i))
    out = {"frames": frames, "pcm": pcm, "frame_starts": np.array([s for s, _ in starts], dtype=np.int32), "mel_starts": np.array([m for _, m in starts], dtype=np.int32),
           "mel_windows": mel_windows, "face_windows_u8": np.rint(face * 255.0).astype(np.uint8),
           "audio_raw": a_raw.numpy(), "face_raw": f_raw.numpy(), "audio_embedding": a_n.numpy(), "face_embedding": f_n.numpy(),
           "max_shift": np.int64(MAX_SHIFT), "sim": sim, "curve": curve, "counts": counts,
           "face_distance": np.float64(dist(f_n)), "audio_distance": np.float64(dist(a_n))}
    for i in W.SYNCNET_FACE_STAGE_ENDS:
        out[f"tap_sample/face_encoder.{i}"] = sample(taps[i])
        out[f"tap_abssum/face_encoder.{i}"] = np.float64(taps[i].abs().sum().item())
    return out


def main():
    out = generate()
    path = os.path.join(HERE, "syncnet_golden.npz")
    if "--check" in sys.argv:                      # tests/test_sync_host.py: the committed file regenerates bit for bit
        have = dict(np.load(path))
        bad = [k for k in sorted(set(out) | set(have)) if k not in out or k not in have or not np.array_equal(np.asarray(out[k]), have[k])]
        print("differs:", bad) if bad else print("identical:", len(out), "arrays")
        sys.exit(1 if bad else 0)
    print(f"windows {len(out['frame_starts'])}: face embeddings {out['face_distance']:.3e} apart, audio {out['audio_distance']:.3e}; curve {out['curve']}")
    print("raw embedding zeros: face", int((out["face_raw"] == 0).sum()), "audio", int((out["audio_raw"] == 0).sum()), "of", out["face_raw"].size)
    assert min(out["face_distance"], out["audio_distance"]) >= max(MIN_DISTANCE, 10 * SR.TOL_X3), "the fixture separates its windows too little: widen the BatchNorm affine"
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
