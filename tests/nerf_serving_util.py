"""Shared by tests/test_nerf_serving.py (GPU) and tests/test_nerf_serving_host.py (CPU): a deterministic stand-in for the wav2vec2 net, seeded PCM, and the
reference's way of stepping one `NerfASRFrontend` per session (nerfreal.py:139-141)."""
from types import SimpleNamespace

import numpy as np
import torch

CHUNK, T_NET = 320, 27                     # 20 ms at 16 kHz; frames the net returns for a window of 28 chunks (tests/test_wav2vec2.py)


class StubNet:
    """[S, 8960] samples -> `.logits` (or `.last_hidden_state`) [S, 27, dim]: row t is vec * x[320 t + 7] + x[320 t + 100].  Elementwise only, so a window's
    rows are the same bits whatever else is in the batch: the net's rounding plays no part in what the pool is held to."""

    def __init__(self, dim, device, hidden=False):
        self.device, self.hidden, self.calls = torch.device(device), hidden, []
        self.vec = (torch.arange(dim, dtype=torch.float32) * 0.37 - 3.0).to(self.device)

    def __call__(self, x):
        x = torch.as_tensor(x).to(self.device, torch.float32)
        x = x[None] if x.dim() == 1 else x
        self.calls.append(int(x.shape[0]))
        a, b = x[:, 7::CHUNK][:, :T_NET], x[:, 100::CHUNK][:, :T_NET]
        out = a[:, :, None] * self.vec[None, None, :] + b[:, :, None]
        return SimpleNamespace(last_hidden_state=out) if self.hidden else SimpleNamespace(logits=out)


def pcm(session, frame):
    """the two 20 ms chunks of frame `frame` of session `session`"""
    rng = np.random.default_rng(1000 * session + frame)
    return [rng.standard_normal(CHUNK).astype(np.float32) for _ in range(2)]


def warmed_frontend(net, dim, att, device):
    """a `NerfASRFrontend` as `NerfASR.__init__` + `warm_up()` leave it (nerfasr.py:146-152)"""
    from mere_fusion_amd.ernerf.asr import NerfASRFrontend
    fe = NerfASRFrontend(net, att=att, audio_dim=dim, device=device)
    for _ in range(fe.warm_up_steps):
        fe.run_step()
    return fe


def reference_frame(fe, chunks):
    """nerfreal.py:139-141 for one frame"""
    for c in chunks:
        fe.put_audio_frame(c)
    fe.run_step()
    fe.run_step()
    return fe.get_next_feat()


def counters(fe):
    return len(fe.frames), fe.feat_buffer_idx, fe.front, fe.tail


def pool_counters(pool, k):
    return pool.frames[k], pool.feat_buffer_idx[k], pool.front[k], pool.tail[k]
