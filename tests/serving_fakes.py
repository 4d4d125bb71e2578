"""Stand-ins the host tests of the serving stacks share (tests/test_serving_host.py, test_muse_driver.py, test_lip_batcher_host.py, test_nerf_serving_host.py):
a FrameRing without shared memory, a batcher without a model, and events without a device."""
from types import SimpleNamespace

import torch


class FakeRing:
    """the surface of transport.FrameRing the schedulers use: `places` slots, `taken` of them reserved or holding a message; `open` / `begun` / `aborted` keep
    the reservations that are neither begun nor returned, the tokens begun and the tokens aborted, so that a test sees a leak"""

    def __init__(self, places):
        self.places, self.taken, self.msgs = places, 0, []
        self.open, self.begun, self.aborted = [], [], []

    def free_slots(self):
        return self.places - self.taken

    def try_reserve(self, n):
        if self.free_slots() < n:
            return None
        self.taken += n
        tok = {"n": n}
        self.open.append(tok)
        return tok

    def unreserve(self, tok):
        self.open = [t for t in self.open if t is not tok]
        self.taken -= tok["n"]

    def begin_batch(self, fr, idx, stream=None, reserved=None):
        self.open = [t for t in self.open if t is not reserved]
        self.begun.append(reserved)
        reserved.update(fr=fr, idx=idx)
        return reserved

    def abort_batch(self, tok):
        self.aborted.append(tok)
        self.taken -= tok["n"]

    def commit_batch(self, tok, audio):
        self.msgs += [(None if tok["fr"] is None else tok["fr"][i], tok["idx"][i], audio[2 * i:2 * i + 2]) for i in range(len(tok["idx"]))]

    def get(self):
        self.taken -= 1
        return self.msgs.pop(0)


class FakeBatcher:
    """n sessions, `cap` per step, B frames each: a picked session's indices count up from 0, its frames are filled with its number (None for a None input)"""

    def __init__(self, n, cap, batch_size=2, device="cpu"):
        self.sessions, self.max_sessions_per_step, self.batch_size, self.device = [None] * n, cap, batch_size, torch.device(device)
        self.steps, self.index = [], [0] * n

    def step(self, chunks, only=None):
        self.steps.append((sorted(only), [None if c is None else "mel" for c in chunks]))
        out = [None] * len(self.sessions)
        for k in only:
            idx = list(range(self.index[k], self.index[k] + self.batch_size))
            self.index[k] += self.batch_size
            out[k] = (None if chunks[k] is None else torch.full((self.batch_size, 4, 4, 3), float(k)), idx)
        return out


def fake_cuda_events(monkeypatch):
    """torch.cuda.Event / current_stream for a box without a device: every event is complete at once"""
    ev = SimpleNamespace(record=lambda *_: None, query=lambda: True, synchronize=lambda: None)
    monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: ev)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: None)
    return ev
