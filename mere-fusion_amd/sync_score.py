"""Lip-sync scoring of served frames on the device: does the mouth move with the audio?

`SyncScorer` runs the SyncNet expert (wav2lip/models/syncnet.py, here wav2lip.models.SyncNet_color) over a clip's 5-frame lower-half windows and their mel windows
and reduces the audio / video similarity over a band of shifts (mf_sync_score); `SyncMonitor` keeps the last seconds of a serving session in two device rings and
scores them on demand.  Neither is wired into the schedulers: a deployment calls `push` beside its own step.

[upstream-knowledge] The windowing rule and the score are upstream Wav2Lip's (color_syncnet_train.py, hparams.py: window i starts at frame i, its mel window at
column int(80 * i / fps), syncnet_mel_step_size = 16 columns of the hop-200 mel at 16 kHz); that file is not part of the reference tree, which ships the module
alone.  The network is pinned to the reference's module; no real checkpoint has been loaded here, and scores on seeded weights say nothing about sync."""
from types import SimpleNamespace

import torch

from . import _lib, ops

T, MEL_STEP, MEL_PER_SECOND, SAMPLE_RATE, HOP = 5, 16, 80, 16000, 200
FACE = 96


def window_starts(n_frames, n_samples, fps=25):
    """-> [(first frame, first mel column)]: window i covers frames [i, i + 5) and mel[:, int(80 * i / fps) : + 16] of the 1 + n_samples // 200 columns the clip's mel
    has.  A window whose mel would run past the end is dropped, and every later one with it."""
    mel_len = 1 + int(n_samples) // HOP
    out = []
    for i in range(max(0, int(n_frames) - T + 1)):
        m = int(MEL_PER_SECOND * i / float(fps))
        if m + MEL_STEP > mel_len:
            break
        out.append((i, m))
    return out


def reduce_curve(curve, counts, max_shift):
    """Plain Python over the 2 S + 1 values read back: (score, offset, confidence).  score = curve[S]; offset = the shift of the curve's maximum among the shifts with
    counts > 0, a tie going to the smaller |shift| (then to the negative one); confidence = max - median over those shifts."""
    S = int(max_shift)
    valid = [(float(curve[s]), s - S) for s in range(2 * S + 1) if int(counts[s]) > 0]
    if not valid:
        raise ValueError("reduce_curve: no shift has a valid window")
    best = max(v for v, _ in valid)
    offset = min((sh for v, sh in valid if v == best), key=lambda sh: (abs(sh), sh))
    vals = sorted(v for v, _ in valid)
    n = len(vals)
    median = vals[n // 2] if n % 2 else 0.5 * (vals[n // 2 - 1] + vals[n // 2])
    return float(curve[S]), offset, best - median


def sync_score(face_emb, audio_emb, max_shift, out=None):
    """mf_sync_score on two device fp32 [W, dim] embedding sequences (raw or normalised) -> (sim [W, 2 S + 1], curve [2 S + 1] fp32, counts [2 S + 1] int32), device
    tensors; curve and counts are the two halves of one block, so that one copy reads both back.  out: such a (sim, block) pair to write into."""
    if not (face_emb.is_cuda and audio_emb.is_cuda):
        raise RuntimeError("sync_score needs HIP device tensors; no CPU path exists here")
    if face_emb.dim() != 2 or face_emb.shape != audio_emb.shape:
        raise ValueError(f"sync_score: two [W, dim] sequences of one shape expected, got {tuple(face_emb.shape)} and {tuple(audio_emb.shape)}")
    f, a = face_emb.float().contiguous(), audio_emb.float().contiguous()
    W, dim = f.shape
    ns = 2 * int(max_shift) + 1
    sim, block = out if out is not None else (torch.empty((W, max(ns, 1)), dtype=torch.float32, device=f.device), torch.empty(2 * max(ns, 1), dtype=torch.float32, device=f.device))
    curve, counts = block[:ns], block[ns:].view(torch.int32)
    _lib.init_device(f.device.index if f.device.index is not None else torch.cuda.current_device())
    with torch.cuda.device(f.device):
        _lib.check(_lib.lib().mf_sync_score(f.data_ptr(), a.data_ptr(), W, dim, int(max_shift), sim.data_ptr(), curve.data_ptr(), counts.data_ptr(),
                                            _lib.stream_ptr(f.device)), "sync_score")
    return sim, curve, counts


class SyncScorer:
    def __init__(self, syncnet, fps=25, max_shift=15, max_batch=64):
        if not 0 <= int(max_shift) <= 64:
            raise ValueError(f"SyncScorer: max_shift must be in [0, 64], got {max_shift}")
        self.syncnet, self.fps, self.max_shift = syncnet, fps, int(max_shift)
        if getattr(syncnet, "max_batch", max_batch) != int(max_batch):      # the scorer's chunk size is the network's graph capacity
            syncnet.max_batch = int(max_batch)
            syncnet._drop_graphs()

    def score(self, frames_u8, wav):
        """frames_u8: uint8 BGR [N, h, w, 3] on the device, N >= 5 (face crops: LipBatcher's [B, 96, 96, 3] before the paste, MuseTalk's 256 x 256 recon);
        wav: fp32 16 kHz PCM on the device covering the same N / fps seconds.  Everything is enqueued on the current stream; the one sync is the read-back of the
        2 S + 1 curve values and counts.  -> namespace(W, frame_starts, mel_starts, sim, curve (device), counts, score, offset, confidence)"""
        from .wav2lip import audio
        if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and torch.is_tensor(wav) and wav.is_cuda):
            raise RuntimeError("SyncScorer.score needs HIP device tensors; no CPU path exists here")
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < T:
            raise ValueError(f"SyncScorer.score: uint8 [N >= {T}, h, w, 3] frames expected, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        wav = wav.reshape(-1).float().contiguous()
        N, h, w = (int(v) for v in frames_u8.shape[:3])
        starts = window_starts(N, wav.shape[0], self.fps)
        if not starts:
            raise ValueError(f"SyncScorer.score: {N} frames and {wav.shape[0]} samples give no window (a window needs {T} frames and {MEL_STEP} mel columns)")
        frames = frames_u8.contiguous()
        if (h, w) != (FACE, FACE):
            frames = ops.crop_resize_u8(frames, [(0, 0, w, h)] * N, FACE, "linear")
        mel_starts = [m for _, m in starts]
        pad = audio.PAD_MODES[audio.pad_mode]
        # mf_melspec_windows takes 256 starts a launch: 10 s of windows at 25 fps; a longer clip takes one launch more per 256
        mels = [ops.melspec_windows(wav[None], mel_starts[i:i + 256], pad) for i in range(0, len(mel_starts), 256)]
        mel = mels[0] if len(mels) == 1 else torch.cat(mels)
        face_emb = self.syncnet.embed_faces_u8(frames, [f for f, _ in starts])
        audio_emb = self.syncnet.embed_audio(mel)
        sim, curve, counts = sync_score(face_emb, audio_emb, self.max_shift)
        ns = 2 * self.max_shift + 1
        host = torch.cat([curve, counts.view(torch.float32)]).cpu()          # the one read-back (and the one sync)
        curve_h, counts_h = host[:ns].tolist(), host[ns:].view(torch.int32).tolist()
        score, offset, confidence = reduce_curve(curve_h, counts_h, self.max_shift)
        return SimpleNamespace(W=len(starts), frame_starts=[f for f, _ in starts], mel_starts=mel_starts, sim=sim, curve=curve, counts=counts_h, curve_host=curve_h,
                               score=score, offset=offset, confidence=confidence)


def ring_spans(head, n, capacity):
    """the (ring start, source start, length) copies that put n items at `head` of a ring of `capacity`: one span, or two when the write wraps"""
    if not 0 <= head < capacity or not 0 <= n <= capacity:
        raise ValueError(f"ring_spans: head {head}, n {n}, capacity {capacity}")
    first = min(n, capacity - head)
    return [(head, 0, first)] + ([(0, first, n - first)] if n > first else [])


class SyncMonitor:
    """The last `seconds` of one session's face crops and PCM in two device rings, allocated once (plus one linear copy of each that `report` fills): `push` copies
    a serving step into them and allocates nothing; `report` scores what they hold, oldest frame first."""

    def __init__(self, scorer, seconds=4.0, face_size=(FACE, FACE), device="cuda"):
        self.scorer = scorer
        self.capacity = max(T, int(round(seconds * scorer.fps)))
        self.samples_per_frame = 2 * 320                                      # the two 20 ms PCM chunks that travel with a frame (16 kHz, 25 fps)
        self.device = torch.device(device)
        fh, fw = face_size
        self.frames = torch.zeros((self.capacity, fh, fw, 3), dtype=torch.uint8, device=self.device)
        self.pcm = torch.zeros(self.capacity * self.samples_per_frame, dtype=torch.float32, device=self.device)
        self._lin_frames, self._lin_pcm = torch.zeros_like(self.frames), torch.zeros_like(self.pcm)
        self.head, self.count = 0, 0                                          # next slot to write; frames held

    def push(self, frames_u8, pcm):
        """One serving step: frames_u8 uint8 [B, h, w, 3] (LipBatcher's [B, 96, 96, 3] before the paste, or MuseTalk's recon), pcm the step's 2 * 320 * B samples.
        Silent batches are not pushed: they carry no generated mouth (the batcher passes the avatar's own frames through), and silence against a still mouth
        would only flatten the curve."""
        B, spf = int(frames_u8.shape[0]), self.samples_per_frame
        pcm = pcm.reshape(-1)
        if tuple(frames_u8.shape[1:]) != tuple(self.frames.shape[1:]) or frames_u8.dtype != torch.uint8:
            raise ValueError(f"SyncMonitor.push: uint8 [B, {self.frames.shape[1]}, {self.frames.shape[2]}, 3] frames expected, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        if pcm.shape[0] != B * spf:
            raise ValueError(f"SyncMonitor.push: {B} frames travel with {B * spf} samples, got {pcm.shape[0]}")
        if B > self.capacity:                                                 # only the newest fit
            frames_u8, pcm, B = frames_u8[B - self.capacity:], pcm[(B - self.capacity) * spf:], self.capacity
        for dst, src, n in ring_spans(self.head, B, self.capacity):
            self.frames[dst:dst + n].copy_(frames_u8[src:src + n], non_blocking=True)
            self.pcm[dst * spf:(dst + n) * spf].copy_(pcm[src * spf:(src + n) * spf], non_blocking=True)
        self.head = (self.head + B) % self.capacity
        self.count = min(self.capacity, self.count + B)

    def held(self):
        """(frames [count, h, w, 3], pcm [count * 640]) in time order: views of the linear copies"""
        spf, oldest = self.samples_per_frame, (self.head - self.count) % self.capacity
        for src, dst, n in ring_spans(oldest, self.count, self.capacity):
            self._lin_frames[dst:dst + n].copy_(self.frames[src:src + n], non_blocking=True)
            self._lin_pcm[dst * spf:(dst + n) * spf].copy_(self.pcm[src * spf:(src + n) * spf], non_blocking=True)
        return self._lin_frames[:self.count], self._lin_pcm[:self.count * spf]

    def report(self):
        if self.count < T:
            raise ValueError(f"SyncMonitor.report: {self.count} frames held, a window needs {T}")
        return self.scorer.score(*self.held())
