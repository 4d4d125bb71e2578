"""Per-batch glue of the MuseTalk render loop, restated for the GPU path (8f rank 2).

The reference runs this logic inside `MuseASR.run_step` (museasr.py:15-29) and `inference()` (musereal.py:53-122) around mp.Queues, one
process per session, each with its own model copy.  The drop-in keeps those files untouched; this module is the queue-free equivalent
that bench.py, the tests and a multi-session harness drive directly:

  MuseASRFrontend   MuseASR.run_step: sliding audio window -> Whisper features -> one (50, 384) chunk per video frame, never leaving HBM
  MuseSession       one avatar: cached latents (and, optionally, full frames + paste geometry) resident on the device, ping-pong index
  MuseBatcher       ONE UNet + VAE pair serving N sessions: every step gathers each active session's latents by mirror index
                    (mf_gather_rows_f32) and its audio chunks into one N * B-frame batch, runs musereal.py:100-108 once, and hands every
                    session its own uint8 frames (optionally already pasted into the full frame, mf_paste_frames)
  EndToEndScheduler serving.PipelinedScheduler (the model-agnostic session loop; SessionScheduler, pick_sessions and mirror_index are re-exported from there)
                    with the Whisper stage: a window slides when its PCM arrives, the windows of all sessions picked for a step go through ONE encoder call

Cross-session batching is what fills an MI355X: the UNet at 8 frames per step is launch-latency bound, at 64 it is not."""
import ctypes as C
import time

import numpy as np
import torch

from . import _lib
from .serving import (PipelinedScheduler, PooledBatcher, SessionScheduler, SessionWalk, all_silent, mirror_index, pick_sessions,  # noqa: F401  (re-exported)
                      split_batch)


def chunk_left_rows(batch_size, fps, start, audio_feat_length=(2, 2)):
    """First (unclamped) feature row of every chunk of one run_step: `center_idx = int(vid_idx * 50 / fps)`, `left_idx = center_idx -
    audio_feat_length[0] * 2` with vid_idx = i + start (audio2feature.py:29-31, 93-96)."""
    return [int((i + start) * 50 / fps) - audio_feat_length[0] * 2 for i in range(batch_size)]


def feature_chunks_device(feat, left_rows, rows_per_chunk=10, out=None):
    """Audio2Feature.feature2chunks on the device: feat [T, L+1, C] fp32 -> [B, rows_per_chunk * (L+1), C] (= [B, 50, 384])."""
    if not feat.is_cuda:
        raise RuntimeError("feature_chunks_device needs the Whisper features on the HIP device; no CPU path exists here")
    feat = feat.float().contiguous()
    T, L1, Cc = feat.shape
    B = len(left_rows)
    if out is None:
        out = torch.empty((B, rows_per_chunk * L1, Cc), dtype=torch.float32, device=feat.device)
    rows = (C.c_int * B)(*[int(r) for r in left_rows])
    with torch.cuda.device(feat.device):
        _lib.check(_lib.lib().mf_whisper_feature_chunks(feat.data_ptr(), T, L1 * Cc, rows, rows_per_chunk, B, out.data_ptr(),
                                                        _lib.stream_ptr(feat.device)), "whisper_feature_chunks")
    return out


class MuseASRFrontend:
    """MuseASR.run_step without the queues: 2B new 20 ms chunks in, B Whisper chunks [B, 50, 384] out (on the device)."""

    def __init__(self, audio_processor, batch_size, fps=50, stride_left=10, stride_right=10):
        self.audio_processor, self.batch_size, self.fps = audio_processor, batch_size, fps
        self.l, self.r = stride_left, stride_right
        self.frames = []

    def warm_up(self, chunk=320):
        """baseasr.py:53-59: prime the context with l + r silent chunks."""
        self.frames = [np.zeros(chunk, dtype=np.float32) for _ in range(self.l + self.r)]

    def window(self, new_chunks):
        """museasr.py:17-29 up to the encoder call: take the 2B new 20 ms chunks, return the (l + 2B + r) x 320-sample window the encoder sees
        (None while the context is still filling, museasr.py:22-23) and keep the last l + r chunks as the next window's context."""
        self.frames.extend(new_chunks)
        if len(self.frames) <= self.l + self.r:                       # museasr.py:22-23
            return None
        win = np.concatenate(self.frames)                             # museasr.py:25
        self.frames = self.frames[-(self.l + self.r):]                # museasr.py:29
        return win

    def chunks_from_features(self, feat, out=None):
        """museasr.py:27: the B (50, 384) chunks of this step from the window's features [T, 5, 384] (device)."""
        return feature_chunks_device(feat, chunk_left_rows(self.batch_size, self.fps / 2, self.l / 2), out=out)

    def run_step(self, new_chunks, out=None):
        win = self.window(new_chunks)
        if win is None:
            return None
        return self.chunks_from_features(self.audio_processor.audio2feat_device(win), out=out)   # museasr.py:25-27


class MuseSession(SessionWalk):
    """One talking-head session: the avatar's cached latents (musereal.py:64 `torch.load(latents.pt)`: a list of [1, 8, 32, 32] tensors)
    and its position in the ping-pong walk.  `avatar_frames` (mere_fusion_amd.paste.AvatarFrames) enables the GPU paste-back.  custom_videos
    (paste.CustomVideos): what the session shows for non-speech frames of a custom audio type when its scheduler runs with idle_frames=True; frames of another
    size than the avatar's are refused here."""

    def __init__(self, latents, avatar_frames=None, custom_videos=None):
        lat = latents if torch.is_tensor(latents) else torch.cat([torch.as_tensor(x).reshape(1, *torch.as_tensor(x).shape[-3:]) for x in latents], dim=0)
        self.latents = lat.float().contiguous()
        self.length = self.latents.shape[0]
        self.avatar_frames = avatar_frames
        if avatar_frames is not None and avatar_frames.n != self.length:
            raise RuntimeError("one cached full frame per cached latent is required (frame_list_cycle / input_latent_list_cycle)")
        self.attach_custom_videos(custom_videos)


class MuseBatcher(PooledBatcher):
    """N sessions through one UNet / VAE handle per step (BASELINE.json north star: 8 sessions per GPU)."""

    def __init__(self, unet, vae, sessions, batch_size=8, paste=False, device="cuda", max_sessions_per_step=None, max_sessions=None, pool_rows=None):
        """max_sessions, pool_rows (both None: a fixed session list, as ever): sessions may join and leave (add_session / remove_session, serving.PooledBatcher).
        `sessions` is then a list of max_sessions slots (None: vacant) and the pool ONE allocation of pool_rows rows (default: the initial sessions' rows) whose
        address never changes; a step still holds at most max_sessions_per_step sessions (default here: the initial number)."""
        if not torch.cuda.is_available():
            raise RuntimeError("MuseBatcher needs a HIP device; no CPU path exists here")
        self.unet, self.vae, self.sessions, self.batch_size, self.paste = unet, vae, list(sessions), batch_size, paste
        self.device = torch.device(device)
        # more sessions than one step holds: step(..., only=[...]) serves a subset (SessionScheduler)
        self.max_sessions_per_step = len(self.sessions) if max_sessions_per_step is None else int(max_sessions_per_step)
        need = self.max_sessions_per_step * batch_size
        for h, what in ((unet.model.max_batch, "UNet"), (getattr(vae, "max_batch", need), "VAE")):
            if h < need:
                raise RuntimeError(f"{what} handle was created with max_batch {h}; {self.max_sessions_per_step} sessions x {batch_size} frames need {need}")
        self.lat_shape = tuple(self.sessions[0].latents.shape[1:])
        if max_sessions is not None or pool_rows is not None:
            for k, s in enumerate(self.sessions):
                self._check_session(k, s)
        # every session's cached latents in one pool: a batch is one gather
        self.pool = self._build_pool(max_sessions, pool_rows)
        self.row_elems = self.pool.shape[1]
        self.t0 = torch.tensor([0], device=self.device)

    def _check_session(self, k, s):
        if tuple(s.latents.shape[1:]) != self.lat_shape:
            raise RuntimeError(f"session {k}: cached latents of shape {tuple(s.latents.shape[1:])}; this batcher's pool holds {self.lat_shape}")
        if s.avatar_frames is not None and s.avatar_frames.n != s.length:
            raise RuntimeError(f"session {k}: one cached full frame per cached latent is required (frame_list_cycle / input_latent_list_cycle)")

    @staticmethod
    def _session_rows(s):
        return s.latents.reshape(s.length, -1)

    @torch.no_grad()
    def prewarm(self, tune=False):
        """Everything a step size costs the FIRST time -- the eager forward that sizes the split-K workspaces, the hipGraph capture, and (tune=True)
        the explicit launch-configuration measurement (mf_unet_tune / mf_vae_tune, seconds per size) -- for every number of sessions a step can hold,
        so that the serving loop never meets a new batch size.  Session state (frame indices) is left untouched.  Call once at start-up."""
        B = self.batch_size
        zeros = torch.zeros((self.max_sessions_per_step * B, 50, self.unet.model.config["cross_attention_dim"]), dtype=torch.float32, device=self.device)
        lat = torch.zeros((self.max_sessions_per_step * B,) + self.lat_shape, dtype=torch.float32, device=self.device)
        lat.copy_(self.pool[:1].reshape((1,) + self.lat_shape).expand_as(lat))
        fwd = lambda n: self.vae.decode_latents_device(self.unet.model(lat[:n], self.t0, encoder_hidden_states=self.unet.pe(zeros[:n])).sample)  # noqa: E731
        self._prewarm_sizes(tune, fwd, lambda n: (self.unet.model.tune(n), self.vae.tune(n)))

    def step(self, whisper_chunks, only=None):
        """whisper_chunks: per session a device tensor [B, 50, 384] or None (silent); frames: uint8 [B, 256, 256, 3] BGR (`recon`, musereal.py:108) or pasted"""
        return super().step(whisper_chunks, only)

    def _check_input(self, k, ch):
        if ch.shape[0] != self.batch_size or not ch.is_cuda:
            raise RuntimeError(f"session {k}: expected a device tensor of {self.batch_size} whisper chunks, got {tuple(ch.shape)} on {ch.device}")

    def _forward(self, chunks, rows):
        n = len(rows)
        lat = torch.empty((n,) + self.lat_shape, dtype=torch.float32, device=self.device)
        crows = (C.c_int * n)(*rows)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_gather_rows_f32(self.pool.data_ptr(), self.pool.shape[0], self.row_elems, crows, n, lat.data_ptr(),
                                                     _lib.stream_ptr(self.device)), "gather_rows_f32")
        pred = self.unet.model(lat, self.t0, encoder_hidden_states=self.unet.pe(self.cat_inputs(chunks))).sample    # musereal.py:102-107
        return self.vae.decode_latents_device(pred)                                                     # musereal.py:108, frames stay in HBM


class EndToEndScheduler(PipelinedScheduler):
    """The per-GPU MuseTalk session loop: serving.PipelinedScheduler (musereal.py:91-108 through MuseBatcher.step, the paste stage of a batcher built with
    paste=True, delivery through the FrameRings) with the Whisper stage in front:

      museasr.py:15-29    every session's 2B new 20 ms PCM chunks -> its sliding window; the windows of ALL sessions picked for a step go through the
                          Whisper encoder in ONE call (mf_whisper_encode_windows), then `feature2chunks` per session on the device
    submit(k, pcm_chunks, t_arrival)  the 2B chunks of session k that completed a batch at t_arrival (audio_frames = [(chunk, 0)] * 2B)
    Stages can be switched off individually to price them (bench.py `paced_sessions.stages`)."""

    def __init__(self, batcher, frontends, audio_processor, rings=None, period_s=None, hold_s=None, clock=time.perf_counter, depth=2, fixed_chunks=None,
                 asr_stream=True, single_stream=False, frame_format="packed", idle_frames=False):
        if len(frontends) != len(batcher.sessions):
            raise RuntimeError("one MuseASRFrontend per session is required")
        super().__init__(batcher, rings=rings, period_s=period_s, hold_s=hold_s, clock=clock, depth=depth, single_stream=single_stream, frame_format=frame_format,
                         idle_frames=idle_frames)
        # (fixed_chunks: measurement only, this [B, 50, 384] tensor instead of the Whisper stage)
        self.fixed_chunks, self.frontends, self.audio_processor = fixed_chunks, list(frontends), audio_processor
        # The Whisper front-end of a step on its OWN stream: with two steps in flight it runs beside the previous step's VAE instead of between that VAE and
        # this step's UNet.  Its ~25 launches are latency-bound (1.5 ms for seven windows with the GPU mostly idle); beside the VAE's full-chip kernels they cost
        # the step almost nothing.  asr_stream=False: on the step's stream, as before (A/B, bench `stages`); single_stream implies it.
        self.asr_stream = torch.cuda.Stream(device=batcher.device) if asr_stream and not self.single_stream else None

    def submit(self, k, pcm_chunks, t_arrival=None):
        """pcm_chunks: the batch's 2B 20 ms chunks -- bare arrays or (chunk, type) pairs (serving.split_batch).  An all-silent batch skips the networks, as
        musereal.py:82-86 does: its B (None, idx, audio_frames) tuples still reach the session's ring so that `process_frames` keeps audio and idle video in step."""
        self._check_slot(k, "submit")
        chunks, pairs, types = split_batch(pcm_chunks, "EndToEndScheduler.submit")
        win = self.frontends[k].window(chunks)                        # host side of museasr.py:17-29, at arrival time (the window slides for silent batches too)
        super().submit(k, None if all_silent(types) else win, t_arrival, pairs)

    def _check_join(self, k, session, ring, frontend):
        if not isinstance(frontend, MuseASRFrontend):
            raise RuntimeError("EndToEndScheduler: add_session takes the joiner's MuseASRFrontend (frontend=), as the constructor takes one per session")
        super()._check_join(k, session, ring, frontend)

    def _store(self, k, session, ring, frontend):
        super()._store(k, session, ring, frontend)
        self.frontends[k] = frontend

    def _drop(self, k):
        super()._drop(k)
        self.frontends[k] = None

    def _inputs(self, ks, wins, dev):
        """The Whisper stage of one step: wins[k] is the window submit() queued for session k (None: a silent batch, or a context that is still filling)."""
        chunks = [None] * len(self.queues)
        speaking = [k for k in ks if wins[k] is not None]
        if speaking and self.fixed_chunks is not None:
            for k in speaking:
                chunks[k] = self.fixed_chunks
        elif speaking:
            cur = torch.cuda.current_stream(dev)
            side = self.asr_stream if self.asr_stream is not None else cur
            with torch.cuda.stream(side):
                wav = torch.from_numpy(np.stack([wins[k] for k in speaking])).to(dev, non_blocking=True)
                feats = self.audio_processor.audio2feat_windows_device(wav)        # every picked session's window in one encoder call
                for i, k in enumerate(speaking):
                    chunks[k] = self.frontends[k].chunks_from_features(feats[i])
            if side is not cur:
                cur.wait_stream(side)                                              # the UNet below reads the chunks
                for t in [wav, feats] + [chunks[k] for k in speaking]:
                    t.record_stream(cur)
        return chunks
