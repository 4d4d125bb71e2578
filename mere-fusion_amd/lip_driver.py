"""Per-batch glue of the Wav2Lip render loop, restated for the GPU path.

The reference runs this logic inside `LipASR.run_step` (lipasr.py:14-37) and `inference()`
(lipreal.py:75-141) around mp.Queues.  The drop-in keeps those files untouched; this module is
the queue-free equivalent that bench.py and the multi-session harness drive directly:
mel chunking, ping-pong face selection, and the fused uint8 -> generator -> frame*255 step.

Serving many sessions from one generator handle (the Wav2Lip counterpart of muse_driver's stack):

  LipWindowPool / LipASRDeviceFrontend   every session's sliding audio window as one row of a device buffer: a step uploads only the 2B new chunks, the l + r
                                         context is shifted on the device, and ONE mf_melspec_windows launch turns all picked rows into [N * B, 1, 80, 16]
  LipBatcher                             ONE generator handle serving N sessions: every session's cached crops in one uint8 pool, a step is one
                                         forward_u8_rows over the active sessions' mirror-indexed pool rows (+ one AvatarFrames.paste per session)
  LipSessionScheduler                    serving.SessionScheduler over a LipBatcher (mel chunks in, frames out)
  LipEndToEndScheduler                   serving.PipelinedScheduler with the Wav2Lip audio stage: PCM chunks in, (res_frame, idx, audio_frames) tuples out
                                         of each session's FrameRing; pacing, back-pressure, advance-once and delivery are serving.py's code
"""
import time

import numpy as np
import torch

from . import ops
from .serving import (PipelinedScheduler, PooledBatcher, SessionScheduler, SessionWalk, all_silent, live_sessions, mirror_index,  # noqa: F401  (re-exported)
                      pick_sessions, split_batch)
from .wav2lip import audio


def mel_chunk_starts(n_frames, stride_left, stride_right, fps, mel_len, mel_step=16):
    """Start column of every 16-wide mel window of one run_step (lipasr.py:24-35).

    n_frames = number of 20 ms audio chunks in the window (2B + l + r in steady state);
    one video frame consumes two of them, hence the /2 and the 80*2/fps columns per frame.
    Windows that would run past the spectrogram are clamped to its tail (lipasr.py:31-32)."""
    left = max(0, stride_left * 80 / 50)
    mult = 80.0 * 2 / fps
    starts = []
    i = 0
    while i < (n_frames - stride_left - stride_right) / 2:
        s = int(left + i * mult)
        if s + mel_step > mel_len:
            s = mel_len - mel_step
        starts.append(s)
        i += 1
    return starts


class LipASRFrontend:
    """LipASR.run_step without the queues: 2B new 20 ms chunks in, B mel windows [B,1,80,16] out."""

    def __init__(self, batch_size, fps=50, stride_left=10, stride_right=10, device="cuda"):
        self.batch_size, self.fps = batch_size, fps
        self.l, self.r = stride_left, stride_right
        self.device = device
        self.frames = []

    def warm_up(self, chunk=320):
        """baseasr.py:53-59: prime the context with l+r silent chunks."""
        self.frames = [np.zeros(chunk, dtype=np.float32) for _ in range(self.l + self.r)]

    def run_step(self, new_chunks):
        self.frames.extend(new_chunks)
        if len(self.frames) <= self.l + self.r:
            return None
        wav = torch.from_numpy(np.concatenate(self.frames)).to(self.device)
        mel = audio.melspectrogram_device(wav)                       # [80, T] on device
        starts = mel_chunk_starts(len(self.frames), self.l, self.r, self.fps, mel.shape[1])
        idx = torch.tensor(starts, device=mel.device)[:, None] + torch.arange(16, device=mel.device)[None, :]
        chunks = mel[:, idx].permute(1, 0, 2).unsqueeze(1).contiguous()   # [B,1,80,16]
        self.frames = self.frames[-(self.l + self.r):]
        return chunks


class LipSession(SessionWalk):
    """One talking-head session: cached uint8 face crops on the device + the generator.  With `avatar_frames`
    (mere_fusion_amd.paste.AvatarFrames built from frame_list_cycle / coord_list_cycle with lip_order=True) `step_pasted` also does
    process_frames' paste-back (lipreal.py:207-214) on the device.  custom_videos (paste.CustomVideos): what the session shows for non-speech frames of a custom
    audio type when its scheduler runs with idle_frames=True; frames of another size than the avatar's are refused here."""

    def __init__(self, model, faces_u8, avatar_frames=None, custom_videos=None):
        self.model = model
        self.faces = faces_u8 if torch.is_tensor(faces_u8) else torch.from_numpy(np.asarray(faces_u8))
        self.faces = self.faces.to(next(model.parameters()).device)
        self.avatar_frames = avatar_frames
        self.length = self.faces.shape[0]                           # (pool_offset: first row of this session's crops in a LipBatcher's pool)
        self.attach_custom_videos(custom_videos)

    def step(self, mel_batch):
        """lipreal.py:109-137 for one non-silent batch: returns fp32 frames [B,96,96,3] (pred*255) and
        the face indices they belong to; process_frames truncates with astype(uint8) (lipreal.py:211)."""
        idx = self.next_indices(mel_batch.shape[0])
        sel = self.faces[torch.tensor(idx, device=self.faces.device)]
        return self.model.forward_u8(mel_batch, sel), idx

    def step_pasted(self, mel_batch):
        """step() + lipreal.py:207-214: the full uint8 BGR frames [B, H, W, 3] with the generated mouth region resized into the bbox,
        still on the device."""
        if self.avatar_frames is None:
            raise RuntimeError("LipSession.step_pasted needs AvatarFrames (full frames + coords)")
        frames, idx = self.step(mel_batch)
        return self.avatar_frames.paste(frames, idx), idx


class LipWindowPool:
    """The sliding audio windows of N sessions, resident on the device: buf fp32 [N, (2B + l + r) * chunk], row k = session k's window as lipasr.py:17-23
    concatenates it.  A fresh pool (and a row after `warm_up`) holds silence, which is the state baseasr.py:53-59 leaves: l + r zero chunks of context."""

    STAGING_ROWS = 64                                                  # the pinned staging block of a pool built with max_sessions=: one mf_windows_push launch

    def __init__(self, n_sessions, batch_size, fps=50, stride_left=10, stride_right=10, chunk=320, device="cuda", max_sessions=None):
        """max_sessions (None: a fixed set of n_sessions windows, pushed as ever): buf has max_sessions rows, for sessions that come and go, and `push` takes the
        route built for a subset of the rows -- the new samples go through one pinned staging block in one asynchronous copy and ONE mf_windows_push launch
        slides the rows and writes the step's windows: no index tensor, no cat, no scatter."""
        self.batch_size, self.fps, self.l, self.r, self.chunk = int(batch_size), fps, int(stride_left), int(stride_right), int(chunk)
        self.device = torch.device(device)
        self.n_chunks = 2 * self.batch_size + self.l + self.r
        self.n, self.n_new = self.n_chunks * self.chunk, 2 * self.batch_size * self.chunk
        if max_sessions is not None and int(max_sessions) < int(n_sessions):
            raise RuntimeError(f"LipWindowPool: max_sessions={max_sessions} for {n_sessions} sessions")
        self.buf = torch.zeros((int(n_sessions if max_sessions is None else max_sessions), self.n), dtype=torch.float32, device=self.device)
        self.starts = mel_chunk_starts(self.n_chunks, self.l, self.r, fps, 1 + self.n // 200)       # the same for every row: all windows have n samples
        if len(self.starts) != self.batch_size:
            raise RuntimeError(f"{len(self.starts)} mel windows for {self.batch_size} frames: l + r + 2B chunks must give B windows (lipasr.py:24-35)")
        self.staging = None
        if max_sessions is not None:
            if self.device.type != "cuda":
                raise RuntimeError("LipWindowPool(max_sessions=) pushes through mf_windows_push and needs a HIP device; no CPU path exists here")
            # rows of the block are handed out round robin; a push waits only for the copy that last read the rows it is about to refill (`_staged`), which
            # lies a whole turn of the block back
            self.staging = torch.empty((self.STAGING_ROWS, self.n_new), dtype=torch.float32).pin_memory()
            self._stage_at, self._staged = 0, []                      # next free staging row; [(first, end, event)] of the copies that may still be reading

    def reset_row(self, k):
        """row k holds silence again, the state warm_up leaves (baseasr.py:53-59): what a joiner's window starts from.  Stream-ordered."""
        self.buf[int(k)].zero_()

    def _stage(self, blocks):
        """blocks (at most STAGING_ROWS host_blocks) -> their device copy [len(blocks), n_new], through the pinned block, one asynchronous copy"""
        m = len(blocks)
        if self._stage_at + m > self.STAGING_ROWS:
            self._stage_at = 0
        a, b = self._stage_at, self._stage_at + m
        keep = []
        for first, end, ev in self._staged:
            if first < b and a < end:
                ev.synchronize()                                      # (a copy issued a turn of the block ago: done long since)
            else:
                keep.append((first, end, ev))
        host = self.staging[a:b]
        np.stack(blocks, out=host.numpy())
        new = host.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._staged, self._stage_at = keep + [(a, b, ev)], b
        return new

    def push_rows(self, ks, blocks):
        """`push` for a pool built with max_sessions=: returns the pushed windows [len(ks), n] in the order of ks, which `mel` takes as they are"""
        ks = [int(k) for k in ks]
        if len(set(ks)) != len(ks):
            raise RuntimeError(f"push: a session appears twice in {ks}")
        if not ks or len(blocks) != len(ks):
            raise RuntimeError(f"push: {len(blocks)} blocks for {len(ks)} sessions (at least one, and one block per session)")
        bad = [k for k in ks if not 0 <= k < self.buf.shape[0]]
        if bad:
            raise RuntimeError(f"push: sessions {bad} are out of range: the pool has rows 0 to {self.buf.shape[0] - 1}")
        win = torch.empty((len(ks), self.n), dtype=torch.float32, device=self.device)
        for i in range(0, len(ks), self.STAGING_ROWS):
            part = slice(i, i + self.STAGING_ROWS)
            ops.windows_push(self.buf, ks[part], self._stage(blocks[part]), out=win[part])
        return win

    def host_block(self, new_chunks):
        """the 2B new 20 ms chunks of one session as one fp32 [2B * chunk] array; refuses anything else (before any window moves)"""
        if len(new_chunks) != 2 * self.batch_size:
            raise RuntimeError(f"expected {2 * self.batch_size} new chunks (two per frame), got {len(new_chunks)}")
        a = np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1) for c in new_chunks])
        if a.shape[0] != self.n_new:
            raise RuntimeError(f"expected chunks of {self.chunk} samples ({self.n_new} in all), got {a.shape[0]} samples")
        return a

    def rows(self, ks):
        """the windows of sessions ks as a contiguous [len(ks), n] tensor (the pool itself when ks is every session in order)"""
        ks = list(ks)
        if ks == list(range(self.buf.shape[0])):
            return self.buf
        if len(ks) == 1:
            return self.buf[ks[0]:ks[0] + 1]
        return self.buf[torch.tensor(ks, device=self.device)]

    def push(self, ks, blocks):
        """lipasr.py:17-21 + :36 for sessions ks at once: blocks[i] (host_block) is appended to session ks[i]'s window and the oldest 2B chunks fall out.
        One upload of the new samples; the l + r context moves on the device.  (A pool built with max_sessions=: push_rows, which also returns the windows.)"""
        if self.staging is not None:
            return self.push_rows(ks, blocks)
        ks = list(ks)
        if len(set(ks)) != len(ks):
            raise RuntimeError(f"push: a session appears twice in {ks}")
        # (the block is pageable host memory, so this copy is in effect synchronous; a subset of sessions also uploads a small index tensor below.  Both are
        # inside the step times of DESIGN.md section 4: a pool built with max_sessions= takes them out -- a pinned staging block, the row table in mf_windows_push's launch arguments: push_rows)
        new = torch.from_numpy(np.stack(blocks)).to(self.device, non_blocking=True)
        win = torch.cat([self.rows(ks)[:, self.n_new:], new], dim=1)
        if ks == list(range(self.buf.shape[0])):
            self.buf.copy_(win)
        elif len(ks) == 1:
            self.buf[ks[0]].copy_(win[0])
        else:
            self.buf[torch.tensor(ks, device=self.device)] = win

    def mel(self, wav):
        """wav [n_windows, n] (rows of this pool) -> every window's B mel chunks [n_windows * B, 1, 80, 16] in one launch (lipasr.py:23-35)"""
        return ops.melspec_windows(wav, self.starts, audio.PAD_MODES[audio.pad_mode])


class LipASRDeviceFrontend:
    """LipASRFrontend with the window on the device: row `row` of a LipWindowPool (LipBatcher.frontends() hands out one per session).  run_step returns what
    LipASRFrontend.run_step returns after warm_up, from an upload of the 2B new chunks only.  The window starts as warm_up leaves it; a caller that never
    warms up gets silence as context instead of the shorter first windows of lipasr.py (lipreal.py always warms up)."""

    def __init__(self, pool, row):
        self.pool, self.row = pool, int(row)
        self.batch_size, self.fps, self.l, self.r = pool.batch_size, pool.fps, pool.l, pool.r

    def warm_up(self, chunk=320):
        """baseasr.py:53-59: the context is l + r silent chunks"""
        if chunk != self.pool.chunk:
            raise RuntimeError(f"the pool was built for chunks of {self.pool.chunk} samples, not {chunk}")
        self.pool.buf[self.row].zero_()

    def run_step(self, new_chunks):
        self.pool.push([self.row], [self.pool.host_block(new_chunks)])
        return self.pool.mel(self.pool.rows([self.row]))


class LipBatcher(PooledBatcher):
    """N Wav2Lip sessions through one generator handle per step (BASELINE.json configs[3]: per-GPU batching).  The argument list is MuseBatcher's, with the
    generator in the place of the UNet / VAE pair."""

    def __init__(self, model, sessions, batch_size=16, paste=False, device="cuda", max_sessions_per_step=None, max_sessions=None, pool_rows=None):
        """max_sessions, pool_rows (both None: a fixed session list, as ever): sessions may join and leave (add_session / remove_session, serving.PooledBatcher).
        `sessions` is then a list of max_sessions slots (None: vacant) and the pool ONE allocation of pool_rows rows (default: the initial sessions' rows) whose
        address never changes; a step still holds at most max_sessions_per_step sessions (default here: the initial number)."""
        self.model, self.sessions, self.batch_size, self.paste = model, list(sessions), int(batch_size), bool(paste)
        self.device = torch.device(device)
        if not self.sessions:
            raise RuntimeError("LipBatcher needs at least one session")
        # more sessions than one step holds: step(..., only=[...]) serves a subset (LipSessionScheduler)
        self.max_sessions_per_step = len(self.sessions) if max_sessions_per_step is None else int(max_sessions_per_step)
        for k, s in enumerate(self.sessions):
            self._check_session(k, s)
        # every session's cached crops in one pool: the generator's input kernel reads a batch's faces from it by row
        self.pool = self._build_pool(max_sessions, pool_rows)
        self.window_pool = None

    @staticmethod
    def _check_session(k, s):
        if s.faces.dtype != torch.uint8 or s.faces.dim() != 4 or tuple(s.faces.shape[1:]) != (96, 96, 3):
            raise RuntimeError(f"session {k}: the cached crops must be uint8 [n,96,96,3], got {s.faces.dtype} {tuple(s.faces.shape)}")
        if s.avatar_frames is not None and s.avatar_frames.n != s.length:
            raise RuntimeError(f"session {k}: one cached full frame per cached crop is required (frame_list_cycle / face_list_cycle)")

    @staticmethod
    def _session_rows(s):
        return s.faces

    def frontends(self, fps=50, stride_left=10, stride_right=10):
        """One LipASRDeviceFrontend per session over a window pool this batcher owns (created here, once).  Sessions that come and go: the pool has a window for
        every slot and pushes through mf_windows_push (LipWindowPool(max_sessions=)); a vacant slot's entry is None."""
        if self.window_pool is None:
            self.window_pool = LipWindowPool(len(self.live()), self.batch_size, fps, stride_left, stride_right, device=self.device,
                                             max_sessions=None if self.row_pool is None else len(self.sessions))
        elif (self.window_pool.fps, self.window_pool.l, self.window_pool.r) != (fps, stride_left, stride_right):
            raise RuntimeError("this batcher's window pool was built with another fps / stride")
        return [None if s is None else LipASRDeviceFrontend(self.window_pool, k) for k, s in enumerate(self.sessions)]

    @torch.no_grad()
    def prewarm(self, tune=False):
        """Everything a step size costs the FIRST time -- the eager forward, the hipGraph capture and (tune=True) the launch-configuration measurement -- for every
        number of sessions a step can hold (k * B frames), so that the serving loop never meets a new batch size.  Session state is left untouched.
        A Wav2Lip handle has no max_batch: its workspace grows with the largest batch it has seen, and growing drops every captured graph.  So the LARGEST step
        runs first, once, and the sizes are then warmed inside a workspace that no longer moves."""
        B = self.batch_size
        top = self.max_sessions_per_step * B
        mel = torch.zeros((top, 1, 80, 16), dtype=torch.float32, device=self.device)
        self.model.forward_u8_rows(mel, self.pool, [0] * top)              # sizes the handle
        self._prewarm_sizes(tune, lambda n: self.model.forward_u8_rows(mel[:n], self.pool, [0] * n), lambda n: self.model.tune(n))

    def step(self, mel_chunks, only=None):
        """mel_chunks: per session a device tensor [B, 1, 80, 16] or None (silent); frames: fp32 [B, 96, 96, 3] (`pred * 255`, lipreal.py:126), pasted: uint8 BGR"""
        return super().step(mel_chunks, only)

    def _check_input(self, k, ch):
        B = self.batch_size
        if not torch.is_tensor(ch) or tuple(ch.shape) != (B, 1, 80, 16) or ch.device.type != self.device.type:
            what = f"{tuple(ch.shape)} on {ch.device}" if torch.is_tensor(ch) else type(ch).__name__
            raise RuntimeError(f"session {k}: expected a tensor [{B}, 1, 80, 16] of mel chunks on {self.device}, got {what}")

    def _forward(self, mels, rows):
        return self.model.forward_u8_rows(self.cat_inputs(mels), self.pool, rows)      # lipreal.py:109-126, once for everybody


class LipSessionScheduler(SessionScheduler):
    """serving.SessionScheduler over a LipBatcher: submit(k, mel_chunks [B, 1, 80, 16] or None, t_arrival).  Period default: B x 40 ms (lipreal.py's 25 fps)."""


class LipEndToEndScheduler(PipelinedScheduler):
    """The whole per-GPU Wav2Lip session loop: what reaches a session's `process_frames` thread, from what its ASR thread saw.

      lipasr.py:14-37     submit(k, chunks, t): the 2B new 20 ms PCM chunks of session k.  When the batch is picked its samples are uploaded and its window slides
                          on the device (LipWindowPool.push, all picked sessions at once); the windows of ALL speaking sessions go through ONE
                          mf_melspec_windows launch
      lipreal.py:96-137   LipBatcher.step for the picked sessions: one forward_u8_rows, silent batches only advance the walk
      lipreal.py:207-214  paste-back on the device (batcher built with paste=True)
      lipreal.py:104,136  each session's B (res_frame, idx, audio_frames[2i:2i+2]) tuples leave through ITS FrameRing

    Everything else (picking, reservation, deferral episodes in `ring_full`, publish order, the waiter thread, close(), single_stream) is PipelinedScheduler's code.
    A window slides when its batch is PICKED, not when it is submitted, and once (`_advance`): it is one device row per session, and several batches may be queued."""

    def __init__(self, batcher, frontends=None, rings=None, period_s=None, hold_s=None, clock=time.perf_counter, depth=2, single_stream=False, frame_format="packed",
                 idle_frames=False):
        fes = batcher.frontends() if frontends is None else list(frontends)
        if len(fes) != len(batcher.sessions):                             # before anything (streams, the parent's state) is created
            raise RuntimeError("one LipASRDeviceFrontend per session is required")
        live = live_sessions(batcher)
        pool = fes[live[0]].pool if isinstance(fes[live[0]], LipASRDeviceFrontend) else None
        for k, fe in enumerate(fes):
            if k not in live and fe is None:                              # (a vacant slot of a batcher whose sessions come and go)
                continue
            if not isinstance(fe, LipASRDeviceFrontend) or fe.pool is not pool or fe.row != k or fe.batch_size != batcher.batch_size:
                raise RuntimeError(f"frontend {k}: one LipASRDeviceFrontend per session, row k of one pool, is required (LipBatcher.frontends())")
        if getattr(batcher, "row_pool", None) is not None and (pool.staging is None or pool.buf.shape[0] < len(batcher.sessions)):
            raise RuntimeError(f"LipEndToEndScheduler: a batcher whose sessions come and go needs a window for every slot: LipWindowPool(..., "
                               f"max_sessions={len(batcher.sessions)}) (LipBatcher.frontends())")
        if frame_format == "i420" and not batcher.paste:
            raise RuntimeError("LipEndToEndScheduler: frame_format='i420' converts the pasted uint8 frames; the batcher was built with paste=False (fp32 crops)")
        super().__init__(batcher, rings=rings, period_s=period_s, hold_s=hold_s, clock=clock, depth=depth, single_stream=single_stream, frame_format=frame_format,
                         idle_frames=idle_frames)
        self.frontends, self.windows = fes, pool

    def submit(self, k, pcm_chunks, t_arrival=None):
        """pcm_chunks: the batch's 2B 20 ms chunks (serving.split_batch).  An all-silent batch skips the network (lipreal.py:96-105): its B (None, idx,
        audio_frames) tuples still reach the ring, and its samples still enter the window (lipasr.py:17-21 does not look at the type)."""
        self._check_slot(k, "submit")
        chunks, pairs, types = split_batch(pcm_chunks, "LipEndToEndScheduler.submit")
        block = self.windows.host_block(chunks)                          # refuses a malformed batch here, before it is queued
        super().submit(k, {"block": block, "silent": all_silent(types)}, t_arrival, pairs)

    def _advance(self, ks, batches):
        if self.windows.staging is None:
            self.windows.push(ks, [batches[k]["block"] for k in ks])     # lipasr.py:17-21 + :36: the picked sessions' windows slide, one upload
            return
        # sessions that come and go: one mf_windows_push launch slides the rows and writes the step's windows, the speaking sessions' first -- they are what the
        # mel launch of _inputs takes, as they lie.  A batch keeps its window (a view) for a retry.
        order = [k for k in ks if not batches[k]["silent"]] + [k for k in ks if batches[k]["silent"]]
        win = self.windows.push(order, [batches[k]["block"] for k in order])
        for i, k in enumerate(order):
            batches[k]["win"] = (win, i)

    def _step_windows(self, speaking, batches):
        """the windows of the speaking sessions as one [len(speaking), n] tensor"""
        if self.windows.staging is None:
            return self.windows.rows(speaking)
        wins = [batches[k]["win"] for k in speaking]
        if all(w is wins[0][0] and i == j for j, (w, i) in enumerate(wins)):
            return wins[0][0][:len(speaking)]                            # one push, speaking sessions first: no copy
        return torch.stack([w[i] for w, i in wins])                      # (a retried step whose sessions were pushed by different launches)

    def _check_join(self, k, session, ring, frontend):
        if frontend is not None:
            raise RuntimeError("LipEndToEndScheduler: add_session makes the joiner's LipASRDeviceFrontend itself (row k of the scheduler's window pool): frontend=None")
        if self.windows.staging is None or k >= self.windows.buf.shape[0]:
            raise RuntimeError(f"LipEndToEndScheduler: add_session needs a window pool with a row for slot {k} (LipWindowPool(..., max_sessions=))")
        super()._check_join(k, session, ring, frontend)

    def _store(self, k, session, ring, frontend):
        super()._store(k, session, ring, frontend)
        self.windows.reset_row(k)                                        # silence, as warm_up leaves it (baseasr.py:53-59)
        self.frontends[k] = LipASRDeviceFrontend(self.windows, k)

    def _drop(self, k):
        super()._drop(k)
        self.frontends[k] = None

    def _inputs(self, ks, batches, dev):
        chunks = [None] * len(self.queues)
        speaking = sorted(k for k in ks if not batches[k]["silent"])
        if speaking:
            B = self.batcher.batch_size
            mel = self.windows.mel(self._step_windows(speaking, batches))  # every speaking session's B chunks in one launch
            for i, k in enumerate(speaking):
                chunks[k] = mel[i * B:(i + 1) * B]
        return chunks
