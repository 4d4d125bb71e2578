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
  LipSessionScheduler                    muse_driver.SessionScheduler over a LipBatcher (mel chunks in, frames out)
  LipEndToEndScheduler                   muse_driver.EndToEndScheduler with the Wav2Lip audio stage: PCM chunks in, (res_frame, idx, audio_frames) tuples out
                                         of each session's FrameRing; pacing, silence, back-pressure and delivery are the inherited code
"""
import time

import numpy as np
import torch

from . import ops
from .muse_driver import EndToEndScheduler, SessionScheduler, pick_sessions  # noqa: F401  (pick_sessions: the policy both models' schedulers share)
from .wav2lip import audio


def mirror_index(size, index):
    """Ping-pong walk over the cached face crops (lipreal.py:65-72, basereal.py:133-139)."""
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


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


class LipSession:
    """One talking-head session: cached uint8 face crops on the device + the generator.  With `avatar_frames`
    (mere_fusion_amd.paste.AvatarFrames built from frame_list_cycle / coord_list_cycle with lip_order=True) `step_pasted` also does
    process_frames' paste-back (lipreal.py:207-214) on the device."""

    def __init__(self, model, faces_u8, avatar_frames=None):
        self.model = model
        self.faces = faces_u8 if torch.is_tensor(faces_u8) else torch.from_numpy(np.asarray(faces_u8))
        self.faces = self.faces.to(next(model.parameters()).device)
        self.avatar_frames = avatar_frames
        self.index = 0
        self.length = self.faces.shape[0]
        self.pool_offset = None                                     # first row of this session's crops in a LipBatcher's pool

    def next_indices(self, n):
        """the next n face indices of the ping-pong walk; the walk moves on (lipreal.py:102-105 for a silent batch, :112-114 for a spoken one)"""
        idx = [mirror_index(self.length, self.index + i) for i in range(n)]
        self.index += n
        return idx

    def step(self, mel_batch):
        """lipreal.py:109-137 for one non-silent batch: returns fp32 frames [B,96,96,3] (pred*255) and
        the face indices they belong to; process_frames truncates with astype(uint8) (lipreal.py:211)."""
        B = mel_batch.shape[0]
        n = self.faces.shape[0]
        idx = [mirror_index(n, self.index + i) for i in range(B)]
        self.index += B
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

    def __init__(self, n_sessions, batch_size, fps=50, stride_left=10, stride_right=10, chunk=320, device="cuda"):
        self.batch_size, self.fps, self.l, self.r, self.chunk = int(batch_size), fps, int(stride_left), int(stride_right), int(chunk)
        self.device = torch.device(device)
        self.n_chunks = 2 * self.batch_size + self.l + self.r
        self.n, self.n_new = self.n_chunks * self.chunk, 2 * self.batch_size * self.chunk
        self.buf = torch.zeros((int(n_sessions), self.n), dtype=torch.float32, device=self.device)
        self.starts = mel_chunk_starts(self.n_chunks, self.l, self.r, fps, 1 + self.n // 200)       # the same for every row: all windows have n samples
        if len(self.starts) != self.batch_size:
            raise RuntimeError(f"{len(self.starts)} mel windows for {self.batch_size} frames: l + r + 2B chunks must give B windows (lipasr.py:24-35)")

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
        One upload of the new samples; the l + r context moves on the device."""
        ks = list(ks)
        if len(set(ks)) != len(ks):
            raise RuntimeError(f"push: a session appears twice in {ks}")
        # (the block is pageable host memory, so this copy is in effect synchronous; a subset of sessions also uploads a small index tensor below.  Both are
        # inside the step times of DESIGN.md section 4: pinned staging buffers and a device-side row table are what is left to take out of them)
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


class LipBatcher:
    """N Wav2Lip sessions through one generator handle per step (BASELINE.json configs[3]: per-GPU batching).  The argument list is MuseBatcher's, with the
    generator in the place of the UNet / VAE pair."""

    def __init__(self, model, sessions, batch_size=16, paste=False, device="cuda", max_sessions_per_step=None):
        self.model, self.sessions, self.batch_size, self.paste = model, list(sessions), int(batch_size), bool(paste)
        self.device = torch.device(device)
        if not self.sessions:
            raise RuntimeError("LipBatcher needs at least one session")
        # more sessions than one step holds: step(..., only=[...]) serves a subset (LipSessionScheduler)
        self.max_sessions_per_step = len(self.sessions) if max_sessions_per_step is None else int(max_sessions_per_step)
        off = 0
        for k, s in enumerate(self.sessions):
            if s.faces.dtype != torch.uint8 or s.faces.dim() != 4 or tuple(s.faces.shape[1:]) != (96, 96, 3):
                raise RuntimeError(f"session {k}: the cached crops must be uint8 [n,96,96,3], got {s.faces.dtype} {tuple(s.faces.shape)}")
            if s.avatar_frames is not None and s.avatar_frames.n != s.length:
                raise RuntimeError(f"session {k}: one cached full frame per cached crop is required (frame_list_cycle / face_list_cycle)")
            s.pool_offset = off
            off += s.length
        # every session's cached crops in one pool: the generator's input kernel reads a batch's faces from it by row
        self.pool = torch.cat([s.faces.to(self.device) for s in self.sessions], dim=0).contiguous()
        self.window_pool = None

    def frontends(self, fps=50, stride_left=10, stride_right=10):
        """One LipASRDeviceFrontend per session over a window pool this batcher owns (created here, once)."""
        if self.window_pool is None:
            self.window_pool = LipWindowPool(len(self.sessions), self.batch_size, fps, stride_left, stride_right, device=self.device)
        elif (self.window_pool.fps, self.window_pool.l, self.window_pool.r) != (fps, stride_left, stride_right):
            raise RuntimeError("this batcher's window pool was built with another fps / stride")
        return [LipASRDeviceFrontend(self.window_pool, k) for k in range(len(self.sessions))]

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
        for k in range(1, self.max_sessions_per_step + 1):
            n = k * B
            for it in range(3 if tune else 2):                             # eager (+ table lookup), [tune + eager], capture: tune drops the graph, so the
                self.model.forward_u8_rows(mel[:n], self.pool, [0] * n)    # capture that follows records the measured configurations
                if tune and it == 0:
                    self.model.tune(n)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    @torch.no_grad()
    def step(self, mel_chunks, only=None):
        """mel_chunks: one entry per session -- a device tensor [B, 1, 80, 16] (LipASRFrontend.run_step / melspec_windows) or None for an all-silent batch
        (lipreal.py:102-105: the net is skipped, only the face indices advance).  Returns one (frames, indices) per session: frames = fp32 [B, 96, 96, 3]
        (`pred * 255`, lipreal.py:126) or, with paste=True, the composed uint8 BGR full frames [B, H, W, 3] (lipreal.py:207-214); None for a silent session.
        only: session numbers that take part in this step; every other session is left untouched (its index does not move, its entry is None)."""
        B = self.batch_size
        if len(mel_chunks) != len(self.sessions):
            raise RuntimeError(f"{len(mel_chunks)} entries for {len(self.sessions)} sessions")
        take = None if only is None else set(int(k) for k in only)
        if take is not None and (min(take, default=0) < 0 or max(take, default=0) >= len(self.sessions)):
            raise RuntimeError(f"only={sorted(take)}: session numbers run from 0 to {len(self.sessions) - 1}")
        picked = [k for k in range(len(self.sessions)) if take is None or k in take]
        active = [k for k in picked if mel_chunks[k] is not None]
        if len(active) > self.max_sessions_per_step:
            raise RuntimeError(f"{len(active)} active sessions in one step; a step holds {self.max_sessions_per_step} x {B} frames")
        for k in active:                                                 # every input is checked BEFORE any session's face index moves
            ch = mel_chunks[k]
            if not torch.is_tensor(ch) or tuple(ch.shape) != (B, 1, 80, 16) or ch.device.type != self.device.type:
                what = f"{tuple(ch.shape)} on {ch.device}" if torch.is_tensor(ch) else type(ch).__name__
                raise RuntimeError(f"session {k}: expected a tensor [{B}, 1, 80, 16] of mel chunks on {self.device}, got {what}")
            if self.paste and self.sessions[k].avatar_frames is None:
                raise RuntimeError(f"session {k} has no AvatarFrames to paste into")
        out = [None] * len(self.sessions)
        rows = []
        for k in picked:                                                 # lipreal.py:102-105, 134-137: silent or not, the walk advances by B
            s = self.sessions[k]
            idx = s.next_indices(B)
            out[k] = (None, idx)
            if mel_chunks[k] is not None:
                rows.extend(s.pool_offset + i for i in idx)
        if not active:
            return out
        mel = mel_chunks[active[0]] if len(active) == 1 else torch.cat([mel_chunks[k] for k in active], dim=0)
        frames = self.model.forward_u8_rows(mel, self.pool, rows)      # lipreal.py:109-126, once for everybody
        for j, k in enumerate(active):
            fr, idx = frames[j * B:(j + 1) * B], out[k][1]
            if self.paste:
                fr = self.sessions[k].avatar_frames.paste(fr, idx)        # lipreal.py:207-214, one launch per session (sizes differ between avatars)
            out[k] = (fr, idx)
        return out


class LipSessionScheduler(SessionScheduler):
    """muse_driver.SessionScheduler over a LipBatcher: submit(k, mel_chunks [B, 1, 80, 16] or None, t_arrival), run_once(now), next_due() -- the same queues,
    the same pick_sessions policy, one batch of B frames per session and step.  Period default: B x 40 ms (25 fps, lipreal.py / basereal's pacing)."""


class LipEndToEndScheduler(EndToEndScheduler):
    """The whole per-GPU Wav2Lip session loop: what reaches a session's `process_frames` thread, from what its ASR thread saw.

      lipasr.py:14-37     submit(k, chunks, t): the 2B new 20 ms PCM chunks of session k.  When the batch is picked its samples are uploaded and its window slides
                          on the device (LipWindowPool.push, all picked sessions at once); the windows of ALL speaking sessions go through ONE
                          mf_melspec_windows launch
      lipreal.py:96-137   LipBatcher.step for the picked sessions: one forward_u8_rows, silent batches only advance the walk
      lipreal.py:207-214  paste-back on the device (batcher built with paste=True)
      lipreal.py:104,136  each session's B (res_frame, idx, audio_frames[2i:2i+2]) tuples leave through ITS FrameRing

    Everything else -- pick_sessions, try_reserve before anything irreversible, deferral episodes in `ring_full`, publish order, the waiter thread started by the
    first step, close() / the context manager, single_stream -- is EndToEndScheduler's code, unchanged.  A window slides when its batch is
    PICKED, not when it is submitted: the window is one device row per session, and a session may have several batches queued."""

    def __init__(self, batcher, frontends=None, rings=None, period_s=None, hold_s=None, clock=time.perf_counter, depth=2, single_stream=False):
        fes = batcher.frontends() if frontends is None else list(frontends)
        for k, fe in enumerate(fes):                                      # before anything (streams, the parent's state) is created
            if not isinstance(fe, LipASRDeviceFrontend) or fe.pool is not fes[0].pool or fe.row != k or fe.batch_size != batcher.batch_size:
                raise RuntimeError(f"frontend {k}: one LipASRDeviceFrontend per session, row k of one pool, is required (LipBatcher.frontends())")
        super().__init__(batcher, fes, None, rings=rings, period_s=period_s, hold_s=hold_s, clock=clock, depth=depth, asr_stream=False, single_stream=single_stream)
        self.windows = fes[0].pool

    def submit(self, k, pcm_chunks, t_arrival=None):
        """pcm_chunks: the batch's 2B 20 ms chunks -- bare arrays (all speech, type 0) or (chunk, type) pairs as `get_audio_frame` hands them out (baseasr.py:33-45;
        type 1 = silence).  An all-silent batch skips the network (lipreal.py:96-105): its B (None, idx, audio_frames) tuples still reach the ring, and its samples
        still enter the window (lipasr.py:17-21 does not look at the type)."""
        t = self.clock() if t_arrival is None else t_arrival
        pairs = [(c if isinstance(c, tuple) else (c, 0)) for c in pcm_chunks]
        block = self.windows.host_block([c for c, _ in pairs])           # refuses a malformed batch here, before it is queued
        silent = all(ty != 0 for _, ty in pairs)
        self.queues[k].append((t, ({"block": block, "silent": silent, "pushed": False}, pairs)))

    def _audio_stage(self, ks, wins, dev):
        chunks = [None] * len(self.queues)
        # A batch whose step failed returns to the HEAD of its session's queue with "pushed" set: its window has slid already and must not slide again.  No other
        # batch of that session can be picked in between (a session's batches are served in queue order), so the window it meets on the retry is still its own.
        todo = sorted(k for k in ks if not wins[k]["pushed"])
        if todo:
            self.windows.push(todo, [wins[k]["block"] for k in todo])
            for k in todo:
                wins[k]["pushed"] = True
        speaking = sorted(k for k in ks if not wins[k]["silent"])
        if speaking:
            B = self.batcher.batch_size
            mel = self.windows.mel(self.windows.rows(speaking))          # every speaking session's B chunks in one launch
            for i, k in enumerate(speaking):
                chunks[k] = mel[i * B:(i + 1) * B]
        return chunks
