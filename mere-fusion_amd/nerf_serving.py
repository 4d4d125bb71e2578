"""Many ER-NeRF sessions on one GPU: the counterpart of muse_driver's and lip_driver's serving stacks for the third model the reference serves.

  NerfFeaturePool / NerfASRDeviceFrontend   the `NerfASR` state of N sessions (nerfasr.py:15-126) in one place: feature rings [N, R, dim] and attention-window
                                            histories [N, 8, dim, 16] on the device, counters and the 28-chunk PCM windows on the host.  `step` runs
                                            `run_step, run_step, get_next_feat` (nerfreal.py:139-141) for B frames of every picked session in lockstep: the
                                            windows that complete go through ONE net call and ONE mf_nerf_feat_scatter launch, and every frame's `auds` of all
                                            sessions come out of ONE mf_nerf_feat_windows launch
  NerfBatcher                               a list of NerfSessions (several may share one model object: one avatar resident once) stepped B frames each; the
                                            lip-smoothing EMA, which lives in the model, is kept per session
  NerfSessionScheduler                      serving.SessionScheduler over a NerfBatcher
  NerfEndToEndScheduler                     serving.PipelinedScheduler with the ER-NeRF audio stage: PCM chunks in, (frame, idx, audio_frames) tuples out of each
                                            session's FrameRing; picking, back-pressure, advance-once and publication are serving.py's code

`ernerf.asr.NerfASRFrontend` stays the per-session restatement of the reference these are tested against."""
import os
import time

import numpy as np
import torch

from . import ops
from .serving import PipelinedScheduler, SessionScheduler, live_sessions, refuse as _refuse, split_batch, step_sessions


def host_rows_load(rings, hist, rows, src_ring=None, src_hist=None):
    """what ops.nerf_feat_rows_load does, for a pool whose buffers are host tensors (device="cpu": the pools the CPU tests step; nothing is served from one)"""
    for t, src in ((rings, src_ring), (hist, src_hist)):
        if t is not None:
            t[list(rows)] = 0.0 if src is None else src.clone()


class NerfFeaturePool:
    """model: `HipWav2Vec2ForCTC(max_windows >= n_sessions)` or any callable that takes the raw samples [S, (m + l + r) * chunk] as a device tensor and returns an
    object with `.logits` or `.last_hidden_state` [S, T, audio_dim] on the device (normalisation is the callable's business, as with `RawProcessor`).
    A fresh pool is in the state `NerfASR.__init__` leaves; `warm_up` adds `NerfASR.warm_up()` (nerfreal.py always warms up).
    max_sessions=: rows are taken and given back while the others go on (`join`, `leave`, `warm_state`)."""

    HIST = 8                                                          # windows of one `auds` with att > 0 (nerfasr.py:77)

    def __init__(self, n_sessions, model, audio_dim, att=2, m=8, l=10, r=10, fps=50, device="cuda", max_sessions=None):
        who = "NerfFeaturePool"
        self.model, self.audio_dim, self.att = model, int(audio_dim), int(att)
        self.m, self.l, self.r, self.chunk = int(m), int(l), int(r), 16000 // fps
        if int(n_sessions) < 1:
            _refuse(who, "at least one session is required")
        # max_sessions: sessions come and go.  The buffers hold max_sessions rows, of which the first n_sessions are live, and one scratch row behind them that
        # is never handed out: `warm_state` warms it up once and `join` copies it.  `n_sessions` is the number of session rows either way.
        self.max_sessions = None if max_sessions is None else int(max_sessions)
        if self.max_sessions is not None and self.max_sessions < int(n_sessions):
            _refuse(who, f"max_sessions={max_sessions} for {n_sessions} initial sessions")
        self.n_sessions = int(n_sessions) if self.max_sessions is None else self.max_sessions
        self.vacant = set(range(int(n_sessions), self.n_sessions))
        self.scratch = None if self.max_sessions is None else self.n_sessions
        if not 1 <= self.audio_dim <= 1024:
            _refuse(who, f"audio_dim {audio_dim} (1..1024)")
        if self.m < 2 or self.l < 0 or self.r < 0 or self.l + self.r < 1:
            _refuse(who, f"m = {m}, l = {l}, r = {r}: m >= 2 and l + r >= 1 are required (with l + r == 0 nerfasr.py:117 keeps every chunk it has seen)")
        self.device = torch.device(device)
        self.feat_buffer_size = 4                                       # nerfasr.py:48
        self.R = self.feat_buffer_size * self.m
        if self.R < 16:
            _refuse(who, f"a ring of {self.R} rows cannot hold a 16-row window")
        self.total = self.m + self.l + self.r                          # chunks of one net window; also NerfASR.warm_up_steps (nerfasr.py:58)
        self.warm_up_steps = self.total
        N = self.n_sessions + (self.scratch is not None)
        self.rings = torch.zeros((N, self.R, self.audio_dim), dtype=torch.float32, device=self.device)
        self.hist = torch.zeros((N, self.HIST, self.audio_dim, 16), dtype=torch.float32, device=self.device) if self.att > 0 else None
        self.pcm = np.zeros((N, self.total, self.chunk), np.float32)
        self.frames, self.feat_buffer_idx, self.front, self.tail, self.head, self.first = [0] * N, [0] * N, [0] * N, [0] * N, [0] * N, [True] * N
        self.win_fronts = [[] for _ in range(N)]                        # ring rows the windows `att_feats` holds start at, oldest first; -1: a zero window
        for k in range(N):
            self._reset_counters(k)
        self.launches = self.net_calls = 0                              # kernel launches of this module's entries / calls of the net, since creation
        self._warm = None                                               # warm_state(): the scratch row's host state once it has been warmed up

    # ---- host state ----------------------------------------------------------------------------------------------------------------------
    def _reset_counters(self, k):
        self.pcm[k] = 0.0
        self.frames[k] = self.l                                         # nerfasr.py:35-36: l chunks of silence
        self.feat_buffer_idx[k] = 0                                     # :49
        self.front[k], self.tail[k] = self.R - 8, 8                     # :52-53
        self.head[k], self.first[k] = 4, True                           # :55: four zero windows; the first get_next_feat appends four more (:77)
        self.win_fronts[k] = [-1] * 4 if self.att > 0 else []

    def _rows(self, ks, who):
        ks = [int(k) for k in ks]
        if not ks:
            _refuse(who, "no session picked")
        if len(set(ks)) != len(ks):
            _refuse(who, f"a session appears twice in {ks}")
        if min(ks) < 0 or max(ks) >= self.n_sessions:
            _refuse(who, f"sessions {ks}: rows run from 0 to {self.n_sessions - 1}")
        if self.vacant.intersection(ks):
            _refuse(who, f"sessions {ks}: rows {sorted(self.vacant.intersection(ks))} are vacant (live rows: {self.live()})")
        return ks

    def live(self):
        """the rows that hold a session"""
        return [k for k in range(self.n_sessions) if k not in self.vacant]

    def host_block(self, chunks, n_frames):
        """the 2 * n_frames new 20 ms chunks of one session as one fp32 [2 * n_frames, chunk] array; refuses anything else (before any state moves)"""
        if len(chunks) != 2 * n_frames:
            _refuse("NerfFeaturePool", f"expected {2 * n_frames} chunks (two per frame), got {len(chunks)}")
        return np.stack([self._chunk(c) for c in chunks])

    def _chunk(self, c):
        a = np.asarray(c, dtype=np.float32).reshape(-1)
        if a.shape[0] != self.chunk:
            _refuse("NerfFeaturePool", f"expected chunks of {self.chunk} samples, got one of {a.shape[0]}")
        return a

    def _advance(self, k, chunk):
        """the host side of one `run_step` (nerfasr.py:105-117): the completed window [total * chunk] (a copy) when the net is due, else None"""
        self.pcm[k, self.frames[k]] = chunk
        self.frames[k] += 1
        if self.frames[k] < self.total:
            return None
        win = self.pcm[k].reshape(-1).copy()
        keep = self.l + self.r
        self.pcm[k, :keep] = self.pcm[k, self.total - keep:].copy()
        self.frames[k] = keep
        return win

    # ---- device state --------------------------------------------------------------------------------------------------------------------
    def _fire(self, due):
        """nerfasr.py:119-124 + 128-143 for every session whose window completed: due = [(session, window)].  One upload, one net call, one scatter."""
        if not due:
            return
        cuda = self.device.type == "cuda"
        host = torch.empty((len(due), self.total * self.chunk), dtype=torch.float32, pin_memory=cuda)
        np.stack([w for _, w in due], out=host.numpy())
        res = self.model(host.to(self.device, non_blocking=True))
        self.net_calls += 1
        logits = res.last_hidden_state if hasattr(res, "last_hidden_state") else res.logits
        if logits.dim() != 3 or logits.shape[0] != len(due) or logits.shape[2] != self.audio_dim:
            _refuse("NerfFeaturePool", f"the net returned {tuple(logits.shape)} for {len(due)} windows of audio_dim {self.audio_dim}")
        T = int(logits.shape[1])
        left, right = max(0, self.l), min(T, T - self.r + 1)          # nerfasr.py:140-141
        ks = [k for k, _ in due]
        ops.nerf_feat_scatter(logits, left, right, self.rings, ks, [self.feat_buffer_idx[k] * self.m for k in ks])
        self.launches += 1
        for k in ks:
            self.feat_buffer_idx[k] = (self.feat_buffer_idx[k] + 1) % self.feat_buffer_size

    def run_step(self, ks, chunks):
        """one `run_step` of sessions ks at once: chunks[i] is session ks[i]'s next 20 ms chunk"""
        ks = self._rows(ks, "NerfFeaturePool.run_step")
        blocks = [self._chunk(c) for c in chunks]
        if len(blocks) != len(ks):
            _refuse("NerfFeaturePool.run_step", f"{len(blocks)} chunks for {len(ks)} sessions")
        self._run_step(ks, blocks)

    def _run_step(self, ks, blocks):
        self._fire([(k, w) for k, w in ((k, self._advance(k, c)) for k, c in zip(ks, blocks)) if w is not None])

    def next_feat(self, ks, out=None):
        """`get_next_feat` of sessions ks in one launch -> [len(ks), 8 or 1, audio_dim, 16]"""
        ks = self._rows(ks, "NerfFeaturePool.next_feat")
        n_new = [(4 if self.first[k] else 1) if self.att > 0 else 1 for k in ks]                   # nerfasr.py:77: `while len(self.att_feats) < 8`
        fronts = [self.win_fronts[k] + [(self.front[k] + 2 * j) % self.R for j in range(n)] for k, n in zip(ks, n_new)]
        out = ops.nerf_feat_windows(self.rings, self.hist, ks, fronts, [self.head[k] for k in ks], n_new, self.att, out=out)
        self.launches += 1
        for k, n, f in zip(ks, n_new, fronts):
            self.front[k], self.tail[k] = (self.front[k] + 2 * n) % self.R, (self.tail[k] + 2 * n) % self.R
            self.head[k], self.first[k] = (self.head[k] + n) % self.HIST, False
            self.win_fronts[k] = f[1:] if self.att > 0 else []         # :90
        return out

    def step(self, ks, chunks, B):
        """nerfreal.py:139-141 for B frames of sessions ks in lockstep: chunks[i] holds session ks[i]'s 2B new chunks.  Returns [len(ks), B, 8 or 1, audio_dim, 16]
        (a view: entry [i, b] is contiguous).  Launches besides the net: the B window launches and one scatter per frame in which some session's net window
        completes -- ONE for sessions in phase (each session is due once per m / 2 frames; sessions that joined on a step boundary of B = m / 2 frames share it),
        whatever their number.  The scatter sits between the window launches exactly where the reference's run_step fires."""
        ks = self._rows(ks, "NerfFeaturePool.step")
        B = int(B)
        if B < 1 or len(chunks) != len(ks):
            _refuse("NerfFeaturePool.step", f"{len(chunks)} chunk blocks for {len(ks)} sessions, B = {B}")
        blocks = [self.host_block(c, B) for c in chunks]               # everything is checked before any session moves
        buf = torch.empty((B, len(ks), self.HIST if self.att > 0 else 1, self.audio_dim, 16), dtype=torch.float32, device=self.device)
        for b in range(B):
            due = []
            for k, blk in zip(ks, blocks):
                for c in (2 * b, 2 * b + 1):
                    w = self._advance(k, blk[c])
                    if w is not None:
                        due.append((k, w))
            self._fire(due)
            self.next_feat(ks, out=buf[b])
        return buf.transpose(0, 1)

    def _load_rows(self, ks, ring=None, hist=None):
        """rows ks of both buffers from one source row (None: zeros) in ONE launch (mf_nerf_feat_rows_load); nothing waits and nothing is allocated.  A pool
        on the host -- the stand-in the CPU tests step -- has no device to launch on: `host_rows_load` states the same assignment."""
        if not ks:                                                       # (reset() / warm_up() of a pool everyone has left)
            return
        (ops.nerf_feat_rows_load if self.rings.is_cuda else host_rows_load)(self.rings, self.hist, ks, ring, hist)
        self.launches += 1

    def _reset_rows(self, ks):
        for k in ks:
            self._reset_counters(k)
        self._load_rows(ks)

    def _warm_up_rows(self, ks):
        self._reset_rows(ks)
        silence = np.zeros(self.chunk, np.float32)
        for _ in range(self.warm_up_steps):
            self._run_step(ks, [silence] * len(ks))

    def reset(self, ks=None):
        """sessions ks (default: all live ones) back to the state `NerfASR.__init__` leaves"""
        ks = self.live() if ks is None else self._rows([ks] if isinstance(ks, int) else ks, "NerfFeaturePool.reset")
        self._reset_rows(ks)
        return ks

    def warm_up(self, ks=None):
        """sessions ks (one number, a list; default: all live ones) to the state `NerfASR.__init__` plus `warm_up()` leave (nerfasr.py:146-152: m + l + r
        run_steps on silence), so that a session can start again while the others go on.  (A session that JOINS takes that state from `join`, without the net.)"""
        ks = self.live() if ks is None else self._rows([ks] if isinstance(ks, int) else ks, "NerfFeaturePool.warm_up")
        self._warm_up_rows(ks)

    # ---- rows that are taken and given back (max_sessions=) ---------------------------------------------------------------------------------
    def _dynamic(self, what):
        if self.scratch is None:
            _refuse("NerfFeaturePool", f"{what}: this pool was built for a fixed list of sessions; NerfFeaturePool(..., max_sessions=) lets sessions come and go")

    def warm_state(self):
        """What `warm_up([k])` leaves in a row, computed ONCE (here, or from NerfBatcher.prewarm, before the serving loop): the scratch row runs exactly what
        warm_up runs -- S = 1 net calls on silence -- and stays as the device snapshot; the host state stands beside it.  Silence gives every joiner the same
        features, so installing this IS warm_up([k]): bit for bit where the net gives the same bits run to run."""
        self._dynamic("warm_state")
        if self._warm is None:
            s = self.scratch
            self._warm_up_rows([s])
            self._warm = dict(pcm=self.pcm[s].copy(), frames=self.frames[s], feat_buffer_idx=self.feat_buffer_idx[s], front=self.front[s], tail=self.tail[s],
                              head=self.head[s], first=self.first[s], win_fronts=list(self.win_fronts[s]))
        return self._warm

    def join(self, ks, warm=True):
        """Vacant rows ks are taken: each gets the state `warm_up` leaves (warm=False: the state `NerfASR.__init__` leaves) through ONE launch on the current
        stream -- no net call, no synchronisation, no allocation (the first join of a pool whose warm_state nobody has asked for computes it).  The caller
        knows that no step in flight still reads these rows (NerfEndToEndScheduler releases a leaver's row only when its last batch has retired)."""
        who = "NerfFeaturePool.join"
        self._dynamic("join")
        ks = [int(k) for k in ([ks] if isinstance(ks, int) else ks)]
        if not ks or len(set(ks)) != len(ks) or min(ks) < 0 or max(ks) >= self.n_sessions:
            _refuse(who, f"rows {ks}: distinct rows from 0 to {self.n_sessions - 1}")
        if set(ks) - self.vacant:
            _refuse(who, f"rows {sorted(set(ks) - self.vacant)} hold a session (vacant rows: {sorted(self.vacant)})")
        w = self.warm_state() if warm else None
        s = self.scratch
        self._load_rows(ks, self.rings[s] if warm else None, self.hist[s] if warm and self.hist is not None else None)
        for k in ks:
            if warm:
                self.pcm[k] = w["pcm"]
                self.frames[k], self.feat_buffer_idx[k], self.front[k], self.tail[k] = w["frames"], w["feat_buffer_idx"], w["front"], w["tail"]
                self.head[k], self.first[k], self.win_fronts[k] = w["head"], w["first"], list(w["win_fronts"])
            else:
                self._reset_counters(k)
            self.vacant.discard(k)
        return ks

    def leave(self, k):
        """row k is vacant again: refused by step / next_feat / run_step until a joiner takes it"""
        self._dynamic("leave")
        k = int(k)
        if not 0 <= k < self.n_sessions or k in self.vacant:
            _refuse("NerfFeaturePool.leave", f"row {k}: no session there (live rows: {self.live()})")
        self.vacant.add(k)


class NerfASRDeviceFrontend:
    """The per-session surface of `NerfASRFrontend` over row `row` of a NerfFeaturePool: put_audio_frame / run_step / get_next_feat / warm_up."""

    def __init__(self, pool, row):
        self.pool, self.row = pool, int(row)
        if not 0 <= self.row < pool.n_sessions:
            _refuse("NerfASRDeviceFrontend", f"row {row} of a pool of {pool.n_sessions} sessions")
        self.att, self.audio_dim, self.device, self.chunk, self.warm_up_steps = pool.att, pool.audio_dim, pool.device, pool.chunk, pool.warm_up_steps
        self.pending = []

    def put_audio_frame(self, frame):
        self.pending.append(np.asarray(frame, np.float32))

    def run_step(self):
        self.pool.run_step([self.row], [self.pending.pop(0) if self.pending else np.zeros(self.chunk, np.float32)])

    def get_next_feat(self):
        return self.pool.next_feat([self.row])[0]

    def warm_up(self):
        self.pool.warm_up([self.row])


class NerfBatcher:
    """The `batcher` the schedulers drive, over a list of NerfSessions.  batch_size 4 is one wav2vec2 cadence (m / 2 frames): every picked session's net window
    completes in every step.  Sessions may share one model object; the lip-smoothing EMA `model.enc_a` (the drop-in module and the bare HipHeadRenderer keep it
    there) is then one value per session here, installed before the session's frames and read back after them.

    A step has three stages: `NerfSession.begin` for every frame of every picked session; the render jobs that leaves, grouped by model, ray count and render_kw,
    rendered `frames_per_render` at a time by ONE head call each (`render_frames`: mf_nerf_head_batch_render); `NerfSession.end` into the step's output blocks.  Each
    job carries its session's EMA value in a box the renderer reads before and writes after the frame's audio, so sessions that share a model share a head call
    and still keep their own EMA.  A session or model without these entry points, and everyone under MF_NERF_BATCH=0, takes one `step` per frame.

    frame_batch: the stages around the head call go out once per step too (nerf_driver.NerfFrameBatch, HipTorso.run_torso_batch): `begin` defers the torso image
    over the background and the custom-video frames, ONE background launch serves every frame of a render size in front of the head calls, and ONE frame-out
    launch per output size writes the finished frames -- rendered and custom-video ones -- into a block the
    sessions' [B, h, w, 3] results are views of.  Frames of unequal size never share a call (`_frame_groups`).  Same bits per frame as the per-frame launches; a
    session without `out_key` keeps them.  torso_batch: the torso branches of a head call's frames are one launch as well; off by default, because alone it
    measured faster at 64 x 64 and slower at 512 x 512 than one launch per frame (profiles/nerf_frame_batch_timing.md)."""

    MAX_FRAMES_PER_RENDER = 64          # mf_nerf_head_batch's limit per call
    frame_order = "rgb"                 # channel 0 of the uint8 frames a step returns (mf_nerf_frame_out)

    def frame_hw(self, k):
        """(H, W) of session k's frames"""
        return self.out_shape[k][:2]

    @staticmethod
    def session_hw(s):
        """(H, W) of a session's frames, in the batcher or about to join"""
        return (int(s.fullbody_frames.shape[1]), int(s.fullbody_frames.shape[2])) if s.fullbody_frames is not None else (s.GH, s.GW)

    def __init__(self, sessions, batch_size=4, pool=None, device="cuda", max_sessions_per_step=None, frames_per_render=32, frame_batch=True, torso_batch=False,
                 max_sessions=None, max_pixels=None):
        """max_sessions= (and max_pixels=): sessions come and go (add_session / remove_session).  `sessions`, `enc_a` and `out_shape` are then
        lists of max_sessions slots, None where vacant, and everything a running step uses is sized by the limits, not by who is here: a head call's frame slots
        (`_most_frames`), the frame batch (max_pixels rendered pixels per frame; default: the largest initial session) and the feature pool's rows."""
        who = "NerfBatcher"
        self.sessions, self.batch_size, self.pool, self.device = list(sessions), int(batch_size), pool, torch.device(device)
        if not self.sessions:
            _refuse(who, "at least one session is required")
        if self.batch_size < 1:
            _refuse(who, f"batch_size {batch_size}")
        if int(frames_per_render) < 1:
            _refuse(who, f"frames_per_render {frames_per_render}")
        self.frames_per_render = min(int(frames_per_render), self.MAX_FRAMES_PER_RENDER)
        self.dynamic = max_sessions is not None or max_pixels is not None
        n_slots = len(self.sessions) if max_sessions is None else int(max_sessions)
        if n_slots < len(self.sessions):
            _refuse(who, f"max_sessions={max_sessions} for {len(self.sessions)} initial sessions")
        self.max_sessions_per_step = n_slots if max_sessions_per_step is None else int(max_sessions_per_step)
        if pool is not None and pool.n_sessions != n_slots:
            _refuse(who, f"a feature pool of {pool.n_sessions} rows for {n_slots} sessions")
        self.frame_batch, self.torso_batch, self._fb = bool(frame_batch), bool(torso_batch), None
        self.max_pixels = None
        self.out_shape = [self._check_session(k, s) for k, s in enumerate(self.sessions)]
        if self.dynamic:
            most = max((s.H * s.W for s in self.sessions if self._can_frame_batch(s)), default=0)
            self.max_pixels = most if max_pixels is None else int(max_pixels)
            if self.max_pixels < most:
                _refuse(who, f"max_pixels={max_pixels}: an initial session renders {most} pixels per frame")
        self.sessions += [None] * (n_slots - len(self.sessions))
        self.out_shape += [None] * (n_slots - len(self.out_shape))
        self.enc_a = [None] * n_slots

    def _check_session(self, k, s):
        """what the constructor checks for one session, and add_session for the joiner (slot k), before anything is stored: the custom-video frames have the
        size of the session's frames, the session can be stepped (the two halves with a model that renders batches, or `step`), and -- where sessions come and
        go -- its rendered frames fit the frame batch.  Returns the session's output shape."""
        who = "NerfBatcher"
        hw = (int(s.fullbody_frames.shape[1]), int(s.fullbody_frames.shape[2])) if s.fullbody_frames is not None else (s.GH, s.GW)
        for t, cycle in s.custom_img_cycle.items():
            for f in cycle:
                if tuple(f.shape[:2]) != hw:
                    _refuse(who, f"session {k}: custom_img_cycle[{t}] holds a {f.shape[1]} x {f.shape[0]} frame, the session's frames are {hw[1]} x {hw[0]} "
                                 f"(a step's {self.batch_size} frames leave as one block)")
        if not self._can_batch(s) and not callable(getattr(s, "step", None)):
            _refuse(who, f"session {k}: neither begin / end / bind_aabb over a model with render_frames nor step")
        if self.max_pixels is not None and self.frame_batch and self._can_frame_batch(s) and s.H * s.W > self.max_pixels:
            _refuse(who, f"session {k}: its frames are rendered at {s.W} x {s.H} = {s.H * s.W} pixels; the frame batch was sized for {self.max_pixels} "
                         f"(NerfBatcher(..., max_pixels=))")
        return hw + (3,)

    # ---- sessions that come and go (max_sessions=) ------------------------------------------------------------------------------------------
    def live(self):
        """the occupied slot numbers"""
        return [k for k, s in enumerate(self.sessions) if s is not None]

    def vacant_slot(self):
        """the slot the next add_session takes: the lowest vacant one.  Refuses a batcher built for a fixed session list, and a full one."""
        self._check_dynamic("add_session", "makes room for joiners")
        for k, s in enumerate(self.sessions):
            if s is None:
                return k
        _refuse("NerfBatcher", f"add_session: all {len(self.sessions)} session slots are taken (max_sessions)")

    def _check_dynamic(self, what, gain="lets sessions come and go"):
        if not self.dynamic:
            _refuse("NerfBatcher", f"{what}: this batcher was built for a fixed list of sessions; NerfBatcher(..., max_sessions=, max_pixels=) {gain}")

    def add_session(self, session):
        """A session joins: the lowest vacant slot.  The constructor's checks run for this one session and refuse before anything changes.  Nothing a running
        step uses is resized and nothing is rendered: a session over a model object that is already here meets no first-time cost; one that brings a new model
        object pays that model's (handles, workspaces, ray directions of a new size) at its first step, unless the caller ran `prewarm_session(session)` before.
        The slot's EMA starts at None: a joiner's first frame is not smoothed against a leaver's.  Returns the slot."""
        k = self.vacant_slot()
        shape = self._check_session(k, session)
        self.sessions[k], self.out_shape[k], self.enc_a[k] = session, shape, None
        return k

    def remove_session(self, k):
        """Session k leaves: its slot is free for a joiner.  The caller knows that no step still renders it (a scheduler waits for the session's last batch in
        flight).  Returns the session object."""
        self._check_dynamic("remove_session")
        k = int(k)
        if not 0 <= k < len(self.sessions) or self.sessions[k] is None:
            _refuse("NerfBatcher", f"remove_session({k}): no session there (live sessions: {self.live()})")
        s = self.sessions[k]
        self.sessions[k], self.out_shape[k], self.enc_a[k] = None, None, None
        return s

    def _check_input(self, k, inp):
        B = self.batch_size
        if not (isinstance(inp, (tuple, list)) and len(inp) == 2):
            _refuse("NerfBatcher", f"session {k}: expected (windows [{B}, 8 or 1, dim, 16], {B} audiotype pairs), got {type(inp).__name__} (ER-NeRF renders silent "
                                   f"batches too: there is no None input)")
        auds, types = inp
        if not torch.is_tensor(auds) or auds.dim() != 4 or auds.shape[0] != B or auds.shape[1] not in (1, 8) or auds.shape[3] != 16 \
                or auds.device.type != self.device.type:
            what = f"{tuple(auds.shape)} on {auds.device}" if torch.is_tensor(auds) else type(auds).__name__
            _refuse("NerfBatcher", f"session {k}: expected windows [{B}, 8 or 1, dim, 16] on {self.device}, got {what}")
        try:
            ok = len(types) == B and all(len(t) == 2 and all(int(v) == v for v in t) for t in types)
        except TypeError:
            ok = False
        if not ok:
            _refuse("NerfBatcher", f"session {k}: expected {B} (audiotype, audiotype) pairs")

    @torch.no_grad()
    def step(self, inputs, only=None):
        """inputs: one entry per session -- (windows [B, 8 or 1, dim, 16] as NerfFeaturePool.step returns them, the B frames' audiotype pairs).  Returns one
        (frames uint8 [B, h, w, 3] RGB on the device, the B mirrored indices) per session, on the caller's stream.  only: session numbers that take part; every
        other session is left untouched (index, custom-video counters and EMA do not move; its entry is None and its input is not looked at)."""
        B = self.batch_size
        picked, _ = step_sessions(self, inputs, only, skip_none=False)          # (ER-NeRF renders silent batches too)
        for k in picked:                                                 # every input is checked BEFORE any session moves
            self._check_input(k, inputs[k])
        batched = os.environ.get("MF_NERF_BATCH", "1") != "0"           # read per step; "0": one NerfSession.step per frame for everyone (A/B, cross-checks)
        out = [None] * len(self.sessions)
        jobs, ema = [], {}              # jobs: (session, frame, render job) in session order then frame order; ema: per session, the one-element box its jobs carry
        fb = batched and self.frame_batch
        ends = []                       # frame_batch: (session, slot of the frame in its size's block, job) for every deferred frame, custom-video ones included
        blocks = self._blocks([k for k in picked if fb and self._can_frame_batch(self.sessions[k])], inputs) if fb else {}
        try:
            # ---- begin: every frame of every picked session (loader, custom-video frames, rays, background); nothing is rendered yet
            for k in picked:
                s, (auds, types) = self.sessions[k], inputs[k]
                defer = k in blocks
                frames = blocks[k][0][blocks[k][1]:blocks[k][1] + B] if defer else torch.empty((B,) + self.out_shape[k], dtype=torch.uint8, device=auds.device)
                idx = []
                shared = hasattr(s.model, "enc_a")
                if batched and self._can_batch(s):
                    if shared:
                        ema[k] = [self.enc_a[k]]
                    for b in range(B):
                        at = (int(types[b][0]), int(types[b][1]))
                        job = s.begin(auds[b], at, defer=True) if defer else s.begin(auds[b], at, out=frames[b])
                        idx.append(s.last_index)
                        if defer:
                            ends.append((k, blocks[k][1] + b, job))
                        if isinstance(job, dict) and "custom" not in job:   # (anything else: a custom-video frame, finished in frames[b] or deferred)
                            if shared:
                                job["ema"] = ema[k]
                            jobs.append((k, b, job))
                else:                                                    # a session (or model) without the two halves: one step per frame
                    if shared:
                        s.model.enc_a = self.enc_a[k]
                    try:
                        for b in range(B):
                            s.step(auds[b], (int(types[b][0]), int(types[b][1])), out=frames[b])
                            idx.append(s.last_index)
                    finally:
                        if shared:
                            self.enc_a[k] = s.model.enc_a
                out[k] = (frames, idx)
            # ---- the deferred backgrounds: one launch per render size
            for group in self._frame_groups([(k, job) for k, _, job in jobs if job.get("bg_pending") and k in blocks], lambda s: s.bg_key()):
                for c in range(0, len(group), self._frame_batch().max_frames):
                    chunk = group[c:c + self._frame_batch().max_frames]
                    bgs = self._frame_batch().background([self.sessions[k] for k, _ in chunk], [job["mi"] for _, job in chunk])
                    for (k, job), bg in zip(chunk, bgs):
                        self.sessions[k].set_background(job, bg)
            # ---- group and render, then end into the step's output blocks
            for group in self._groups(jobs):
                s0 = self.sessions[group[0][0]]
                extra = {"torso_batch": True} if (fb and self.torso_batch and getattr(s0.model, "FRAME_BATCH", False)) else {}
                for c in range(0, len(group), self.frames_per_render):
                    chunk = group[c:c + self.frames_per_render]
                    s0.bind_aabb()
                    res = s0.model.render_frames([job for _, _, job in chunk], reserve_frames=self._most_frames(s0.model), **extra, **s0.render_kw)
                    for (k, b, job), r in zip(chunk, res):
                        if k in blocks:
                            job["image"] = r["image"]
                        else:
                            self.sessions[k].end(job, r["image"], out=out[k][0][b])
            # ---- the deferred frames: one launch per output size and run of neighbouring slots of its block
            for run in self._out_runs(ends, blocks):
                k0, slot0, _ = run[0]
                self._frame_batch().frame_out([self.sessions[k] for k, _, _ in run], [job.get("image") for _, _, job in run],
                                              [job["custom"] if "custom" in job else job["body"] for _, _, job in run], blocks[k0][0][slot0:slot0 + len(run)])
        finally:
            for k, box in ema.items():
                self.enc_a[k] = box[0]
        return out

    # ---- the stages around the head call, once per step (frame_batch) ---------------------------------------------------------------------
    @staticmethod
    def _can_frame_batch(s):
        return NerfBatcher._can_batch(s) and all(hasattr(s, n) for n in ("out_key", "bg_key", "set_background"))

    def _frame_batch(self):
        if self._fb is None:
            from .nerf_driver import NerfFrameBatch
            most = self.max_pixels if self.dynamic else max(s.H * s.W for s in self.sessions if self._can_frame_batch(s))
            self._fb = NerfFrameBatch(NerfFrameBatch.MAX_FRAMES, most)   # (sessions that come and go: sized once, by max_pixels; add_session refuses more)
        return self._fb

    def _frame_groups(self, items, key):
        """items: (session number, anything) in step order, grouped by key(session): frames of unequal size land in different calls; a group keeps the order of
        `items`, the groups the order in which their first item appears"""
        groups = {}
        for it in items:
            groups.setdefault(key(self.sessions[it[0]]), []).append(it)
        return list(groups.values())

    def _blocks(self, ks, inputs):
        """{session: (block, first slot)}: per output size one uint8 block [n * B, h, w, 3] for the n sessions of `ks` with that size; session k's B frames are the
        slots from its first slot on, so its result is a view and neighbours in `ks` of one size are neighbours in the block"""
        B, by_key = self.batch_size, {}
        for k in ks:
            by_key.setdefault(self.sessions[k].out_key(), []).append(k)
        blocks = {}
        for key, members in by_key.items():
            block = torch.empty((len(members) * B,) + self.out_shape[members[0]], dtype=torch.uint8, device=inputs[members[0]][0].device)
            for i, k in enumerate(members):
                blocks[k] = (block, i * B)
        return blocks

    def _out_runs(self, ends, blocks):
        """the deferred frames as the frame-out calls take them: per output size (one block each) in slot order, cut into runs of at most max_frames frames"""
        runs = []
        for group in self._frame_groups(ends, lambda s: s.out_key()):
            group = sorted(group, key=lambda e: e[1])
            cap = self._frame_batch().max_frames
            runs += [group[c:c + cap] for c in range(0, len(group), cap)]
        return runs

    @staticmethod
    def _can_batch(s):
        return all(hasattr(s, n) for n in ("begin", "end", "bind_aabb")) and hasattr(s.model, "render_frames")

    def _most_frames(self, model):
        """the most frames one head call over `model` can get from this batcher: what its batch handle is sized for at the first call, so that it never has to be
        rebuilt (a synchronising free of every frame slot) in the serving loop.  Where sessions come and go it does not depend on who is here"""
        if self.dynamic:
            return min(self.frames_per_render, self.batch_size * self.max_sessions_per_step)
        n = sum(1 for s in self.sessions if s.model is model and self._can_batch(s))
        return min(self.frames_per_render, self.batch_size * min(n, self.max_sessions_per_step))

    def _groups(self, jobs):
        """the step's render jobs grouped by what one batched head call shares: the model object, the ray count, render_kw (and, for a bare renderer, the session's
        box); a group keeps the order of `jobs`, the groups the order in which their first job appears"""
        groups = {}
        for k, b, job in jobs:
            s = self.sessions[k]
            key = (id(s.model), int(job["rays_o"].numel()) // 3, tuple(sorted(s.render_kw.items())), id(getattr(s, "aabb_infer", None)))
            groups.setdefault(key, []).append((k, b, job))
        return list(groups.values())

    def _prewarm_auds(self, auds, who):
        if auds is None:
            if self.pool is None:
                _refuse(who, "without a feature pool the windows of one frame must be given")
            auds = torch.zeros((self.pool.HIST if self.pool.att > 0 else 1, self.pool.audio_dim, 16), dtype=torch.float32, device=self.device)
        return auds

    @staticmethod
    def _save(s):
        return (s.index, s.last_index, s.last_audio_index, dict(s.custom_index), s.model.enc_a if hasattr(s.model, "enc_a") else None)

    @staticmethod
    def _restore(s, keep):
        s.index, s.last_index, s.last_audio_index = keep[:3]
        s.custom_index.clear()
        s.custom_index.update(keep[3])
        if hasattr(s.model, "enc_a"):
            s.model.enc_a = keep[4]

    def _prewarm_one(self, s, auds):
        keep = self._save(s)
        try:
            s.step(auds, (0, 0))
        finally:
            self._restore(s, keep)

    @torch.no_grad()
    def prewarm_session(self, session, auds=None):
        """`prewarm`'s per-session part for a session that is about to join (before add_session, outside the serving loop's step): one rendered frame, and -- for
        a session that takes the batched route -- one head call of batch_size frames over its model with the frame slots a serving step reserves, so that a
        model object the batcher has not seen builds its handles here.  The session's state is left as it was; the batcher's is not touched."""
        auds = self._prewarm_auds(auds, "NerfBatcher.prewarm_session")
        shape = self._check_session("(joining)", session)
        self._prewarm_one(session, auds)
        if self._can_batch(session) and os.environ.get("MF_NERF_BATCH", "1") != "0":
            B, keep = self.batch_size, self._save(session)
            frames = torch.empty((B,) + shape, dtype=torch.uint8, device=auds.device)
            try:
                jobs = [(b, session.begin(auds, (0, 0), out=frames[b])) for b in range(B)]
                jobs = [(b, job) for b, job in jobs if isinstance(job, dict) and "custom" not in job]
                box = [None]
                for _, job in jobs:
                    if hasattr(session.model, "enc_a"):
                        job["ema"] = box
                session.bind_aabb()
                res = session.model.render_frames([job for _, job in jobs], reserve_frames=self._most_frames(session.model), **session.render_kw)
                for (b, job), r in zip(jobs, res):
                    session.end(job, r["image"], out=frames[b])
            finally:
                self._restore(session, keep)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    @torch.no_grad()
    def prewarm(self, auds=None):
        """One rendered frame per session, so that the serving loop meets no first-time cost (ray directions per size, handles, workspaces).  Session state --
        the loader's position, custom-video counters, the EMA -- is left as it was.  auds: one frame's windows; default: zeros of the pool's shape."""
        auds = self._prewarm_auds(auds, "NerfBatcher.prewarm")
        save, restore = self._save, self._restore
        for k in self.live():
            self._prewarm_one(self.sessions[k], auds)
        if self.pool is not None and getattr(self.pool, "scratch", None) is not None:
            self.pool.warm_state()                                       # (sessions that come and go: the joiners' audio state, computed here and not at a join)
        # ... and whole steps of rendered frames through the batched route, at most max_sessions_per_step sessions each as a serving step has them (the fullest
        # slices first), so that the batch handles exist with their frame slots and every session's size has been through the batched kernels
        ks = [k for k in self.live() if self._can_batch(self.sessions[k])]
        if ks and os.environ.get("MF_NERF_BATCH", "1") != "0":
            B, cap = self.batch_size, max(1, self.max_sessions_per_step)
            inp = (auds.unsqueeze(0).expand(B, *auds.shape), [(0, 0)] * B)
            keeps, emas = [save(self.sessions[k]) for k in ks], list(self.enc_a)
            try:
                for c in range(0, len(ks), cap):
                    part = ks[c:c + cap]
                    self.step([inp if k in part else None for k in range(len(self.sessions))], only=part)
            finally:
                for k, keep in zip(ks, keeps):
                    restore(self.sessions[k], keep)
                self.enc_a = emas
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


class NerfSessionScheduler(SessionScheduler):
    """serving.SessionScheduler over a NerfBatcher: submit(k, (windows, audiotype pairs), t_arrival).  Period default: B x 40 ms (25 fps)."""


class NerfEndToEndScheduler(PipelinedScheduler):
    """The whole per-GPU ER-NeRF session loop: what reaches a session's consumer, from what its ASR thread saw.

      nerfasr.py:105-124   submit(k, chunks, t): the 2B new 20 ms PCM chunks of session k.  When the batch is picked, NerfFeaturePool.step runs the run_steps and
      nerfasr.py:75-103    get_next_feats of all picked sessions in lockstep: one net call for the windows that complete, B + 1 launches around it
      nerfreal.py:70-127   NerfBatcher.step: B frames per picked session; a frame whose two chunks carry a custom audio type is the custom-video frame (:98)
      the ring             each session's B (frame, idx, audio_frames[2i:2i+2]) tuples leave through ITS FrameRing

    ER-NeRF has no silent-batch skip: an all-silent batch renders like any other.  Everything else (picking, reservation, deferral, publish order, the waiter
    thread, close(), single_stream) is PipelinedScheduler's code.  A session's features advance when its batch is PICKED, not when it is submitted, and once."""

    def __init__(self, batcher, pool=None, rings=None, period_s=None, hold_s=None, clock=time.perf_counter, depth=2, single_stream=False, frame_format="packed"):
        pool = batcher.pool if pool is None else pool
        if not isinstance(pool, NerfFeaturePool) or pool.n_sessions != len(batcher.sessions):     # before anything (streams, the parent's state) is created
            _refuse("NerfEndToEndScheduler", "a NerfFeaturePool with one row per session of the batcher is required")
        if pool.live() != live_sessions(batcher):
            _refuse("NerfEndToEndScheduler", f"the pool's live rows {pool.live()} are not the batcher's live sessions {live_sessions(batcher)}")
        super().__init__(batcher, rings=rings, period_s=period_s, hold_s=hold_s, clock=clock, depth=depth, single_stream=single_stream, frame_format=frame_format)
        self.pool = pool

    # ---- sessions that come and go (NerfBatcher(..., max_sessions=) over NerfFeaturePool(..., max_sessions=)) ---------------------------------
    def _check_join(self, k, session, ring, frontend):
        """the constructor's checks for the joiner (slot k) and its ring, the batcher's included, before anything is stored anywhere"""
        who = type(self).__name__
        if frontend is not None:
            _refuse(who, "add_session: the audio stage is the feature pool's row of the slot (frontend=None)")
        self.pool._dynamic("NerfEndToEndScheduler.add_session")
        if k not in self.pool.vacant:
            _refuse(who, f"add_session: slot {k} is vacant in the batcher, but row {k} of the feature pool holds a session")
        hw = self.batcher._check_session(k, session)[:2]
        super()._check_join(k, session, ring, frontend)                  # (a ring as the scheduler was built; under i420 one of the frames' planes)
        if ring is not None and self.frame_format == "packed" and tuple(getattr(ring, "frame_shape", ())) != hw + (3,):
            _refuse(who, f"add_session: ring {k} has slots of shape {tuple(getattr(ring, 'frame_shape', ()))}; session {k}'s {hw[0]} x {hw[1]} frames need "
                         f"{hw + (3,)} (FrameRing(slots, (H, W, 3)))")

    def add_session(self, session, ring=None, frontend=None):
        """A client connects: everything is checked first; then row k of the feature pool takes the warmed-up state (NerfFeaturePool.join: one launch on the
        current stream, no net call, nothing waits) and the session takes slot k of the batcher.  The row was released only after the last batch of whoever
        held it before had retired (`_drop`), so no step in flight reads what the launch writes.  Returns k."""
        return super().add_session(session, ring=ring, frontend=frontend)   # (vacant_slot, _check_join, the batcher's add_session, _store: serving.py)

    def _store(self, k, session, ring, frontend):
        self.pool.join([k])
        super()._store(k, session, ring, frontend)

    def remove_session(self, k):
        """serving.SessionScheduler.remove_session; a batcher or a pool built for a fixed list refuses here, before the slot is marked as leaving"""
        self.batcher._check_dynamic("remove_session")
        self.pool._dynamic("NerfEndToEndScheduler.remove_session")
        super().remove_session(k)

    def flush(self, k):
        """serving.SessionScheduler.flush.  ER-NeRF's features advance when a batch is PICKED, so the audio of a dropped batch never enters the context: the
        session's next batch continues the windows where the last picked one left them, as if the dropped audio had not been sent (Wav2Lip's window behaves
        the same way; MuseTalk's slides at submit() and has seen it)."""
        return super().flush(k)

    def _drop(self, k):
        """called when the leaver's last batch in flight has retired (`_release_left`): only now may a joiner's launch write row k -- a batch in flight holds
        its `feats`, but the windows kernel reads non-wrapping windows as views of the ring on later frames of a step that picked the row"""
        super()._drop(k)
        self.pool.leave(k)

    def submit(self, k, pcm_chunks, t_arrival=None):
        """pcm_chunks: the batch's 2B 20 ms chunks, bare or (chunk, type) pairs (nerfasr.py:60-73; serving.split_batch).  Refused here when malformed."""
        who, B = "NerfEndToEndScheduler.submit", self.batcher.batch_size
        if not 0 <= int(k) < len(self.queues):
            _refuse(who, f"session {k}: numbers run from 0 to {len(self.queues) - 1}")
        chunks, pairs, types = split_batch(pcm_chunks, who)
        block = self.pool.host_block(chunks, B)
        try:
            types = [(int(types[2 * i]), int(types[2 * i + 1])) for i in range(B)]            # nerfreal.py:81-88
        except (TypeError, ValueError):
            _refuse(who, "audio types must be integers")
        super().submit(int(k), {"block": block, "types": types, "feats": None}, t_arrival, pairs)

    def _advance(self, ks, batches):
        feats = self.pool.step(ks, [batches[k]["block"] for k in ks], self.batcher.batch_size)
        for i, k in enumerate(ks):
            batches[k]["feats"] = feats[i]                                # kept with the batch: a retried step renders from the same windows

    def _inputs(self, ks, batches, dev):
        return [(batches[k]["feats"], batches[k]["types"]) if k in batches else None for k in range(len(self.queues))]
