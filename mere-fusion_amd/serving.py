"""The model-agnostic part of serving many sessions from one GPU: what muse_driver, lip_driver and nerf_serving share.

  mirror_index, SessionWalk, split_batch, all_silent   the ping-pong walk over an avatar's cached frames; a submitted batch of PCM chunks taken apart
  step_sessions, PooledBatcher                         a batcher step's `only=` handling; the step and prewarm loop of a batcher with its frames in one pool
  pick_sessions, SessionScheduler, PipelinedScheduler  the per-GPU serving loop, and the same with steps in flight and delivery through FrameRings: a model's
                                                       scheduler adds `submit`, what advancing its audio state means (`_advance`) and the batcher's `_inputs`
Nothing here knows a model; a batcher is anything with `sessions`, `batch_size`, `max_sessions_per_step`, `device` and `step(inputs, only=)`."""
import queue
import threading
import time
import weakref
from collections import deque

import torch

from .transport import i420_shape, is_i420_shape


def refuse(who, msg):
    raise RuntimeError(f"{who}: {msg}")


def mirror_index(size, index):
    """`__mirror_index` (musereal.py:44-50, lipreal.py:65-72, basereal.py:133-139; provider.py:276-283): ping-pong walk over the cached frames."""
    turn, res = divmod(index, size)
    return res if turn % 2 == 0 else size - res - 1


def choose_frames(pairs, idx, custom_index, custom_lengths):
    """What each frame of one batch shows, decided per FRAME as the reference's `process_frames` does (lipreal.py:198-205, musereal.py:229-236).  pairs: the
    batch's 2B (pcm, type) pairs, two per frame; idx: its B walk indices; custom_index: the dict the deployment's `BaseReal` holds ({audiotype: frames shown so
    far}), read, NOT modified; custom_lengths: {audiotype: n_frames} of the custom videos.  Returns (choices, increments):
      choices      one entry per frame -- ("speech", idx_i): the generated frame; ("idle", idx_i): the avatar's cached frame idx_i; ("custom", audiotype, j): frame
                   j = mirror_index(n, custom_index[audiotype] + the custom frames of that type earlier in this batch) of that video
      increments   {audiotype: custom frames shown}: what the caller adds to custom_index once the batch is on its way (a batch that is retried moves it once)
    A frame is non-speech when BOTH of its chunks have type != 0; its audiotype is the FIRST chunk's; a custom video is used when custom_index.get(audiotype) is not
    None."""
    B = len(idx)
    if len(pairs) != 2 * B:
        refuse("choose_frames", f"{len(pairs)} (pcm, type) pairs for {B} frames (two per frame)")
    choices, inc = [], {}
    for i in range(B):
        t0, t1 = pairs[2 * i][1], pairs[2 * i + 1][1]
        if t0 != 0 and t1 != 0:                                      # lipreal.py:198
            if custom_index.get(t0) is not None:                     # :199-203
                if t0 not in custom_lengths:
                    refuse("choose_frames", f"custom_index names audio type {t0!r}, but no custom video of that type is attached (types: {sorted(custom_lengths)})")
                choices.append(("custom", t0, mirror_index(custom_lengths[t0], custom_index[t0] + inc.get(t0, 0))))
                inc[t0] = inc.get(t0, 0) + 1
            else:
                choices.append(("idle", idx[i]))                     # :205
        else:
            choices.append(("speech", idx[i]))
    return choices, inc


class SessionWalk:
    """A session's place in the ping-pong walk over its `length` cached frames (the session sets it), and where those frames start in its batcher's pool.
    custom_videos: the session's paste.CustomVideos, or None (attach_custom_videos checks their size against the avatar's frames)."""
    index, pool_offset, custom_videos = 0, None, None

    def attach_custom_videos(self, custom_videos):
        av = getattr(self, "avatar_frames", None)
        if custom_videos is not None and av is not None:
            custom_videos.check_size(av.H, av.W, type(self).__name__)
        self.custom_videos = custom_videos

    def next_indices(self, n):
        """the next n indices of the walk; the walk moves on (silent batch or spoken one: musereal.py:82-97, lipreal.py:102-105, 112-114)"""
        idx = [mirror_index(self.length, self.index + i) for i in range(n)]
        self.index += n
        return idx


def split_batch(pcm_chunks, who):
    """One submitted batch -- bare arrays (all speech, type 0) or (chunk, type) pairs exactly as `get_audio_frame` hands them out (baseasr.py:33-45; type 1 =
    silence, above 1 = a custom video's audio) -> (the chunks, the (chunk, type) pairs that travel with the frames, the types)."""
    pairs = [(c if isinstance(c, tuple) else (c, 0)) for c in pcm_chunks]
    if any(len(p) != 2 for p in pairs):
        refuse(who, "expected chunks or (chunk, type) pairs")
    return [c for c, _ in pairs], pairs, [ty for _, ty in pairs]


def all_silent(types):
    return all(ty != 0 for ty in types)                              # musereal.py:82-86, lipreal.py:96-105: no type-0 chunk, the networks are skipped


class RowPool:
    """First-fit allocator of contiguous row ranges in a pool of `capacity` rows: where a session's cached frames live in a batcher's pool while sessions come and
    go.  alloc(n) takes the LOWEST gap that holds n rows; free(offset) returns a range and joins it to the gaps beside it.  Nothing is ever moved: a joiner that
    fits nowhere is refused, and the caller sizes the pool (`pool_rows`).  Deterministic, no torch."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        if self.capacity < 1:
            refuse("RowPool", f"capacity {capacity} (at least one row)")
        self.gaps, self.taken = [(0, self.capacity)], {}             # gaps: (offset, length), sorted, never adjacent; taken: {offset: length}

    def alloc(self, n):
        n = int(n)
        if n < 1:
            refuse("RowPool", f"alloc({n}): at least one row")
        for i, (off, length) in enumerate(self.gaps):
            if length >= n:
                self.gaps[i:i + 1] = [(off + n, length - n)] if length > n else []
                self.taken[off] = n
                return off
        refuse("RowPool", f"no gap of {n} rows: the largest free gap has {self.largest_gap()} of {self.capacity} rows ({self.used()} in use)")

    def free(self, offset):
        if offset not in self.taken:
            refuse("RowPool", f"free({offset}): no range starts there (ranges start at {sorted(self.taken)})")
        n = self.taken.pop(offset)
        gaps = sorted(self.gaps + [(offset, n)])
        self.gaps = gaps[:1]
        for off, length in gaps[1:]:
            last_off, last_len = self.gaps[-1]
            if last_off + last_len == off:
                self.gaps[-1] = (last_off, last_len + length)
            else:
                self.gaps.append((off, length))

    def used(self):
        return sum(self.taken.values())

    def largest_gap(self):
        return max((length for _, length in self.gaps), default=0)


def live_sessions(batcher):
    """the occupied session slots of a batcher (one without `live()` has none vacant)"""
    live = getattr(batcher, "live", None)
    return list(live()) if callable(live) else list(range(len(batcher.sessions)))


def step_sessions(batcher, inputs, only, skip_none=True):
    """The `only=` handling of a batcher step.  inputs: one entry per session; only: session numbers that take part (None: all).  Returns (picked, active):
    the sessions whose state moves in this step, and those of them that reach the networks (skip_none: a None input is a silent batch and does not).  Refuses a
    list of another length, a session number out of range and more active sessions than a step holds -- all before anything moves.  A vacant slot of a batcher
    whose sessions come and go is absent: never picked, refused in `only`, and its input must be None."""
    who, n_sessions, capacity = type(batcher).__name__, len(batcher.sessions), batcher.max_sessions_per_step
    if len(inputs) != n_sessions:
        refuse(who, f"{len(inputs)} entries for {n_sessions} sessions")
    take = None if only is None else set(int(k) for k in only)
    if take is not None and (min(take, default=0) < 0 or max(take, default=0) >= n_sessions):
        refuse(who, f"only={sorted(take)}: session numbers run from 0 to {n_sessions - 1}")
    live = set(live_sessions(batcher))
    if len(live) != n_sessions:
        vacant = [k for k in range(n_sessions) if k not in live]
        if take is not None and take - live:
            refuse(who, f"only={sorted(take)}: slots {sorted(take - live)} are vacant (live sessions: {sorted(live)})")
        full = [k for k in vacant if inputs[k] is not None]
        if full:
            refuse(who, f"slots {full} are vacant: their entries must be None (live sessions: {sorted(live)})")
    picked = [k for k in range(n_sessions) if k in live and (take is None or k in take)]
    active = [k for k in picked if inputs[k] is not None] if skip_none else picked
    if len(active) > capacity:
        refuse(who, f"{len(active)} active sessions in one step; a step holds {capacity} x {batcher.batch_size} frames")
    return picked, active


class PooledBatcher:
    """N sessions (SessionWalks) through one set of handles per step, every session's cached frames in one pool.  A model's batcher says: _check_input(k, x), which
    refuses session k's input if the forward cannot take it; _forward(xs, rows): the active sessions' inputs (`cat_inputs` joins them) and pool rows -> frames."""

    frame_order = "bgr"                                                  # channel 0 of the uint8 frames a step returns (Wav2Lip and MuseTalk: cv2's order)

    row_pool = None                                                      # the RowPool of a batcher whose sessions come and go (max_sessions= / pool_rows=)

    def session_hw(self, session):
        """(H, W) of a session's pasted frames; None where the size is not known before a step (paste=False)"""
        av = session.avatar_frames if self.paste else None
        return None if av is None else (av.H, av.W)

    def frame_hw(self, k):
        """session_hw of session k"""
        return self.session_hw(self.sessions[k])

    def live(self):
        """the occupied slot numbers"""
        return [k for k, s in enumerate(self.sessions) if s is not None]

    def _build_pool(self, max_sessions, pool_rows):
        """The pool of the constructor's sessions (each already through `_check_session`).  max_sessions and pool_rows both None: the sessions' rows (`_session_rows`)
        concatenated, as many rows as they have.  Otherwise ONE allocation of pool_rows rows (default: what the initial sessions need) that lives as long as the
        batcher -- captured graphs and prewarmed handles may hold its address -- with the sessions laid out by a RowPool (first fit from an empty pool: the
        offsets of the concatenation), and `sessions` becomes a list of max_sessions slots, None where vacant."""
        if max_sessions is None and pool_rows is None:
            self._lay_out_pool()
            return torch.cat([self._session_rows(s).to(self.device) for s in self.sessions], dim=0).contiguous()
        who, need = type(self).__name__, sum(s.length for s in self.sessions)
        max_sessions = len(self.sessions) if max_sessions is None else int(max_sessions)
        pool_rows = need if pool_rows is None else int(pool_rows)
        if max_sessions < len(self.sessions):
            refuse(who, f"max_sessions={max_sessions} for {len(self.sessions)} initial sessions")
        if pool_rows < need:
            refuse(who, f"pool_rows={pool_rows}: the {len(self.sessions)} initial sessions have {need} rows")
        self.row_pool = RowPool(pool_rows)
        first = self._session_rows(self.sessions[0])
        pool = torch.zeros((pool_rows,) + tuple(first.shape[1:]), dtype=first.dtype, device=self.device)
        for s in self.sessions:
            s.pool_offset = self.row_pool.alloc(s.length)
            pool[s.pool_offset:s.pool_offset + s.length].copy_(self._session_rows(s))
        self.sessions = self.sessions + [None] * (max_sessions - len(self.sessions))
        return pool

    def vacant_slot(self):
        """the slot the next add_session takes: the lowest vacant one.  Refuses a batcher built for a fixed session list, and a full one."""
        who = type(self).__name__
        if self.row_pool is None:
            refuse(who, f"add_session: this batcher was built for a fixed list of sessions; {who}(..., max_sessions=, pool_rows=) makes room for joiners")
        for k, s in enumerate(self.sessions):
            if s is None:
                return k
        refuse(who, f"add_session: all {len(self.sessions)} session slots are taken (max_sessions)")

    def add_session(self, session):
        """A session joins: the lowest vacant slot, `session.length` rows of the pool (RowPool: the lowest gap that fits), its rows copied there on the current
        stream -- stream-ordered, so a step enqueued after this call reads them and nothing waits.  The same checks as the constructor's, for this one session;
        refused before anything changes.  No forward, no tune, no capture: the handles are sized by max_sessions_per_step, not by who is here.  Returns the slot."""
        k = self.vacant_slot()
        self._check_session(k, session)
        rows = self._session_rows(session)
        off = self.row_pool.alloc(session.length)                         # (refuses with the largest free gap; nothing has changed yet)
        self.pool[off:off + session.length].copy_(rows, non_blocking=True)
        session.pool_offset = off
        self.sessions[k] = session
        return k

    def remove_session(self, k):
        """Session k leaves: its rows and its slot are free for a joiner.  The caller knows that no step still reads them (a scheduler waits for the session's
        last batch in flight).  Returns the session object."""
        who = type(self).__name__
        if self.row_pool is None:
            refuse(who, f"remove_session: this batcher was built for a fixed list of sessions; {who}(..., max_sessions=, pool_rows=) lets sessions come and go")
        k = int(k)
        if not 0 <= k < len(self.sessions) or self.sessions[k] is None:
            refuse(who, f"remove_session({k}): no session there (live sessions: {self.live()})")
        s = self.sessions[k]
        self.row_pool.free(s.pool_offset)
        self.sessions[k], s.pool_offset = None, None
        return s

    def idle_source(self, k, i):
        """the device view of session k's cached full frame i, uint8 [H, W, 3] in `frame_order`: what the session shows while it listens"""
        av = self.sessions[k].avatar_frames
        if av is None:
            raise RuntimeError(f"session {k} has no AvatarFrames: no idle frame to show")
        return av.source(i)

    def _lay_out_pool(self):
        for k, s in enumerate(self.sessions):                            # every session's first row in the pool its frames are concatenated into
            s.pool_offset = sum(t.length for t in self.sessions[:k])

    @staticmethod
    def cat_inputs(xs):
        return xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)

    def _prewarm_sizes(self, tune, forward, measure):
        for k in range(1, self.max_sessions_per_step + 1):
            n = k * self.batch_size
            for it in range(3 if tune else 2):                             # eager (+ table lookup), [tune + eager], capture: tune drops the graph, so the
                forward(n)                                                 # capture that follows records the measured configurations
                if tune and it == 0:
                    measure(n)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    @torch.no_grad()
    def step(self, inputs, only=None):
        """inputs: one entry per session -- what the forward takes for B frames, or None for an all-silent batch (musereal.py:82-86, lipreal.py:102-105: the net
        is skipped, only the frame indices advance).  Returns one (frames, indices) per session: frames = B frames on the device -- with paste=True the composed
        full frames [B, H, W, 3] (musereal.py:238-247, lipreal.py:207-214) -- or None for a silent session.  only: session numbers that take part; every other
        session is left untouched (its index does not move, its entry is None, its input is not looked at): sessions on their own clocks do not all have a batch."""
        B = self.batch_size
        picked, active = step_sessions(self, inputs, only)
        for k in active:                                                 # every input is checked BEFORE any session's frame index moves
            self._check_input(k, inputs[k])
            if self.paste and self.sessions[k].avatar_frames is None:
                raise RuntimeError(f"session {k} has no AvatarFrames to paste into")
        out, rows = [None] * len(self.sessions), []
        for k in picked:                                                 # musereal.py:82-97, lipreal.py:102-105, 134-137: silent or not, the walk advances by B
            s = self.sessions[k]
            idx = s.next_indices(B)
            out[k] = (None, idx)
            if inputs[k] is not None:
                rows.extend(s.pool_offset + i for i in idx)
        if not active:
            return out
        frames = self._forward([inputs[k] for k in active], rows)        # once for everybody
        for j, k in enumerate(active):
            fr, idx = frames[j * B:(j + 1) * B], out[k][1]
            if self.paste:
                fr = self.sessions[k].avatar_frames.paste(fr, idx)        # one launch per session (sizes differ between avatars)
            out[k] = (fr, idx)
        return out


def pick_sessions(pending, now, capacity, hold):
    """Which sessions share the next step.  pending: {session number: arrival time of its OLDEST queued batch}.  Oldest first (ties: lower
    session number); a step goes out as soon as `capacity` sessions wait, or once the oldest batch has waited `hold` seconds -- a partly
    filled step costs almost what a full one does (the UNet is latency-bound at 8 frames), so a short hold buys throughput and
    its cost is bounded by `hold`.  Returns [] while it is better to wait.  Pure host logic (tests/test_muse_driver.py runs it on the CPU)."""
    if not pending or capacity < 1:
        return []
    order = sorted(pending, key=lambda k: (pending[k], k))
    if len(order) >= capacity or now - pending[order[0]] >= hold:
        return order[:capacity]
    return []


class SessionScheduler:
    """Serving loop of one GPU over a batcher, for sessions that arrive on their own clocks (one batch of B frames per B * 40 ms of audio each,
    musereal.py:53-58 / basereal's 25 fps pacing): queues every session's batches, picks which sessions share the next step (oldest first, up to the handle's
    capacity; a short hold lets a step fill), and stamps every batch's arrival -> frames-ready latency.  bench.py's `paced_sessions` leg measures
    BASELINE.json's "max concurrent >= 25 fps sessions" with it (p99 batch latency <= B * 40 ms) instead of dividing a free-running rate by 25.

    submit(k, inputs, t_arrival)   queue one batch of session k (inputs: what the batcher's step takes for one session, or None = silent batch)
    run_once(now)                  if pick_sessions says so, run ONE batcher step for the picked sessions, wait for its frames and
                                   return [(k, frames, indices, latency_s)]; [] when nothing is due
    next_due()                     the time at which run_once would act on what is queued now (None: nothing queued)
    A session's batches are served in arrival order, one per step (its frame indices are consecutive: musereal.py:92-97)."""

    def __init__(self, batcher, period_s=None, hold_s=None, clock=time.perf_counter, sync=None):
        self.batcher = batcher
        self.capacity = batcher.max_sessions_per_step
        self.period = batcher.batch_size * 0.040 if period_s is None else float(period_s)          # B frames at 25 fps
        self.hold = self.period / 4 if hold_s is None else float(hold_s)
        self.clock = clock
        self.sync = sync if sync is not None else (lambda: torch.cuda.synchronize(batcher.device))
        live = set(live_sessions(batcher))
        self.queues = [deque() if k in live else None for k in range(len(batcher.sessions))]       # (None: a vacant slot of a batcher whose sessions come and go)
        self.leaving = set()                                         # slots whose session has been removed and still has a batch in flight
        self.steps = 0
        self.sessions_served = 0
        self.busy_s = 0.0

    # ---- sessions that come and go (a batcher built with max_sessions= / pool_rows=) -------------------------------------------------------------------
    def _check_slot(self, k, what):
        """refuses `what` on a slot that is vacant or whose session is leaving"""
        if not 0 <= k < len(self.queues) or self.queues[k] is None:
            refuse(type(self).__name__, f"{what}({k!r}): no session there (live sessions: {[j for j, q in enumerate(self.queues) if q is not None]})")
        if k in self.leaving:
            refuse(type(self).__name__, f"{what}({k}): the session is leaving (remove_session was called; its last batches in flight are being delivered)")

    def add_session(self, session, ring=None, frontend=None):
        """A client connects: the session joins the batcher (PooledBatcher.add_session: the lowest vacant slot, its rows copied into the pool on the current
        stream; no forward, no capture) and gets a queue; ring / frontend are what the constructor takes per session.  Everything the constructor checks for a
        session and its ring is checked for this one, before anything is stored.  Returns the slot number k the caller submits to."""
        k = self.batcher.vacant_slot()
        self._check_join(k, session, ring, frontend)
        got = self.batcher.add_session(session)
        if got != k:
            refuse(type(self).__name__, f"add_session: the batcher put the session into slot {got}, not {k}")
        self._store(k, session, ring, frontend)
        self.queues[k] = deque()
        return k

    def flush(self, k):
        """The `pause_talk` of the batched path (lipreal.py:187-189, baseasr.py:30-31): drops session k's queued batches that have not been picked and returns how
        many.  Batches in flight are delivered; the frame walk and `custom_index` have not moved for a dropped batch and do not move."""
        self._check_slot(k, "flush")
        return self._flush(k)

    def _flush(self, k):
        n = len(self.queues[k])
        self.queues[k].clear()
        return n

    def remove_session(self, k):
        """A client goes: its queued batches are dropped (flush) and the slot is LEAVING -- nothing can be submitted to it, and it is not offered to add_session --
        until the session's last batch in flight has retired.  Only then are its pool rows, its slot and what the scheduler holds for it released: with steps in
        flight one of them may still read those rows, and a joiner's rows must not be copied over them."""
        self._check_slot(k, "remove_session")
        self._flush(k)
        self.leaving.add(k)
        self._release_left()

    def _release_left(self):
        for k in sorted(self.leaving):
            if not self._in_flight(k):
                self.leaving.discard(k)
                self.queues[k] = None
                self._drop(k)
                self.batcher.remove_session(k)

    def _in_flight(self, k):
        return False                                                 # (run_once waits for its step)

    def _check_join(self, k, session, ring, frontend):
        if ring is not None or frontend is not None:
            refuse(type(self).__name__, "add_session: this scheduler delivers no frames through rings and runs no audio stage (ring=None, frontend=None)")

    def _store(self, k, session, ring, frontend):
        pass

    def _drop(self, k):
        pass

    def submit(self, k, inputs, t_arrival=None):
        self._check_slot(k, "submit")
        self.queues[k].append((self.clock() if t_arrival is None else t_arrival, inputs))

    def pending(self):
        return {k: q[0][0] for k, q in enumerate(self.queues) if q}

    def backlog(self):
        return max((len(q) for q in self.queues if q is not None), default=0)

    def next_due(self):
        p = self.pending()
        if not p:
            return None
        t = sorted(p.values())
        return t[self.capacity - 1] if len(t) >= self.capacity else t[0] + self.hold

    def run_once(self, now=None):
        now = self.clock() if now is None else now
        ks = pick_sessions(self.pending(), now, self.capacity, self.hold)
        if not ks:
            return []
        chunks = [None] * len(self.queues)
        arrival = {}
        for k in ks:
            arrival[k], chunks[k] = self.queues[k].popleft()
        t0 = self.clock()
        out = self.batcher.step(chunks, only=ks)
        self.sync()
        t1 = self.clock()
        self.steps += 1
        self.sessions_served += len(ks)
        self.busy_s += t1 - t0
        return [(k, out[k][0], out[k][1], t1 - arrival[k]) for k in ks]


class PipelinedScheduler(SessionScheduler):
    """The whole per-GPU session loop in one place, for any model: what reaches a session's `process_frames` thread, from what its ASR
    thread saw.  A step is: pick -> reserve ring places -> the model's audio stage -> batcher.step -> each session's frames leave through ITS FrameRing as
    (res_frame, idx, audio_frames) tuples (musereal.py:116,153; lipreal.py:104,136): the D2H runs on a copy stream behind the step (the next step's kernels do
    not wait for it) and the descriptors are published when its event is done.  run_once(now) -> finished batches [(k, frames_or_None, indices, latency_s)]:
    latency = arrival -> descriptors published (rings given) or frames complete in HBM (rings=None).  With rings=None or single_stream=True no stream is created.
    frame_format="i420": each session's uint8 [B, H, W, 3] block is converted to planar YUV 4:2:0 (ops.frames_to_i420, the batcher's `frame_order`) on the step's
    stream right before its begin_batch, so the rings (built with transport.i420_shape) and the D2H carry 1.5 bytes per pixel and the consumer's line is
    `VideoFrame.from_ndarray(frame, format="yuv420p")`; run_once then reports those frames.  Nothing else changes: silent batches still travel as None.
    idle_frames=True (default False: nothing changes): EVERY tuple a ring carries holds a finished frame in the ring's format.  The choice the reference's
    `process_frames` makes per frame (lipreal.py:198-205, musereal.py:229-236: a frame whose two chunks are both non-speech shows the avatar's cached frame, or
    a frame of a custom video) is made here (`choose_frames`), and the chosen frames are written by ops.gather_frames on the step's stream: a batch that generated
    nothing (silent, or a context that is still filling) gets a new block of B frames filled by one gather -- a frame typed speech for which nothing was generated
    shows the cached frame idx, where the reference drops it -- and in a batch that did, the non-speech frames of the delivered block are overwritten (after the I420
    conversion).  Needs rings, a batcher with `idle_source(k, i)` that pastes, and AvatarFrames on every session; a session's custom videos are its
    `custom_videos` (paste.CustomVideos).  THE WALK: the scheduler owns `custom_index`, the deployment only resets it.  It moves once per batch, after every
    begin_batch of the step has succeeded, so a batch whose step raises and is retried moves it once.  A `set_curr_state(audiotype, reinit=True)` or
    `init_customindex()` on the deployment's side is seen by the next batch PICKED: up to `depth` batches already in flight keep the old walk."""

    FRAME_FORMATS = ("packed", "i420")

    def __init__(self, batcher, rings=None, period_s=None, hold_s=None, clock=time.perf_counter, depth=2, single_stream=False, frame_format="packed",
                 idle_frames=False):
        self._check_frame_format(batcher, rings, frame_format)       # before anything (streams, the parent's state) is created
        if idle_frames:
            self._check_idle_frames(batcher, rings)
        super().__init__(batcher, period_s=period_s, hold_s=hold_s, clock=clock)
        self.rings = None if rings is None else list(rings)         # (a list of its own: add_session / remove_session change entries)
        self.frame_format = frame_format
        self.idle_frames = bool(idle_frames)
        self.depth = max(int(depth), 1)                              # steps in flight: the one computing + the one whose frames are being copied
        # single_stream: a model's audio stage, the step and the D2H of its frames all on the caller's stream -- no cross-stream event wait anywhere (with handles
        # created under MF_NO_GRAPH=2 the whole rank is one launch chain: no runtime thread spins, see mf_musetalk.hip); costs the copy / Whisper overlap
        self.single_stream = bool(single_stream)
        self.copy_stream = torch.cuda.Stream(device=batcher.device) if rings is not None and not self.single_stream else None
        self.inflight = deque()
        # The serving loop SLEEPS between steps (polling run_once at 2 - 5 kHz was part of the 1.3 - 1.9 host cores a rank cost at
        # capacity): every step's event goes to one waiter thread that does nothing but hipEventQuery it every 0.5 ms and then sets `_wake`; the loop sleeps
        # in idle_wait() until then or until the next arrival is due.  (Not hipEventSynchronize: on ROCm 7.2 it spins a full core for as long as the GPU is
        # busy, with or without the blocking-sync event flag, and hipDeviceScheduleBlockingSync hangs on this driver: tools/host_wait_probe.py.)
        self._wake = threading.Event()
        self._evq = queue.SimpleQueue()
        self._waiter = None                                          # started by the first step: a scheduler that never steps owns no thread
        self.waiter_errors = []                                      # exceptions hipEventQuery raised in the waiter (a device error is not a completion)
        self.ring_full = 0                                           # deferral EPISODES (a session found its ring full), not polls
        self._deferred = {}                                          # session -> time at which it is offered again even if its ring still looks full
        self._busy_until = 0.0

    @classmethod
    def _check_frame_format(cls, batcher, rings, frame_format):
        """frame_format "i420": every session's rings carry planar YUV 4:2:0 slots (transport.i420_shape) and the batcher says which channel its frames start with
        (`frame_order`).  A ring of another slot shape is refused HERE, not at the first copy.  "packed" (the default) checks nothing: the frames leave as they are."""
        who = cls.__name__
        if frame_format not in cls.FRAME_FORMATS:
            refuse(who, f"frame_format must be one of {cls.FRAME_FORMATS}, got {frame_format!r}")
        if frame_format == "packed":
            return
        if rings is None:
            refuse(who, "frame_format='i420' is what the rings carry; without rings the frames stay packed in HBM")
        if getattr(batcher, "frame_order", None) not in ("bgr", "rgb"):
            refuse(who, f"frame_format='i420': {type(batcher).__name__} does not state its frames' channel order (frame_order = 'bgr' or 'rgb')")
        if len(rings) != len(batcher.sessions):
            refuse(who, f"{len(rings)} rings for {len(batcher.sessions)} sessions")
        frame_hw = getattr(batcher, "frame_hw", None)
        for k in live_sessions(batcher):
            cls._check_session_format(k, rings[k], frame_hw(k) if frame_hw is not None else None)

    @classmethod
    def _check_session_format(cls, k, ring, hw):
        """frame_format "i420", one session: ring k carries the planes of session k's frames (hw: their size where it is known before a step).  The constructor
        runs it for every session, add_session for the joiner."""
        who = cls.__name__
        have = tuple(getattr(ring, "frame_shape", ()))
        if hw is not None and (hw[0] % 2 or hw[1] % 2):
            refuse(who, f"frame_format='i420': session {k}'s frames are {hw[0]} x {hw[1]} (H x W); 4:2:0 needs even sizes")
        if hw is not None and have != i420_shape(*hw):
            refuse(who, f"frame_format='i420': ring {k} has slots of shape {have}; session {k}'s {hw[0]} x {hw[1]} frames need {i420_shape(*hw)} "
                        f"(FrameRing(slots, transport.i420_shape(H, W)))")
        if not is_i420_shape(have):
            refuse(who, f"frame_format='i420': ring {k} has slots of shape {have}, which is no [H * 3 / 2, W] plane block (FrameRing(slots, transport.i420_shape(H, W)))")

    @classmethod
    def _check_idle_frames(cls, batcher, rings):
        """idle_frames=True: what the gather needs is there before a step runs -- a ring to deliver into, a batcher that hands out its sessions' cached frames
        and pastes (the frame size of a batch that runs no network must be known), custom videos of the avatar's size"""
        who, name = cls.__name__, type(batcher).__name__
        if rings is None:
            refuse(who, "idle_frames=True fills the tuples the rings carry; without rings a silent batch stays None")
        if len(rings) != len(batcher.sessions):
            refuse(who, f"{len(rings)} rings for {len(batcher.sessions)} sessions")
        if not callable(getattr(batcher, "idle_source", None)):
            refuse(who, f"idle_frames=True: {name} has no idle_source(k, i) (cached full frames to show while a session listens)")
        if getattr(batcher, "frame_order", None) not in ("bgr", "rgb"):
            refuse(who, f"idle_frames=True: {name} does not state its frames' channel order (frame_order = 'bgr' or 'rgb')")
        if not getattr(batcher, "paste", False):
            refuse(who, f"idle_frames=True: {name} was built with paste=False; the frames of a batch that runs no network have the pasted frames' size")
        for k in live_sessions(batcher):
            cls._check_session_idle(k, batcher.sessions[k], batcher.frame_hw(k) if callable(getattr(batcher, "frame_hw", None)) else None)

    @classmethod
    def _check_session_idle(cls, k, session, hw):
        """idle_frames=True, one session: its frame size is known before a step and its custom videos have that size (constructor and add_session)"""
        who = cls.__name__
        if hw is None:
            refuse(who, f"idle_frames=True: session {k} has no AvatarFrames (its frame size is not known before a step)")
        cv = getattr(session, "custom_videos", None)
        if cv is not None:
            cv.check_size(hw[0], hw[1], f"{who}: session {k}")

    def _check_join(self, k, session, ring, frontend):
        """what the constructor checks for a session and its ring, for the joiner (slot k): before anything is stored"""
        who, bat = type(self).__name__, self.batcher
        if (ring is None) != (self.rings is None):
            refuse(who, "add_session: a ring per session, as the scheduler was built (rings=None: none)")
        hw = bat.session_hw(session) if callable(getattr(bat, "session_hw", None)) else None
        if self.frame_format == "i420":
            self._check_session_format(k, ring, hw)
        if self.idle_frames:
            self._check_session_idle(k, session, hw)

    def _store(self, k, session, ring, frontend):
        if self.rings is not None:
            self.rings[k] = ring

    def _drop(self, k):
        if self.rings is not None:
            self.rings[k] = None
        self._deferred.pop(k, None)

    def _flush(self, k):
        self._deferred.pop(k, None)                                  # (an empty queue has no deferred batch)
        return super()._flush(k)

    def _in_flight(self, k):
        return any(k in item["ks"] for item in self.inflight)

    def _finish_frames(self, ks, out, audio):
        """idle_frames: every picked session's block of B finished frames in the ring's format, on the step's stream (one gather per session that has a non-speech
        or ungenerated frame).  Returns {session: (custom_index, increments)}: the moves of the custom walks, applied by the caller once the step is on its way."""
        from . import ops
        bat, moves = self.batcher, {}
        B, dev = bat.batch_size, bat.device
        for k in ks:
            fr, idx = out[k]
            cv = getattr(bat.sessions[k], "custom_videos", None)
            ci, lengths = ({}, {}) if cv is None else (cv.custom_index, cv.lengths)
            choices, inc = choose_frames(audio[k], idx, ci, lengths)
            srcs, dst = [], []
            for i, c in enumerate(choices):
                if c[0] == "custom":
                    srcs.append(cv.source(c[1], c[2]))
                elif c[0] == "idle" or fr is None:                   # (typed speech, nothing generated: a context that is still filling shows the cached frame)
                    srcs.append(bat.idle_source(k, c[1]))
                else:
                    continue
                dst.append(i)
            if fr is None:
                H, W = bat.frame_hw(k)
                fr = torch.empty((B,) + (i420_shape(H, W) if self.frame_format == "i420" else (H, W, 3)), dtype=torch.uint8, device=dev)
            if srcs:
                ops.gather_frames(srcs, dst, fr, fmt=self.frame_format, order=bat.frame_order)
            out[k] = (fr, idx)
            if inc:
                moves[k] = (ci, inc)
        return moves

    def _delivered(self, fr):
        """the frames of one session as they enter its ring: as they are, or (frame_format "i420") converted on the step's stream, one launch for the block"""
        if fr is None or self.frame_format == "packed":
            return fr
        from . import ops
        return ops.frames_to_i420(fr, order=self.batcher.frame_order)

    @staticmethod
    def _wait_loop(evq, wake, errors):
        """The waiter holds the queue, the wake flag and the error list -- NOT the scheduler: an abandoned scheduler (no close()) is collected with its batcher,
        rings and GPU handles, and its finaliser below stops this thread."""
        while True:
            ev = evq.get()
            if ev is None:
                return
            try:
                while not ev.query():
                    time.sleep(5e-4)
            except Exception as e:                                   # recorded, then the loop is woken: _retire's own query raises the same error to the caller
                errors.append(e)
            wake.set()

    def _start_waiter(self):
        if self._waiter is None:
            self._waiter = threading.Thread(target=PipelinedScheduler._wait_loop, args=(self._evq, self._wake, self.waiter_errors), daemon=True)
            self._waiter.start()
            weakref.finalize(self, self._evq.put, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def idle_wait(self, timeout):
        """Sleeps until a step in flight completes or `timeout` seconds have passed, whichever is first (nothing in flight: a plain sleep).  What a serving
        loop calls between run_once()s instead of polling."""
        if timeout is None or timeout <= 0:
            return
        if self.inflight:
            self._wake.wait(timeout)
            self._wake.clear()
        else:
            time.sleep(timeout)

    def close(self):
        """stops the waiter thread (after drain(); `with ...Scheduler(...) as sch:` calls it)"""
        if self._waiter is not None:
            self._evq.put(None)
            self._waiter.join(timeout=2.0)
            self._waiter = None

    def submit(self, k, payload, t_arrival=None, pairs=()):
        """(a model's submit takes PCM chunks and ends here.)  A queue entry is (arrival, (payload, pairs)); a third item marks a batch that has advanced"""
        if self.idle_frames and len(pairs) != 2 * self.batcher.batch_size:
            refuse(type(self).__name__ + ".submit", f"idle_frames=True chooses every frame from its two (pcm, type) pairs: {len(pairs)} pairs for "
                                                    f"{self.batcher.batch_size} frames")
        self._check_slot(k, "submit")
        self.queues[k].append((self.clock() if t_arrival is None else t_arrival, (payload, list(pairs))))

    def _retire(self, block=False):
        done = []
        while self.inflight:
            item = self.inflight[0]
            if block:
                item["event"].synchronize()
            elif not item["event"].query():
                break
            self.inflight.popleft()
            t1 = self.clock()
            for k in item["ks"]:
                fr, idx = item["out"][k]
                tok = item["tokens"].get(k)
                if tok is not None:
                    # speech: the B frames' descriptors; a silent batch or a session whose context is still filling: B (None, idx, audio_frames[2i:2i+2])
                    # tuples as the reference puts them (musereal.py:82-86, lipreal.py:104) -- ONE message either way, on slots reserved before the step
                    # started, so nothing here can block the scheduler thread
                    self.rings[k].commit_batch(tok, item["audio"][k])
                    t1 = self.clock()
                done.append((k, fr, idx, t1 - item["arrival"][k]))
            self.busy_s += max(t1 - max(item["t0"], self._busy_until), 0.0)      # union of the steps' [launch, done] intervals
            self._busy_until = max(self._busy_until, t1)
        if self.leaving:                                                 # a removed session's last batch has retired: its rows, slot and ring go now
            self._release_left()
        return done

    def pending(self):
        """Sessions whose oldest batch can be picked now.  A session deferred because its ring was full is left out until the ring reports B free slots or a
        back-off of a quarter period has passed (it otherwise sits at the head of the order with an arrival time in the past, next_due() lies in the
        past, the serving loop spins a host core on run_once, and its age makes every other session's step launch partly filled)."""
        p = super().pending()
        if self._deferred:
            now, B = self.clock(), self.batcher.batch_size
            for k in list(self._deferred):
                if k not in p:
                    del self._deferred[k]
                elif self.rings[k].free_slots() >= B or now >= self._deferred[k]:
                    del self._deferred[k]                            # (a new episode is counted if it is deferred again)
                else:
                    del p[k]
        return p

    def next_due(self):
        """when run_once would next act on what is QUEUED (None: nothing queued).  Steps in flight do not enter: idle_wait() wakes the loop when one completes."""
        t = super().next_due()
        if self._deferred:
            t_def = min(self._deferred.values())
            t = t_def if t is None else min(t, t_def)
        return t

    def run_once(self, now=None):
        now = self.clock() if now is None else now
        done = self._retire()
        if len(self.inflight) >= self.depth:
            return done
        ks = pick_sessions(self.pending(), now, self.capacity, self.hold)
        if not ks:
            return done
        dev = self.batcher.device
        # Ring slots for every picked session are taken BEFORE anything irreversible happens (queue entries popped, frame indices and ASR state advanced): a
        # session whose consumer is behind is DEFERRED -- its batch stays at the head of its queue and is picked again later -- and the other sessions go ahead;
        # the reference's loop likewise back-pressures only the one session's queue.
        reserved = {}
        if self.rings is not None:
            B = self.batcher.batch_size
            pend = self.pending()
            ok = []
            try:
                for k in sorted(pend, key=lambda k_: (pend[k_], k_)):     # oldest first; a waiting session takes the place of one that has to be deferred
                    if len(ok) == len(ks):
                        break
                    sl = self.rings[k].try_reserve(B)                     # (silent batches too: their B (None, idx, audio) tuples take B of the ring's places)
                    if sl is None:
                        self.ring_full += 1
                        self._deferred[k] = now + self.period / 4
                        continue
                    reserved[k] = sl
                    ok.append(k)
            except BaseException:
                for k in list(reserved):                                  # a ring that raised (closed, torn down) must not leave the others' places open
                    self.rings[k].unreserve(reserved[k])
                raise
            ks = ok
            if not ks:
                return done
        # Everything from here to the last begin_batch sits in ONE try: the rings publish in begin order, so a reservation left open by an exception anywhere
        # on the way (the queue pop, the H2D copy, the audio stage, the step, a begin_batch) would wedge its ring for good -- every later batch queued behind
        # an entry that never completes.  On any exception the reservations go back and the popped batches return to the HEAD of their queues.
        arrival, audio, wins, tokens, popped, advanced, moves = {}, {}, {}, {}, [], set(), {}
        try:
            for k in ks:
                item = self.queues[k].popleft()
                popped.append((k, item))
                arrival[k], (wins[k], audio[k]) = item[:2]
                advanced.update([k] * (len(item) > 2))
            t0 = self.clock()
            chunks = self._audio_stage(ks, wins, dev, advanced)
            out = self.batcher.step(chunks, only=ks)
            ev = torch.cuda.Event()
            if self.rings is not None:
                cur = torch.cuda.current_stream(dev)
                for k in ks:                                             # (i420: each session's block is converted on the step's stream, before the copy stream waits)
                    out[k] = (self._delivered(out[k][0]), out[k][1])
                if self.idle_frames:                                     # (every block complete on the step's stream: begin_batch below always gets frames)
                    moves = self._finish_frames(ks, out, audio)
                if self.copy_stream is not None:
                    self.copy_stream.wait_stream(cur)
                for k in ks:
                    fr, idx = out[k]
                    tokens[k] = self.rings[k].begin_batch(fr, idx, stream=self.copy_stream, reserved=reserved.pop(k))   # (fr None: B silent frames)
                    if fr is not None and self.copy_stream is not None:
                        fr.record_stream(self.copy_stream)
                ev.record(self.copy_stream if self.copy_stream is not None else cur)
        except BaseException:
            # nothing of this step is published: tokens already begun and reservations not yet used go back (the rings publish in begin order whatever order
            # this happens in)
            for k in list(tokens):
                self.rings[k].abort_batch(tokens[k])
            for k in list(reserved):
                self.rings[k].unreserve(reserved[k])
            for k, item in reversed(popped):                       # the batches of this step are not lost: they are picked again
                self.queues[k].appendleft(item[:2] + (True,) if k in advanced else item)
            raise
        if self.rings is None:
            ev.record(torch.cuda.current_stream(dev))
        for ci, inc in moves.values():                                   # the custom walks move ONCE per batch: only here, behind everything that can raise
            for ty, n in inc.items():
                if ci.get(ty) is not None:                               # (a video the deployment has detached since the choice: nothing to move)
                    ci[ty] += n
        self.inflight.append({"ks": ks, "out": out, "tokens": tokens, "audio": audio, "arrival": arrival, "event": ev, "t0": t0})
        self._start_waiter()
        self._evq.put(ev)
        self.steps += 1
        self.sessions_served += len(ks)
        return done

    def _audio_stage(self, ks, wins, dev, advanced=None):
        """The audio front end of one step: wins[k] is the payload submit() queued for session k.  Returns the batcher's per-session input list.
        ADVANCE ONCE: a batch whose step failed returns to the HEAD of its session's queue marked as advanced (`advanced`: those sessions) -- its session's audio
        state (Wav2Lip's window, ER-NeRF's features) has moved on for it already and must not move again.  No other batch of that session can be picked in between
        (a session's batches are served in queue order), so the state it meets on the retry is still its own.  (MuseTalk's window slides at submit(), on arrival.)"""
        advanced = set() if advanced is None else advanced
        todo = sorted(k for k in ks if k not in advanced)
        if todo:
            self._advance(todo, wins)
            advanced.update(todo)
        return self._inputs(ks, wins, dev)

    def _advance(self, ks, payloads):
        """move the audio state of sessions ks (sorted) on by their batches; once per batch, when it is first picked.  What it computes is kept in the payload"""

    def _inputs(self, ks, payloads, dev):
        """the batcher's input list (None for every session that is silent or not picked); runs on every try of a batch.  Here: the payload is the input"""
        return [payloads.get(k) for k in range(len(self.queues))]

    def drain(self):
        """Waits for everything in flight (end of a run)."""
        return self._retire(block=True)
