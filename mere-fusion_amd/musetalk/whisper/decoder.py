"""`WhisperDecoder`: the text decoder of a Whisper checkpoint on the MI355X (`mf_whisper_decoder_*`, csrc/mf_whisper_dec.hip).

    dec = WhisperDecoder(state_dict, n_head=6, max_batch=8)       # the "decoder.*" tensors (weights.decoder_state_dict)
    dec.begin(enc)                                                # enc [B, T_audio, n_state] on the device: one segment per sequence
    logits = dec.logits(tokens)                                   # teacher-forced, appended at the caches' offset (TextDecoder.forward)
    ids, logprobs = dec.greedy(prompts, eot=50257, max_new=224)   # token ids per sequence, summed log-probabilities
    rules = DecodeRules(eot=50257, timestamp_begin=50364, no_timestamps=50363, max_initial_timestamp_index=50, blank=220, no_speech=50362, sot=50258)
    ids, logprobs, no_speech = dec.decode(prompts, rules, max_new=224)   # the same under the reference's logit filters (decoding.py:387-441)
    lang_ids, probs = dec.detect_language(50258, language_token_ids)     # directly after begin(); the handle stands as after begin() again

There is no CPU path: without a HIP device the constructor raises."""
import ctypes as C

import numpy as np
import torch

from ... import _lib


class DecodeRules:
    """What the reference's logit filters need to know (decoding.py:387-441); -1 (or None) switches a part off.
      timestamp_begin              first timestamp id; -1: no timestamp rules
      no_timestamps                <|notimestamps|>, never chosen under the timestamp rules
      max_initial_timestamp_index  cap of the first timestamp (DecodingOptions.max_initial_timestamp / 0.02 s)
      blank                        tokenizer.encode(" ") as ONE id: at the first sampled position it and eot are out (SuppressBlank)
      no_speech, sot               <|nospeech|> and <|startoftranscript|>: with both, decode returns softmax(logits at sot)[no_speech] per sequence"""

    def __init__(self, eot, timestamp_begin=-1, no_timestamps=-1, max_initial_timestamp_index=-1, blank=-1, no_speech=-1, sot=-1):
        def off(v):
            return -1 if v is None else int(v)
        self.eot, self.timestamp_begin, self.no_timestamps = int(eot), off(timestamp_begin), off(no_timestamps)
        self.max_initial_timestamp_index, self.blank, self.no_speech, self.sot = off(max_initial_timestamp_index), off(blank), off(no_speech), off(sot)

    def check(self, n_vocab, who="WhisperDecoder.decode"):
        """the limits mf_whisper_decoder_decode refuses, refused here first: nothing reaches the library"""
        V = int(n_vocab)
        if not 0 <= self.eot < V:
            raise RuntimeError(f"{who}: end-of-text token {self.eot} outside the vocabulary ({V})")
        if self.timestamp_begin != -1 and not self.eot < self.timestamp_begin <= V:
            raise RuntimeError(f"{who}: timestamp_begin = {self.timestamp_begin}; eot ({self.eot}) < timestamp_begin <= n_vocab ({V}), or -1 for no timestamp rules")
        for name in ("no_timestamps", "blank", "no_speech", "sot"):
            if not -1 <= getattr(self, name) < V:
                raise RuntimeError(f"{who}: {name} token {getattr(self, name)} outside the vocabulary ({V})")
        n_ts = V - self.timestamp_begin if self.timestamp_begin >= 0 else 0
        if not -1 <= self.max_initial_timestamp_index < max(n_ts, 1):
            raise RuntimeError(f"{who}: max_initial_timestamp_index = {self.max_initial_timestamp_index}, the vocabulary holds {n_ts} timestamps (-1: none)")
        if self.no_speech >= 0 and self.sot < 0:
            raise RuntimeError(f"{who}: the no-speech probability is read at the <|startoftranscript|> token; give its id as sot")

    def sot_indices(self, prompts, who="WhisperDecoder.decode"):
        """index of <|startoftranscript|> in every prompt (DecodingTask.sot_index, decoding.py:468)"""
        out = []
        for b, p in enumerate(prompts):
            if self.sot not in p:
                raise RuntimeError(f"{who}: prompt {b} does not hold the sot token {self.sot}, where the no-speech probability is read")
            out.append(p.index(self.sot))
        return out


class WhisperDecoder:
    def __init__(self, state_dict, n_head, precision="bf16x3", max_batch=1, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("WhisperDecoder needs a HIP device; no CPU path exists here")
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        _lib.init_device(idx)
        arr, keep = _lib.tensor_array(state_dict)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_create(arr, len(keep), int(n_head), _lib.PRECISIONS[precision], int(max_batch), C.byref(h)),
                       "whisper_decoder_create")
        self._h = h.value
        d = [C.c_int() for _ in range(4)]
        _lib.check(_lib.lib().mf_whisper_decoder_dims(self._h, *[C.byref(v) for v in d]), "whisper_decoder_dims")
        self.n_layer, self.n_text_ctx, self.n_state, self.n_vocab = (v.value for v in d)
        self.max_batch, self.batch = int(max_batch), 0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().mf_whisper_decoder_destroy(self._h)
        except Exception:
            pass

    def begin(self, enc, t_audio=None):
        """enc: [B, T, n_state] (or [T, n_state]) float32 on the device; t_audio (default T): only the first t_audio rows of a
        single sequence's buffer are read -- a short utterance does not pay for 1500 keys."""
        if not (torch.is_tensor(enc) and enc.is_cuda):
            raise RuntimeError("WhisperDecoder.begin: the encoder states must be a tensor on the HIP device")
        enc = enc.to(torch.float32)
        if enc.dim() == 2:
            enc = enc[None]
        if enc.dim() != 3 or enc.shape[2] != self.n_state:
            raise RuntimeError(f"WhisperDecoder.begin: encoder states [B, T, {self.n_state}] expected, got {tuple(enc.shape)}")
        B, T = enc.shape[:2]
        if t_audio is not None and int(t_audio) != T:
            if B != 1 or not 1 <= int(t_audio) <= T:
                raise RuntimeError("WhisperDecoder.begin: t_audio shortens the buffer of ONE sequence")
            T = int(t_audio)
        enc = enc.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_begin(self._h, enc.data_ptr(), int(T), int(B), _lib.stream_ptr(self.device)), "whisper_decoder_begin")
        self.batch = B

    def logits(self, tokens):
        """tokens [B, n] integers -> logits [B, n, n_vocab] float32 on the device, for n tokens appended at the current offset"""
        t = torch.as_tensor(tokens)
        if t.dim() == 1:
            t = t[None]
        t = t.to(self.device, torch.int32).contiguous()
        B, n = t.shape
        out = torch.empty((B, n, self.n_vocab), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_logits(self._h, t.data_ptr(), int(n), out.data_ptr(), int(B), _lib.stream_ptr(self.device)),
                       "whisper_decoder_logits")
        return out

    def suppress_mask(self, token_ids):
        """the additive mask of `SuppressTokens` (decoding.py): -inf at token_ids, 0 elsewhere; float32 [n_vocab] on the device"""
        m = torch.zeros(self.n_vocab, dtype=torch.float32)
        if len(token_ids):
            m[torch.as_tensor(list(token_ids), dtype=torch.long)] = float("-inf")
        return m.to(self.device)

    def greedy(self, prompts, eot, max_new, suppress=None, check_every=8):
        """prompts: one list of token ids per sequence of the batch given to begin().  suppress: a mask from suppress_mask(), a list of
        token ids, or None.  Returns ([ids of sequence 0, ids of sequence 1, ...], float32 array of summed log-probabilities)."""
        prompts = [[int(t) for t in p] for p in prompts]
        B = len(prompts)
        lens = (C.c_int * B)(*[len(p) for p in prompts])
        flat = [t for p in prompts for t in p]
        toks = (C.c_int * max(len(flat), 1))(*flat)
        if suppress is not None and not torch.is_tensor(suppress):
            suppress = self.suppress_mask(suppress)
        if suppress is not None and (not suppress.is_cuda or suppress.dtype != torch.float32 or suppress.numel() != self.n_vocab):
            raise RuntimeError("WhisperDecoder.greedy: the suppression mask is a float32 [n_vocab] tensor on the device")
        n_out = max(int(max_new), 1)
        out = np.zeros((B, n_out), dtype=np.int32)
        out_lens = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_greedy(
                self._h, toks, lens, suppress.data_ptr() if suppress is not None else None, int(eot), int(max_new), int(check_every),
                out.ctypes.data, out_lens.ctypes.data, lp.ctypes.data, B, _lib.stream_ptr(self.device)), "whisper_decoder_greedy")
        self.last_out = out
        return [out[b, : out_lens[b]].tolist() for b in range(B)], lp

    def _mask(self, suppress, who):
        if suppress is not None and not torch.is_tensor(suppress):
            suppress = self.suppress_mask(suppress)
        if suppress is not None and (not suppress.is_cuda or suppress.dtype != torch.float32 or suppress.numel() != self.n_vocab):
            raise RuntimeError(f"WhisperDecoder.{who}: the suppression mask is a float32 [n_vocab] tensor on the device")
        return suppress

    def decode(self, prompts, rules, max_new, suppress=None, check_every=8):
        """greedy() under a `DecodeRules`: SuppressBlank, the suppression mask, the timestamp rules, in the launch that chooses the token.
        Returns (ids per sequence, float32 summed log-probabilities, float32 no-speech probabilities -- NaN where the rules name no no_speech token,
        as the reference's `_main_loop` leaves them)."""
        prompts = [[int(t) for t in p] for p in prompts]
        B = len(prompts)
        if B > self.max_batch:
            raise RuntimeError(f"WhisperDecoder.decode: batch {B} exceeds the handle's max_batch {self.max_batch}")
        rules.check(self.n_vocab)
        nsp_on = rules.no_speech >= 0
        sot_index = (C.c_int * B)(*rules.sot_indices(prompts)) if nsp_on else None
        lens = (C.c_int * B)(*[len(p) for p in prompts])
        flat = [t for p in prompts for t in p]
        toks = (C.c_int * max(len(flat), 1))(*flat)
        suppress = self._mask(suppress, "decode")
        out = np.zeros((B, max(int(max_new), 1)), dtype=np.int32)
        out_lens = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        nsp = np.full(B, np.nan, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_decode(
                self._h, toks, lens, suppress.data_ptr() if suppress is not None else None, rules.eot, int(max_new), int(check_every),
                rules.timestamp_begin, rules.no_timestamps, rules.max_initial_timestamp_index, rules.blank, rules.no_speech, sot_index,
                out.ctypes.data, out_lens.ctypes.data, lp.ctypes.data, nsp.ctypes.data if nsp_on else None, B, _lib.stream_ptr(self.device)),
                "whisper_decoder_decode")
        self.last_out = out
        return [out[b, : out_lens[b]].tolist() for b in range(B)], lp, nsp

    def detect_language(self, sot, language_token_ids):
        """`detect_language` of decoding.py directly after begin(): (int32 [B] chosen language token, float32 [B, n] probabilities over
        language_token_ids in the order given).  A decode afterwards equals one without this call."""
        ids = [int(t) for t in language_token_ids]
        if not ids or len(set(ids)) != len(ids) or not all(0 <= t < self.n_vocab for t in ids):
            raise RuntimeError(f"WhisperDecoder.detect_language: the language tokens are distinct ids inside the vocabulary ({self.n_vocab})")
        if not 0 <= int(sot) < self.n_vocab:
            raise RuntimeError(f"WhisperDecoder.detect_language: sot token {int(sot)} outside the vocabulary ({self.n_vocab})")
        if not self.batch:
            raise RuntimeError("WhisperDecoder.detect_language: call begin() first")
        B = self.batch
        got = np.zeros(B, dtype=np.int32)
        probs = np.zeros((B, len(ids)), dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_detect_language(self._h, int(sot), (C.c_int * len(ids))(*ids), len(ids), got.ctypes.data, probs.ctypes.data, B,
                                                                     _lib.stream_ptr(self.device)), "whisper_decoder_detect_language")
        return got, probs

    def choose(self, logits, history, rules, suppress=None, tokens=None, logprobs=None, done=None):
        """test seam: the rule kernel's choice alone.  logits: float32 [B, n_vocab] on the device; history: per sequence (tokens sampled so far,
        the last, the one before).  tokens / logprobs / done: what the outputs hold on entry (a sequence whose done flag is set keeps them).
        Returns (int32 tokens, float32 log-probabilities, int32 done flags)."""
        if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == self.n_vocab):
            raise RuntimeError(f"WhisperDecoder.choose: logits are float32 [B, {self.n_vocab}] on the device")
        B = logits.shape[0]
        if B > self.max_batch:
            raise RuntimeError(f"WhisperDecoder.choose: batch {B} exceeds the handle's max_batch {self.max_batch}")
        rules.check(self.n_vocab, "WhisperDecoder.choose")
        hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32).reshape(B, 3))
        for b in range(B):
            n = int(hist[b, 0])
            if n < 0 or any(not 0 <= int(t) < self.n_vocab for t in hist[b, 1:1 + min(n, 2)]):
                raise RuntimeError(f"WhisperDecoder.choose: sequence {b}: history {hist[b].tolist()} is no count and ids inside the vocabulary ({self.n_vocab})")
        suppress = self._mask(suppress, "choose")
        tok = np.zeros(B, np.int32) if tokens is None else np.array(tokens, dtype=np.int32)
        lp = np.zeros(B, np.float32) if logprobs is None else np.array(logprobs, dtype=np.float32)
        dn = np.zeros(B, np.int32) if done is None else np.array(done, dtype=np.int32)
        logits = logits.contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_choose(
                self._h, logits.data_ptr(), hist.ctypes.data, suppress.data_ptr() if suppress is not None else None, rules.eot, rules.timestamp_begin,
                rules.no_timestamps, rules.max_initial_timestamp_index, rules.blank, tok.ctypes.data, lp.ctypes.data, dn.ctypes.data, B,
                _lib.stream_ptr(self.device)), "whisper_decoder_choose")
        return tok, lp, dn

    def cache(self, layer, seq):
        """(k, v, length) of one layer's self-attention cache for one sequence: float32 [n_text_ctx, n_state] arrays (test seam)"""
        k = np.empty((self.n_text_ctx, self.n_state), dtype=np.float32)
        v = np.empty_like(k)
        n = C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_cache_read(self._h, int(layer), int(seq), k.ctypes.data, v.ctypes.data, C.byref(n)), "whisper_decoder_cache_read")
        return k, v, n.value
