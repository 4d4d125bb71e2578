"""`WhisperDecoder`: the text decoder of a Whisper checkpoint on the MI355X (`mf_whisper_decoder_*`, csrc/mf_whisper_dec.hip).

    dec = WhisperDecoder(state_dict, n_head=6, max_batch=8)       # the "decoder.*" tensors (weights.decoder_state_dict)
    dec.begin(enc)                                                # enc [B, T_audio, n_state] on the device: one segment per sequence
    logits = dec.logits(tokens)                                   # teacher-forced, appended at the caches' offset (TextDecoder.forward)
    ids, logprobs = dec.greedy(prompts, eot=50257, max_new=224)   # token ids per sequence, summed log-probabilities

There is no CPU path: without a HIP device the constructor raises."""
import ctypes as C

import numpy as np
import torch

from ... import _lib


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

    def cache(self, layer, seq):
        """(k, v, length) of one layer's self-attention cache for one sequence: float32 [n_text_ctx, n_state] arrays (test seam)"""
        k = np.empty((self.n_text_ctx, self.n_state), dtype=np.float32)
        v = np.empty_like(k)
        n = C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_whisper_decoder_cache_read(self._h, int(layer), int(seq), k.ctypes.data, v.ctypes.data, C.byref(n)), "whisper_decoder_cache_read")
        return k, v, n.value
