"""Speech to token ids on the device: the Whisper encoder the MuseTalk path already holds, plus the text decoder with greedy decoding.

    a2f = Audio2Feature(model_path=...)                           # the encoder handle every MuseTalk deployment has
    dec = WhisperDecoder(decoder_state_dict(ckpt["model_state_dict"]), n_head=ckpt["dims"]["n_text_head"], max_batch=8)
    tr = Transcriber(a2f, dec, tokenizer)                         # tokenizer: the reference's whisper.tokenizer.get_tokenizer(...), or None
    ids, text = tr.transcribe(wav_16k, language="en")

What it is: `whisper.transcribe` reduced to no-timestamps greedy decoding (decoding.py at temperature 0, `without_timestamps=True`).
What it is not: timestamp rules, beam search, temperature fallback, `suppress_blank`, conditioning a window on the previous window's text,
and the `ASRBase` adapter of whisper_online.py (which needs word times) are not built.  Windows of a long recording are cut from the
WAVEFORM, so each window's log-mel has its own `max - 8` floor; the reference computes one log-mel over the whole file."""
import json
import os

import numpy as np
import torch

N_SAMPLES_SEGMENT = 480000      # 30 s at 16 kHz (whisper/audio.py:13-19)
MIN_TAIL = 400                  # a last window shorter than one FFT frame holds no log-mel column worth decoding


class SpecialTokens:
    """ids of the special tokens decoding needs.  The multilingual vocabulary puts them after the 50257 text tokens in the order
    tokenizer.py:279-288 adds them: end-of-text, start-of-transcript, one token per language, translate, transcribe, start-of-lm,
    start-of-prev, no-speech, no-timestamps."""

    def __init__(self, eot, sot, language_tokens, translate, transcribe, sot_lm, sot_prev, no_speech, no_timestamps):
        self.eot, self.sot, self.language_tokens = int(eot), int(sot), dict(language_tokens)
        self.translate, self.transcribe, self.sot_lm, self.sot_prev = int(translate), int(transcribe), int(sot_lm), int(sot_prev)
        self.no_speech, self.no_timestamps = int(no_speech), int(no_timestamps)

    @classmethod
    def multilingual(cls, language_codes=("en",), n_languages=99, eot=50257):
        """language_codes: the checkpoint's languages in vocabulary order (only the ones named can be asked for; "en" is the first)"""
        sot = eot + 1
        t = sot + 1 + n_languages
        return cls(eot, sot, {c: sot + 1 + i for i, c in enumerate(language_codes)}, t, t + 1, t + 2, t + 3, t + 4, t + 5)

    @classmethod
    def from_added_tokens(cls, added, eot):
        """added: {"<|en|>": 50259, ...} as `added_tokens.json` of a tokenizer directory (or GPT2TokenizerFast.get_added_vocab()) holds it"""
        named = {"<|startoftranscript|>", "<|translate|>", "<|transcribe|>", "<|startoflm|>", "<|startofprev|>", "<|nospeech|>", "<|notimestamps|>"}
        langs = {k[2:-2]: v for k, v in added.items() if k.startswith("<|") and k.endswith("|>") and k not in named and k != "<|endoftext|>"
                 and not k[2:-2].replace(".", "").isdigit()}
        return cls(eot, added["<|startoftranscript|>"], langs, added["<|translate|>"], added["<|transcribe|>"], added["<|startoflm|>"],
                   added["<|startofprev|>"], added["<|nospeech|>"], added["<|notimestamps|>"])

    @classmethod
    def from_dir(cls, path, eot=50257):
        """the special tokens of a tokenizer directory the deployment names (the reference's whisper/assets/multilingual)"""
        with open(os.path.join(path, "added_tokens.json")) as f:
            return cls.from_added_tokens(json.load(f), eot)

    @classmethod
    def from_tokenizer(cls, tokenizer):
        """from the reference's `Tokenizer` wrapper (tokenizer.py:129): its GPT2TokenizerFast knows the added tokens"""
        return cls.from_added_tokens(tokenizer.tokenizer.get_added_vocab(), tokenizer.eot)


def start_sequence(specials, language="en", task="transcribe", timestamps=False):
    """tokenizer.py:320-331 `sot_sequence` for a multilingual model, plus <|notimestamps|> (`sot_sequence_including_notimestamps`)"""
    if task not in ("transcribe", "translate"):
        raise ValueError(f"task must be transcribe or translate, not {task!r}")
    if language not in specials.language_tokens:
        raise ValueError(f"language {language!r} is not among the tokens this SpecialTokens knows ({len(specials.language_tokens)} languages)")
    seq = [specials.sot, specials.language_tokens[language], specials.transcribe if task == "transcribe" else specials.translate]
    return seq if timestamps else seq + [specials.no_timestamps]


def windows(n_samples, segment=N_SAMPLES_SEGMENT, min_tail=MIN_TAIL):
    """[(start, stop)] of the 30 s windows `transcribe` walks without timestamps (transcribe.py: seek advances by a whole segment); a tail
    shorter than min_tail samples is dropped"""
    out = [(s, min(s + segment, n_samples)) for s in range(0, max(n_samples, 0), segment)]
    if out and out[-1][1] - out[-1][0] < min_tail:
        out.pop()
    return out


class Transcriber:
    def __init__(self, whisper_handle, decoder, tokenizer=None, specials=None, suppress=None):
        """whisper_handle: the `Audio2Feature` that owns the encoder; decoder: a `WhisperDecoder` built WITH encoder.ln_post (the encoder handle
        returns the last block's output before that LayerNorm); tokenizer: the reference's Tokenizer wrapper or None; specials: SpecialTokens
        (default: from the tokenizer, else the multilingual layout with English alone); suppress: token ids never chosen (default: the
        tokenizer's non-speech list plus the control tokens, decoding.py `_get_suppress_tokens`; without a tokenizer only the control tokens)."""
        self.enc, self.dec, self.tokenizer = whisper_handle, decoder, tokenizer
        if self.enc.n_state != self.dec.n_state:
            raise RuntimeError(f"encoder width {self.enc.n_state} and decoder width {self.dec.n_state} are not one checkpoint's")
        self.specials = specials or (SpecialTokens.from_tokenizer(tokenizer) if tokenizer is not None else SpecialTokens.multilingual())
        sp = self.specials
        if suppress is None:
            suppress = list(tokenizer.non_speech_tokens) if tokenizer is not None else []
            suppress = sorted(set(suppress) | {sp.sot, sp.sot_prev, sp.sot_lm, sp.no_speech})
        self.suppress = [int(t) for t in suppress]
        self._mask = self.dec.suppress_mask(self.suppress)

    def prompt(self, language="en", task="transcribe", prompt_tokens=None):
        """[<|startofprev|> + the tail of the previous text] + the start sequence, at most n_text_ctx / 2 tokens (decoding.py `_get_initial_tokens`)"""
        start = start_sequence(self.specials, language, task)
        if not prompt_tokens:
            return start
        room = self.dec.n_text_ctx // 2 - 1 - len(start)
        return [self.specials.sot_prev] + [int(t) for t in prompt_tokens][-room:] + start

    def _encode(self, wav):
        """last encoder block's output [1500, n_state] of one window of <= 30 s, on the device"""
        from . import _lib
        w = self.enc._wav(wav)
        emb = torch.empty((self.enc.n_layer + 1, self.enc.n_ctx, self.enc.n_state), dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(_lib.lib().mf_whisper_encode_audio(self.enc._h, w.data_ptr(), w.numel(), emb.data_ptr(), _lib.stream_ptr(w.device)), "whisper_encode_audio")
        return emb[self.enc.n_layer]

    def decode_windows(self, wavs, prompts, max_new=None, check_every=8):
        """wavs: windows of <= 30 s, one per sequence; prompts: their prompt token lists.  One begin + one greedy call per max_batch windows."""
        ids, logprobs = [], []
        B = self.dec.max_batch
        for i in range(0, len(wavs), B):
            enc = torch.stack([self._encode(w) for w in wavs[i:i + B]], dim=0)
            ps = prompts[i:i + B]
            budget = min(self.dec.n_text_ctx // 2, self.dec.n_text_ctx - min(len(p) for p in ps) + 1)
            self.dec.begin(enc)
            got, lp = self.dec.greedy(ps, self.specials.eot, min(int(max_new), budget) if max_new else budget, suppress=self._mask, check_every=check_every)
            ids += got
            logprobs += lp.tolist()
        return ids, logprobs

    def transcribe(self, wav_16k, language="en", prompt_tokens=None, task="transcribe", max_new=None):
        """token ids of one recording (16 kHz float32); longer than 30 s: cut into 30 s windows that decode as one batch, ids concatenated.
        With a tokenizer: (ids, text)."""
        wav = np.asarray(wav_16k.detach().cpu() if torch.is_tensor(wav_16k) else wav_16k, dtype=np.float32).reshape(-1)
        cuts = windows(wav.size)
        if not cuts:
            raise RuntimeError(f"transcribe: {wav.size} samples hold no window of at least {MIN_TAIL}")
        p = self.prompt(language, task, prompt_tokens)
        got, _ = self.decode_windows([wav[a:b] for a, b in cuts], [p] * len(cuts), max_new)
        ids = [t for g in got for t in g]
        return (ids, self.tokenizer.decode(ids)) if self.tokenizer is not None else ids

    def transcribe_batch(self, wavs, languages=None, prompt_tokens=None, max_new=None):
        """one utterance (<= 30 s) per session, decoded together: prompts of different lengths, sequences that end at different steps"""
        n = len(wavs)
        languages = languages or ["en"] * n
        prompt_tokens = prompt_tokens or [None] * n
        for w in wavs:
            if len(w) > N_SAMPLES_SEGMENT:
                raise RuntimeError("transcribe_batch: one utterance holds at most 30 s; use transcribe() for a long recording")
        ids, _ = self.decode_windows([np.asarray(w, dtype=np.float32) for w in wavs],
                                     [self.prompt(l, "transcribe", p) for l, p in zip(languages, prompt_tokens)], max_new)
        return [(i, self.tokenizer.decode(i)) for i in ids] if self.tokenizer is not None else ids
