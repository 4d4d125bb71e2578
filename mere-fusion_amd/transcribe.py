"""Speech to token ids on the device: the Whisper encoder the MuseTalk path already holds, plus the text decoder with greedy decoding.

    a2f = Audio2Feature(model_path=...)                           # the encoder handle every MuseTalk deployment has
    dec = WhisperDecoder(decoder_state_dict(ckpt["model_state_dict"]), n_head=ckpt["dims"]["n_text_head"], max_batch=8)
    tr = Transcriber(a2f, dec, tokenizer)                         # tokenizer: the reference's whisper.tokenizer.get_tokenizer(...), or None
    ids, text = tr.transcribe(wav_16k, language="en")

    t = tr.transcribe(wav_16k, language=None, timestamps=True)    # Transcript: segments with times, avg_logprob and no_speech_prob per window

What it is: `whisper.transcribe` reduced to greedy decoding at temperature 0 (decoding.py `DecodingTask`): by default `without_timestamps=True`
and one suppression mask; with `timestamps=True` the reference's SuppressBlank and ApplyTimestampRules, the no-speech probability, and language
detection when no language is named.
What it is not: beam search, temperature fallback and its thresholds, word-level times, a non-decreasing rule for timestamps (the reference's
ApplyTimestampRules has none), conditioning a window on the previous window's text, and the `ASRBase` adapter of whisper_online.py (which needs
word times) are not built.  Windows of a long recording are cut from the WAVEFORM and stay independent 30 s cuts so that they batch: each
window's log-mel has its own `max - 8` floor (the reference computes one log-mel over the whole file), and no window starts where the last
timestamp of the one before it fell."""
import collections
import json
import os

import numpy as np
import torch

N_SAMPLES_SEGMENT = 480000      # 30 s at 16 kHz (whisper/audio.py:13-19)
SAMPLE_RATE = 16000
TIME_PRECISION = 0.02           # seconds per timestamp token: CHUNK_LENGTH / n_audio_ctx = 30 / 1500 (decoding.py:491)
MIN_TAIL = 400                  # a last window shorter than one FFT frame holds no log-mel column worth decoding


class SpecialTokens:
    """ids of the special tokens decoding needs.  The multilingual vocabulary puts them after the 50257 text tokens in the order
    tokenizer.py:279-288 adds them: end-of-text, start-of-transcript, one token per language, translate, transcribe, start-of-lm,
    start-of-prev, no-speech, no-timestamps."""

    def __init__(self, eot, sot, language_tokens, translate, transcribe, sot_lm, sot_prev, no_speech, no_timestamps, blank=None):
        self.eot, self.sot, self.language_tokens = int(eot), int(sot), dict(language_tokens)
        self.translate, self.transcribe, self.sot_lm, self.sot_prev = int(translate), int(transcribe), int(sot_lm), int(sot_prev)
        self.no_speech, self.no_timestamps = int(no_speech), int(no_timestamps)
        self.blank = None if blank is None else int(blank)       # tokenizer.encode(" ") as one id (SuppressBlank); None: no tokenizer to ask

    @property
    def timestamp_begin(self):
        """the first timestamp token <|0.00|>: the vocabulary puts the timestamps directly after <|notimestamps|> (tokenizer.py:288-289, 226-228)"""
        return self.no_timestamps + 1

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
        sp = cls.from_added_tokens(tokenizer.tokenizer.get_added_vocab(), tokenizer.eot)
        sp.blank = blank_token(tokenizer)
        return sp


def blank_token(tokenizer):
    """`tokenizer.encode(" ")` as the ONE id the choose kernel takes; SuppressBlank (decoding.py:394) would take a list, no Whisper vocabulary gives one"""
    ids = [int(t) for t in tokenizer.encode(" ")]
    if len(ids) != 1:
        raise RuntimeError(f"this tokenizer encodes a blank as {len(ids)} tokens {ids}; suppress_blank is built for a single blank token")
    return ids[0]


Transcript = collections.namedtuple("Transcript", "ids segments avg_logprob no_speech_prob languages text")
Transcript.__doc__ = """`transcribe(..., timestamps=True)`: ids = the text tokens of all windows (timestamps taken out); segments = [(start_s, end_s, ids[, text])];
avg_logprob, no_speech_prob, languages = one entry per 30 s window; text = the decoded ids, or None without a tokenizer"""


def avg_logprob(sum_logprob, n_tokens):
    """decoding.py:676: the summed log-probability (end-of-text's term included) over the tokens + 1"""
    return float(sum_logprob) / (int(n_tokens) + 1)


def cut_segments(ids, timestamp_begin, offset_s=0.0, window_s=30.0, precision=TIME_PRECISION):
    """[(start_s, end_s, text ids)] of one window's sampled tokens.

    [upstream-knowledge] UNPINNED: this is the rule of upstream Whisper's `transcribe.py`; the reference's copy of that file was rewritten for
    MuseTalk and does not contain it, so it is restated here and tested against hand-written token lists only.  Two consecutive timestamp tokens
    end one segment and start the next; a single timestamp at the very end closes the last segment; a slice's times are its first and last token
    minus timestamp_begin, times `precision`, plus the window's start.  Without any consecutive pair the window is one segment from its start to
    its last timestamp (to its end when there is none, or when that timestamp is <|0.00|>).
    Where this departs, because windows here are independent cuts: upstream moves its seek back to the last pair and decodes the text after it
    again; here that text is kept as a last segment that ends with the window.  A slice that does not open with a timestamp (the reference's
    rules do not force one) starts where the one before it ended.  Segments without text tokens are dropped."""
    ids = [int(t) for t in ids]
    tb = int(timestamp_begin)
    is_ts = [t >= tb for t in ids]
    cuts = [i + 1 for i in range(len(ids) - 1) if is_ts[i] and is_ts[i + 1]]
    if len(ids) >= 2 and is_ts[-1] and not is_ts[-2]:
        cuts.append(len(ids))
    segs = []

    def add(start, end, toks):
        text = [t for t in toks if t < tb]
        if text:
            segs.append((offset_s + start, offset_s + end, text))

    if not cuts:
        stamps = [t for t in ids if t >= tb]
        end = (stamps[-1] - tb) * precision if stamps and stamps[-1] != tb else window_s
        add(0.0, end, ids)
        return segs
    last, prev_end = 0, 0.0
    for c in cuts:
        sl = ids[last:c]
        start = (sl[0] - tb) * precision if sl[0] >= tb else prev_end
        end = (sl[-1] - tb) * precision
        add(start, end, sl)
        last, prev_end = c, end
    rest = ids[last:]
    if rest:
        add((rest[0] - tb) * precision if rest[0] >= tb else prev_end, window_s, rest)
    return segs


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

    def prompt(self, language="en", task="transcribe", prompt_tokens=None, timestamps=False):
        """[<|startofprev|> + the tail of the previous text] + the start sequence, at most n_text_ctx / 2 tokens (decoding.py `_get_initial_tokens`)"""
        start = start_sequence(self.specials, language, task, timestamps)
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

    def decode_windows(self, wavs, prompts, max_new=None, check_every=8, rules=None, detect=False):
        """wavs: windows of <= 30 s, one per sequence; prompts: their prompt token lists.  One begin + one greedy call per max_batch windows.
        rules: a `DecodeRules` -- the call is then `WhisperDecoder.decode`, and a third list, the no-speech probabilities, is returned;
        detect: language detection after each begin, the chosen language token written behind <|startoftranscript|> (decoding.py:579-589) --
        a fourth list, the language codes, is returned."""
        ids, logprobs, no_speech, languages = [], [], [], []
        B = self.dec.max_batch
        sp = self.specials
        for i in range(0, len(wavs), B):
            enc = torch.stack([self._encode(w) for w in wavs[i:i + B]], dim=0)
            ps = [list(p) for p in prompts[i:i + B]]
            budget = min(self.dec.n_text_ctx // 2, self.dec.n_text_ctx - min(len(p) for p in ps) + 1)
            self.dec.begin(enc)
            if detect:
                codes = list(sp.language_tokens)
                chosen, _ = self.dec.detect_language(sp.sot, [sp.language_tokens[c] for c in codes])
                by_id = {sp.language_tokens[c]: c for c in codes}
                for p, t in zip(ps, chosen.tolist()):
                    p[p.index(sp.sot) + 1] = int(t)
                    languages.append(by_id[int(t)])
            n_new = min(int(max_new), budget) if max_new else budget
            if rules is None:
                got, lp = self.dec.greedy(ps, sp.eot, n_new, suppress=self._mask, check_every=check_every)
            else:
                got, lp, nsp = self.dec.decode(ps, rules, n_new, suppress=self._mask, check_every=check_every)
                no_speech += nsp.tolist()
            ids += got
            logprobs += lp.tolist()
        if rules is None and not detect:
            return ids, logprobs
        return ids, logprobs, no_speech, languages

    def rules(self, timestamps=True, max_initial_timestamp=1.0, suppress_blank=True):
        """the `DecodeRules` of the reference's `DecodingOptions` defaults (decoding.py:71-104): suppress_blank, max_initial_timestamp = 1.0 s
        (index 50 at 0.02 s a token), the no-speech probability read at <|startoftranscript|>"""
        from .musetalk.whisper.decoder import DecodeRules
        sp = self.specials
        index = round(max_initial_timestamp / TIME_PRECISION) if max_initial_timestamp else None        # decoding.py:493-494: 0 and None both mean no cap
        return DecodeRules(sp.eot, timestamp_begin=sp.timestamp_begin if timestamps else -1, no_timestamps=sp.no_timestamps,
                           max_initial_timestamp_index=index if timestamps else None, blank=sp.blank if suppress_blank else None, no_speech=sp.no_speech, sot=sp.sot)

    def _timed(self, wavs, starts_s, prompts, max_new, detect, max_initial_timestamp):
        """the windows under the timestamp rules -> one Transcript per window"""
        sp = self.specials
        ids, lps, nsp, langs = self.decode_windows(wavs, prompts, max_new, rules=self.rules(True, max_initial_timestamp), detect=detect)
        out = []
        for i, (got, w, t0) in enumerate(zip(ids, wavs, starts_s)):
            segments = [(a, b, toks, self.tokenizer.decode(toks)) if self.tokenizer is not None else (a, b, toks)
                        for a, b, toks in cut_segments(got, sp.timestamp_begin, t0, len(w) / SAMPLE_RATE)]
            text_ids = [t for t in got if t < sp.timestamp_begin]
            out.append(Transcript(text_ids, segments, [avg_logprob(lps[i], len(got))], [nsp[i]], langs[i:i + 1],
                                  self.tokenizer.decode(text_ids) if self.tokenizer is not None else None))
        return out

    def transcribe(self, wav_16k, language="en", prompt_tokens=None, task="transcribe", max_new=None, timestamps=False, max_initial_timestamp=1.0):
        """token ids of one recording (16 kHz float32); longer than 30 s: cut into 30 s windows that decode as one batch, ids concatenated.
        With a tokenizer: (ids, text).
        timestamps=True: the start sequence without <|notimestamps|>, the reference's logit rules, and a `Transcript` with segments in seconds
        of the recording; language=None then detects the language of every window first (the first known language otherwise stands in the prompt)."""
        wav = np.asarray(wav_16k.detach().cpu() if torch.is_tensor(wav_16k) else wav_16k, dtype=np.float32).reshape(-1)
        cuts = windows(wav.size)
        if not cuts:
            raise RuntimeError(f"transcribe: {wav.size} samples hold no window of at least {MIN_TAIL}")
        if timestamps:
            p = self.prompt(language or next(iter(self.specials.language_tokens)), task, prompt_tokens, timestamps=True)
            per = self._timed([wav[a:b] for a, b in cuts], [a / SAMPLE_RATE for a, _ in cuts], [p] * len(cuts), max_new, language is None, max_initial_timestamp)
            merged = [sum((list(t[f]) for t in per), []) for f in range(5)]
            return Transcript(*merged, "".join(t.text for t in per) if self.tokenizer is not None else None)
        if language is None:
            raise RuntimeError("transcribe: language detection (language=None) comes with timestamps=True")
        p = self.prompt(language, task, prompt_tokens)
        got, _ = self.decode_windows([wav[a:b] for a, b in cuts], [p] * len(cuts), max_new)
        ids = [t for g in got for t in g]
        return (ids, self.tokenizer.decode(ids)) if self.tokenizer is not None else ids

    def transcribe_batch(self, wavs, languages=None, prompt_tokens=None, max_new=None, timestamps=False, max_initial_timestamp=1.0):
        """one utterance (<= 30 s) per session, decoded together: prompts of different lengths, sequences that end at different steps.
        timestamps=True: one `Transcript` per utterance (times from the utterance's start); languages=None then detects each utterance's language."""
        n = len(wavs)
        detect = timestamps and languages is None
        languages = languages or [next(iter(self.specials.language_tokens)) if detect else "en"] * n
        prompt_tokens = prompt_tokens or [None] * n
        for w in wavs:
            if len(w) > N_SAMPLES_SEGMENT:
                raise RuntimeError("transcribe_batch: one utterance holds at most 30 s; use transcribe() for a long recording")
        if timestamps:
            ws = [np.asarray(w, dtype=np.float32) for w in wavs]
            return self._timed(ws, [0.0] * n, [self.prompt(l, "transcribe", p, timestamps=True) for l, p in zip(languages, prompt_tokens)], max_new, detect,
                               max_initial_timestamp)
        ids, _ = self.decode_windows([np.asarray(w, dtype=np.float32) for w in wavs],
                                     [self.prompt(l, "transcribe", p) for l, p in zip(languages, prompt_tokens)], max_new)
        return [(i, self.tokenizer.decode(i)) for i in ids] if self.tokenizer is not None else ids
