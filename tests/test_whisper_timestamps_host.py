"""CPU side of decoding with timestamps: the segment cut on hand-written token lists, the time arithmetic, the special tokens against the
tokenizer facts recorded from the reference (tests/golden/make_whisper_timestamps_golden.py), avg_logprob, and every new refusal of
`WhisperDecoder.decode / choose / detect_language` -- raised before anything reaches the library (a library that fails the test when called)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mere_fusion_amd import _lib
from mere_fusion_amd import transcribe as T
from mere_fusion_amd.musetalk.whisper import weights as DW
from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules, WhisperDecoder

TB = 50364


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "whisper_timestamps_golden.npz")))


@pytest.fixture(scope="module")
def old_gold():
    return dict(np.load(os.path.join(GOLDEN, "whisper_decoder_golden.npz")))


def ts(seconds):
    return TB + round(seconds / 0.02)


# ---- segments ---------------------------------------------------------------------------------------------------------
def test_consecutive_timestamp_pairs_cut_segments():
    ids = [ts(0.0), 11, 12, ts(2.5), ts(2.5), 13, ts(4.0), ts(4.2), 14, 15, 16, ts(7.5)]
    assert T.cut_segments(ids, TB) == [(0.0, 2.5, [11, 12]), (2.5, 4.0, [13]), (pytest.approx(4.2), 7.5, [14, 15, 16])]


def test_a_trailing_single_timestamp_closes_the_last_segment():
    ids = [ts(1.0), 11, ts(2.0), ts(2.0), 12, 13, ts(3.0)]
    assert T.cut_segments(ids, TB) == [(1.0, 2.0, [11]), (2.0, 3.0, [12, 13])]
    # ... and without it the text after the last pair ends with the window (upstream would decode it again from there; windows here are independent)
    assert T.cut_segments(ids[:-1], TB, window_s=12.0) == [(1.0, 2.0, [11]), (2.0, 12.0, [12, 13])]


def test_no_pair_gives_one_segment():
    assert T.cut_segments([ts(0.0), 11, 12, ts(3.0)], TB) == [(0.0, 3.0, [11, 12])]            # [False, True] at the end: a cut at the end
    assert T.cut_segments([11, 12], TB, window_s=7.0) == [(0.0, 7.0, [11, 12])]
    assert T.cut_segments([ts(0.5), 11, 12], TB, window_s=7.0) == [(0.0, 0.5, [11, 12])]       # upstream: the last timestamp is the duration
    assert T.cut_segments([ts(0.0), 11], TB, window_s=7.0) == [(0.0, 7.0, [11])]               # ... unless it is <|0.00|>
    assert T.cut_segments([], TB) == [] and T.cut_segments([ts(1.0), ts(1.0)], TB) == [] and T.cut_segments([ts(1.0)], TB) == []


def test_times_are_tokens_times_20_ms_plus_the_window_start():
    assert T.TIME_PRECISION == 0.02 and T.SAMPLE_RATE == 16000
    segs = T.cut_segments([TB + 75, 11, TB + 150, TB + 150, 12, TB + 1500], TB, offset_s=60.0)
    assert [(a, b) for a, b, _ in segs] == [(pytest.approx(61.5), pytest.approx(63.0)), (pytest.approx(63.0), pytest.approx(90.0))]
    assert T.cut_segments([11, TB + 10, TB + 20, 12, TB + 30], TB, offset_s=30.0) == [(30.0, pytest.approx(30.2), [11]), (pytest.approx(30.4), pytest.approx(30.6), [12])]


def test_avg_logprob_counts_the_end_of_text_term():
    assert T.avg_logprob(-6.0, 2) == -2.0 and T.avg_logprob(-1.5, 0) == -1.5              # decoding.py:676: sum / (len(tokens) + 1)


# ---- special tokens -------------------------------------------------------------------------------------------------------
def test_special_tokens_know_timestamp_begin_and_the_blank(gold, old_gold):
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["tokenizer_facts"])
    assert len(gold["tokenizer_facts"]) == 6                                                 # the reference's tokenizer encodes " " as ONE token
    added = {str(k): int(v) for k, v in zip(old_gold["added_tokens"], old_gold["added_ids"])}
    for sp in (T.SpecialTokens.from_added_tokens(added, eot), T.SpecialTokens.multilingual()):
        assert (sp.eot, sp.sot, sp.no_speech, sp.no_timestamps, sp.timestamp_begin) == (eot, sot, no_speech, no_ts, tb)
        assert sp.timestamp_begin == sp.no_timestamps + 1 == TB and sp.blank is None         # no tokenizer to ask

    class Tok:
        def __init__(self, ids):
            self.ids = ids

        def encode(self, text):
            assert text == " "
            return self.ids

    assert T.blank_token(Tok([blank])) == blank == 220
    with pytest.raises(RuntimeError, match="single blank token"):
        T.blank_token(Tok([1, 2]))


def test_start_sequences_with_and_without_timestamps(gold, old_gold):
    sp = T.SpecialTokens.multilingual([str(c) for c in old_gold["lang_codes"]])
    assert T.start_sequence(sp, "en", timestamps=True) == gold["sot_sequence_en"].tolist() == gold["tiny_prompt"].tolist()
    assert T.start_sequence(sp, "en") == gold["sot_sequence_en"].tolist() + [sp.no_timestamps] == old_gold["sot_en_transcribe"].tolist()
    assert T.start_sequence(sp, "de", "translate", timestamps=True) == old_gold["sot_de_translate"].tolist()[:-1]


def test_make_decoder_state_dict_gain_moves_only_the_timestamp_rows():
    d = DW.WHISPER_SMALL_TEST
    a, b = DW.make_decoder_state_dict(3, d), DW.make_decoder_state_dict(3, d, timestamp_begin=200, timestamp_gain=1.5)
    for k in a:
        if k != "decoder.token_embedding.weight":
            assert a[k].equal(b[k])
    ea, eb = a["decoder.token_embedding.weight"], b["decoder.token_embedding.weight"]
    assert ea[:200].equal(eb[:200]) and np.allclose(eb[200:].numpy(), 1.5 * ea[200:].numpy(), rtol=1e-6, atol=0) and not ea[200:].equal(eb[200:])


# ---- refusals: before any launch --------------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: a refused call must not reach the library")


@pytest.fixture
def dec(monkeypatch):
    """a WhisperDecoder of the small geometry without a device: every call into the library fails the test"""
    monkeypatch.setattr(_lib, "lib", lambda: NoLibrary())
    d = object.__new__(WhisperDecoder)
    d._h, d.n_layer, d.n_text_ctx, d.n_state, d.n_vocab, d.max_batch, d.batch = None, 2, 80, 128, 257, 3, 3
    return d


GOOD = dict(eot=192, timestamp_begin=200, no_timestamps=199, max_initial_timestamp_index=5, blank=32, no_speech=198, sot=193)


def test_good_rules_pass_the_check():
    DecodeRules(**GOOD).check(257)
    DecodeRules(192).check(257)                                       # everything off
    DecodeRules(192, timestamp_begin=257).check(257)                   # a vocabulary without timestamps: timestamp_begin == n_vocab
    r = DecodeRules(192, timestamp_begin=None, blank=None)
    assert (r.timestamp_begin, r.blank, r.no_speech, r.max_initial_timestamp_index) == (-1, -1, -1, -1)
    assert DecodeRules(**GOOD).sot_indices([[193, 1], [5, 6, 193, 2]]) == [0, 2]


@pytest.mark.parametrize("change, match", [
    (dict(eot=257), "end-of-text token 257"),
    (dict(eot=-1), "end-of-text token -1"),
    (dict(timestamp_begin=192), "timestamp_begin = 192"),             # eot < timestamp_begin
    (dict(timestamp_begin=258), "timestamp_begin = 258"),
    (dict(timestamp_begin=0), "timestamp_begin = 0"),
    (dict(no_timestamps=257), "no_timestamps token 257"),
    (dict(blank=300), "blank token 300"),
    (dict(blank=-2), "blank token -2"),
    (dict(no_speech=257), "no_speech token 257"),
    (dict(sot=999), "sot token 999"),
    (dict(sot=-1), "give its id as sot"),
    (dict(max_initial_timestamp_index=57), "max_initial_timestamp_index = 57"),      # 257 - 200 = 57 timestamps: indices 0..56
    (dict(max_initial_timestamp_index=-2), "max_initial_timestamp_index = -2"),
])
def test_decode_refuses_bad_rules_before_any_launch(dec, change, match):
    rules = DecodeRules(**{**GOOD, **change})
    with pytest.raises(RuntimeError, match=match):
        dec.decode([[193, 194, 197]], rules, 4)


def test_decode_refuses_a_prompt_without_sot_and_a_batch_above_max_batch(dec):
    with pytest.raises(RuntimeError, match="prompt 1 does not hold the sot token 193"):
        dec.decode([[193, 194], [1, 2, 3]], DecodeRules(**GOOD), 4)
    with pytest.raises(RuntimeError, match="batch 4 exceeds the handle's max_batch 3"):
        dec.decode([[193]] * 4, DecodeRules(**GOOD), 4)


def test_detect_language_refuses_bad_lists_before_any_launch(dec):
    for ids, sot in (([], 193), ([194, 194], 193), ([194, 257], 193), ([-1], 193), ([194, 195], 257)):
        with pytest.raises(RuntimeError, match="outside the vocabulary|distinct ids"):
            dec.detect_language(sot, ids)
    dec.batch = 0
    with pytest.raises(RuntimeError, match="begin"):
        dec.detect_language(193, [194, 195])


def test_transcribe_without_timestamps_refuses_detection():
    tr = object.__new__(T.Transcriber)
    tr.specials = T.SpecialTokens.multilingual()
    with pytest.raises(RuntimeError, match="timestamps=True"):
        tr.transcribe(np.zeros(16000, np.float32), language=None)
