"""CPU side of the transcription path: the decoder's weight keys, the 30 s windowing and the start-sequence builder, against facts recorded from
the reference's own modules (tests/golden/make_whisper_decoder_golden.py: `Whisper.state_dict()`, tokenizer.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mere_fusion_amd import transcribe as T
from mere_fusion_amd.musetalk.whisper import weights as DW


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "whisper_decoder_golden.npz")))


def test_decoder_keys_are_the_reference_state_dict_names(gold):
    d = DW.WHISPER_SMALL_TEST
    want = {str(k): tuple(int(v) for v in s if v) for k, s in zip(gold["ref_decoder_keys"], gold["ref_decoder_shapes"])}
    mine = {k: tuple(f(d["n_vocab"], d["n_text_ctx"], d["n_text_state"])) for k, f in DW.decoder_keys(d["n_text_layer"]).items()}
    assert mine == want
    sd = DW.make_decoder_state_dict(0, d)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any(k.endswith("key.bias") for k in mine) and len(mine) == 4 + 24 * d["n_text_layer"]


def test_decoder_state_dict_takes_the_decoder_half_and_ln_post():
    full = {"encoder.conv1.weight": 1, "encoder.ln_post.weight": 2, "encoder.ln_post.bias": 3, "decoder.ln.weight": 4, "decoder.blocks.0.mlp.0.bias": 5}
    assert DW.decoder_state_dict(full) == {"encoder.ln_post.weight": 2, "encoder.ln_post.bias": 3, "decoder.ln.weight": 4, "decoder.blocks.0.mlp.0.bias": 5}
    assert DW.decoder_state_dict(full, with_ln_post=False) == {"decoder.ln.weight": 4, "decoder.blocks.0.mlp.0.bias": 5}


def test_windows_cut_thirty_seconds():
    S = T.N_SAMPLES_SEGMENT
    assert S == 480000
    assert T.windows(16000) == [(0, 16000)]
    assert T.windows(S) == [(0, S)]
    assert T.windows(S + 1) == [(0, S)]                                  # a 1-sample tail holds no log-mel frame
    assert T.windows(S + T.MIN_TAIL) == [(0, S), (S, S + T.MIN_TAIL)]
    assert T.windows(2 * S + 12345) == [(0, S), (S, 2 * S), (2 * S, 2 * S + 12345)]
    assert T.windows(0) == [] and T.windows(T.MIN_TAIL - 1) == []
    cuts = T.windows(5 * S + 7777)
    assert all(a2 == b1 for (_, b1), (a2, _) in zip(cuts, cuts[1:])) and all(b - a <= S for a, b in cuts)


def test_start_sequence_equals_the_reference_tokenizer(gold):
    added = {str(k): int(v) for k, v in zip(gold["added_tokens"], gold["added_ids"])}
    eot, sot, sot_lm, sot_prev, no_speech, no_ts = (int(v) for v in gold["specials"])
    for sp in (T.SpecialTokens.from_added_tokens(added, eot), T.SpecialTokens.multilingual([str(c) for c in gold["lang_codes"]])):
        assert (sp.eot, sp.sot, sp.sot_lm, sp.sot_prev, sp.no_speech, sp.no_timestamps) == (eot, sot, sot_lm, sot_prev, no_speech, no_ts)
        assert len(sp.language_tokens) == len(gold["lang_codes"]) == 99
        for lang, task in (("en", "transcribe"), ("de", "translate"), ("zh", "transcribe")):
            assert T.start_sequence(sp, lang, task) == gold[f"sot_{lang}_{task}"].tolist()
            assert T.start_sequence(sp, lang, task, timestamps=True) == gold[f"sot_{lang}_{task}"].tolist()[:-1]
    only_en = T.SpecialTokens.multilingual()
    assert T.start_sequence(only_en) == gold["sot_en_transcribe"].tolist() == gold["tiny_prompt"].tolist()
    with pytest.raises(ValueError, match="language"):
        T.start_sequence(only_en, "de")
    with pytest.raises(ValueError, match="task"):
        T.start_sequence(only_en, "en", "summarise")


def test_special_tokens_from_a_tokenizer_directory(tmp_path, gold):
    import json
    added = {str(k): int(v) for k, v in zip(gold["added_tokens"], gold["added_ids"])}
    (tmp_path / "added_tokens.json").write_text(json.dumps(added))
    sp = T.SpecialTokens.from_dir(str(tmp_path))
    assert T.start_sequence(sp, "zh") == gold["sot_zh_transcribe"].tolist()
    assert not set(gold["non_speech_tokens"].tolist()) & {sp.eot, sp.sot, sp.no_timestamps}
