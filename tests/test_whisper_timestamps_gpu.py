"""Decoding under the reference's logit rules on the device (mf_whisper_decoder_decode / _choose / _detect_language) against goldens recorded
from the reference's own SuppressBlank, SuppressTokens, ApplyTimestampRules, GreedyDecoder and detect_language
(tests/golden/make_whisper_timestamps_golden.py).

Gates.  Choose cases: token and done flag equal; the log-probability within `choose_logprob_gate` = 8 x the largest gap between the reference's
own float32 filters + log-softmax and float64 on the same cases (1.6e-6 -> 1.3e-5; recorded by the generator, not taken from the kernel).
Decode runs: ids equal token for token (the generator asserts a margin of 4 x GATE x max|logit| on both of the step's decisions); summed
log-probabilities within 2 x GATE x max|logit| x (tokens + 1), the formula of tests/test_whisper_decoder_gpu.py; no-speech and language
probabilities within 2 x GATE x max|logit| (a probability moves by at most the logit's error plus the log-sum-exp's)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mere_fusion_amd import weights as W
from mere_fusion_amd.musetalk.whisper import weights as DW

pytestmark = pytest.mark.gpu

GATE = 3e-4


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "whisper_timestamps_golden.npz")))
    assert g["gate"] == GATE and g["small_margin"] >= 4 * GATE and g["tiny_margin"] >= 4 * GATE
    assert g["choose_logprob_gate"] == 8 * g["choose_ref_fp32_vs_fp64"]
    return g


@pytest.fixture(scope="module")
def old_gold():
    return dict(np.load(os.path.join(GOLDEN, "whisper_decoder_golden.npz")))


@pytest.fixture(scope="module")
def decoders(lib_built, gold, old_gold):
    from mere_fusion_amd.musetalk.whisper.decoder import WhisperDecoder
    cache = {}

    def make(geom, precision="bf16x3"):
        """small: the timestamp golden's weights (3 sequences); small8: any small weights, 8 sequences (the choose seam reads no weight);
        old_small: the greedy golden's weights; tiny / tiny_post: the tiny dims without / with encoder.ln_post, 2 sequences"""
        if (geom, precision) not in cache:
            tb_small = int(gold["small_tokens"][4])
            if geom in ("small", "small8"):
                sd = DW.make_decoder_state_dict(int(gold["small_seed"]), DW.WHISPER_SMALL_TEST, timestamp_begin=tb_small, timestamp_gain=float(gold["small_gain"]))
                cache[geom, precision] = WhisperDecoder(sd, n_head=2, precision=precision, max_batch=8 if geom == "small8" else 3)
            elif geom == "old_small":
                cache[geom, precision] = WhisperDecoder(DW.make_decoder_state_dict(int(old_gold["small_seed"]), DW.WHISPER_SMALL_TEST), n_head=2, precision=precision, max_batch=3)
            else:
                sd = DW.make_decoder_state_dict(int(gold["tiny_seed"]), DW.WHISPER_TINY_TEXT, timestamp_begin=int(gold["tokenizer_facts"][4]), timestamp_gain=float(gold["tiny_gain"]))
                if geom == "tiny_post":
                    esd = W.make_whisper_encoder_state_dict(0)
                    sd.update({"encoder.ln_post." + k: esd["ln_post." + k] for k in ("weight", "bias")})
                cache[geom, precision] = WhisperDecoder(sd, n_head=6, precision=precision, max_batch=2)
        return cache[geom, precision]

    return make


def small_rules(gold, **change):
    from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["small_tokens"])
    kw = dict(eot=eot, timestamp_begin=tb, no_timestamps=no_ts, max_initial_timestamp_index=int(gold["small_max_init"]), blank=blank, no_speech=no_speech, sot=sot)
    kw.update(change)
    return DecodeRules(**kw)


def tiny_rules(gold):
    from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["tokenizer_facts"])
    return DecodeRules(eot, timestamp_begin=tb, no_timestamps=no_ts, max_initial_timestamp_index=50, blank=blank, no_speech=no_speech, sot=sot)


def logprob_tol(n_tokens, gate, absmax):
    """tests/test_whisper_decoder_gpu.py: every chosen token's log-probability moves by at most 2 x the logits' error"""
    return 2 * gate * absmax * (np.asarray(n_tokens) + 1)


# ---- the choose kernel alone ------------------------------------------------------------------------------------------------
def case_logits(gold, name):
    p = f"choose_{name}_"
    if p + "logits" in gold:
        return gold[p + "logits"]
    V = 51865
    lg = (np.random.default_rng(int(gold[p + "seed"])).standard_normal(V) * float(gold[p + "scale"])).astype(np.float32)
    lg[V - len(gold[p + "ts_row"]):] = gold[p + "ts_row"]
    lg[gold[p + "plant_ids"]] = gold[p + "plant_vals"]
    assert float(lg.astype(np.float64).sum()) == float(gold[p + "checksum"]), "the seeded base of this case is not the one the golden was recorded on"
    return lg[None]


def test_the_golden_holds_every_case_the_kernel_must_meet(gold):
    names = set(str(n) for n in gold["choose_names"])
    assert {"first_cap", "first_blank", "pair_ts_ts", "n1_ts", "ts_text_eot", "ts_text_ts", "lse_fires", "lse_not", "no_timestamps_max", "timestamp_begin_max",
            "tie_text", "tie_ts", "nothing", "batch8", "big_first_cap", "big_lse_fires", "big_lse_not", "big_tie"} <= names


@pytest.mark.parametrize("name", ["first_cap", "first_blank", "pair_ts_ts", "n1_ts", "ts_text_eot", "ts_text_ts", "lse_fires", "lse_not", "no_timestamps_max",
                                  "timestamp_begin_max", "tie_text", "tie_ts", "nothing", "no_cap", "no_blank_rule", "batch8",
                                  "big_first_cap", "big_lse_fires", "big_lse_not", "big_tie", "big_diffuse_text"])
def test_choose_equals_the_reference_filters(decoders, gold, name):
    from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules
    p = f"choose_{name}_"
    big = name.startswith("big_")
    dec = decoders("tiny" if big else "small8")
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["tokenizer_facts" if big else "small_tokens"])
    rules = DecodeRules(eot, timestamp_begin=tb, no_timestamps=no_ts, max_initial_timestamp_index=int(gold[p + "max_init"]), blank=blank if int(gold[p + "blank_on"]) else -1)
    logits = torch.from_numpy(case_logits(gold, name)).cuda()
    done_in = gold[p + "done_in"]
    B = len(done_in)
    sentinel_t, sentinel_lp = np.full(B, -7, np.int32), np.full(B, -7.0, np.float32)
    runs = [dec.choose(logits, gold[p + "hist"], rules, suppress=gold[p + "suppress"].tolist(), tokens=sentinel_t, logprobs=sentinel_lp, done=done_in) for _ in range(2)]
    tok, lp, done = runs[0]
    err = np.abs(lp.astype(np.float64) - gold[p + "logprob"])
    print(f"choose {name}: tokens {tok.tolist()} done {done.tolist()} log-probability error {err.max():.3e} (gate {float(gold['choose_logprob_gate']):.3e})")
    assert tok.tolist() == gold[p + "token"].tolist() and done.tolist() == gold[p + "done"].tolist()
    assert (err <= float(gold["choose_logprob_gate"])).all()
    for b in np.flatnonzero(done_in):                                   # a finished sequence keeps what the outputs held
        assert tok[b] == -7 and lp[b] == -7.0 and done[b] == 1
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


# ---- decode with rules ----------------------------------------------------------------------------------------------------------
def small_batch(gold):
    prompts = [gold[f"small_prompt_{b}"].tolist() for b in range(3)]
    ids = [gold[f"small_ids_{b}"].tolist() for b in range(3)]
    lps = np.asarray([float(gold[f"small_logprob_{b}"]) for b in range(3)])
    nsp = np.asarray([float(gold[f"small_no_speech_{b}"]) for b in range(3)])
    return prompts, ids, lps, nsp


@pytest.fixture(scope="module")
def small_run(decoders, gold):
    prompts = small_batch(gold)[0]
    enc = torch.from_numpy(gold["small_enc"]).cuda()

    def run(precision="bf16x3", max_new=None, check_every=8, detect=False):
        dec = decoders("small", precision)
        dec.begin(enc)
        if detect:
            dec.detect_language(int(gold["small_tokens"][1]), [194, 195, 196])
        ids, lp, nsp = dec.decode(prompts, small_rules(gold), max_new or int(gold["small_max_new"]), suppress=gold["small_suppress"].tolist(), check_every=check_every)
        return ids, lp, nsp, dec.last_out.copy()

    return run


def test_decode_small_batch_equals_the_golden(small_run, gold):
    _, want_ids, want_lp, want_nsp = small_batch(gold)
    ids, lp, nsp, _ = small_run()
    tb = int(gold["small_tokens"][4])
    assert any(t >= tb for i in want_ids for t in i) and any(t < tb for i in want_ids for t in i)
    assert ids == want_ids
    absmax = float(gold["small_absmax"])
    tol = logprob_tol([len(i) for i in want_ids], GATE, absmax)
    print("summed log-probabilities", lp, "golden", want_lp, "tolerance", tol)
    print("no-speech probabilities", nsp, "golden", want_nsp, "tolerance", 2 * GATE * absmax)
    assert (np.abs(lp - want_lp) <= tol).all()
    assert (np.abs(nsp - want_nsp) <= 2 * GATE * absmax).all()


def test_decode_does_not_depend_on_check_every(small_run):
    ids, lp, nsp, out = small_run(check_every=8)
    for ce in (8, 1, 3):
        ids2, lp2, nsp2, out2 = small_run(check_every=ce)
        assert ids2 == ids and lp2.tobytes() == lp.tobytes() and nsp2.tobytes() == nsp.tobytes() and np.array_equal(out2, out), ce


def test_a_finished_sequence_keeps_its_cache_rows(decoders, small_run, gold):
    dec = decoders("small")
    _, want_ids, _, _ = small_batch(gold)
    lens = [len(i) for i in want_ids]
    seq = int(np.argmin(lens))
    assert lens[seq] < max(lens)                                          # it meets end-of-text while the others still run
    budget = lens[seq] + 1

    def snapshot():
        return [dec.cache(layer, seq) for layer in range(dec.n_layer)]

    ids_a, lp_a, _, out_a = small_run(max_new=budget)
    before = snapshot()
    ids_b, lp_b, _, out_b = small_run()
    after = snapshot()
    assert ids_a[seq] == ids_b[seq] == want_ids[seq] and lp_a[seq].tobytes() == lp_b[seq].tobytes()
    assert out_a[seq].tobytes() == out_b[seq, :budget].tobytes() and not out_b[seq, budget:].any()
    for (k0, v0, n0), (k1, v1, n1) in zip(before, after):
        assert n0 == n1 == len(gold[f"small_prompt_{seq}"]) + lens[seq]
        assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes()
        assert not k1[n1:].any() and not v1[n1:].any() and k1[:n1].any()


def test_decode_small_batch_bf16(small_run, gold):
    """the single-plane precision against the same golden: ids where the golden's margins allow it, log-probabilities within 2**8 x the gate"""
    _, want_ids, want_lp, want_nsp = small_batch(gold)
    ids, lp, nsp, _ = small_run("bf16")
    gate = GATE * 2 ** 8
    absmax = float(gold["small_absmax"])
    print(f"bf16: golden margin {float(gold['small_margin']):.2e} of max|logit| against a gate of {gate:.2e}: ids equal: {[a == b for a, b in zip(ids, want_ids)]}")
    print("bf16 no-speech", nsp, "golden", want_nsp, "summed log-probabilities", lp, "golden", want_lp)
    assert (np.abs(nsp - want_nsp) <= 2 * gate * absmax).all()           # the prefill's sot row: no decision stands before it
    if float(gold["small_margin"]) >= 4 * gate:
        assert ids == want_ids
    for b in range(3):                                                     # reported above otherwise: a 3.6e-3 margin does not bind a 7.7e-2 gate
        if ids[b] == want_ids[b]:
            assert abs(lp[b] - want_lp[b]) <= logprob_tol([len(ids[b])], gate, absmax)[0]


@pytest.mark.parametrize("which", ["tiny", "wire"])
def test_decode_tiny_equals_the_golden(decoders, gold, which):
    if which == "tiny":
        dec = decoders("tiny")
        enc = torch.from_numpy(np.random.default_rng(int(gold["tiny_enc_seed"])).standard_normal((1, 1500, 384)).astype(np.float32)).cuda()
    else:
        from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
        from mere_fusion_amd.transcribe import Transcriber
        dec = decoders("tiny_post")
        tr = Transcriber(Audio2Feature(state_dict=W.make_whisper_encoder_state_dict(0), n_head=6), dec, suppress=gold["tiny_suppress"].tolist())
        enc = tr._encode(W.make_speech_like_wav(16000, int(gold["wire_wav_seed"])))[None]
    dec.begin(enc)
    ids, lp, nsp = dec.decode([gold["tiny_prompt"].tolist()], tiny_rules(gold), 24, suppress=gold["tiny_suppress"].tolist())
    want = gold[f"{which}_ids"].tolist()
    tb = int(gold["tokenizer_facts"][4])
    absmax = float(gold[f"{which}_absmax"])
    tol = logprob_tol([len(want)], GATE, absmax)[0]
    print(f"{which}: summed log-probability {lp[0]} golden {float(gold[which + '_logprob'])} tolerance {tol}; no-speech {nsp[0]} golden {float(gold[which + '_no_speech'])}")
    assert ids[0] == want and any(t >= tb for t in want) and any(t < tb for t in want)
    assert abs(lp[0] - float(gold[f"{which}_logprob"])) <= tol
    assert abs(nsp[0] - float(gold[f"{which}_no_speech"])) <= 2 * GATE * absmax


# ---- rules off ---------------------------------------------------------------------------------------------------------------------
def test_rules_off_is_bit_equal_to_greedy(decoders, old_gold):
    from mere_fusion_amd.musetalk.whisper.decoder import DecodeRules
    dec = decoders("old_small")
    prompts = [old_gold[f"small_prompt_{b}"].tolist() for b in range(3)]
    enc = torch.from_numpy(old_gold["small_enc_70"]).cuda()
    mask = dec.suppress_mask(old_gold["small_suppress"].tolist())
    eot = int(old_gold["small_eot"])
    dec.begin(enc)
    ids_g, lp_g = dec.greedy(prompts, eot, 80, suppress=mask)
    out_g = dec.last_out.copy()
    dec.begin(enc)
    ids_d, lp_d, nsp = dec.decode(prompts, DecodeRules(eot), 80, suppress=mask)
    assert ids_g == ids_d == [old_gold[f"small_ids_{b}"].tolist() for b in range(3)]
    assert lp_g.tobytes() == lp_d.tobytes() and out_g.tobytes() == dec.last_out.tobytes() and np.isnan(nsp).all()


# ---- language detection ------------------------------------------------------------------------------------------------------------
def test_detect_language_equals_the_reference(decoders, gold):
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    from mere_fusion_amd.transcribe import Transcriber
    dec = decoders("tiny_post")
    tr = Transcriber(Audio2Feature(state_dict=W.make_whisper_encoder_state_dict(0), n_head=6), dec, suppress=gold["tiny_suppress"].tolist())
    wire = tr._encode(W.make_speech_like_wav(16000, int(gold["wire_wav_seed"])))
    # golden row 0: seeded features handed to the decoder as they are (no ln_post) -> the plain handle; row 1: the wiring wave through the encoder
    seeded = torch.from_numpy(np.random.default_rng(int(gold["tiny_enc_seed"])).standard_normal((1, 1500, 384)).astype(np.float32)).cuda()
    sot = int(gold["tokenizer_facts"][1])
    langs = gold["lang_tokens"].tolist()
    tol = 2 * GATE * float(gold["lang_absmax"])
    for row, (d, enc) in enumerate(((decoders("tiny"), seeded), (dec, wire[None]))):
        d.begin(enc)
        chosen, probs = d.detect_language(sot, langs)
        err = np.abs(probs[0].astype(np.float64) - gold["lang_probs"][row]).max()
        print(f"detect_language row {row}: chosen {chosen.tolist()} golden {int(gold['lang_chosen'][row])}; probabilities off by {err:.3e} (tolerance {tol:.3e})")
        assert chosen.tolist() == [int(gold["lang_chosen"][row])] and err <= tol and abs(float(probs.sum()) - 1) < 1e-5
        for layer in range(d.n_layer):
            k, v, n = d.cache(layer, 0)
            assert n == 0 and not k.any() and not v.any()                  # the handle stands as after begin()
    with pytest.raises(RuntimeError, match="directly after"):
        dec.logits([[1]])
        dec.detect_language(sot, langs)


def test_a_decode_after_detection_equals_one_without(small_run):
    ids, lp, nsp, out = small_run()
    ids2, lp2, nsp2, out2 = small_run(detect=True)
    assert ids2 == ids and lp2.tobytes() == lp.tobytes() and nsp2.tobytes() == nsp.tobytes() and out2.tobytes() == out.tobytes()


# ---- refusals that need the handle ----------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_wrapper_refuses(decoders, gold):
    """straight at the C ABI, past the wrapper's own checks: refused through mf_last_error, and the handle decodes afterwards as before"""
    import ctypes as C
    from mere_fusion_amd import _lib
    dec = decoders("small")
    prompts, want_ids, _, _ = small_batch(gold)
    enc = torch.from_numpy(gold["small_enc"]).cuda()
    dec.begin(enc[:1])
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["small_tokens"])
    p = (C.c_int * 3)(*prompts[0])
    n = (C.c_int * 1)(3)
    out, ol, lp, ns = np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.float32)

    def call(tb_=tb, no_ts_=no_ts, mi=5, blank_=blank, nsp_=no_speech, sot_index=0, eot_=eot):
        si = (C.c_int * 1)(sot_index)
        return _lib.lib().mf_whisper_decoder_decode(dec._h, p, n, None, eot_, 4, 8, tb_, no_ts_, mi, blank_, nsp_, si, out.ctypes.data, ol.ctypes.data, lp.ctypes.data, ns.ctypes.data, 1, None)

    for kw, match in ((dict(tb_=eot), "timestamp_begin"), (dict(tb_=258), "timestamp_begin"), (dict(no_ts_=257), "no_timestamps"), (dict(mi=57), "max_initial"),
                      (dict(blank_=257), "blank"), (dict(nsp_=257), "no_speech"), (dict(sot_index=3), "sot index 3"), (dict(sot_index=-1), "sot index -1"), (dict(eot_=257), "end-of-text")):
        with pytest.raises(RuntimeError, match=match):
            _lib.check(call(**kw), "decode")
    for layer in range(dec.n_layer):
        k, v, length = dec.cache(layer, 0)
        assert length == 0 and not k.any()                                 # nothing was launched
    with pytest.raises(RuntimeError, match="max_batch"):
        dec.choose(torch.zeros((4, 257), device="cuda"), np.zeros((4, 3), np.int32), small_rules(gold))
    hist = np.asarray([[1, 257, 0]], np.int32)
    tok, l, d = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    with pytest.raises(RuntimeError, match="history token 257"):
        _lib.check(_lib.lib().mf_whisper_decoder_choose(dec._h, torch.zeros((1, 257), device="cuda").data_ptr(), hist.ctypes.data, None, eot, tb, no_ts, 5, blank,
                                                        tok.ctypes.data, l.ctypes.data, d.ctypes.data, 1, None), "choose")
    ids, _, _ = dec.decode(prompts[:1], small_rules(gold), int(gold["small_max_new"]), suppress=gold["small_suppress"].tolist())
    assert ids[0] == want_ids[0]


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
def test_transcriber_with_timestamps_returns_the_reference_ids_and_segments(decoders, gold):
    from mere_fusion_amd import transcribe as T
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["tokenizer_facts"])
    sp = T.SpecialTokens.multilingual()
    sp.blank = blank                                                       # what SpecialTokens.from_tokenizer reads from the tokenizer
    tr = T.Transcriber(Audio2Feature(state_dict=W.make_whisper_encoder_state_dict(0), n_head=6), decoders("tiny_post"), specials=sp, suppress=gold["tiny_suppress"].tolist())
    assert tr.prompt("en", timestamps=True) == gold["tiny_prompt"].tolist()
    r = tr.rules()
    assert (r.timestamp_begin, r.no_timestamps, r.max_initial_timestamp_index, r.blank, r.no_speech, r.sot) == (tb, no_ts, 50, blank, no_speech, sot)
    t = tr.transcribe(W.make_speech_like_wav(16000, int(gold["wire_wav_seed"])), language="en", timestamps=True, max_new=24)
    want = gold["wire_ids"].tolist()
    assert t.ids == [i for i in want if i < tb]
    # the golden's ids cut by hand (seeded weights: the timestamps follow no clock): nine text tokens up to the pair <|6.32|><|6.32|>, one up to the pair
    # <|21.30|><|6.32|>, one up to <|9.86|><|23.66|>, one up to <|9.56|><|4.92|>, and two closed by the single <|6.32|> at the end
    by_hand = [(0.0, 6.32, [46650] * 9), (6.32, 21.3, [8480]), (6.32, 9.86, [46650]), (23.66, 9.56, [46650]), (4.92, 4.92, [28989, 46650])]
    assert len(t.segments) == len(by_hand)
    for (a0, b0, i0), (a1, b1, i1) in zip(t.segments, by_hand):
        assert a0 == pytest.approx(a1) and b0 == pytest.approx(b1) and i0 == i1
    assert t.segments == T.cut_segments(want, tb, 0.0, 1.0)
    assert abs(t.avg_logprob[0] - float(gold["wire_logprob"]) / (len(want) + 1)) <= logprob_tol([len(want)], GATE, float(gold["wire_absmax"]))[0] / (len(want) + 1)
    assert abs(t.no_speech_prob[0] - float(gold["wire_no_speech"])) <= 2 * GATE * float(gold["wire_absmax"])
    ids_plain = tr.transcribe(W.make_speech_like_wav(16000, int(gold["wire_wav_seed"])), language="en", max_new=4)
    assert isinstance(ids_plain, list) and len(ids_plain) <= 4             # the default call returns what it always did: a list of ids


def test_transcriber_detects_the_language_and_writes_it_into_the_prompt(decoders, gold, old_gold):
    """`language=None`: detection after begin, the chosen token behind <|startoftranscript|> (decoding.py:579-589); alone and in a batch of two"""
    from mere_fusion_amd import transcribe as T
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    eot, sot, no_speech, no_ts, tb, blank = (int(v) for v in gold["tokenizer_facts"])
    codes = [str(c) for c in old_gold["lang_codes"]]
    sp = T.SpecialTokens.multilingual(codes)
    sp.blank = blank
    assert [sp.language_tokens[c] for c in codes] == gold["lang_tokens"].tolist()
    dec = decoders("tiny_post")
    tr = T.Transcriber(Audio2Feature(state_dict=W.make_whisper_encoder_state_dict(0), n_head=6), dec, specials=sp, suppress=gold["tiny_suppress"].tolist())
    wav = W.make_speech_like_wav(16000, int(gold["wire_wav_seed"]))
    chosen = int(gold["lang_chosen"][1])                                   # the reference's detect_language on this wave
    code = codes[gold["lang_tokens"].tolist().index(chosen)]
    t = tr.transcribe(wav, language=None, timestamps=True, max_new=12)
    assert t.languages == [code] and len(t.avg_logprob) == len(t.no_speech_prob) == 1
    # the same window decoded by hand with that language token in the prompt
    dec.begin(tr._encode(wav)[None])
    ids, lp, nsp = dec.decode([[sot, chosen, sp.transcribe]], tr.rules(), 12, suppress=gold["tiny_suppress"].tolist())
    assert t.ids == [i for i in ids[0] if i < tb] and t.segments == T.cut_segments(ids[0], tb, 0.0, 1.0)
    assert t.avg_logprob[0] == pytest.approx(float(lp[0]) / (len(ids[0]) + 1), rel=1e-6) and t.no_speech_prob[0] == float(nsp[0])
    assert abs(t.no_speech_prob[0] - float(gold["wire_no_speech"])) <= 2 * GATE * float(gold["wire_absmax"])   # the sot row stands before the language token
    named = tr.transcribe(wav, language=code, timestamps=True, max_new=12)
    assert named.ids == t.ids and named.segments == t.segments and named.languages == []
    # two utterances in one call: one Transcript each, the first equal to the window alone
    other = W.make_speech_like_wav(12000, 3)
    both = tr.transcribe_batch([wav, other], timestamps=True, max_new=12)
    assert len(both) == 2 and both[0].ids == t.ids and both[0].segments == t.segments and both[0].languages == [code]
    assert len(both[1].languages) == 1 and both[1].languages[0] in codes and all(b <= 30.0 for _, b, _ in both[1].segments)
    plain = tr.transcribe_batch([wav, other], max_new=4)
    assert len(plain) == 2 and all(isinstance(i, list) for i in plain)     # the default call returns what it always did


def test_decode_batch_of_eight_with_no_speech(decoders, gold):
    """max_batch sequences with the no-speech row on: the prefill's head call has 16 rows, two row blocks of the linear kernel.  The golden's three
    sequences, repeated in another order, must each come out as the golden has them"""
    dec = decoders("small8")
    prompts, want_ids, want_lp, want_nsp = small_batch(gold)
    order = [0, 1, 2, 2, 0, 1, 1, 2]
    dec.begin(torch.from_numpy(gold["small_enc"][order]).cuda())
    ids, lp, nsp = dec.decode([prompts[b] for b in order], small_rules(gold), int(gold["small_max_new"]), suppress=gold["small_suppress"].tolist())
    absmax = float(gold["small_absmax"])
    assert ids == [want_ids[b] for b in order]
    assert (np.abs(lp - want_lp[order]) <= logprob_tol([len(want_ids[b]) for b in order], GATE, absmax)).all()
    assert (np.abs(nsp - want_nsp[order]) <= 2 * GATE * absmax).all()
    for i, b in enumerate(order):                                           # a row's arithmetic does not depend on its place in the batch
        j = order.index(b)
        assert nsp[i].tobytes() == nsp[j].tobytes() and lp[i].tobytes() == lp[j].tobytes()
