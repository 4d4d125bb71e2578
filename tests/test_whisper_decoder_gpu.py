"""Whisper text decoder on the device (mf_whisper_decoder_*) against the float64 goldens recorded from the reference's own `TextDecoder`
(tests/golden/make_whisper_decoder_golden.py): teacher-forced logits, the step path, greedy decoding, refusals, and the Transcriber wiring.

Gates.  GATE_X3 = 3e-4 relative to max|logits| is the encoder parity test's (tests/test_whisper.py: TOL_FEAT 2e-3 at |x| ~ 6); the generator
asserts a margin of 4 x that gate at every greedy step.  The encoder test has no single-plane figure; GATE_BF16 = 2**8 x GATE_X3 because a
bf16 operand carries 8 mantissa bits (unit roundoff 2**-9) where a (hi, lo) pair carries 16 (2**-17).  The reference's own float32 stands
9.8e-7 from its float64 on the tiny row (recorded in the golden), so the encoder gate is the larger of the two and is used as it is."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mere_fusion_amd import weights as W
from mere_fusion_amd.musetalk.whisper import weights as DW

pytestmark = pytest.mark.gpu

GATE = {"bf16x3": 3e-4, "bf16": 3e-4 * 2 ** 8}
ROWS = (1, 63, 64, 65, 79)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLDEN, "whisper_decoder_golden.npz")))
    assert g["gate"] == GATE["bf16x3"] and g["small_margin"] >= 4 * GATE["bf16x3"] and g["tiny_margin"] >= 4 * GATE["bf16x3"]
    return g


@pytest.fixture(scope="module")
def decoders(lib_built, gold):
    """WhisperDecoder per (geometry, precision), built once"""
    from mere_fusion_amd.musetalk.whisper.decoder import WhisperDecoder
    cache = {}

    def make(geom, precision="bf16x3"):
        """small: the reduced geometry, 3 sequences; tiny: the published tiny dims; tiny_post: tiny with encoder.ln_post, as a deployment builds it"""
        if (geom, precision) not in cache:
            if geom == "small":
                sd = DW.make_decoder_state_dict(int(gold["small_seed"]), DW.WHISPER_SMALL_TEST)
                cache[geom, precision] = WhisperDecoder(sd, n_head=2, precision=precision, max_batch=3)
            else:
                sd = DW.make_decoder_state_dict(int(gold["tiny_seed"]), DW.WHISPER_TINY_TEXT)
                if geom == "tiny_post":
                    esd = W.make_whisper_encoder_state_dict(0)
                    sd.update({"encoder.ln_post." + k: esd["ln_post." + k] for k in ("weight", "bias")})
                cache[geom, precision] = WhisperDecoder(sd, n_head=6, precision=precision, max_batch=1)
        return cache[geom, precision]

    return make


def rel_err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def small_batch(gold):
    prompts = [gold[f"small_prompt_{b}"].tolist() for b in range(3)]
    ids = [gold[f"small_ids_{b}"].tolist() for b in range(3)]
    lps = np.asarray([float(gold[f"small_logprob_{b}"]) for b in range(3)])
    return prompts, ids, lps


def logprob_tol(n_tokens, gate, absmax):
    """every chosen token's log-probability moves by at most 2 x the logits' error (the logit itself and the log-sum-exp)"""
    return 2 * gate * absmax * (np.asarray(n_tokens) + 1)


# ---- logits parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("t_audio", [7, 70])
@pytest.mark.parametrize("n", ROWS)
def test_teacher_forced_logits_small(decoders, gold, precision, t_audio, n):
    dec = decoders("small", precision)
    dec.begin(torch.from_numpy(gold[f"small_enc_{t_audio}"][:1]).cuda())
    got = dec.logits(gold[f"small_row_{n}"])[0].cpu().numpy()
    want = gold[f"small_logits_{t_audio}_{n}"]
    assert got.shape == want.shape == (n, 257)
    err = rel_err(got, want)
    print(f"small logits {precision} T_audio={t_audio} n={n}: max err / max|logit| = {err:.3e} (gate {GATE[precision]:.1e})")
    assert err <= GATE[precision]


def tiny_enc(gold):
    return torch.from_numpy(np.random.default_rng(int(gold["tiny_enc_seed"])).standard_normal((1, 1500, 384)).astype(np.float32)).cuda()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_teacher_forced_logits_tiny(decoders, gold, precision):
    plain = decoders("tiny", precision)
    assert (plain.n_layer, plain.n_text_ctx, plain.n_state, plain.n_vocab) == (4, 448, 384, 51865)
    plain.begin(tiny_enc(gold))
    got = plain.logits(gold["tiny_row"])[0].cpu().numpy()
    absmax = float(gold["tiny_logits_absmax"])
    stride = int(gold["tiny_stride"])
    e1 = np.abs(got[:, ::stride].astype(np.float64) - gold["tiny_logits_sample"]).max() / absmax
    e2 = np.abs(got.max(axis=1).astype(np.float64) - gold["tiny_logits_max"]).max() / absmax
    print(f"tiny logits {precision}: sampled columns {e1:.3e}, row maxima {e2:.3e} of max|logit| (gate {GATE[precision]:.1e}; reference fp32 vs fp64 "
          f"{float(gold['tiny_ref_fp32_vs_fp64']):.1e})")
    assert max(e1, e2) <= GATE[precision]
    if precision == "bf16x3":
        assert np.array_equal(got.argmax(axis=1), gold["tiny_logits_argmax"])


# ---- the step path against the one-pass path ------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 79])
def test_token_by_token_equals_one_pass(decoders, gold, n):
    dec = decoders("small")
    enc = torch.from_numpy(gold["small_enc_70"][:1]).cuda()
    row = gold[f"small_row_{n}"]
    dec.begin(enc)
    whole = dec.logits(row)[0].cpu().numpy()
    dec.begin(enc)
    steps = np.concatenate([dec.logits(row[i:i + 1])[0].cpu().numpy() for i in range(n)], axis=0)
    want = gold[f"small_logits_70_{n}"]
    err = rel_err(steps, whole.astype(np.float64))
    print(f"n={n}: token by token vs one pass {err:.3e}; token by token vs golden {rel_err(steps, want):.3e}")
    assert err <= GATE["bf16x3"] and rel_err(steps, want) <= GATE["bf16x3"]
    with pytest.raises(RuntimeError, match="n_text_ctx"):
        dec.logits(row[: 80 - n + 1])                          # one more than the cache holds


# ---- greedy ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_run(decoders, gold):
    dec = decoders("small")
    prompts, _, _ = small_batch(gold)
    enc = torch.from_numpy(gold["small_enc_70"]).cuda()
    mask = dec.suppress_mask(gold["small_suppress"].tolist())

    def run(max_new=80, check_every=8, which=(0, 1, 2)):
        dec.begin(enc[list(which)])
        room = 80 - min(len(prompts[b]) for b in which) + 1          # what the cache holds after the shortest prompt; more is refused
        ids, lp = dec.greedy([prompts[b] for b in which], int(gold["small_eot"]), min(max_new, room), suppress=mask, check_every=check_every)
        return ids, lp, dec.last_out.copy()

    return run


def test_greedy_batch_of_three_equals_the_golden(small_run, gold):
    _, want_ids, want_lp = small_batch(gold)
    ids, lp, _ = small_run()
    assert [len(i) for i in ids] == [len(i) for i in want_ids] == [0, len(want_ids[1]), 41]
    assert ids == want_ids
    absmax = max(float(np.abs(gold[f"small_logits_70_{n}"]).max()) for n in ROWS)
    tol = logprob_tol([len(i) for i in want_ids], GATE["bf16x3"], absmax)
    print("summed log-probabilities", lp, "golden", want_lp, "tolerance", tol)
    assert (np.abs(lp - want_lp) <= tol).all()


def test_greedy_is_repeatable_and_independent_of_check_every(small_run):
    ids, lp, out = small_run(check_every=8)
    for ce in (8, 1, 3):
        ids2, lp2, out2 = small_run(check_every=ce)
        assert ids2 == ids and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32)) and np.array_equal(out2, out), ce


def test_greedy_tiny_equals_the_golden(decoders, gold):
    dec = decoders("tiny")
    dec.begin(tiny_enc(gold))
    ids, lp = dec.greedy([gold["tiny_prompt"].tolist()], 50257, 24, suppress=gold["tiny_suppress"].tolist())
    assert ids[0] == gold["tiny_ids"].tolist() and len(ids[0]) == 24
    tol = logprob_tol([24], GATE["bf16x3"], float(gold["tiny_logits_absmax"]))[0]
    print("tiny summed log-probability", lp[0], "golden", float(gold["tiny_logprob"]), "tolerance", tol)
    assert abs(lp[0] - float(gold["tiny_logprob"])) <= tol


def test_a_finished_sequence_is_left_alone(decoders, small_run, gold):
    dec = decoders("small")
    _, want_ids, _ = small_batch(gold)

    def snapshot(seq):
        return [dec.cache(layer, seq) for layer in range(dec.n_layer)]

    for seq, budget in ((0, 1), (1, len(want_ids[1]) + 1)):       # the budget at which this sequence has just met end-of-text
        ids_a, lp_a, out_a = small_run(max_new=budget)
        before = snapshot(seq)
        ids_b, lp_b, out_b = small_run(max_new=80)                 # the others take up to 40 more steps
        after = snapshot(seq)
        assert ids_a[seq] == ids_b[seq] == want_ids[seq] and lp_a[seq].tobytes() == lp_b[seq].tobytes()
        assert out_a[seq].tobytes() == out_b[seq, :budget].tobytes() and not out_b[seq, budget:].any()
        for (k0, v0, n0), (k1, v1, n1) in zip(before, after):
            assert n0 == n1 == len(gold[f"small_prompt_{seq}"]) + len(want_ids[seq])
            assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes()
            assert not k1[n1:].any() and not v1[n1:].any() and k1[:n1].any()       # rows past its length were never written


def test_each_sequence_of_a_batch_equals_itself_alone(small_run, gold):
    ids, lp, _ = small_run()
    absmax = max(float(np.abs(gold[f"small_logits_70_{n}"]).max()) for n in ROWS)
    for b in range(3):
        one_ids, one_lp, _ = small_run(which=(b,))
        assert one_ids[0] == ids[b]
        assert abs(one_lp[0] - lp[b]) <= logprob_tol([len(ids[b])], GATE["bf16x3"], absmax)[0]


# ---- short audio ------------------------------------------------------------------------------------------------
def test_keys_beyond_t_audio_are_never_read(decoders, gold):
    dec = decoders("small")
    row = gold["small_row_65"]
    for t_audio in (7, 1):
        buf = torch.full((1, 1500, 128), float("nan"), device="cuda")
        buf[0, :t_audio] = torch.from_numpy(gold["small_enc_7"][0, :t_audio]).cuda()
        dec.begin(buf, t_audio=t_audio)
        got = dec.logits(row)[0].cpu().numpy()
        assert np.isfinite(got).all()
        dec.begin(buf[:, :t_audio].contiguous())
        assert np.array_equal(got, dec.logits(row)[0].cpu().numpy())
        if t_audio == 7:
            assert rel_err(got, gold["small_logits_7_65"]) <= GATE["bf16x3"]
        ids, _ = dec.greedy([[3, 5]], int(gold["small_eot"]), 4)
        assert len(ids[0]) <= 4 and dec.cache(0, 0)[2] <= 2 + 4


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_limits_are_refused_and_the_handle_stays_usable(decoders, gold):
    from mere_fusion_amd import _lib
    dec = decoders("small")
    enc = torch.from_numpy(gold["small_enc_70"]).cuda()
    dec.begin(enc[:1])
    first = dec.logits(gold["small_row_1"])[0].cpu().numpy()
    state = dec.cache(0, 0)
    with pytest.raises(RuntimeError, match="max_batch"):
        dec.begin(torch.cat([enc, enc[:1]]))
    dec.begin(enc[:1])
    dec.logits(gold["small_row_1"])
    for bad_t in (0, 1501):
        with pytest.raises(RuntimeError, match="T_audio"):
            _lib.check(_lib.lib().mf_whisper_decoder_begin(dec._h, enc.data_ptr(), bad_t, 1, None), "begin")
    dec.begin(enc[:1])
    dec.logits(gold["small_row_1"])
    eot = int(gold["small_eot"])
    with pytest.raises(RuntimeError, match="prompt 0 has 41 tokens"):
        dec.greedy([[1] * 41], eot, 4)
    with pytest.raises(RuntimeError, match="prompt 0 has 0 tokens"):
        dec.greedy([[]], eot, 4)
    with pytest.raises(RuntimeError, match="outside the vocabulary"):
        dec.greedy([[1, 257]], eot, 4)
    with pytest.raises(RuntimeError, match="max_new = 80"):
        dec.greedy([[1, 2]], eot, 80)                              # 80 - 2 + 1 = 79 is what the cache holds
    with pytest.raises(RuntimeError, match="max_new = 0"):
        dec.greedy([[1, 2]], eot, 0)
    with pytest.raises(RuntimeError, match="check_every"):
        dec.greedy([[1, 2]], eot, 4, check_every=0)
    with pytest.raises(RuntimeError, match="batch 2"):
        dec.greedy([[1], [2]], eot, 4)
    with pytest.raises(RuntimeError, match="n_text_ctx"):
        dec.logits(np.zeros(80, np.int32))                         # one token is already in the cache
    after = dec.cache(0, 0)                                         # nothing was launched: the cache and its length are as the last good call left them
    assert after[2] == state[2] == 1 and after[0].tobytes() == state[0].tobytes() and after[1].tobytes() == state[1].tobytes()
    ids, _ = dec.greedy([[1, 2]], eot, 79)
    assert len(ids[0]) <= 79
    with pytest.raises(RuntimeError, match="begin first"):
        dec.logits(gold["small_row_1"])                            # the caches are ragged after a greedy run
    dec.begin(enc[:1])
    assert np.array_equal(dec.logits(gold["small_row_1"])[0].cpu().numpy(), first)


# ---- wiring ---------------------------------------------------------------------------------------------------------
def test_transcriber_returns_the_reference_ids(decoders, gold):
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    from mere_fusion_amd.transcribe import Transcriber
    a2f = Audio2Feature(state_dict=W.make_whisper_encoder_state_dict(0), n_head=6)
    tr = Transcriber(a2f, decoders("tiny_post"), suppress=gold["wire_suppress"].tolist())
    assert tr.prompt("en") == gold["tiny_prompt"].tolist()
    ids = tr.transcribe(W.make_speech_like_wav(16000, int(gold["wire_wav_seed"])), language="en", max_new=24)
    assert ids == gold["wire_ids"].tolist()
