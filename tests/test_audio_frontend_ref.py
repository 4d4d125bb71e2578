"""CPU tier of the audio front-end floor / clamp tests: the float64 models of tests/audio_frontend_ref.py are the same operations as the oracles, the
seeded signals put the cells where the GPU tests need them (shown on the models ALONE), and each one-line kernel mistake the GPU tests are meant to catch
moves the MODEL by far more than the GPU tolerance.  The GPU tests (test_whisper.py, test_mel.py, test_wav2vec2.py) ask the same shares of the kernels."""
import os

import numpy as np
import pytest
import torch

import audio_frontend_ref as A
from conftest import GOLDEN
from mere_fusion_amd import weights as W
from oracle import mel_ref
from oracle import whisper_ref as R

TOL_LOGMEL, TOL_FEAT, TOL_MEL, TOL_W2V = 2e-5, 2e-3, 1e-5, 2e-3          # the GPU bounds of test_whisper.py / test_mel.py / test_wav2vec2.py

from audio_frontend_ref import (MEL_SHARES, MEL_SIGNAL_N, WHISPER_DYN_SHARE, WHISPER_LENGTHS, WHISPER_POW_SHARE, mel_signal, w2v_lengths,
                                w2v_rows)


# ---- Whisper ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16640, 11520, 1600])
def test_whisper_f64_model_is_the_oracles_operation(n):
    """on the speech-like signals (no floor active) the float64 model, the float32 oracle and the vectors recorded from the reference agree to 2e-5"""
    gold = np.load(os.path.join(GOLDEN, "whisper_golden.npz"))
    wav = W.make_speech_like_wav(n, 0)
    mine = A.whisper_log_mel_f64(wav)
    assert mine.dtype == np.float32 and mine.shape == (80, n // 160)
    assert np.abs(mine - R.log_mel_spectrogram(wav).numpy()).max() <= TOL_LOGMEL
    if f"logmel_{n}" in gold:
        assert np.abs(mine - gold[f"logmel_{n}"]).max() <= TOL_LOGMEL
    assert A.whisper_floor_shares(wav)[:2] == (0.0, 0.0)                 # which is why these signals never tested the floors


def test_whisper_oracle_drift_on_floor_signals_is_recorded():
    """NOT an assertion on the drift: the float32 oracle against the float64 model where the floors are active.  Measured L-inf: gain 1 at 3200 1.5e-5,
    at 11520 1.3e-5; gain 1e-3 1.7e-6 / 1.9e-6; zeros 0; speech-like <= 8.3e-7.  The drift grows with the share of floored cells
    and with the step at the burst's end; this signal stays under the 2e-5 bound, which is no promise for the next one: the GPU tests use the float64 model."""
    for n in (3200, 11520):
        for name, wav in (("gain 1", A.burst_silence_hiss(n, 1.0)), ("gain 1e-3", A.burst_silence_hiss(n, 1e-3)), ("zeros", np.zeros(n, np.float32))):
            d = np.abs(R.log_mel_spectrogram(wav).numpy() - A.whisper_log_mel_f64(wav))
            print(f"[whisper f32 oracle vs f64 model] n {n} {name}: L-inf {d.max():.2e}, cells over {TOL_LOGMEL}: {(d > TOL_LOGMEL).sum()} of {d.size}")
            assert np.isfinite(d).all()


@pytest.mark.parametrize("n", WHISPER_LENGTHS + (11520,))
def test_whisper_signals_sit_on_the_floors(n):
    dyn, pw, m = A.whisper_floor_shares(A.burst_silence_hiss(n, 1.0))
    assert dyn >= WHISPER_DYN_SHARE[n] and pw == 0.0 and m > 0
    dyn, pw, m = A.whisper_floor_shares(A.burst_silence_hiss(n, 1e-3))
    assert pw >= WHISPER_POW_SHARE[n] and dyn == 0.0 and m < 0        # a negative window maximum: the other branch of the ordered-uint atomicMax
    assert A.whisper_floor_shares(np.zeros(n, np.float32)) == (0.0, 1.0, -10.0)
    assert (A.whisper_log_mel_f64(np.zeros(n, np.float32)) == -1.5).all()
    if n >= 3200:
        assert WHISPER_DYN_SHARE[n] >= 0.5 and WHISPER_POW_SHARE[n] >= 0.5


def test_whisper_floor_mistakes_move_the_model():
    """`- 8` -> `- 7` and 1e-10 -> 1e-9, applied to the model: every floored cell moves by 0.25, 12500 x the GPU bound; at a length where >= 30 % of the
    cells are floored no such kernel passes test_hip_log_mel_floor_cases."""
    for n in (480, 1600, 3200):
        raw = A.whisper_raw_f64(A.burst_silence_hiss(n, 1.0))
        d = np.abs(A.whisper_finish(raw, span=7.0) - A.whisper_finish(raw))
        assert d.max() >= 0.2499 and (d > 100 * TOL_LOGMEL).mean() >= WHISPER_DYN_SHARE[n]
        raw = A.whisper_raw_f64(A.burst_silence_hiss(n, 1e-3))
        d = np.abs(A.whisper_finish(np.maximum(raw, np.float32(-9.0))) - A.whisper_finish(raw))
        assert d.max() >= 0.2499 and (d > 100 * TOL_LOGMEL).mean() >= WHISPER_POW_SHARE[n]
    z = np.full((80, 20), -10.0, np.float32)
    assert np.abs(A.whisper_finish(np.maximum(z, np.float32(-9.0))) - A.whisper_finish(z)).min() == 0.25


@pytest.mark.parametrize("n", WHISPER_LENGTHS)
def test_whisper_reflect_branches_move_the_model(n):
    """Either end zero-padded instead of reflected (what a kernel without that branch would compute, if it did not fault).  The left end shows at every
    length; the right end only where the last KEPT frame reaches past the signal -- frame n // 160 - 1 ends at 160 * (n // 160 - 1) + 199, so not at
    201 and 479 (the frame that would need it is the one the operation drops)."""
    wav = W.make_speech_like_wav(n, 0)
    want = A.whisper_log_mel_f64(wav)
    left = np.abs(A.whisper_finish(A.whisper_raw_f64(wav, left="constant")) - want).max()
    right = np.abs(A.whisper_finish(A.whisper_raw_f64(wav, right="constant")) - want).max()
    assert left > 100 * TOL_LOGMEL
    if 160 * (n // 160 - 1) + 199 >= n:
        assert right > 100 * TOL_LOGMEL
    else:
        assert right == 0.0


@pytest.mark.parametrize("n", [3200, 11520])
def test_whisper_window_maximum_mixup_moves_the_features(n):
    """The batched path keeps one maximum per window.  Window 1 (gain 1e-3) floored against window 0's maximum (gain 1; gain ratio 1000): the reference's
    own features move by 2.7 (n = 3200) and 3.0 (n = 11520), over 1000 x TOL_FEAT, so test_hip_per_window_maximum cannot pass with a shared maximum."""
    wsd = W.make_whisper_encoder_state_dict(0)
    loud, quiet = A.burst_silence_hiss(n, 1.0), A.burst_silence_hiss(n, 1e-3)
    moved = np.abs(A.whisper_features(wsd, quiet, gmax=A.whisper_raw_f64(loud).max()) - A.whisper_features(wsd, quiet)).max()
    print(f"[whisper] n {n}: window 1 floored from window 0's maximum moves the features by {moved:.3f}")
    assert moved > 10 * TOL_FEAT


# ---- Wav2Lip mel ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MEL_SHARES))
@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_mel_signals_sit_on_the_floor(name, mode):
    lo, hi, inside, top = A.mel_shares(mel_signal(name, MEL_SIGNAL_N), mode)
    assert lo >= MEL_SHARES[name][0] and inside >= MEL_SHARES[name][1] and hi == 0.0
    if name == "burst":
        assert lo >= 0.25 and inside >= 0.25


def test_mel_min_level_mistake_moves_the_model():
    """min_level 1e-4 instead of 1e-5 lifts every cell below -3.2 to -3.2: all the cells at -4 move by 0.8, and the cells in (-4, -3.2) by less"""
    for name in ("burst", "burst_quiet"):
        m = mel_ref.melspectrogram(mel_signal(name, MEL_SIGNAL_N))
        wrong = np.maximum(m, -3.2)
        assert ((wrong - m) > 1000 * TOL_MEL).mean() >= MEL_SHARES[name][0]
        assert ((m > -4.0) & (m < -3.2)).any()


def _mel_operator():
    """(401, 801) complex: pre-emphasis, Hann window and DFT of one interior frame as a linear map of the 801 samples it reads"""
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(800) / 800)
    P = np.zeros((800, 801))
    P[np.arange(800), np.arange(800) + 1], P[np.arange(800), np.arange(800)] = 1.0, -0.97
    return np.exp(-2j * np.pi * np.outer(np.arange(401), np.arange(800)) / 800) @ (win[:, None] * P)


def test_mel_plus_four_is_out_of_reach_of_a_full_scale_signal():
    """+4 needs a mel amplitude of 10 in one band.  None of these gets there with |x| <= 1, so the GPU tests hold NO case at +4 (the signal is not scaled
    past 1): loud_tone, the best of a sweep of full-scale square waves, reaches 3.46 (amplitude 4.7); random signs 2.99; and an ascent on the +-1
    sequences of one frame (the band amplitude is convex in x, so its maximum over the cube is at a vertex; x <- sign(gradient) climbs to a local one)
    ends at amplitudes <= 6.95 (3.75), largest in the bands near 6 kHz, where the pre-emphasis gain of 1.9 meets the widest triangles."""
    m = mel_ref.melspectrogram(A.loud_tone(7040))
    assert 3.4 < m[:, 4:-4].max() < 3.5 and (m == 4.0).sum() == 0
    t = np.arange(7040) / 16000.0
    for f in (1250.0, 2250.0, 4250.0, 6250.0):
        assert mel_ref.melspectrogram(np.where(np.sin(2 * np.pi * f * t + 0.3) >= 0, 1.0, -1.0))[:, 4:-4].max() <= m[:, 4:-4].max()
    M, B = _mel_operator(), mel_ref.mel_basis().astype(np.float64)
    rng = np.random.default_rng(0)
    for b in (20, 63, 71, 79):
        k = np.nonzero(B[b])[0]
        Mk, Bk = M[k], B[b, k]
        x = np.sign(rng.standard_normal(801))
        for _ in range(60):
            z = Mk @ x
            nxt = np.where(np.real((Bk * np.conj(z) / np.maximum(np.abs(z), 1e-30)) @ Mk) >= 0, 1.0, -1.0)
            if (nxt == x).all():
                break
            x = nxt
        amp = float(Bk @ np.abs(Mk @ x))
        print(f"[mel] band {b}: sign ascent ends at amplitude {amp:.2f} of the 10 that +4 needs")
        assert amp < 8.0


@pytest.mark.parametrize("n", [401, 599, 600, 601, 1000])
def test_mel_reflect_branches_move_the_model(n):
    """reflect against zero padding differ by far more than the GPU bound in the first and in the last frames: a kernel that lost either branch of its
    reflect (and so zero-pads that end) fails test_hip_mel_edge_lengths"""
    d = np.abs(mel_ref.melspectrogram(W.make_speech_like_wav(n, n), "reflect") - mel_ref.melspectrogram(W.make_speech_like_wav(n, n), "constant"))
    assert d[:, 0].max() > 1000 * TOL_MEL and d[:, -1].max() > 1000 * TOL_MEL


# ---- wav2vec2 -------------------------------------------------------------------------------------------------------------------------------------
def test_w2v_min_samples_is_the_extractors():
    assert A.w2v_min_samples(W.WAV2VEC2_SMALL) == 400 and w2v_lengths()[1] % 320 != 0 and w2v_lengths()[1] % 1024 != 0


@pytest.mark.parametrize("n", w2v_lengths())
def test_w2v_epsilon_mistake_moves_the_reference(n):
    """dc_quiet at gain 1e-3 has a variance of ~1.7e-8, below the 1e-7: with 1e-5 in its place the reference's own logits move by 2.06 (n = 8960) and
    2.07 (n = 401), 1000 x the 2e-3 of the GPU tests.  (Gain 2e-3: 1.7, 5e-3: 0.8, 1e-2: 0.39 -- all above 10 x 2e-3; 1e-3 is the gain used.)  The
    float64 normalisation and transformers' float32 one agree on every row well inside the bound (2.8e-4 on the dc_quiet row, <= 2.3e-6 elsewhere)."""
    from oracle import wav2vec2_ref as WV
    cfg = W.WAV2VEC2_SMALL
    model = WV.build(cfg, W.make_wav2vec2_state_dict(cfg, 0))
    rows = w2v_rows(n)
    good, wrong = A.w2v_logits(model, rows[2], 1e-7), A.w2v_logits(model, rows[2], 1e-5)
    print(f"[wav2vec2] n {n}, gain {A.DC_QUIET_GAIN}: 1e-5 in place of 1e-7 moves the logits by {np.abs(good - wrong).max():.3f}")
    assert np.abs(good - wrong).max() > 10 * TOL_W2V
    hf = WV.frame_to_logits(model, rows)
    assert np.isfinite(hf).all() and np.abs(hf - A.w2v_logits(model, rows)).max() <= TOL_W2V / 4
    assert (A.w2v_normalize(rows[1]) == 0).all() and (A.w2v_normalize(rows[3]) == 0).all()
