"""MuseTalk Whisper feature path: oracle against the vectors recorded from the real
reference modules (CPU), HIP path against the oracle and the goldens (GPU)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from mere_fusion_amd import weights as W
from oracle import whisper_ref as R

FEAT_STRIDE = 13


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "whisper_golden.npz")))


@pytest.fixture(scope="module")
def wsd():
    return W.make_whisper_encoder_state_dict(0)


def test_mel_filterbank_matches_reference_asset(gold):
    # audio.py:80-87: the asset IS librosa.filters.mel(sr=16000, n_fft=400, n_mels=80)
    mine = R.mel_filters()
    assert mine.shape == gold["mel_filters"].shape == (80, 201) and mine.dtype == np.float32
    np.testing.assert_allclose(mine, gold["mel_filters"], rtol=0, atol=2e-7)


@pytest.mark.parametrize("n", [16640, 11520])
def test_oracle_log_mel(gold, n):
    got = R.log_mel_spectrogram(W.make_speech_like_wav(n, 0)).numpy()
    assert got.shape == gold[f"logmel_{n}"].shape == (80, n // 160)
    np.testing.assert_allclose(got, gold[f"logmel_{n}"], rtol=0, atol=2e-5)


@pytest.mark.parametrize("n,B", [(16640, 16), (11520, 8)])
def test_oracle_audio2feat_and_chunks(gold, wsd, n, B):
    feat = R.audio2feat(wsd, W.make_speech_like_wav(n, 0))
    assert list(feat.shape) == list(gold[f"feat_shape_{n}"]) == [n // 320, 5, 384]
    np.testing.assert_allclose(feat.reshape(-1)[::FEAT_STRIDE], gold[f"feat_sample_{n}"], rtol=0, atol=3e-4)
    np.testing.assert_allclose(feat[:2], gold[f"feat_first_{n}"], rtol=0, atol=3e-4)
    np.testing.assert_allclose(np.abs(feat.astype(np.float64)).sum(), gold[f"feat_abssum_{n}"], rtol=1e-5)
    # museasr.py:27: feature2chunks(feature_array, fps=opt.fps/2, batch_size, start=stride_left/2)
    chunks, idxs = R.feature2chunks(feat, fps=25.0, batch_size=B, start=5.0)
    np.testing.assert_array_equal(np.asarray(idxs), gold[f"chunk_idx_{n}"])
    assert idxs[0] == list(range(6, 16)) and idxs[-1] == list(range(2 * (B + 4) - 4, 2 * (B + 4) + 6))
    np.testing.assert_allclose(chunks[-1], gold[f"chunk_last_{n}"], rtol=0, atol=3e-4)
    assert all(np.array_equal(c, feat[i].reshape(-1, 384)) for c, i in zip(chunks, idxs))


def test_sliced_feature_clamps_at_the_edges():
    feat = np.arange(20 * 5 * 384, dtype=np.float32).reshape(20, 5, 384)
    _, idx = R.get_sliced_feature(feat, 0)
    assert idx == [0, 0, 0, 0, 0, 1, 2, 3, 4, 5]
    _, idx = R.get_sliced_feature(feat, 9)
    assert idx == [14, 15, 16, 17, 18, 19, 19, 19, 19, 19]


# ---- GPU: HIP path vs oracle and goldens -----------------------------------------------------------------
TOL_LOGMEL = 2e-5      # fp64 DFT vs torch's fp32 stft; log-mel lives in [-1.5, 1.5]
TOL_FEAT = 2e-3        # bf16x3 through 4 transformer blocks; embeddings reach |x| ~ 6 (relative 3e-4)


@pytest.fixture(scope="module")
def a2f(lib_built, wsd):
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    return Audio2Feature(state_dict=wsd, n_head=6, precision="bf16x3")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16640, 11520, 480000, 1600])
def test_hip_log_mel(a2f, gold, n):
    wav = W.make_speech_like_wav(n, 0)
    got = a2f.log_mel_spectrogram(wav).cpu().numpy()
    want = R.log_mel_spectrogram(wav).numpy()
    assert got.shape == want.shape == (80, n // 160)
    assert np.abs(got - want).max() <= TOL_LOGMEL
    if f"logmel_{n}" in gold:
        assert np.abs(got - gold[f"logmel_{n}"]).max() <= TOL_LOGMEL


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [(16640, 16), (11520, 8)])
def test_hip_audio2feat_vs_oracle_and_golden(a2f, gold, wsd, n, B):
    wav = W.make_speech_like_wav(n, 0)
    got = a2f.audio2feat(wav)
    want = R.audio2feat(wsd, wav)
    assert got.shape == want.shape == (n // 320, 5, 384) and got.dtype == np.float32
    err = np.abs(got - want)
    # per layer: the error must not grow out of the bf16x3 class through the stack
    for l in range(5):
        assert err[:, l].max() <= TOL_FEAT, (l, err[:, l].max())
    np.testing.assert_allclose(got.reshape(-1)[::FEAT_STRIDE], gold[f"feat_sample_{n}"], rtol=0, atol=TOL_FEAT)
    chunks = a2f.feature2chunks(feature_array=got, fps=25.0, batch_size=B, start=5.0)
    assert len(chunks) == B and all(c.shape == (50, 384) for c in chunks)
    np.testing.assert_allclose(chunks[-1], gold[f"chunk_last_{n}"], rtol=0, atol=TOL_FEAT)
    _, idx = a2f.get_sliced_feature(got, 5.0)
    assert idx == list(gold[f"chunk_idx_{n}"][0])


@pytest.mark.gpu
def test_hip_audio2feat_other_signal_and_repeatability(a2f, wsd):
    wav = W.make_speech_like_wav(6400, 3)          # 20 tokens kept
    a = a2f.audio2feat(wav)
    b = a2f.audio2feat(wav)
    assert a.shape == (20, 5, 384) and np.array_equal(a, b)
    assert np.abs(a - R.audio2feat(wsd, wav)).max() <= TOL_FEAT
    silent = a2f.audio2feat(np.zeros(3200, np.float32))   # log-mel of silence: all bins at the clamp
    assert np.isfinite(silent).all() and np.abs(silent - R.audio2feat(wsd, np.zeros(3200, np.float32))).max() <= TOL_FEAT


@pytest.mark.gpu
def test_hip_whisper_error_paths(a2f):
    with pytest.raises(RuntimeError, match="frames"):
        a2f.log_mel_spectrogram(np.zeros(480160, np.float32))
    with pytest.raises(RuntimeError, match="float32 waveform"):
        a2f.audio2feat("some.wav")


@pytest.mark.gpu
def test_hip_streaming_windows_exact_modes_and_batch(a2f, wsd):
    """the streaming form.  'exact' (pruned last block, only the consumed rows leave the device) equals the literal
    'exact_full' evaluation; three sessions' windows in ONE call equal three separate calls; every window is held to the oracle."""
    n = 11520                                                   # the B = 8 window of museasr.py: 36 feature rows
    wavs = np.stack([W.make_speech_like_wav(n, s) for s in (0, 5, 9)])
    try:
        a2f.set_mode("exact_full")
        full = a2f.audio2feat_windows_device(torch.from_numpy(wavs)).cpu().numpy()
        a2f.set_mode("exact")
        one = np.stack([a2f.audio2feat(wavs[i]) for i in range(3)])
        bat = a2f.audio2feat_windows_device(torch.from_numpy(wavs)).cpu().numpy()
        again = a2f.audio2feat_windows_device(torch.from_numpy(wavs[:2])).cpu().numpy()     # a smaller batch on the grown workspace
    finally:
        a2f.set_mode("exact")
    assert full.shape == one.shape == bat.shape == (3, 36, 5, 384)
    assert np.abs(one - full).max() <= 2e-4 and np.abs(bat - full).max() <= 2e-4           # same arithmetic, other GEMM tilings
    assert np.abs(again - bat[:2]).max() <= 2e-4
    for i in range(3):
        assert np.abs(bat[i] - R.audio2feat(wsd, wavs[i])).max() <= TOL_FEAT, i


@pytest.mark.gpu
def test_hip_windowed_context_is_an_approximation_and_says_so(a2f, wsd):
    """A shortened context is NOT the reference's result (global unmasked attention over 1500 tokens): the error is measured, it is
    well above the exact modes' and it shrinks as the context grows; full context through the same code path is exact again."""
    wav = W.make_speech_like_wav(11520, 2)
    want = R.audio2feat(wsd, wav)
    errs = {}
    try:
        for ctx in (64, 512, 1500):
            a2f.set_mode("windowed", ctx)
            errs[ctx] = float(np.abs(a2f.audio2feat(wav) - want).max())
    finally:
        a2f.set_mode("exact")
    print("windowed-context L-inf vs oracle:", errs)
    assert errs[1500] <= TOL_FEAT
    assert errs[64] > 10 * TOL_FEAT or errs[64] > errs[1500] * 5
    assert np.isfinite(list(errs.values())).all()


@pytest.mark.gpu
def test_hip_long_audio_is_refused(a2f):
    with pytest.raises(RuntimeError, match="30 s"):
        a2f.audio2feat(np.zeros(480000 + 320, np.float32))


# ---- floors, per-window maximum, stale state: against the float64 model of tests/audio_frontend_ref.py ------------------------------------
# (the float32 oracle drifts where the floor decides the value; what each signal covers is pinned on the model alone in test_audio_frontend_ref.py)
import audio_frontend_ref as A                                                    # noqa: E402
from audio_frontend_ref import WHISPER_DYN_SHARE, WHISPER_LENGTHS, WHISPER_POW_SHARE         # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("n", WHISPER_LENGTHS)
def test_hip_log_mel_floor_cases(a2f, n):
    """201: one frame; 320 / 479 / 480: two or three frames, all of them touching an end; every length above 200 takes the left reflect branch, 320, 480,
    1600 and 3200 the right one too.  gain 1: `max - 8` decides 30-74 % of the cells from 480 samples on; gain 1e-3: the 1e-10 floor does and the window
    maximum is negative; zeros: every cell at the power floor, maximum -10."""
    cases = [("gain 1", A.burst_silence_hiss(n, 1.0), WHISPER_DYN_SHARE[n]), ("gain 1e-3", A.burst_silence_hiss(n, 1e-3), WHISPER_POW_SHARE[n]),
             ("zeros", np.zeros(n, np.float32), 1.0), ("speech-like", W.make_speech_like_wav(n, 0), 0.0)]
    for name, wav, share in cases:
        got = a2f.log_mel_spectrogram(wav).cpu().numpy()
        want = A.whisper_log_mel_f64(wav)
        assert got.shape == want.shape == (80, n // 160)
        err = np.abs(got - want).max()
        floored = want == want.min()
        at_floor = float((got == got.min()).mean()) if share else 0.0
        print(f"[whisper log-mel] n {n} {name}: L-inf vs float64 model {err:.2e}; at the floor: model {floored.mean() if share else 0.0:.3f}, kernel {at_floor:.3f}")
        assert np.isfinite(got).all() and err <= TOL_LOGMEL, (name, err)
        if share:
            assert floored.mean() >= share and at_floor >= share, (name, floored.mean(), at_floor)
            assert np.abs(got[floored] - want.min()).max() <= TOL_LOGMEL, name
    assert (a2f.log_mel_spectrogram(np.zeros(n, np.float32)).cpu().numpy() == -1.5).all()


_window_refs = {}


def _window_case(wsd, n):
    """the four windows of a batched call and the reference's features of each, computed once per length"""
    if n not in _window_refs:
        wavs = np.stack([A.burst_silence_hiss(n, 1.0), A.burst_silence_hiss(n, 1e-3), np.zeros(n, np.float32), W.make_speech_like_wav(n, 0)])
        _window_refs[n] = wavs, [A.whisper_features(wsd, w) for w in wavs]
    return _window_refs[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3200, 11520])
def test_hip_per_window_maximum(a2f, wsd, n):
    """Four windows whose maxima differ (1.66, -4.34, -10, 0.44) in ONE call: each row is its own single-window call and the reference on the float64
    log-mel.  With window 0's maximum window 1's features would move by ~3 (test_whisper_window_maximum_mixup_moves_the_features)."""
    wavs, wants = _window_case(wsd, n)
    a2f.set_mode("exact")
    bat = a2f.audio2feat_windows_device(torch.from_numpy(wavs)).cpu().numpy()
    assert bat.shape == (4, n // 320, 5, 384) and np.isfinite(bat).all()
    for i in range(4):
        one = a2f.audio2feat(wavs[i])
        e1, e2 = np.abs(bat[i] - one).max(), np.abs(bat[i] - wants[i]).max()
        print(f"[whisper windows] n {n} window {i}: vs its single call {e1:.2e}, vs the reference {e2:.2e}")
        assert e1 <= 2e-4, (i, e1)
        assert e2 <= TOL_FEAT, (i, e2)


@pytest.mark.gpu
def test_hip_whisper_no_stale_state(lib_built, wsd):
    """A short quiet window after a long loud one, and again after set_batch regrew the workspace, gives the bits of a fresh handle: the frames past the
    window's end and the window maximum (here negative, after a positive one) are reset by every call."""
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    short, long_ = A.burst_silence_hiss(1600, 1e-3), W.make_speech_like_wav(16640, 1)
    fresh = Audio2Feature(state_dict=wsd, n_head=6, precision="bf16x3")
    want_mel, want = fresh.log_mel_spectrogram(short).cpu(), fresh.audio2feat_device(short).cpu()
    used = Audio2Feature(state_dict=wsd, n_head=6, precision="bf16x3")
    used.audio2feat_device(long_)
    assert torch.equal(used.audio2feat_device(short).cpu(), want)
    used.log_mel_spectrogram(long_)
    assert torch.equal(used.log_mel_spectrogram(short).cpu(), want_mel)
    used.audio2feat_windows_device(torch.from_numpy(np.stack([long_, long_[::-1].copy(), long_ * 0.5])))      # set_batch(3): the workspace is reallocated
    assert torch.equal(used.audio2feat_device(short).cpu(), want)
    assert torch.equal(used.log_mel_spectrogram(short).cpu(), want_mel)


@pytest.mark.gpu
def test_hip_per_head_attention_fallback_vs_oracle(lib_built):
    """Head width 48 (n_state 96, 2 heads: a multiple of 8 that mf_attention_supported declines) puts the handle on the per-head attention -- pack K, scores GEMM,
    row softmax, pack V^T, weights x V GEMM -- which serves mf_whisper_encode_audio alone.  One window of 3200 samples, one layer: both hidden states of all
    1500 tokens against the oracle, at the tolerance of test_hip_audio2feat_vs_oracle_and_golden."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.musetalk.whisper.audio2feature import Audio2Feature
    sd = W.make_whisper_encoder_state_dict(0, dict(W.WHISPER_TINY, n_audio_state=96, n_audio_head=2, n_audio_layer=1))
    a2f = Audio2Feature(state_dict=sd, n_head=2, precision="bf16x3")
    assert (a2f.n_layer, a2f.n_ctx, a2f.n_state) == (1, 1500, 96)
    wav = W.make_speech_like_wav(3200, 0)
    dev = a2f._wav(wav)
    emb = torch.empty((2, 1500, 96), dtype=torch.float32, device=dev.device)
    _lib.check(_lib.lib().mf_whisper_encode_audio(a2f._h, dev.data_ptr(), dev.numel(), emb.data_ptr(), _lib.stream_ptr(dev.device)), "whisper_encode_audio")
    _, want = R.encoder_forward(sd, R.pad_or_trim(R.log_mel_spectrogram(wav))[None], n_head=2, n_layer=1)          # (1, 2, 1500, 96)
    err = np.abs(emb.cpu().numpy() - want[0].numpy())
    for l in range(2):
        print(f"[whisper per-head attention] hidden state {l}: L-inf vs oracle {err[l].max():.2e} (tol {TOL_FEAT})")
        assert err[l].max() <= TOL_FEAT, (l, err[l].max())
    with pytest.raises(RuntimeError, match="needs the fused attention kernel"):      # the batched / pruned call is the fused kernel's: the handle is on the fallback
        a2f.audio2feat(wav)
