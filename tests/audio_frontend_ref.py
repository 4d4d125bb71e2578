"""TEST INFRASTRUCTURE: plain high-precision models of the three audio front ends, and the seeded signals on which their floors and clamps decide
the result.  Never imported by the product.

  * `whisper_log_mel_f64`   the steps of oracle/whisper_ref.log_mel_spectrogram with the STFT, |.|^2 and the mel product in float64; log10 is rounded
                            ONCE to float32 (mf_whisper.hip stores `raw` as float32), then `max - 8`, `+ 4`, `/ 4` in float32 as the kernel does.
                            The float32 oracle drifts from this by up to ~5e-5 where the floor is active (its float32 STFT moves the window maximum
                            and the cells next to the floor), which is above the suite's 2e-5: it cannot judge the fp64 kernel there.
  * `w2v_normalize`         Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm in float64 with the epsilon as a parameter.
  * the Wav2Lip mel already has a float64 model: oracle/mel_ref.melspectrogram.

Signals are seeded functions of n, |x| <= 1, float32.  tests/test_audio_frontend_ref.py pins, from the models alone, where each one puts the cells."""
import numpy as np
import torch

from oracle import mel_ref
from oracle import whisper_ref as WR

WHISPER_RAW_FLOOR = np.float32(-10.0)          # log10(1e-10), exact in float32


# ---- Whisper log-mel ------------------------------------------------------------------------------------------------------------------------------
def whisper_raw_f64(wav, left="reflect", right="reflect"):
    """float32 (80, n // 160): log10(max(1e-10, mel . |stft|^2)), everything before the rounding in float64.  left / right: np.pad modes of the two
    ends ("reflect" is the operation; "constant" at one end is what a kernel without that end's reflect branch would compute, for sensitivity checks)."""
    x = np.asarray(wav, dtype=np.float32).astype(np.float64)
    h = WR.N_FFT // 2
    x = torch.from_numpy(np.concatenate([np.pad(x, (h, 0), mode=left)[:h], x, np.pad(x, (0, h), mode=right)[len(x):]]))
    win = torch.hann_window(WR.N_FFT, periodic=True, dtype=torch.float64)
    st = torch.stft(x, WR.N_FFT, WR.HOP_LENGTH, window=win, center=False, return_complex=True)
    power = st[:, :-1].abs() ** 2
    mel = torch.from_numpy(WR.mel_filters()).double() @ power
    return torch.clamp(mel, min=1e-10).log10().float().numpy()


def whisper_finish(raw, gmax=None, span=8.0):
    """`max - span` floor and the affine map, in float32.  gmax: the maximum to floor against (default: this window's own)."""
    raw = np.asarray(raw, np.float32)
    m = np.float32(raw.max() if gmax is None else gmax)
    floor_v = np.float32(m - np.float32(span))
    return ((np.maximum(raw, floor_v) + np.float32(4.0)) / np.float32(4.0)).astype(np.float32)


def whisper_log_mel_f64(wav):
    return whisper_finish(whisper_raw_f64(wav))


def whisper_floor_shares(wav):
    """(share of cells at the `max - 8` floor, share at the 1e-10 power floor, window maximum of raw), from the model alone.  A cell counts for the
    floor that decides its value: where max - 8 < -10 the power floor is the one that binds."""
    raw = whisper_raw_f64(wav)
    m = np.float32(raw.max())
    dyn = np.float32(m - np.float32(8.0))
    at_dyn = (raw <= dyn) if dyn >= WHISPER_RAW_FLOOR else np.zeros(raw.shape, bool)
    at_pow = (raw == WHISPER_RAW_FLOOR) & ~at_dyn
    return float(at_dyn.mean()), float(at_pow.mean()), float(m)


def whisper_features(wsd, wav, gmax=None):
    """(n // 320, 5, 384) float32: oracle encoder on the float64-model log-mel, sliced as Audio2Feature.audio2feat does."""
    wav = np.asarray(wav, np.float32)
    mel = torch.from_numpy(whisper_finish(whisper_raw_f64(wav), gmax))
    _, emb = WR.encoder_forward(wsd, WR.pad_or_trim(mel)[None])
    return emb[0].permute(1, 0, 2)[: len(wav) // 320].contiguous().numpy()


# ---- wav2vec2 input normalisation -----------------------------------------------------------------------------------------------------------------
def w2v_normalize(wav, eps=1e-7):
    """(x - mean) / sqrt(var + eps) per row, population variance, float64 -> float32 [S, n]"""
    x = np.atleast_2d(np.asarray(wav, np.float32)).astype(np.float64)
    return ((x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + eps)).astype(np.float32)


def w2v_logits(model, wav, eps=1e-7):
    """transformers' model on the float64 normalisation (eps = 1e-7 is what its feature extractor applies)"""
    with torch.no_grad():
        return model(torch.from_numpy(w2v_normalize(wav, eps))).logits.numpy()


def w2v_min_samples(cfg):
    """the shortest waveform the convolutional feature extractor turns into one frame"""
    n = 1
    for k, s in zip(reversed(cfg["conv_kernel"]), reversed(cfg["conv_stride"])):
        n = (n - 1) * s + k
    return n


# ---- signals ----------------------------------------------------------------------------------------------------------------------------------------
def burst_silence_hiss(n, gain=1.0, seed=0):
    """two tones in the first quarter, exact zeros in the second, 1e-4 noise in the second half; the whole scaled by `gain`"""
    rng = np.random.default_rng(7100 + seed)
    t = np.arange(n) / 16000.0
    q, h = n // 4, n // 2
    x = np.zeros(n)
    x[:q] = 0.45 * np.sin(2 * np.pi * 440.0 * t[:q]) + 0.35 * np.sin(2 * np.pi * 2500.0 * t[:q] + 0.7)
    x[h:] = 1e-4 * rng.standard_normal(n - h)
    return (gain * x).astype(np.float32)


LOUD_TONE_HZ = 3250.0


def loud_tone(n):
    """full-scale square wave at the frequency where a sweep of square waves drives the Wav2Lip mel highest (3.46 of 4; test_audio_frontend_ref.py)"""
    t = np.arange(n) / 16000.0
    return np.where(np.sin(2 * np.pi * LOUD_TONE_HZ * t + 0.3) >= 0, 1.0, -1.0).astype(np.float32)


DC_QUIET_GAIN = 1e-3


def dc_quiet(n, gain=DC_QUIET_GAIN, dc=0.1, seed=0):
    """a quiet speech-like signal riding on a DC offset: variance ~ (0.13 * gain)^2, next to the normalisation's 1e-7"""
    from mere_fusion_amd import weights as W
    return (dc + gain * W.make_speech_like_wav(n, 40 + seed).astype(np.float64)).astype(np.float32)


def mel_shares(wav, pad_mode="constant"):
    """Wav2Lip mel from the float64 oracle: (share at -4, share at +4, share strictly inside, maximum)"""
    m = mel_ref.melspectrogram(np.asarray(wav, np.float32), pad_mode)
    return float((m == -4.0).mean()), float((m == 4.0).mean()), float(((m > -4.0) & (m < 4.0)).mean()), float(m.max())


# ---- what the CPU tier (test_audio_frontend_ref.py) pins on the models alone and the GPU tests then ask of the kernels ----------------------------
WHISPER_LENGTHS = (201, 320, 479, 480, 1600, 3200)
# least share of cells the float64 model puts at the `max - 8` floor (burst_silence_hiss, gain 1) and at the 1e-10 power floor (gain 1e-3), per length.
# Measured: 480: 33 % / 40 %, 1600: 60 % / 67 %, 3200: 74 % / 82 %, 11520: 89 % / 92 %; below 480 samples the burst fills the only frames there are.
WHISPER_DYN_SHARE = {201: 0.0, 320: 0.0, 479: 0.0, 480: 0.30, 1600: 0.55, 3200: 0.70, 11520: 0.85}
WHISPER_POW_SHARE = {201: 0.0, 320: 0.0, 479: 0.0, 480: 0.35, 1600: 0.60, 3200: 0.75, 11520: 0.90}
# Wav2Lip mel, least share at -4 / strictly inside (-4, 4).  Measured at 3200: gain 1 61 % / 39 %, gain 1e-3 97.5 % / 2.5 %, loud_tone 5 % / 95 %.
MEL_SHARES = {"burst": (0.55, 0.35), "burst_quiet": (0.95, 0.01), "loud": (0.0, 0.90)}
MEL_SIGNAL_N = 3200


def mel_signal(name, n):
    return {"burst": lambda: burst_silence_hiss(n, 1.0), "burst_quiet": lambda: burst_silence_hiss(n, 1e-3), "loud": lambda: loud_tone(n)}[name]()


def w2v_rows(n):
    from mere_fusion_amd import weights as W
    """[speech-like x 0.6, zeros (what NerfASRFrontend feeds for the first 17 steps), quiet on a DC offset, a constant]"""
    return np.stack([W.make_speech_like_wav(n, 0) * np.float32(0.6), np.zeros(n, np.float32), dc_quiet(n, DC_QUIET_GAIN, 0.1),
                     np.full(n, 0.25, np.float32)])


def w2v_lengths():
    from mere_fusion_amd import weights as W
    return (8960, w2v_min_samples(W.WAV2VEC2_SMALL) + 1)
