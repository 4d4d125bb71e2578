"""What the lip-sync tests share (test_sync_host.py, test_sync_gpu.py, golden/make_syncnet_golden.py): the seeded golden clip, the float64 statements of the
window rule and of mf_sync_score, and the gates.

Gates.  The embedding gates are set the way TOL_X3 of test_wav2lip_gpu.py was: the error against the float64 golden measured on the MI355X, times about 4, never
above the project's bf16x3 bound of 1e-3.  mf_sync_score's own gate is the fp32 dot-product bound (dim + 4) 2^-24 at dim 512 (unit vectors: sum |a_i b_i| <= 1),
4e-5, and 7e-5 at dim 1024.  `sim` of the whole path gets no number of its own: two unit vectors off by e_f and e_a move their cosine by at most
e_a + e_f + e_a e_f, plus the kernel's 4e-5."""
import numpy as np

TOL_X3 = 1.6e-5      # measured on the MI355X over batches 1, 2 and 5 (chunked): face 3.5e-6, audio 3.9e-6 (L-inf of the normalised embeddings vs the float64 golden)
TOL_BF16 = 8e-3      # measured: face 1.9e-3, audio 1.2e-3
TOL_SCORE = 4e-5
TOL_SCORE_1024 = 7e-5

FPS, T, MEL_STEP, MEL_PER_SECOND = 25, 5, 16, 80
N_FRAMES, N_SAMPLES = 6, 3840


def sim_bound(tol):
    return 2 * tol + tol * tol + TOL_SCORE


def golden_frames(n=N_FRAMES, size=96, seed=0):
    """uint8 BGR [n, size, size, 3]: a vertical gradient, two soft blobs that travel between frames and a little noise -- large-scale structure that moves, because
    the face encoder averages plain noise away (embeddings of different noise windows lie 2e-3 apart)"""
    rng = np.random.default_rng(4000 + seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    out = np.empty((n, size, size, 3), dtype=np.uint8)
    for i in range(n):
        img = np.empty((size, size, 3))
        for c in range(3):
            img[..., c] = 40 + 60 * (yy / size) * (1 + 0.3 * c)
        for b, (amp, sig) in enumerate(((150.0, 10.0), (-90.0, 16.0))):
            cx = size * (0.25 + 0.1 * i + 0.3 * b)
            cy = size * (0.62 + 0.05 * i * (1 - 2 * b) + 0.12 * b)
            blob = amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig))
            for c in range(3):
                img[..., c] += blob * (1.0 - 0.25 * c)
        img += rng.uniform(-6, 6, img.shape)
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def golden_pcm(n=N_SAMPLES, seed=0):
    from mere_fusion_amd import weights as W
    return W.make_speech_like_wav(n, seed)


def window_starts(n_frames, n_samples, fps=FPS):
    """[(first frame, first mel column)] of the windows a clip gives: window i starts at frame i, its mel window at int(80 * i / fps), 16 columns of the
    1 + n_samples // 200 the mel has; a window whose mel would run past the end is dropped (and every later one with it)"""
    mel_len = 1 + n_samples // 200
    out = []
    for i in range(max(0, n_frames - T + 1)):
        m = int(MEL_PER_SECOND * i / fps)
        if m + MEL_STEP > mel_len:
            break
        out.append((i, m))
    return out


def face_windows(frames_u8, starts):
    """float64 [W, 15, H / 2, W]: 5 BGR frames on the channel axis, / 255., lower half"""
    h = frames_u8.shape[1]
    return np.stack([np.concatenate([frames_u8[s + t] for t in range(T)], axis=2)[h // 2:].transpose(2, 0, 1) / 255.0 for s in starts])


def sync_score_ref(face, audio, S):
    """float64 mf_sync_score: (sim [W, 2 S + 1], curve, counts)"""
    f, a = np.asarray(face, dtype=np.float64), np.asarray(audio, dtype=np.float64)
    W = f.shape[0]
    fn = np.maximum(np.sqrt((f * f).sum(1)), 1e-12)
    an = np.maximum(np.sqrt((a * a).sum(1)), 1e-12)
    sim = np.zeros((W, 2 * S + 1))
    counts = np.zeros(2 * S + 1, dtype=np.int32)
    for w in range(W):
        for s in range(2 * S + 1):
            j = w + s - S
            if 0 <= j < W:
                sim[w, s] = (f[w] * a[j]).sum() / (fn[w] * an[j])
                counts[s] += 1
    curve = np.where(counts > 0, sim.sum(0) / np.maximum(counts, 1), 0.0)
    return sim, curve, counts
