"""GPU: the lip-sync scorer on the device -- the window-input kernel bit for bit, mf_sync_score against float64, the two conv geometries SyncNet adds, the whole
network against the float64 golden of the reference's own module, SyncScorer on the golden clip and SyncMonitor's rings.  Gates: tests/sync_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import sync_ref as SR
import syncnet_geometry_cases as SG

pytestmark = pytest.mark.gpu
PRECS = ["bf16x3", "bf16"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "syncnet_golden.npz")))


@pytest.fixture(scope="module")
def models(lib_built):
    """SyncNet_color on cuda:0 with the seeded weights, cached per (precision, max_batch)"""
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.wav2lip.models import SyncNet_color
    sd, cache = W.syncnet_state_dict(0), {}

    def make(prec, max_batch=4):
        if (prec, max_batch) not in cache:
            m = SyncNet_color(precision=prec, max_batch=max_batch)
            m.load_state_dict(sd)
            cache[(prec, max_batch)] = m.to("cuda").eval()
        return cache[(prec, max_batch)]

    return make


# ---- mf_net_set_input_u8_windows -----------------------------------------------------------------------------------------------------------------------------
# (n_frames, H, W, starts, T, row0, rows)
WINDOW_CASES = [
    ("one window, exactly 5 frames", 5, 12, 16, [0], 5, 6, 6),
    ("overlap and the last legal start", 7, 12, 16, [0, 2], 5, 6, 6),
    ("odd geometry", 4, 8, 10, [1, 0, 1], 3, 4, 4),
    ("96 x 96, T 5", 6, 96, 96, [0, 1], 5, 48, 48),
]


def _window_net(prec, T, rows, W, cap=4):
    from mere_fusion_amd.avatar.net import Net
    n = Net(cap, prec, "cuda")
    return n, n.buffer(3 * T, rows, W, 1)


def _float_windows(frames, starts, T, row0, rows):
    f = frames.cpu().numpy()
    return torch.from_numpy(np.stack([np.concatenate([f[s + t] for t in range(T)], axis=2)[row0:row0 + rows].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
                                      for s in starts]))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_u8_windows_bit_equal_to_float_input(lib_built, prec, case):
    _, nf, H, W, starts, T, row0, rows = case
    g = torch.Generator().manual_seed(nf * H + W)
    frames = torch.randint(0, 256, (nf, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    n, buf = _window_net(prec, T, rows, W)
    Cb = (3 * T + 7) // 8 * 8                                               # read the zero padding channels too
    want_f = _float_windows(frames, starts, T, row0, rows)
    poison = torch.full((len(starts), 3 * T, rows, W), 7.0)
    n.set_input(buf, poison)
    assert n.set_input_u8_windows(buf, frames, starts, T, row0, rows) == len(starts)
    got = n.output(buf, Cb, len(starts)).cpu()
    n.set_input(buf, poison)
    n.set_input(buf, want_f)
    want = n.output(buf, Cb, len(starts)).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not bool((got[:, :3 * T] == 7.0).any()) and bool((got[:, 3 * T:] == 0).all())
    assert (got[:, :3 * T] - want_f).abs().max().item() <= (2.0 ** -16 if prec == "bf16x3" else 2.0 ** -8)


def test_u8_windows_refusals_leave_the_buffer_untouched(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    nf, H, W, T = 7, 12, 16, 5
    frames = torch.randint(0, 256, (nf, H, W, 3), dtype=torch.uint8).cuda()
    n, buf = _window_net("bf16x3", T, 6, W, cap=2)
    other = n.buffer(3, 6, W, 1)
    n.set_input(buf, torch.full((2, 15, 6, W), 7.0))
    before = n.output(buf, 16, 2).cpu()

    def call(b, starts, n_frames=nf, h=H, w=W, t=T, row0=6, rows=6):
        rc = l.mf_net_set_input_u8_windows(n._h, b, C.c_void_p(frames.data_ptr()), n_frames, h, w, (C.c_int * len(starts))(*starts), len(starts), t, row0, rows, None)
        return rc, l.mf_last_error().decode()

    for args, word in ((dict(b=buf, starts=[-1]), "outside the 7 given"), (dict(b=buf, starts=[0, 3]), "outside the 7 given"),
                       (dict(b=buf, starts=[0], row0=7), "outside the frame height 12"), (dict(b=buf, starts=[0, 1, 2]), "exceed the capacity 2"),
                       (dict(b=other, starts=[0]), "channels"), (dict(b=buf, starts=[0], t=6), "channels"), (dict(b=buf, starts=[0], row0=0, rows=12), "the windows are 12 x 16"),
                       (dict(b=buf, starts=[0], w=15), "the windows are 6 x 15"), (dict(b=99, starts=[0]), "no buffer 99")):
        rc, msg = call(**args)
        assert rc == -1 and word in msg, (args, msg)
    torch.cuda.synchronize()
    assert torch.equal(n.output(buf, 16, 2).cpu(), before)
    rc, msg = call(b=buf, starts=[2, 0])                                    # (and the legal call still works)
    assert rc == 0, msg
    assert not torch.equal(n.output(buf, 16, 2).cpu(), before)


# ---- mf_sync_score ------------------------------------------------------------------------------------------------------------------------------------------------
SCORE_CASES = [(1, 0, 4), (1, 3, 512), (3, 5, 512), (65, 15, 512), (8, 64, 1024)]


def _embeddings(W, dim, seed):
    rng = np.random.default_rng(seed)
    f, a = np.maximum(rng.standard_normal((W, dim)), 0), np.maximum(rng.standard_normal((W, dim)), 0)         # post-ReLU, like the network's
    f, a = f / np.linalg.norm(f, axis=1, keepdims=True), a / np.linalg.norm(a, axis=1, keepdims=True)
    return f.astype(np.float32), a.astype(np.float32)


def _score(f, a, S):
    from mere_fusion_amd.sync_score import sync_score
    W = f.shape[0]
    out = (torch.full((W, 2 * S + 1), float("nan"), device="cuda"), torch.full((2 * (2 * S + 1),), float("nan"), device="cuda"))
    sim, curve, counts = sync_score(torch.from_numpy(f).cuda(), torch.from_numpy(a).cuda(), S, out=out)
    return sim.cpu(), curve.cpu(), counts.cpu()


@pytest.mark.parametrize("W,S,dim", SCORE_CASES)
def test_sync_score_vs_fp64(lib_built, W, S, dim):
    f, a = _embeddings(W, dim, W * 1000 + S)
    if W >= 3:
        f[1] = 0                                                            # an all-zero row scores 0, never NaN
        a[2] *= 1e4                                                         # the kernel normalises
    if W >= 8:
        a[5] = 0
        f[6] *= 1e4
    tol = SR.TOL_SCORE_1024 if dim == 1024 else SR.TOL_SCORE
    sim, curve, counts = _score(f, a, S)
    want_sim, want_curve, want_counts = SR.sync_score_ref(f, a, S)
    assert np.array_equal(counts.numpy(), want_counts)
    e_sim, e_curve = np.abs(sim.numpy() - want_sim).max(), np.abs(curve.numpy() - want_curve).max()
    print(f"[sync_score] W {W} S {S} dim {dim}: sim error {e_sim:.3e}, curve error {e_curve:.3e} (gate {tol})")
    assert e_sim <= tol and e_curve <= tol                                  # (NaN, an entry nobody wrote, fails)
    if W >= 3:
        assert bool((sim[1] == 0).all())
        assert bool((sim.numpy()[want_sim == 0] == 0).all())                # entries outside [0, W) are written as exact zeros
    if (W, S) == (1, 3):
        assert counts.tolist() == [0, 0, 0, 1, 0, 0, 0] and curve[:3].abs().sum() == 0 and curve[4:].abs().sum() == 0
    sim2, curve2, counts2 = _score(f, a, S)                                 # summed in a fixed order: two runs, the same bits
    assert torch.equal(sim.view(torch.int32), sim2.view(torch.int32)) and torch.equal(curve.view(torch.int32), curve2.view(torch.int32)) and torch.equal(counts, counts2)


# ---- the two new conv geometries ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch", SG.BATCHES)
@pytest.mark.parametrize("case", SG.CASES, ids=[c[0] for c in SG.CASES])
def test_syncnet_conv_geometries_vs_fp64(lib_built, prec, batch, case):
    from test_conv_configs import Layer
    name, d = case
    lay = Layer(d, prec, seed=sum(map(ord, name)), bn=True)
    try:
        assert not lay.rc, lay.err
        assert (lay.oh, lay.ow) == SG.OUT_HW[name]
        cfg = lay.config(batch)
        x = lay.input(batch)
        y, _ = lay.forward(x)
        e = lay.check(x, y, f"{name} {prec} batch {batch} {cfg}")
        print(f"[syncnet conv] {name} {prec} batch {batch}: {cfg['family']} tile {cfg['tile']} split {cfg['split']}, worst {e:.4f} U A")
    finally:
        lay.close()


# ---- the whole network ---------------------------------------------------------------------------------------------------------------------------------------------
def _inputs(golden, rows):
    mel = torch.from_numpy(golden["mel_windows"][rows]).cuda()
    face = torch.from_numpy((golden["face_windows_u8"][rows].astype(np.float32) / np.float32(255.0))).cuda()
    return mel, face


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows", [[0], [0, 1], [1, 0, 1, 1, 0]], ids=["batch1", "batch2", "batch5_chunked"])
def test_syncnet_vs_golden(models, golden, prec, rows):
    """normalised embeddings against the reference's module in float64; batch 5 on max_batch 4 takes the chunked path (4 + 1)"""
    m = models(prec, 4)
    mel, face = _inputs(golden, rows)
    with torch.no_grad():
        a, f = m(mel, face)
    assert a.is_cuda and f.is_cuda and a.shape == f.shape == (len(rows), 512)
    e_a = np.abs(a.cpu().numpy().astype(np.float64) - golden["audio_embedding"][rows]).max()
    e_f = np.abs(f.cpu().numpy().astype(np.float64) - golden["face_embedding"][rows]).max()
    tol = SR.TOL_X3 if prec == "bf16x3" else SR.TOL_BF16
    print(f"[syncnet] {prec} batch {len(rows)}: audio embedding error {e_a:.3e}, face embedding error {e_f:.3e} (gate {tol})")
    assert e_a <= tol and e_f <= tol
    assert np.abs(np.linalg.norm(a.cpu().numpy().astype(np.float64), axis=1) - 1).max() <= 1e-6
    # the raw embeddings through the score kernel: the derived bound, no number of its own
    from mere_fusion_amd.sync_score import sync_score
    S = int(golden["max_shift"])
    if rows == [0, 1]:
        sim, curve, counts = sync_score(m.embed_faces(face), m.embed_audio(mel), S)
        bound = SR.sim_bound(tol)
        assert np.abs(sim.cpu().numpy() - golden["sim"]).max() <= bound and np.abs(curve.cpu().numpy() - golden["curve"]).max() <= bound
        assert np.array_equal(counts.cpu().numpy(), golden["counts"])


def test_syncnet_stage_taps_vs_golden(models, golden):
    """the face encoder after each of its 6 stages (bf16x3, batch 2), sampled as the golden samples them: within the project's bf16x3 bound of 1e-3, taken relative
    to the stage's largest sampled activation (the bound is stated for O(1) outputs; the stages are not normalised)"""
    import geometry_cases as G
    from mere_fusion_amd import weights as W
    m = models("bf16x3", 4)
    mel, face = _inputs(golden, [0, 1])
    with torch.no_grad():
        m(mel, face)
    for i in W.SYNCNET_FACE_STAGE_ENDS:
        got = m.read_tap(f"face_encoder.{i}", 2).cpu().reshape(-1).numpy()[:: G.TAP_STRIDE][: G.TAP_MAX]
        want = golden[f"tap_sample/face_encoder.{i}"]
        assert got.shape == want.shape
        e, scale = np.abs(got - want).max(), max(1.0, np.abs(want).max())
        print(f"[syncnet tap] face_encoder.{i}: error {e:.3e} at scale {scale:.2f}")
        assert e <= 1e-3 * scale, i


# ---- scorer and monitor ----------------------------------------------------------------------------------------------------------------------------------------------
def test_scorer_on_the_golden_clip(models, golden):
    from mere_fusion_amd.sync_score import SyncScorer, reduce_curve
    S = int(golden["max_shift"])
    scorer = SyncScorer(models("bf16x3", 4), fps=25, max_shift=S, max_batch=4)
    r = scorer.score(torch.from_numpy(golden["frames"]).cuda(), torch.from_numpy(golden["pcm"]).cuda())
    assert r.W == 2 and r.frame_starts == golden["frame_starts"].tolist() and r.mel_starts == golden["mel_starts"].tolist()
    bound = SR.sim_bound(SR.TOL_X3)
    e_sim, e_curve = np.abs(r.sim.cpu().numpy() - golden["sim"]).max(), np.abs(r.curve.cpu().numpy() - golden["curve"]).max()
    print(f"[scorer] sim error {e_sim:.3e}, curve error {e_curve:.3e} (bound {bound:.3e}); offset {r.offset}, score {r.score:.6f}, confidence {r.confidence:.3e}")
    assert e_sim <= bound and e_curve <= bound
    assert r.counts == golden["counts"].tolist()
    want_score, want_offset, want_conf = reduce_curve(golden["curve"].tolist(), golden["counts"].tolist(), S)
    assert r.offset == want_offset and abs(r.score - want_score) <= bound and abs(r.confidence - want_conf) <= 2 * bound
    # frames that are not 96 x 96 go through the linear resize first (MuseTalk's faces): the same windows, a score of its own
    big = torch.from_numpy(np.ascontiguousarray(golden["frames"].repeat(2, axis=1).repeat(2, axis=2))).cuda()
    r2 = scorer.score(big, torch.from_numpy(golden["pcm"]).cuda())
    assert r2.W == 2 and r2.counts == r.counts and np.isfinite(r2.curve_host).all()
    with pytest.raises(ValueError, match="N >= 5"):
        scorer.score(torch.zeros((4, 96, 96, 3), dtype=torch.uint8, device="cuda"), torch.zeros(3840, device="cuda"))


def test_monitor_two_pushes_equal_the_whole_clip(models, golden):
    from mere_fusion_amd.sync_score import SyncMonitor, SyncScorer
    scorer = SyncScorer(models("bf16x3", 4), fps=25, max_shift=int(golden["max_shift"]), max_batch=4)
    frames, pcm = torch.from_numpy(golden["frames"]).cuda(), torch.from_numpy(golden["pcm"]).cuda()
    whole = scorer.score(frames, pcm)
    for seconds in (4.0, 0.24):                                             # a ring with room to spare, and one of exactly 6 frames
        mon = SyncMonitor(scorer, seconds=seconds)
        if seconds < 1:
            assert mon.capacity == 6
            mon.push(frames[2:6], pcm[2 * 640:6 * 640])                     # older content that the two pushes below must overwrite, across the wrap
        mon.push(frames[:4], pcm[:4 * 640])
        mon.push(frames[4:], pcm[4 * 640:])
        r = mon.report()
        assert r.W == whole.W and r.counts == whole.counts
        assert torch.equal(r.sim.view(torch.int32), whole.sim.view(torch.int32)) and torch.equal(r.curve.view(torch.int32), whole.curve.view(torch.int32))
        assert (r.score, r.offset, r.confidence) == (whole.score, whole.offset, whole.confidence)
