"""The device ops behind the DWPose landmark network, one at a time, in the manner of test_net_ops.py: float64 (or the exact numpy restatement of
tests/dwpose_ref.py) on the CPU, bounds from the storage format's unit roundoff U[prec] and fp32's F32, never measured; output buffers pre-filled with SENT and
inputs flanked by BIG so that a write or read outside the op's channel slice shows.  The oracle is UNPINNED (dwpose_ref.py says why)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwpose_ref as R
from conv_numerics import F32, U, exact
from test_net_ops import BIG, PRECS, SENT, _assert_untouched, _get, _net, _sentinel, _set, _with_neighbours, pad8  # noqa: F401

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- depthwise conv --------------------------------------------------------------------------------------------------------------------------
DW_MAPS = [(1, 1), (3, 5), (12, 9), (17, 13), (9, 9)]                          # 9 x 9: one more than the kernel's 8 x 8 output tile in each direction (stride 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("hw", DW_MAPS + [(18, 17)], ids=lambda m: f"{m[0]}x{m[1]}")   # 18 x 17 at stride 2 gives the 9 x 9 output
def test_dwconv(lib_built, prec, k, stride, hw):
    """Conv2d(C, C, k, stride, k // 2, groups=C) + BatchNorm2d(eps 1e-3) + SiLU against float64, on one net of capacity 2 run at batch 1 and at batch 2 (item 1 differs from item 0).
    Bound per element, with A = sum |x| |w'| + |b'| over the taps (w', b' the folded weights): the folded weights are fp32 roundings of a float64 fold (F32 each), the
    k * k products accumulate in fp32 and the bias is added ((k * k + 2) F32 A in all, worst case), SiLU's slope is below 1.1; the fast exponential and the division
    are allowed 16 fp32 ulp of the result; the store rounds to the format: U[prec] |y|."""
    H, W = hw
    rng = np.random.default_rng(100 * k + 10 * stride + H)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    for Cn, xoff, yoff in ((5, 0, 0), (8, 8, 0), (19, 3, 5), (64, 0, 8)):
        x = exact(rng, (2, Cn, H, W), prec)
        w = rng.standard_normal((Cn, 1, k, k)).astype(np.float32)
        g, be, m, v = (rng.uniform(0.5, 2, Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32),
                       rng.uniform(0.5, 2, Cn).astype(np.float32))
        n = _net(prec)
        wi, wo = pad8(xoff + Cn + 1), pad8(yoff + Cn + 1)
        ib, ob = n.buffer(wi, H, W, 0), n.buffer(wo, Ho, Wo, 1)
        n.dwconv(torch.from_numpy(w), ib, ob, stride, act=4, bn=tuple(torch.from_numpy(a) for a in (g, be, m, v)), bn_eps=1e-3, in_coff=xoff, out_coff=yoff)
        _set(n, ib, _with_neighbours(x, xoff, wi))
        sc = g.astype(np.float64) / np.sqrt(v.astype(np.float64) + 1e-3)
        wf, bf = torch.from_numpy(w.astype(np.float64) * sc.reshape(-1, 1, 1, 1)), torch.from_numpy(be - m * sc)
        xt = torch.from_numpy(x).double()
        z = F.conv2d(xt, wf, bf, stride, k // 2, groups=Cn)
        A = F.conv2d(xt.abs(), wf.abs(), bf.abs(), stride, k // 2, groups=Cn).numpy()
        want = F.silu(z).numpy()
        bound = 1.1 * (k * k + 2) * F32 * A + 16 * F32 * np.abs(want) + U[prec] * np.abs(want) + 1e-30
        keep = np.zeros(wo, bool); keep[yoff:yoff + Cn] = True
        for batch in (1, 2):                                                    # the same net (capacity 2) at batch 1, then at batch 2
            _sentinel(n, ob, 2)
            n.run(batch)
            got = _get(n, ob, 2)
            assert (got[batch:] == SENT).all(), f"dwconv C={Cn}: a run at batch {batch} wrote into item {batch}"
            _assert_untouched(got[:batch], keep, f"dwconv C={Cn} batch {batch}")
            err = np.abs(got[:batch, yoff:yoff + Cn] - want[:batch])
            r = err / bound[:batch]
            assert (r <= 1).all(), f"C={Cn}, batch {batch}: worst error / bound = {r.max():.3f} at {np.unravel_index(r.argmax(), err.shape)}"


def test_dwconv_refusals(lib_built):
    n = _net("bf16x3")
    a, b = n.buffer(8, 6, 6, 0), n.buffer(8, 6, 6, 0)
    w7 = torch.zeros(8, 1, 7, 7)
    with pytest.raises(RuntimeError, match="k must be 3 or 5"):
        n.dwconv(w7, a, b)
    with pytest.raises(RuntimeError, match="does not match"):
        n.dwconv(torch.zeros(8, 1, 3, 3), a, b, 2)
    with pytest.raises(RuntimeError, match="channel slice"):
        n.dwconv(torch.zeros(8, 1, 3, 3), a, b, 1, in_coff=1)


# ---- channel attention -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cn", [13, 128])
def test_chan_attn(lib_built, prec, Cn):
    """x * hardsigmoid(fc(pooled)).  The fc's bias places a third of the channels below -3, a third inside the linear range and a third above 3, so all three
    branches of hard-sigmoid run (asserted on the float64 pre-activations).  Bound: z = sum_j w p + b over C terms in fp32, worst case (C + 1) F32 A with
    A = sum |w| |p| + |b|; hard-sigmoid's slope is 1 / 6 and its own two operations round twice; the product and the store: (2 F32 + U[prec]) |y|."""
    rng = np.random.default_rng(Cn)
    H, W, xoff, yoff = 5, 7, 8, 16
    x, p = exact(rng, (2, Cn, H, W), prec), exact(rng, (2, Cn, 1, 1), prec)
    w = (rng.standard_normal((Cn, Cn)) / np.sqrt(Cn)).astype(np.float32)
    b = np.where(np.arange(Cn) % 3 == 0, -8.0, np.where(np.arange(Cn) % 3 == 1, 0.25, 8.0)).astype(np.float32)
    n = _net(prec)
    wi, wo = pad8(xoff + Cn + 1), pad8(yoff + Cn + 1)
    xb, pb, ob = n.buffer(wi, H, W, 1), n.buffer(Cn, 1, 1, 0), n.buffer(wo, H, W, 0)
    n.chan_attn(xb, Cn, pb, torch.from_numpy(w), torch.from_numpy(b), ob, x_coff=xoff, out_coff=yoff)
    _set(n, xb, _with_neighbours(x, xoff, wi)); _set(n, pb, p); _sentinel(n, ob, 2)
    n.run(2)
    got = _get(n, ob, 2)
    keep = np.zeros(wo, bool); keep[yoff:yoff + Cn] = True
    _assert_untouched(got, keep, "chan_attn")
    p64 = p.reshape(2, Cn).astype(np.float64)
    z = p64 @ w.astype(np.float64).T + b
    assert (z < -3).any() and (z > 3).any() and ((z > -3) & (z < 3)).any()
    A = np.abs(p64) @ np.abs(w.astype(np.float64)).T + np.abs(b)
    s = np.clip(z / 6 + 0.5, 0, 1)
    want = x.astype(np.float64) * s[:, :, None, None]
    ds = ((Cn + 1) * F32 * A / 6 + 2 * F32)[:, :, None, None]
    bound = np.abs(x) * ds + (2 * F32 + U[prec]) * np.abs(want) + 1e-30
    err = np.abs(got[:, yoff:yoff + Cn] - want)
    assert (err <= bound).all(), f"worst error / bound = {(err / bound).max():.3f}"


# ---- RTMCC head ------------------------------------------------------------------------------------------------------------------------------
def _head_case(K, hw, hidden, s, bx, by, batch, prec, seed):
    from mere_fusion_amd import _lib
    rng = np.random.default_rng(seed)
    h, w = hw
    head = R.RTMCCHead(8, K, (bx // 2, by // 2), (w, h), hidden, s).double()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in head.named_parameters():
            if name.endswith(".g"):
                t.copy_(torch.rand(1, generator=g).double() * 0.4 + 0.8)
            elif name == "gau.o.weight":
                t.copy_(torch.randn(t.shape, generator=g).double() * 0.05 / np.sqrt(t.shape[1]))
            elif t.dim() == 2 and "gau.gamma" not in name and "gau.beta" not in name:
                t.copy_(torch.randn(t.shape, generator=g).double() * 1.5 / np.sqrt(t.shape[1]))
            else:
                t.copy_(torch.rand(t.shape, generator=g).double())
    maps = exact(rng, (batch, K, h, w), prec)
    with torch.no_grad():
        t64 = head.tokens(torch.from_numpy(maps).double())
        want = head.cls_x(t64).numpy(), head.cls_y(t64).numpy()
    n = _net(prec, max_batch=batch)
    coff = 8
    mb = n.buffer(pad8(coff + K + 1), h, w, 0)
    _set(n, mb, _with_neighbours(maps, coff, pad8(coff + K + 1)))
    sd = {k: v.detach().float().contiguous() for k, v in head.state_dict().items()}
    hh = C.c_void_p()
    keys = ("mlp.0.g", "mlp.1.weight", "gau.ln.g", "gau.uv.weight", "gau.gamma", "gau.beta", "gau.o.weight", "gau.res_scale.scale", "cls_x.weight", "cls_y.weight")
    _lib.check(_lib.lib().mf_rtmcc_head_create(K, h * w, hidden, s, bx, by, *[_p(sd[k]) for k in keys], batch, C.byref(hh)), "rtmcc_head_create")
    try:
        lx = torch.full((batch + 1, K, bx), SENT, device="cuda")
        ly = torch.full((batch + 1, K, by), SENT, device="cuda")
        _lib.check(_lib.lib().mf_rtmcc_head_forward(hh, n._h, mb, coff, batch, _p(lx), _p(ly), _stream()), "rtmcc_head_forward")
        torch.cuda.synchronize()
        lx, ly = lx.cpu().numpy(), ly.cpu().numpy()
    finally:
        _lib.lib().mf_rtmcc_head_destroy(hh)
    assert (lx[batch] == SENT).all() and (ly[batch] == SENT).all(), "the head wrote past its batch"
    # the head's weights are fp32 roundings of the float64 module's (F32 each) and every product chain runs in fp32: dot lengths flat, hidden (uv), s (q k^T), K
    # (kernel v), 2 hidden (out), hidden (cls); the worst case of a length-n fp32 dot is n F32 of its sum of magnitudes.  The squared kernel doubles q k^T's relative
    # error and u * (kernel v) * o multiplies three erroneous factors: 8 x the summed lengths, relative to the largest logit.
    lengths = h * w + hidden + s + K + 2 * hidden + hidden
    bound = 8 * lengths * F32
    for got, ref, name in ((lx[:batch], want[0], "x"), (ly[:batch], want[1], "y")):
        rel = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"rtmcc head {name}: max|d| / max|oracle| = {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (name, rel, bound)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("batch", [1, 3])
def test_rtmcc_head_reduced(lib_built, prec, batch):
    """17 tokens (three tiles of 8, the last with one token), a 4 x 3 map, hidden 32, s 16, 24 and 32 bins; the maps sit at channel 8 of a wider buffer whose
    other channels hold BIG.  The maps are exact in the storage format, so `prec` only selects the buffer's read path."""
    _head_case(17, (4, 3), 32, 16, 24, 32, batch, prec, 5)


def test_rtmcc_head_full_size(lib_built):
    """133 tokens of 12 x 9, hidden 256, s 128, 576 and 768 bins, once"""
    _head_case(133, (12, 9), 256, 128, 576, 768, 1, "bf16x3", 6)


# ---- SimCC decode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("K,bx,by", [(133, 576, 768), (17, 24, 32), (5, 65, 130)])
def test_simcc_decode_bit_exact(lib_built, flip, K, bx, by):
    """against dwpose_ref.decode on logits with ties (quantised values), all-negative rows (location -1 -> -0.5 after the split ratio), a non-positive maximum of
    exactly 0, and the maximum in the first and in the last bin"""
    from mere_fusion_amd.avatar.dwpose import simcc_decode
    rng = np.random.default_rng(K + flip)
    B = 3

    def draw(n):
        a = np.round(rng.standard_normal((B, K, n)) * 4).astype(np.float32) / 4            # many ties
        a[0, 0] = -np.abs(a[0, 0]) - 1                                                     # all negative
        a[0, 1] = -np.abs(a[0, 1]); a[0, 1, n // 2] = 0                                    # maximum exactly 0
        a[1, 0, 0] = 50; a[1, 1, n - 1] = 50; a[1, 2, 0] = 50; a[1, 2, n - 1] = 50         # first bin, last bin, a tie between them
        a[2, 0] = 1.0                                                                      # every bin ties
        return a
    x, y = draw(bx), draw(by)
    xf, yf = (draw(bx), draw(by)) if flip else (None, None)
    pairs = R.flip_indices(K)
    center, scale = np.array([320.0, 240.5], np.float32), np.array([800.0, 1066.6666], np.float32)
    want_k, want_s = R.decode(x, y, center, scale, xf, yf, pairs, (bx // 2, by // 2))
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()
    kp, sc = simcc_decode(t(x), t(y), t(xf), t(yf), pairs if flip else None, (bx // 2, by // 2), center, scale)
    assert np.array_equal(kp.cpu().numpy().view(np.uint32), want_k.view(np.uint32))
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
    assert (want_k[0, 0] == ((np.float32(-0.5) / np.array([bx // 2, by // 2], np.float32)) * scale + center) - scale * np.float32(0.5)).all()


# ---- warp ------------------------------------------------------------------------------------------------------------------------------------
def _warp_device(frames, minv, in_wh, prec, mean, std, flip):
    from mere_fusion_amd import _lib
    n = frames.shape[0]
    net = _net(prec, max_batch=2 * n)
    buf = net.buffer(3, in_wh[1], in_wh[0], 1)
    fr, mv = torch.from_numpy(frames).cuda(), torch.from_numpy(np.ascontiguousarray(minv, np.float64)).cuda()
    _lib.check(_lib.lib().mf_warp_affine_u8(net._h, buf, _p(fr), n, frames.shape[1], frames.shape[2], _p(mv), (C.c_float * 3)(*mean), (C.c_float * 3)(*std), 1,
                                            int(flip), _stream()), "warp_affine_u8")
    return _get(net, buf, 2 * n if flip else n)


@pytest.mark.parametrize("hw", [(31, 17), (288, 384), (480, 640)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_warp_affine_u8_is_the_integer_model(lib_built, hw):
    """mean 0 / std 1 make the buffer hold the codes themselves (integers below 256 are exact in both formats): byte-equal to dwpose_ref.warp_affine_int, channels
    reversed, mirrored copies behind the straight ones, padding channels zero.  Job 0 is the top-down map of the whole-image box (its source rectangle is the
    frame padded by 1.25: it leaves the frame on every side); job 1 is a shifted, shrunk map with irrational-looking entries."""
    H, W = hw
    rng = np.random.default_rng(H)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    c, s = R.bbox_center_scale(W, H)
    m0 = R.invert_affine(R.warp_matrix(c, s))
    m1 = np.array([[0.7312345, 0.0213, 3.25], [-0.0171, 0.6698765, 1.75]]) * (W / 288.0)
    out = _warp_device(frames, np.stack([m0, m1]).reshape(2, 6), R.INPUT_SIZE, "bf16", (0, 0, 0), (1, 1, 1), True)
    for j, m in enumerate((m0, m1)):
        want = R.warp_affine_int(frames[j], m, R.INPUT_SIZE)[..., ::-1].transpose(2, 0, 1).astype(np.float32)
        assert np.array_equal(out[j, :3], want), f"job {j}"
        assert np.array_equal(out[2 + j, :3], want[:, :, ::-1]), f"mirror of job {j}"
    assert (out[:, 3:] == 0).all()
    edge = R.warp_affine_int(frames[0], m0, R.INPUT_SIZE)
    assert (edge[0] == 0).all() and (edge[-1] == 0).all() and (edge[:, 0] == 0).all() and (edge[:, -1] == 0).all()      # the border is outside the frame on all sides


@pytest.mark.parametrize("prec", PRECS)
def test_warp_affine_u8_normalises(lib_built, prec):
    """with the config's mean / std the buffer holds the format's rounding of dwpose_ref.normalise, bit for bit"""
    from conv_numerics import stored
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (1, 40, 56, 3), dtype=np.uint8)
    c, s = R.bbox_center_scale(56, 40, input_size=(64, 96))
    m = R.invert_affine(R.warp_matrix(c, s, (64, 96)))
    out = _warp_device(frames, m.reshape(1, 6), (64, 96), prec, R.MEAN, R.STD, False)
    want = stored(R.normalise(R.warp_affine_int(frames[0], m, (64, 96))), prec)
    assert np.array_equal(out[0, :3].view(np.uint32), want.view(np.uint32))


# ---- landmark boxes --------------------------------------------------------------------------------------------------------------------------
def landmark_cases(n, rng, H=480, W=640):
    """n frames cycling through: a normal face, each fallback condition alone, no face, a negative landmark coordinate"""
    kp = np.zeros((n, 133, 2), np.float32)
    boxes = np.zeros((n, 4, 5), np.float32)
    counts = np.ones(n, np.int32)
    for i in range(n):
        face = np.stack([rng.uniform(200, 400, 68), rng.uniform(100, 300, 68)], 1).astype(np.float32)
        face[28, 1], face[29, 1], face[30, 1] = 180.6, 200.3, 221.9
        face[8, 1] = 330.7
        kind = i % 6
        if kind == 1:
            face[:, 1] = 150.2                                                  # y2 - y1 <= 0
        elif kind == 2:
            face[:, 0] = 250.9                                                  # x2 - x1 <= 0
        elif kind == 3:
            face[3, 0] = -1.5                                                   # x1 < 0 (truncates to -1)
        elif kind == 4:
            counts[i] = 0                                                       # no face
        elif kind == 5:
            face[3, 0] = -0.7                                                   # truncates to 0 where floor gives -1: stays a landmark box
        kp[i, R.FACE] = face
        kp[i, :23] = rng.uniform(-50, 700, (23, 2)); kp[i, 91:] = rng.uniform(-50, 700, (42, 2))
        boxes[i, 0] = [rng.uniform(-20, 100), rng.uniform(-20, 100), rng.uniform(500, 700), rng.uniform(400, 520), 0.99]
    return kp, boxes, counts


@pytest.mark.parametrize("n", [1, 6, 33])
@pytest.mark.parametrize("shift", [0, 7, -9])
def test_muse_landmark_boxes_exact(lib_built, n, shift):
    from mere_fusion_amd.avatar.prepare import landmark_boxes_device
    H, W = 480, 640
    kp, boxes, counts = landmark_cases(n, np.random.default_rng(n), H, W)
    det = [R.detector_box(b[0], W, H) if c > 0 else None for b, c in zip(boxes, counts)]
    want, flags, sums = R.landmark_boxes(kp.copy(), det, shift)
    coords, fl, sm = landmark_boxes_device(torch.from_numpy(kp).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), H, W, shift)
    assert fl.cpu().tolist() == flags
    assert [tuple(r) for r in coords.cpu().tolist()] == [tuple(int(v) for v in c) for c in want]
    assert tuple(sm.cpu().tolist()) == sums
    if n >= 6:
        assert set(flags) == {0, 1, 2}
