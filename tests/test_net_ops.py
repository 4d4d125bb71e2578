"""The static-graph executor of avatar preparation (csrc/mf_net.hip, and mf_aux.hip's k_nchw_to_act / k_act_to_nchw behind set_input and
get_output), one op at a time against the same operation in torch float64 on the CPU.

Every GPU case builds a tiny Net graph (input buffer, the op, output buffer) and runs in both storage formats: bf16x3 (hi + lo planes) and
bf16 (no lo plane, so Pl::ld / Pl::st take their other branch).

- Exact ops (max-pool, nearest upsample, the S3FD max-out, the set_input -> get_output round trip) are compared bit for bit, on inputs the
  storage format holds exactly (`exact`; test_exact_inputs_survive_storage checks that claim on the CPU).
- Arithmetic ops are held to a bound in units of the format's relative rounding U[prec]; each test's docstring derives its bound.
- Output buffers are pre-filled with SENT through set_input, so a write outside the op's channel slice (or into the padding channels that
  mf_net_buffer adds to reach a multiple of 8) shows up.  Input buffers carry BIG in the channels beside the slice, so a read outside it shows up.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conv_numerics import F32, U, bf16_rne, bn_fold, exact, stored  # noqa: F401

PRECS = ["bf16x3", "bf16"]
SENT = -8192.0                        # pre-fill of output buffers (exact in both formats)
BIG = 2.0 ** 20                       # neighbours of an input slice (exact in both formats)


def pad8(c):
    return (c + 7) // 8 * 8


# ---- storage-format emulation (CPU): U, F32, bf16_rne, stored, exact, bn_fold live in conv_numerics.py, shared with test_conv_configs.py --------------
def test_exact_inputs_survive_storage():
    rng = np.random.default_rng(0)
    for prec in PRECS:
        for scale, offset in ((1.0, 0.0), (1e-12, 0.0), (1.0, 1e3), (1e3, -5.0), (3e-11, 0.0)):
            x = exact(rng, (4096,), prec, scale, offset)
            assert x.dtype == np.float32
            assert np.array_equal(stored(x, prec).view(np.uint32), x.view(np.uint32)), (prec, scale, offset)
            if prec == "bf16":
                assert np.all(x.view(np.uint32) & 0xFFFF == 0)
        # near the binade edges, where the bf16 spacing halves below a power of two
        edge = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
        x = np.concatenate([edge * (1 + s * np.float32(2.0 ** -e)) for s in (-1, 1) for e in range(7, 20)]).astype(np.float32)
        x = stored(x, prec)
        assert np.array_equal(stored(x, prec).view(np.uint32), x.view(np.uint32)), prec
    for v in (SENT, BIG, -BIG):
        assert bf16_rne(np.float32(v)) == v


def test_stored_matches_the_format_rounding():
    """the emulation itself: bf16 is torch's bf16 rounding, and U bounds (and nearly reaches) each format's relative rounding"""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(1 << 16) * np.exp(rng.uniform(-20, 20, 1 << 16))).astype(np.float32)
    assert np.array_equal(stored(x, "bf16"), torch.from_numpy(x).bfloat16().float().numpy())
    rel = np.abs(stored(x, "bf16x3").astype(np.float64) - x) / np.abs(x)
    assert rel.max() <= U["bf16x3"] and rel.max() > U["bf16x3"] / 8
    rel = np.abs(stored(x, "bf16").astype(np.float64) - x) / np.abs(x)
    assert rel.max() <= U["bf16"] and rel.max() > U["bf16"] / 2


# ---- float64 references (CPU) -----------------------------------------------------------------------------------------------------------
def l2norm_ref(x, w, eps):
    """net_s3fd.py:15-19 (oracle/s3fd_ref.py:_l2norm) in float64"""
    x = torch.as_tensor(x, dtype=torch.float64)
    norm = x.pow(2).sum(dim=1, keepdim=True).sqrt() + eps
    return x / norm * torch.as_tensor(w, dtype=torch.float64).view(1, -1, 1, 1)


def test_l2norm_ref_is_the_oracle():
    from oracle import s3fd_ref
    rng = np.random.default_rng(2)
    x, w = rng.standard_normal((2, 7, 3, 4)), rng.uniform(1, 10, 7)
    want = s3fd_ref._l2norm(torch.from_numpy(x), torch.from_numpy(w))
    assert torch.allclose(l2norm_ref(x, w, 1e-10), want, rtol=1e-15, atol=0)


def test_bn_fold_is_conv_then_batchnorm():
    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((1, 3, 6, 5)), rng.standard_normal((4, 3, 3, 3)), rng.standard_normal(4)
    g, be, m, v = rng.uniform(0.5, 2, 4), rng.standard_normal(4), rng.standard_normal(4), rng.uniform(0.5, 2, 4)
    t = lambda a: torch.from_numpy(a)
    want = F.batch_norm(F.conv2d(t(x), t(w), t(b), padding=1), t(m), t(v), t(g), t(be), training=False, eps=1e-5)
    wf, bf = bn_fold(w, b, g, be, m, v)
    assert torch.allclose(F.conv2d(t(x), t(wf), t(bf), padding=1), want, rtol=1e-12, atol=1e-12)


# ---- device helpers ----------------------------------------------------------------------------------------------------------------------
def _net(prec, max_batch=2):
    from mere_fusion_amd.avatar.net import Net
    return Net(max_batch, prec)


def _set(n, buf, x):
    n.set_input(buf, torch.from_numpy(np.ascontiguousarray(x, np.float32)))


def _get(n, buf, batch, coff=0, Cn=None):
    """channels [coff, coff + Cn) of a buffer (default: to the end of its padded width) as float32 NCHW"""
    if Cn is None:
        Cn = pad8(n.shape[buf][0]) - coff
    return n.output(buf, Cn, batch, coff).cpu().numpy()


def _sentinel(n, buf, batch):
    Cn, H, W = n.shape[buf]
    _set(n, buf, np.full((batch, pad8(Cn), H, W), SENT, np.float32))


def _assert_untouched(got, keep, what):
    """got: the full padded width of an output buffer; keep: channel mask of what the op may write"""
    rest = got[:, ~keep]
    assert np.all(rest == SENT), f"{what}: {int((rest != SENT).sum())} values written outside the op's channels"


def _with_neighbours(x, coff, width):
    """x [B, C, H, W] placed at channel coff of a [B, width, H, W] tensor whose other channels hold BIG (alternating sign by channel)"""
    B, Cn, H, W = x.shape
    full = np.empty((B, width, H, W), np.float32)
    full[:] = (BIG * np.where(np.arange(width) % 2 == 0, 1.0, -1.0)).reshape(1, width, 1, 1)
    full[:, coff:coff + Cn] = x
    return full


# ---- exact ops: bit for bit ------------------------------------------------------------------------------------------------------------
POOL_WINDOWS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (1, 1, 0)]
POOL_MAPS = [(1, 1), (2, 3), (101, 135), (7, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("win,hw", [(w, m) for w in POOL_WINDOWS for m in POOL_MAPS if m[0] + 2 * w[2] >= w[0] and m[1] + 2 * w[2] >= w[0]],
                         ids=lambda v: "k{}s{}p{}".format(*v) if len(v) == 3 else f"{v[0]}x{v[1]}")
def test_maxpool_bit_exact(lib_built, prec, win, hw):
    """F.max_pool2d: batch item 0 holds signed values, item 1 only negative ones (a tap outside the map must not count as 0).
    (A 2 x 2 window on a 1 x 1 map has no F.max_pool2d output: test_maxpool_refusals checks that the ABI refuses it.)"""
    (k, s, p), (H, W) = win, hw
    rng = np.random.default_rng(H * 1000 + W + 7 * k + s)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    for Cn in (3, 8, 13, 64, 72):
        x = np.concatenate([exact(rng, (1, Cn, H, W), prec), -stored(np.abs(exact(rng, (1, Cn, H, W), prec)) + np.float32(0.25), prec)])
        n = _net(prec)
        ib, ob = n.buffer(Cn, H, W, 1), n.buffer(Cn, Ho, Wo, 1)
        n.maxpool(ib, ob, k, s, p)
        _set(n, ib, x)
        n.run(2)
        got = _get(n, ob, 2, 0, Cn)
        want = F.max_pool2d(torch.from_numpy(x).double(), k, s, p).float().numpy()
        assert got.shape == want.shape
        bad = got != want
        assert not bad.any(), f"C={Cn}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"


UPSAMPLE_CASES = [((8, 6), (16, 12)), ((5, 3), (20, 12)), ((5, 7), (7, 5)), ((7, 3), (5, 16)), ((1, 3), (9, 16)), ((3, 1), (16, 9))]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("src,dst", UPSAMPLE_CASES, ids=lambda m: f"{m[0]}x{m[1]}")
def test_upsample_nearest_bit_exact(lib_built, prec, src, dst):
    """F.interpolate(mode='nearest'): x2, x4 and non-integer ratios (5 -> 7, 7 -> 5, 3 -> 16, 1 -> 9) on either axis"""
    rng = np.random.default_rng(src[0] * 100 + dst[1])
    for Cn in (3, 13):
        x = exact(rng, (2, Cn, *src), prec)
        n = _net(prec)
        ib, ob = n.buffer(Cn, *src, 1), n.buffer(Cn, *dst, 1)
        n.upsample_nearest(ib, ob)
        _set(n, ib, x)
        n.run(2)
        got = _get(n, ob, 2)                                                    # the padding channels too: zeros in, zeros out
        want = np.zeros_like(got)
        want[:, :Cn] = F.interpolate(torch.from_numpy(x).double(), size=dst, mode="nearest").float().numpy()
        bad = got != want
        assert not bad.any(), f"C={Cn}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [1, 7, 255, 256, 257, 1000, 65 * 67])
def test_s3fd_maxout_bg_bit_exact(lib_built, hw):
    """net_s3fd.py:123-126 on fp32 NCHW maps (no storage format is involved, so one precision): [B, 4, hw] -> (max(c0, c1, c2), c3)"""
    from mere_fusion_amd import _lib
    _lib.init_device(torch.cuda.current_device())
    B = 3
    g = torch.Generator().manual_seed(hw)
    cls4 = torch.randn((B, 4, hw), generator=g)
    cls4[0, 2] = cls4[0, 0] + 1                                                  # the max in every channel position
    cls4[1, 0] = cls4[1, 1].abs() + 1
    src = cls4.cuda()
    dst = torch.full((B, 2, hw), float("nan"), device="cuda")
    _lib.check(_lib.lib().mf_s3fd_maxout_bg(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), B, hw,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "s3fd_maxout_bg")
    ch = torch.chunk(cls4.double(), 4, 1)
    want = torch.cat([torch.max(torch.max(ch[0], ch[1]), ch[2]), ch[3]], 1).float()
    assert torch.equal(dst.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("Cn", [1, 3, 5, 8, 19])
def test_set_input_get_output_round_trip(lib_built, prec, halo, Cn):
    """set_input stores each value as the format's rounding of it (`stored`, bit for bit, for any fp32 input) and zero-fills the padding
    channels; get_output reads back any channel slice"""
    rng = np.random.default_rng(Cn * 10 + halo)
    B, H, W = 2, 6, 11
    x = (rng.standard_normal((B, Cn, H, W)) * np.exp(rng.uniform(-8, 8, (B, Cn, H, W)))).astype(np.float32)
    x.flat[:4] = [0.0, -0.0, 3.0e38, -1.0e-37]
    n = _net(prec, max_batch=3)
    b = n.buffer(Cn, H, W, halo)
    _set(n, b, x)
    got = _get(n, b, B)
    want = np.zeros((B, pad8(Cn), H, W), np.float32)
    want[:, :Cn] = stored(x, prec)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # an exactly representable input survives unchanged
    xe = exact(rng, (B, Cn, H, W), prec)
    _set(n, b, xe)
    assert np.array_equal(_get(n, b, B, 0, Cn), xe)
    # channel slices inside the wider buffer
    for coff, w in ((1, Cn - 1), (Cn // 2, Cn - Cn // 2), (Cn - 1, pad8(Cn) - Cn + 1)):
        if w >= 1:
            want_s = np.zeros((B, pad8(Cn), H, W), np.float32)
            want_s[:, :Cn] = xe
            assert np.array_equal(_get(n, b, B, coff, w), want_s[:, coff:coff + w]), (coff, w)
    assert np.array_equal(_get(n, b, 1, 0, Cn), xe[:1])                         # a batch below what was set


# ---- arithmetic ops: bounds from the storage format -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cn", [3, 64, 512, 515])
def test_l2norm(lib_built, prec, Cn):
    """k_l2norm, y_c = x_c / (sqrt(sum_c x_c^2) + eps) * w_c, on exact inputs.

    Bound, per element: every step is a product, a quotient or a sum of non-negative terms, so the fp32 error is relative to y_c itself.
    The sum of squares takes ceil(C/64) lane additions and a 6-step butterfly: (ceil(C/64) + 7) F32; sqrt halves that, then + eps,
    reciprocal and two products add one F32 each.  For C = 515: < 16 F32 = U/8 (bf16x3).  Storing y_c adds at most U |y_c|.
    So |got - want| <= (U + (ceil(C/64) + 12) F32) |want| <= 2 U |want|.
    Pixels: signed normals; a norm near eps (eps decides half of the result); a norm far below eps; all zero; one dominant channel."""
    rng = np.random.default_rng(Cn)
    B, H, W = 2, 5, 7
    eps = float(np.float32(1e-10))                                                 # the ABI takes eps as a float
    x = exact(rng, (B, Cn, H, W), prec)
    x[0, :, 0, 0] = exact(rng, Cn, prec, scale=1e-10 / np.sqrt(Cn))
    x[0, :, 0, 1] = exact(rng, Cn, prec, scale=1e-13)
    x[0, :, 0, 2] = 0
    x[1, :, 1, 1] = exact(rng, Cn, prec, scale=1e-2)
    x[1, 0, 1, 1] = 1e3
    w = rng.uniform(0.5, 20, Cn).astype(np.float32)
    n = _net(prec)
    ib, ob = n.buffer(Cn, H, W, 1), n.buffer(Cn, H, W, 1)
    n.l2norm(ib, ob, torch.from_numpy(w), eps)
    _set(n, ib, x)
    _sentinel(n, ob, B)
    n.run(B)
    got = _get(n, ob, B)
    keep = np.arange(pad8(Cn)) < Cn
    _assert_untouched(got, keep, "l2norm")
    want = l2norm_ref(x, w, eps).numpy()
    err = np.abs(got[:, :Cn] - want)
    rel = err / np.maximum(np.abs(want), 1e-300)
    print(f"[l2norm {prec} C={Cn}] max |err| / |want| = {rel.max():.3e} = {rel.max() / U[prec]:.3f} U")
    assert np.all(err <= 2 * U[prec] * np.abs(want)), f"worst {rel.max() / U[prec]:.2f} U at {np.unravel_index(rel.argmax(), rel.shape)}"
    assert np.all(got[0, :Cn, 0, 2] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (17, 13), (64, 64)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_global_avgpool(lib_built, prec, hw):
    """k_gap, the mean over H x W of channels [in_coff, in_coff + C), on exact inputs of mean 1e3 and spread 1.

    Bound: each of the 4 partial sums adds m = ceil(HW / 4) positive terms in fp32, the partials are added (3) and divided (1): the
    computed mean is within (m + 4) F32 * mean|x| of the exact one (first order, recursive summation).  Storing it adds U |mean|.
    So |got - want| <= 2 U |want| + (m + 4) F32 mean|x|.  At 64 x 64 the second term is 1028 F32 ~ 8 U (bf16x3) of the mean; a sum that
    loses precision (a bf16 running sum: its spacing reaches 2^-8 of the sum) exceeds it by far."""
    H, W = hw
    rng = np.random.default_rng(H * 100 + W)
    B = 2
    m = -(-H * W // 4)
    for Cn, coff in itertools.product((1, 63, 64, 65, 512), (0, 5)):
        x = exact(rng, (B, Cn, H, W), prec, scale=1.0, offset=1e3)
        width = coff + Cn + 3
        n = _net(prec)
        ib, ob = n.buffer(width, H, W, 1), n.buffer(Cn, 1, 1, 0)
        n.global_avgpool(ib, Cn, ob, in_coff=coff)
        _set(n, ib, _with_neighbours(x, coff, width))
        _sentinel(n, ob, B)
        n.run(B)
        got = _get(n, ob, B)
        _assert_untouched(got, np.arange(pad8(Cn)) < Cn, f"global_avgpool C={Cn} coff={coff}")
        want = torch.from_numpy(x).double().mean(dim=(2, 3), keepdim=True).numpy()
        err = np.abs(got[:, :Cn] - want)
        bound = 2 * U[prec] * np.abs(want) + (m + 4) * F32 * np.abs(x).astype(np.float64).mean(axis=(2, 3), keepdims=True)
        print(f"[global_avgpool {prec} {H}x{W} C={Cn} coff={coff}] max |err| {err.max():.3e} = {err.max() / (U[prec] * np.abs(want).max()):.3f} U|mean|,"
              f" bound {bound.min():.3e}")
        assert np.all(err <= bound), f"C={Cn} coff={coff}: worst err {err.max():.3e}, bound {bound.min():.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cn", [13, 128])
@pytest.mark.parametrize("st", [(s, t, v, same) for s, t, v in itertools.product((0, 1), repeat=3) for same in ((0, 1) if t else (0,))],
                         ids=lambda c: "s{}t{}v{}".format(*c[:3]) + ("_t_is_x" if c[3] else ""))
def test_scale_add(lib_built, prec, Cn, st):
    """k_scale_add, out[:, out_coff + c] = x[:, x_coff + c] * s[b, c] + t[:, t_coff + c] + v[b, c], every operand present or absent;
    t_is_x: t is x's own slice (feat * atten + feat, bisenet.py:125).

    Bound: at most 3 fp32 roundings (fewer where the compiler fuses), each within F32 of A = |x s| + |t| + |v|, and the store rounds to
    U |y|: |got - want| <= 2 U |want| + 4 F32 A."""
    has_s, has_t, has_v, t_is_x = st
    rng = np.random.default_rng(Cn + 16 * has_s + 8 * has_t + 4 * has_v + 2 * t_is_x)
    B, H, W = 2, 5, 7
    x_coff, t_coff, out_coff = 3, 6, 5
    x = exact(rng, (B, Cn, H, W), prec)
    s = exact(rng, (B, Cn, 1, 1), prec)
    v = exact(rng, (B, Cn, 1, 1), prec)
    n = _net(prec)
    xb = n.buffer(x_coff + Cn + 4, H, W, 1)
    ob = n.buffer(out_coff + Cn + 3, H, W, 1)
    sb = n.buffer(Cn, 1, 1, 0) if has_s else -1
    vb = n.buffer(Cn, 1, 1, 0) if has_v else -1
    if has_t and t_is_x:
        tb, tc, t = xb, x_coff, x
    elif has_t:
        t = exact(rng, (B, Cn, H, W), prec)
        tb, tc = n.buffer(t_coff + Cn + 2, H, W, 1), t_coff
        _set(n, tb, _with_neighbours(t, t_coff, t_coff + Cn + 2))
    else:
        tb, tc, t = -1, t_coff, None
    n.scale_add(xb, Cn, ob, s_buf=sb, t_buf=tb, v_buf=vb, x_coff=x_coff, t_coff=tc, out_coff=out_coff)
    _set(n, xb, _with_neighbours(x, x_coff, x_coff + Cn + 4))
    if has_s:
        _set(n, sb, s)
    if has_v:
        _set(n, vb, v)
    _sentinel(n, ob, B)
    n.run(B)
    got = _get(n, ob, B)
    keep = (np.arange(pad8(out_coff + Cn + 3)) >= out_coff) & (np.arange(pad8(out_coff + Cn + 3)) < out_coff + Cn)
    _assert_untouched(got, keep, "scale_add")
    x64 = x.astype(np.float64)
    want = x64 * s if has_s else x64.copy()
    A = np.abs(want)
    if has_t:
        want = want + t
        A = A + np.abs(t)
    if has_v:
        want = want + v
        A = A + np.abs(v)
    err = np.abs(got[:, out_coff:out_coff + Cn] - want)
    bound = 2 * U[prec] * np.abs(want) + 4 * F32 * A
    print(f"[scale_add {prec} C={Cn} {st}] max |err| {err.max():.3e} = {(err / np.maximum(A, 1e-30)).max() / U[prec]:.3f} U A")
    assert np.all(err <= bound), f"worst err {err.max():.3e} at {np.unravel_index(np.argmax(err - bound), err.shape)}"


BILINEAR_CASES = [((5, 7), (13, 22)), ((17, 13), (6, 5)), ((9, 11), (9, 11)), ((7, 9), (1, 12)), ((7, 9), (10, 1)), ((7, 9), (1, 1)),
                  ((1, 1), (4, 5)), ((2, 33), (3, 64))]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("coff,Cn", [(0, 19), (3, 5)])
@pytest.mark.parametrize("src,dst", BILINEAR_CASES, ids=lambda m: f"{m[0]}x{m[1]}")
def test_output_bilinear(lib_built, prec, coff, Cn, src, dst):
    """get_output_bilinear (k_bilinear_ac) = F.interpolate(mode='bilinear', align_corners=True) of channels [coff, coff + C), fp32 out.

    The inputs are exact and the output is fp32, so no storage rounding enters: the bound is in fp32 units.  The source coordinate
    fl(fl((h - 1) / (H - 1)) * y) is within 2 F32 (h - 1) of the exact one, which moves a lambda by as much and the result by that
    times |v1 - v0| <= 2 M (M = max |x|); per axis 4 (h - 1) F32 M.  The blend itself: at most 8 F32 M.
    So |got - want| <= (8 + 4 (h - 1) + 4 (w - 1)) F32 M (here <= 1.4 U M for bf16x3).  The identity size is exact."""
    (h, w), (H, W) = src, dst
    rng = np.random.default_rng(h * 1000 + w * 10 + H + coff)
    B = 2
    x = exact(rng, (B, Cn, h, w), prec)
    width = coff + Cn + 3
    n = _net(prec)
    ib = n.buffer(width, h, w, 1)
    _set(n, ib, _with_neighbours(x, coff, width))
    got = n.output_bilinear(ib, Cn, B, H, W, coff=coff).cpu().numpy()
    want = F.interpolate(torch.from_numpy(x).double(), size=(H, W), mode="bilinear", align_corners=True).numpy()
    err = np.abs(got - want)
    M = np.abs(x).max()
    bound = (8 + 4 * (h - 1) + 4 * (w - 1)) * F32 * M
    print(f"[output_bilinear {prec} {src}->{dst} coff={coff}] max |err| {err.max():.3e} = {err.max() / (U[prec] * M):.4f} U M, bound {bound:.3e}")
    assert err.max() <= bound, f"worst err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    if (h, w) == (H, W):
        assert np.array_equal(got, x)


# (cin, cout, k, stride, pad, H, W, act, bn, residual, in_coff, out_coff, res_coff): cin 3 / 5 on 20 x 20 maps take the thin kernel, the
# small maps the implicit GEMM (cout 13 there: a split-K candidate), cin 5 stride 2 on 36 x 34 the thin kernel's stride-2 form, 20 -> 24 at
# 16 x 16 the halo tile; every input slice width is off a multiple of 8
CONV_CASES = [
    (3, 8, 3, 1, 1, 20, 20, 1, True, False, 8, 4, 0),
    (5, 12, 3, 2, 1, 36, 34, 2, True, False, 0, 4, 0),
    (5, 13, 3, 1, 1, 9, 11, 0, False, True, 8, 8, 4),
    (13, 6, 1, 1, 0, 7, 5, 1, True, True, 0, 4, 12),
    (3, 13, 7, 2, 3, 23, 19, 1, True, False, 16, 0, 0),
    (20, 24, 3, 1, 1, 16, 16, 1, True, True, 8, 8, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "cin{}_cout{}_k{}s{}p{}_{}x{}_act{}".format(*c[:8]) + ("_bn" if c[8] else "") + ("_res" if c[9] else ""))
def test_conv(lib_built, prec, case):
    """Net.conv: nn.Conv2d [+ BatchNorm folded] [+ residual] + act on channel slices.  The input slice sits among BIG neighbours: the
    executor widens an input view to the padded width where the buffer has room, and those channels must meet zero weights.

    Bound: inputs are exact; each folded weight is stored within U (hi + lo, or bf16); a bf16x3 product drops lo_w lo_x (<= 2^-18 |w x|);
    the K = cin k^2 products are summed in fp32 (<= (K + 4) F32 of A = conv(|x|, |w'|) + |b'| + |res|, first order); ReLU and sigmoid are
    1-Lipschitz (the latter's expf adds a few F32); the store rounds to U |y|.  |got - want| <= (2 U + (K + 8) F32) A + 2 U |want|.
    The epilogue stores channel quads (mf_conv.hip): channels beyond out_coff + round_up(cout, 4) keep their sentinel."""
    cin, cout, k, st, pad, H, W, act, bn, res, in_coff, out_coff, res_coff = case
    rng = np.random.default_rng(cin * 100 + cout + k)
    B = 2
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    x = exact(rng, (B, cin, H, W), prec)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    bnp = (rng.uniform(0.5, 2, cout), rng.standard_normal(cout) * 0.5, rng.standard_normal(cout) * 0.5, rng.uniform(0.5, 2, cout)) if bn else None
    bnp = tuple(a.astype(np.float32) for a in bnp) if bn else None
    r = exact(rng, (B, cout, Ho, Wo), prec) if res else None
    n = _net(prec)
    in_w, out_w, res_w = in_coff + cin + 3, out_coff + cout + 5, res_coff + cout + 3
    ib = n.buffer(in_w, H, W, pad)
    ob = n.buffer(out_w, Ho, Wo, 1)
    rb = n.buffer(res_w, Ho, Wo, 1) if res else -1
    n.conv(torch.from_numpy(w), ib, ob, st, pad, act=act, bias=torch.from_numpy(b), bn=tuple(torch.from_numpy(a) for a in bnp) if bn else None,
           in_coff=in_coff, out_coff=out_coff, res_buf=rb, res_coff=res_coff)
    _set(n, ib, _with_neighbours(x, in_coff, in_w))
    if res:
        _set(n, rb, _with_neighbours(r, res_coff, res_w))
    _sentinel(n, ob, B)
    n.run(B)
    got = _get(n, ob, B)
    ch = np.arange(pad8(out_w))
    _assert_untouched(got, (ch >= out_coff) & (ch < out_coff + (cout + 3) // 4 * 4), "conv")
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    if bn:
        w64, b64 = bn_fold(w64, b64, *(a.astype(np.float64) for a in bnp))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    pre = F.conv2d(t(x), t(w64), t(b64), stride=st, padding=pad)
    A = F.conv2d(t(np.abs(x)), t(np.abs(w64)), t(np.abs(b64)), stride=st, padding=pad)
    if res:
        pre, A = pre + t(r), A + t(np.abs(r))
    want = (pre if act == 0 else torch.relu(pre) if act == 1 else torch.sigmoid(pre)).numpy()
    A = A.numpy()
    K = cin * k * k
    err = np.abs(got[:, out_coff:out_coff + cout] - want)
    bound = (2 * U[prec] + (K + 8) * F32) * A + 2 * U[prec] * np.abs(want)
    print(f"[conv {prec} {case}] max |err| {err.max():.3e} = {(err / A).max() / U[prec]:.3f} U A")
    assert np.all(err <= bound), f"worst err {err.max():.3e} (bound there {bound.flat[np.argmax(err - bound)]:.3e})"


# ---- graph and batch behaviour ----------------------------------------------------------------------------------------------------------
def _pipeline(prec, max_batch):
    """input -> conv 3x3 (BN, ReLU) -> maxpool 3/2/1 -> conv 1x1 (sigmoid) -> gap -> x * gap + x -> nearest x2 -> l2norm"""
    rng = np.random.default_rng(11)
    n = _net(prec, max_batch)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    inp = n.buffer(3, 20, 20, 1)
    c1 = n.buffer(16, 20, 20, 1)
    n.conv(t(rng.standard_normal((16, 3, 3, 3)) / 5), inp, c1, 1, 1, act=1,
           bn=(t(rng.uniform(0.5, 2, 16)), t(rng.standard_normal(16)), t(rng.standard_normal(16)), t(rng.uniform(0.5, 2, 16))))
    p = n.buffer(16, 10, 10, 0)
    n.maxpool(c1, p, 3, 2, 1)
    c2 = n.buffer(13, 10, 10, 1)
    n.conv(t(rng.standard_normal((13, 16, 1, 1)) / 4), p, c2, 1, 0, act=2, bias=t(rng.standard_normal(13)))
    g = n.buffer(13, 1, 1, 0)
    n.global_avgpool(c2, 13, g)
    sa = n.buffer(13, 10, 10, 1)
    n.scale_add(c2, 13, sa, s_buf=g, t_buf=c2)
    up = n.buffer(13, 20, 20, 1)
    n.upsample_nearest(sa, up)
    ln = n.buffer(13, 20, 20, 1)
    n.l2norm(up, ln, t(rng.uniform(1, 10, 13)))

    def run(x):
        B = n.set_input(inp, torch.from_numpy(x))
        n.run(B)
        return [n.output(ln, 13, B).cpu(), n.output_bilinear(sa, 13, B, 7, 9).cpu(), n.output(c2, 13, B).cpu()]
    return run


def _items(prec, monkeypatch, no_graph):
    if no_graph:
        monkeypatch.setenv("MF_NO_GRAPH", "1")                                    # read per handle, by mf_net_create
    else:
        monkeypatch.delenv("MF_NO_GRAPH", raising=False)
    x = np.random.default_rng(12).uniform(-3, 3, (4, 3, 20, 20)).astype(np.float32)
    run = _pipeline(prec, 4)
    seq = [run(x[[0, 1, 2]]), run(x[[3]]), run(x), run(x[[0, 1, 2]]), run(x[[2, 0, 1]])]
    alone = _pipeline(prec, 1)
    single = [alone(x[[i]]) for i in range(4)]
    return seq, single


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_batches_graph_replay_and_no_graph(lib_built, prec, monkeypatch):
    """one handle (max_batch 4) at batches 3, 1, 4, 3, 3 (eager at each first batch size, then the captured graph): every item bit-identical
    to itself run alone on a max_batch-1 handle, the replay identical to the eager run; MF_NO_GRAPH=1 gives the same bits"""
    seq, single = _items(prec, monkeypatch, False)
    order = [[0, 1, 2], [3], [0, 1, 2, 3], [0, 1, 2], [2, 0, 1]]
    for step, (outs, items) in enumerate(zip(seq, order)):
        for j, i in enumerate(items):
            for o, (got, want) in enumerate(zip(outs, single[i])):
                assert torch.equal(got[j], want[0]), f"step {step} (batch {len(items)}), item {i}, output {o}"
    for a, b in zip(seq[0], seq[3]):
        assert torch.equal(a, b)
    nseq, nsingle = _items(prec, monkeypatch, True)
    for outs, nouts in zip(seq + single, nseq + nsingle):
        for a, b in zip(outs, nouts):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_maxpool_refusals(lib_built):
    n = _net("bf16x3")
    a, b = n.buffer(8, 10, 10, 1), n.buffer(8, 5, 5, 1)
    with pytest.raises(RuntimeError, match="net_maxpool: bad window"):
        n.maxpool(a, b, 2, 2, 2)                                                  # pad > k / 2
    with pytest.raises(RuntimeError, match="net_maxpool: bad window"):
        n.maxpool(a, b, 0, 2, 0)
    one, one_out = n.buffer(8, 1, 1, 1), n.buffer(8, 1, 1, 1)
    with pytest.raises(RuntimeError, match="net_maxpool: bad window"):
        n.maxpool(one, one_out, 2, 2, 0)                                          # F.max_pool2d: output size 0
    with pytest.raises(RuntimeError, match="net_maxpool: output buffer 8x6x5 does not match"):
        n.maxpool(a, n.buffer(8, 6, 5, 1), 2, 2, 0)
    with pytest.raises(RuntimeError, match="does not match"):
        n.maxpool(a, n.buffer(16, 5, 5, 1), 2, 2, 0)
    n.maxpool(a, b, 2, 2, 0)                                                      # the matching one is accepted, and only it was appended
    from mere_fusion_amd import _lib
    assert _lib.lib().mf_net_num_ops(n._h) == 1


@pytest.mark.gpu
def test_get_output_refuses_slices_outside_the_buffer(lib_built):
    n = _net("bf16")
    b = n.buffer(5, 4, 4, 1)                                                      # 8 channels once padded
    _set(n, b, np.ones((1, 5, 4, 4), np.float32))
    for coff, Cn in ((5, 4), (0, 9), (-1, 2), (8, 1)):
        with pytest.raises(RuntimeError, match=r"net_get_output: channel slice \[-?\d+, \d+\) outside the buffer \(8\)"):
            n.output(b, Cn, 1, coff)
    assert np.array_equal(_get(n, b, 1, 4, 4)[0, 0], np.ones((4, 4), np.float32))
