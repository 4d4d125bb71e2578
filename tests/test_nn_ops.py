"""The token-sequence ops of mf_nn.hip (plane conversions, LayerNorm, row softmax, GroupNorm, device-packed GEMM, the uint8 tail) and the five-launch
composite attention, one at a time against float64, through the C-ABI test seams of mf_nn_api.hip.

References and bounds: tests/nn_numerics.py.  Every reference is evaluated on the values the (hi, lo) planes hold, so the input conversion is charged
once, to the bit-exact round-trip test.  Every case that takes the whole padded output buffer back asserts that all of it outside the written view is
still the poison the seam filled it with, bit for bit: halo ring, channels beside the view, tokens past a prefix.

The constants K_* scale the fp32-arithmetic term of each bound (nn_numerics.*_terms): 3 x the worst value the first MI355X run needed (printed per case
as `K needed`), recorded beside each constant."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_numerics as N
from conv_numerics import F32

PRECS = ["bf16x3", "bf16"]
# Worst `K needed` of the first MI355X run, per op, bf16x3 / bf16 (in bf16 most of the error sits inside the representation term):
#   LayerNorm   2.21 / 0.71  (C 320 at coff 4: the scalar kernel; the vector kernels 2.20 at C 512, 2.11 at C 1280; worst L-inf 7.5e-5 on the 1e4-outlier token)
#   GroupNorm   3.66 / 1.54  (k_gn_apply<4>, C 320 82 x 160 batch 2; 3.53 at C 4096 32 x 64; k_gn_apply<1> at most 3.13)
#   softmax     0.00 / 0.00  (every error inside the representation term; K_SM = 1 keeps the term's form and no more)
#   composite attention against attention_unit: 0.047 / 0.088 on randn rows, 0.039 / 0.081 on the temperature sweep (worst at temperature 64);
#   uniform rows at most 7.9e-7 of max|v| (bf16x3), one-hot rows inside REPR
K_LN = 7.0
K_SM = 1.0
K_GN = 11.0
K_ATT = 0.27


# ---- CPU: the references are the functions torch.nn.functional defines ------------------------------------------------------------------------------
def test_split_is_the_bfloat16_cast():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * 10 ** torch.randint(-20, 20, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1e-30, 3e38, -3e38])])
    hi, lo = N.split(x.numpy(), "bf16x3")
    want_hi = x.bfloat16().float()
    assert np.array_equal(hi.view(np.uint32), want_hi.numpy().view(np.uint32))
    assert np.array_equal(lo.view(np.uint32), (x - want_hi).bfloat16().float().numpy().view(np.uint32))
    assert N.split(x.numpy(), "bf16")[1] is None
    back = N.join(hi, lo)
    assert np.all(np.abs(back.astype(np.float64) - x.double().numpy()) <= 2.0 ** -16 * np.abs(x.double().numpy()))
    assert np.array_equal(N.stored(back, "bf16x3").view(np.uint32), back.view(np.uint32))          # a stored value splits into itself
    assert N.join(*N.split(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]), "bf16")).tolist() == [1.0, 1.015625]   # ties go to the even neighbour


def test_references_are_torch_functional():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(3, 11, 40, generator=g) * 3 + 1.5).double()
    ga, be = torch.randn(40, generator=g).double(), torch.randn(40, generator=g).double()
    y, pre, sigma = N.layernorm64(x, ga, be, 1e-5, 0)
    assert (y - F.layer_norm(x, (40,), ga, be, 1e-5)).abs().max() < 1e-12
    assert (N.layernorm64(x, ga, be, 1e-5, 3)[0] - F.gelu(F.layer_norm(x, (40,), ga, be, 1e-5))).abs().max() < 1e-12
    p, z = N.softmax64(x, 0.125, 33)
    assert (p - F.softmax(x[..., :33] * 0.125, -1)).abs().max() < 1e-14
    nchw = x.permute(0, 2, 1).reshape(3, 40, 11, 1)
    for groups in (1, 4, 40):
        want = F.group_norm(nchw, groups, ga, be, 1e-6)
        for silu in (False, True):
            y, pre, R, sc, sh = N.groupnorm64(x, ga, be, groups, 1e-6, silu)
            w = F.silu(want) if silu else want
            assert (y - w.reshape(3, 40, 11).permute(0, 2, 1)).abs().max() < 1e-10
            assert (x * sc[:, None] + sh[:, None] - pre).abs().max() < 1e-10
    a, b = x[0], x[1][:7]
    assert (N.gemm_bt64(a, b) - F.linear(a, b)).abs().max() < 1e-12
    q, k, v = N._qkv(2, 5, 7, 2, 8, 0)
    want = F.scaled_dot_product_attention(*(t.double().view(2, -1, 2, 8).transpose(1, 2) for t in (q, k, v))).transpose(1, 2).reshape(2, 5, 16)
    assert (N.attention64(q, k, v, 2)[0] - want).abs().max() < 1e-12


def _u8_inputs(prec, n):
    """RGB values in the storage format: out of range, the ends, the centre of every level, values beside every level boundary (at +-1 and +-2 steps of
    2^-15 relative), 3000 uniform draws, and every exact tie fl(fl(x / 2 + .5) * 255) == k + .5 the format can express near a boundary -- tiled to n values"""
    k = np.arange(256, dtype=np.float64)
    edge = 2 * (k[:255] + 0.5) / 255 - 1
    vals = [np.float64([-3.0, -1.5, -1.0, 0.0, 1.0, 1.25, 7.0]), 2 * k / 255 - 1] + [edge * (1 + j * 2.0 ** -15) for j in (-2, -1, 1, 2)]
    vals.append(np.random.default_rng(0).uniform(-1.1, 1.1, 3000))                 # ordinary pixels
    x = N.stored(np.concatenate(vals).astype(np.float32), prec)
    if prec == "bf16x3":
        hi = N.bf16_rne(edge.astype(np.float32))
        lo0 = N.bf16_rne(edge.astype(np.float32) - hi).view(np.uint32) >> 16
        cand = []
        for j in range(-96, 97):
            lo = ((lo0.astype(np.int64) + j) & 0xFFFF).astype(np.uint32) << 16
            with np.errstate(invalid="ignore", over="ignore"):
                cand.append(N.stored(hi + lo.view(np.float32), prec))
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.concatenate(cand)
        c = np.unique(c[np.isfinite(c) & (np.abs(c) <= 1)])
        t = (c / np.float32(2) + np.float32(0.5)) * np.float32(255)
        tie = t - np.floor(t) == 0.5
        x = np.concatenate([x, c[tie & (np.floor(t) % 2 == 0)][:4], c[tie & (np.floor(t) % 2 == 1)][:4]])      # eight: they count against the 1 % cap
    return np.resize(x, n) if n >= x.size else x[::x.size // n][:n]          # the small map: a strided sample that keeps ends, centres and boundary neighbours


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw", [5 * 7, 64 * 64])
def test_u8_inputs_keep_the_float32_reference_inside_the_exception_cap(prec, hw):
    x = _u8_inputs(prec, hw * 3 * 3).reshape(-1, 3)
    f32 = N.post_u8_f32(x)
    f64, dist = N.post_u8_64(x)
    near = dist <= 2.0 ** -14
    assert np.array_equal(f32[~near], f64[~near])
    assert near.mean() <= 0.01, near.mean()
    assert f32.min() == 0 and f32.max() == 255 and len(np.unique(f32)) == (256 if hw > 35 else len(np.unique(f64)))
    if prec == "bf16x3" and hw > 35:
        # exact ties whose even neighbour is BELOW: round-half-up gives another byte there
        t = (x / np.float32(2) + np.float32(0.5)) * np.float32(255)
        assert np.any((t - np.floor(t) == 0.5) & (np.floor(t) % 2 == 0))


# ---- GPU plumbing -----------------------------------------------------------------------------------------------------------------------------------
def _L():
    from mere_fusion_amd import _lib
    _lib.init_device(0)
    return _lib, _lib.lib()


def _geom(cbuf, coff, c, h, w, halo):
    from mere_fusion_amd import _lib
    return _lib.MfRowsGeom(cbuf, coff, c, h, w, halo)


def _full(g, batch):
    return torch.empty(batch, g.h + 2 * g.halo, g.w + 2 * g.halo, g.cbuf, device="cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_poison_outside(full, g, prec, tokens=0):
    """everything outside channels [coff, coff + c) of the interior pixels (of the first `tokens` tokens) is still the poison, bit for bit"""
    full = full.cpu().numpy()
    written = np.zeros(full.shape, bool)
    inner = written[:, g.halo:g.halo + g.h, g.halo:g.halo + g.w, g.coff:g.coff + g.c]
    t = np.arange(g.h * g.w).reshape(g.h, g.w) < (tokens or g.h * g.w)
    inner[:] = t[None, :, :, None]
    bad = _bits(full)[~written] != _bits(N.POISON[prec])
    assert not bad.any(), f"{int(bad.sum())} elements outside the view were written (first at {np.argwhere(~written)[np.argmax(bad)]})"
    return full[written]


def _needed(err, unit, rest):
    """the K this case needs: max (err - rest) / unit"""
    return float(((err - rest) / unit.clamp_min(1e-300)).clamp_min(0).max())


# ---- rows round trip ----------------------------------------------------------------------------------------------------------------------------------
def _special_values():
    lo_tie = [1 + 2.0 ** -10 * (1 + 2.0 ** -8), 1 + 2.0 ** -10 * (1 + 3 * 2.0 ** -8)]      # x - hi sits on a bf16 tie
    return torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)] + lo_tie + [0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38], dtype=torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w,halo", [(1, 77, 0), (1, 77, 1), (5, 7, 0), (5, 7, 1)])
def test_rows_round_trip_is_the_exact_split(lib_built, prec, h, w, halo):
    _lib, L = _L()
    batch, c, T = 3, 24, h * w
    g = _geom(40, 8, c, h, w, halo)
    gen = torch.Generator().manual_seed(h * 100 + w + halo)
    x = torch.randn(batch, T, c, generator=gen) * 10 ** torch.randint(-3, 4, (batch, T, 1), generator=gen).float()
    sp = _special_values()
    x.view(-1)[:sp.numel()] = sp
    add = torch.randn(T, c, generator=gen)
    for addend in (None, add):
        y, full = torch.empty(batch, T, c, device="cuda"), _full(g, batch)
        xd, addd = x.cuda(), (None if addend is None else addend.cuda())        # (named: a temporary's memory is reused before the call runs)
        _lib.check(L.mf_rows_roundtrip(xd.data_ptr(), _p(addd), y.data_ptr(), None, C.byref(g), batch, 0, 0, 1,
                                       _lib.PRECISIONS[prec], full.data_ptr(), None))
        src = x if addend is None else x + addend            # the kernel's fp32 add, broadcast over the batch
        want = N.stored(src.numpy(), prec)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want))
        inside = assert_poison_outside(full, g, prec)
        assert np.array_equal(_bits(inside), _bits(want).ravel())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layer", [0, 2])
def test_rows_layered_gather_leaves_the_other_layers(lib_built, prec, layer):
    _lib, L = _L()
    batch, c, T, tokens, nl = 3, 24, 77, 50, 3
    g = _geom(c, 0, c, 1, T, 1)
    x = torch.randn(batch, T, c, generator=torch.Generator().manual_seed(layer))
    dst, xd = torch.full((batch, tokens, nl, c), 7.25, device="cuda"), x.cuda()
    _lib.check(L.mf_rows_roundtrip(xd.data_ptr(), None, None, dst.data_ptr(), C.byref(g), batch, tokens, layer, nl, _lib.PRECISIONS[prec], None, None))
    dst = dst.cpu().numpy()
    assert np.array_equal(_bits(dst[:, :, layer]), _bits(N.stored(x[:, :tokens].numpy(), prec)))
    others = [i for i in range(nl) if i != layer]
    assert np.all(dst[:, :, others] == 7.25)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------------------
def _ln_input(batch, T, c, seed):
    """randn x a per-channel ramp, per-token offsets of R sigma (R cycling 0, 4, 100), one constant token, one token with a 1e4 outlier channel"""
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.5, 2.0, c)
    x = torch.randn(batch * T, c, generator=gen) * ramp
    x += (torch.tensor([0.0, 4.0, 100.0])[torch.arange(batch * T) % 3] * 1.3)[:, None]
    if batch * T >= 3:
        x[1] = 3.7
        x[-1, c // 3] = 1e4
    gamma = torch.linspace(-1.0, 2.0, c) if c > 1 else torch.ones(1)
    beta = torch.linspace(0.5, -0.5, c)
    return x.view(batch, T, c), gamma, beta


def _run_ln(x, gamma, beta, g, batch, tokens, act, prec):
    _lib, L = _L()
    T = g.h * g.w
    y, full = torch.empty(batch, T, g.c, device="cuda"), _full(g, batch)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    rc = L.mf_layernorm_forward(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), C.byref(g), C.byref(g), batch, 1e-5,
                                tokens, act, _lib.PRECISIONS[prec], full.data_ptr(), None)
    _lib.check(rc, "layernorm")
    return y.cpu(), full


def _check_ln(c, cbuf, coff, h, w, halo, batch, tokens, act, prec, tag):
    T = h * w
    g = _geom(cbuf, coff, c, h, w, halo)
    x, gamma, beta = _ln_input(batch, T, c, c * 7 + T + batch)
    xs = N.stored_t(x, prec)
    got, full = _run_ln(x, gamma, beta, g, batch, tokens, act, prec)
    assert_poison_outside(full, g, prec, tokens)
    n = tokens or T
    want, pre, sigma = N.layernorm64(xs[:, :n], gamma, beta, 1e-5, act)
    unit, rest = N.layernorm_terms(xs[:, :n], gamma, want, pre, sigma, act, prec)
    err = (got[:, :n].double() - want).abs()
    print(f"[layernorm {tag} C {c} cbuf {cbuf} coff {coff} {h}x{w} halo {halo} batch {batch} tokens {tokens} act {act} {prec}] "
          f"L-inf {float(err.max()):.3e} K needed {_needed(err, unit, rest):.2f} (K_LN {K_LN})")
    assert bool((err <= K_LN * unit + rest).all()), float((err / (K_LN * unit + rest)).max())
    if tokens:
        assert np.all(_bits(got[:, n:].numpy()) == _bits(N.POISON[prec]))


# C on each side of every dispatch boundary of mf_layernorm (k_layernorm_v8<1> to 512, <2> to 1024, <4> to 2048), then the scalar kernel reached four ways:
# C % 8, C % 8 at the register limit, a view that starts off an 8-channel group, a buffer whose pixel stride is no multiple of 8
LN_WIDTHS = [(c, c, 0) for c in (8, 24, 320, 384, 512, 520, 1024, 1032, 1280, 2048)] + [(30, 30, 0), (2047, 2047, 0), (320, 328, 4), (320, 324, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("i", range(len(LN_WIDTHS)), ids=lambda i: "c%d_cbuf%d_coff%d" % LN_WIDTHS[i])
def test_layernorm_every_dispatch_path(lib_built, prec, i):
    c, cbuf, coff = LN_WIDTHS[i]
    _check_ln(c, cbuf, coff, 1, 77, 1, 3, 0, 3 * (i % 2), prec, "width")
    _check_ln(c, cbuf, coff, 1, (1, 3, 5)[i % 3], i % 2, 1, 0, 3 * ((i + 1) % 2), prec, "width")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c,cbuf,coff", [(320, 328, 8), (30, 32, 1)], ids=lambda v: str(v))
def test_layernorm_row_counts_prefix_and_image_views(lib_built, prec, c, cbuf, coff):
    for T in (1, 3, 5, 77):                           # row counts off the 4 rows of a workgroup
        for batch in (1, 3):
            _check_ln(c, cbuf, coff, 1, T, (T + batch) % 2, batch, 0, 3 * (T % 2), prec, "rows")
    for act in (0, 3):
        for halo in (0, 1):
            _check_ln(c, cbuf, coff, 1, 77, halo, 3, 50, act, prec, "prefix")
            _check_ln(c, cbuf, coff, 5, 7, halo, 3, 0, act, prec, "image")
    _check_ln(c, cbuf, coff, 5, 7, 1, 3, 17, 0, prec, "image prefix")


@pytest.mark.gpu
def test_layernorm_rejects_rows_beyond_the_register_limit(lib_built):
    x, gamma, beta = _ln_input(1, 3, 2056, 0)
    with pytest.raises(RuntimeError, match="exceeds 2048"):
        _run_ln(x, gamma, beta, _geom(2056, 0, 2056, 1, 3, 1), 1, 0, 0, "bf16x3")


# ---- softmax ----------------------------------------------------------------------------------------------------------------------------------------------
def _softmax_rows(n_keys, n8, scale, seed):
    """12 rows of every kind, in RAW scores (the kernel multiplies by scale): all-equal (0, 3.5, -1e4), one-hot with margin 200 at keys 0 / 63 / 64 / last,
    randn with the largest logit at 8 / 24 / 64 (twice, two draws).  Pad columns n_keys .. n8-1 hold +1e4: a kernel that reads one of them sees it win."""
    gen = torch.Generator().manual_seed(seed)
    rows = [torch.zeros(n_keys), torch.full((n_keys,), 3.5), torch.full((n_keys,), -1e4)]
    for hot in (0, 63, 64, n_keys - 1):
        r = torch.randn(n_keys, generator=gen)
        r[min(hot, n_keys - 1)] = 200.0
        rows.append(r)
    for temp in (8.0, 24.0, 64.0, 8.0, 64.0):
        r = torch.randn(n_keys, generator=gen)
        rows.append(r * temp / r.abs().max())
    s = torch.full((len(rows), n8), 1e4)
    s[:, :n_keys] = torch.stack(rows) / scale
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_keys", [1, 7, 63, 64, 65, 129, 1024, 1500, 2048])
def test_softmax_rows(lib_built, prec, n_keys):
    _lib, L = _L()
    n8, n64 = (n_keys + 7) // 8 * 8, (n_keys + 63) // 64 * 64
    worst = 0.0
    for scale, (h, w, halo) in ((1.0, (2, 6, 0)), (64 ** -0.5, (1, 12, 1))):
        s1 = _softmax_rows(n_keys, n8, scale, n_keys)
        s = torch.stack([s1, s1.flip(0)])                                     # batch 2, the rows in the other order
        gs, gp = _geom(n8, 0, n8, h, w, halo), _geom(n64 + 8, 0, n64, h, w, halo)
        p, full, sd = torch.empty(2, 12, n64, device="cuda"), _full(gp, 2), s.cuda()
        _lib.check(L.mf_softmax_rows_forward(sd.data_ptr(), p.data_ptr(), C.byref(gs), C.byref(gp), 2, n_keys, scale, _lib.PRECISIONS[prec],
                                             full.data_ptr(), None))
        assert_poison_outside(full, gp, prec)
        p = p.cpu()
        assert np.all(_bits(p[..., n_keys:].numpy()) == 0), "padded columns must be +0 exactly"
        want, z = N.softmax64(N.stored_t(s, prec), scale, n_keys)
        unit, rest = N.softmax_terms(want, z, prec)
        err = (p[..., :n_keys].double() - want).abs()
        worst = max(worst, _needed(err, unit, rest))
        assert bool((err <= K_SM * unit + rest).all()), float((err / (K_SM * unit + rest)).max())
        assert bool(((p[..., :n_keys].double().sum(-1) - 1).abs() <= (K_SM * unit + rest).sum(-1)).all())
        for b, rows in ((0, (0, 1, 2)), (1, (11, 10, 9))):                     # all-equal rows: exactly uniform
            for r in rows:
                assert len(torch.unique(p[b, r, :n_keys])) == 1
        for i, hot in enumerate((0, 63, 64, n_keys - 1)):
            assert abs(float(p[0, 3 + i, min(hot, n_keys - 1)]) - 1) <= N.REPR[prec]
    print(f"[softmax n_keys {n_keys} {prec}] K needed {worst:.2f} (K_SM {K_SM})")


@pytest.mark.gpu
def test_softmax_rejects_rows_beyond_the_register_limit(lib_built):
    _lib, L = _L()
    gs, gp = _geom(2048, 0, 2048, 1, 4, 0), _geom(2112, 0, 2112, 1, 4, 0)
    s, p = torch.zeros(1, 4, 2048, device="cuda"), torch.empty(1, 4, 2112, device="cuda")
    rc = L.mf_softmax_rows_forward(s.data_ptr(), p.data_ptr(), C.byref(gs), C.byref(gp), 1, 2048, 1.0, 1, None, None)
    with pytest.raises(RuntimeError, match="2112 exceeds 2048"):
        _lib.check(rc)


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------------------------
def _gn_input(batch, T, c, groups, seed):
    """randn x per-channel scales with group offsets of R sigma (R cycling 0, 4, 30 over the groups); the last group's channels alternate scales 1 and 1e3"""
    gen = torch.Generator().manual_seed(seed)
    cpg = c // groups
    sc = torch.linspace(0.5, 2.0, c)
    if cpg >= 2:
        sc[c - cpg:] = torch.tensor([1.0, 1e3])[torch.arange(cpg) % 2]
    rms = sc.view(groups, cpg).pow(2).mean(1).sqrt()
    off = (torch.tensor([0.0, 4.0, 30.0])[torch.arange(groups) % 3] * rms).repeat_interleave(cpg)
    x = torch.randn(batch, T, c, generator=gen) * sc + off
    gamma = torch.linspace(-1.0, 2.0, c)
    beta = torch.linspace(0.5, -0.5, c)
    return x, gamma, beta


def _check_gn(c, groups, h, w, halo, batch, prec, cbuf=None, coff=0):
    _lib, L = _L()
    T, eps = h * w, 1e-6
    g = _geom(cbuf or c, coff, c, h, w, halo)
    x, gamma, beta = _gn_input(batch, T, c, groups, c + groups + T)
    xs = N.stored_t(x, prec)
    sums = N.gn_stats64(xs, groups)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    worst = 0.0
    for silu in (0, 1):
        want, pre, R, sc64, sh64 = N.groupnorm64(xs, gamma, beta, groups, eps, silu)
        unit, rest = N.groupnorm_terms(gamma, want, pre, R, silu, prec)
        for have in (0, 1):
            y, full = torch.empty(batch, T, c, device="cuda"), _full(g, batch)
            st = sums.cuda().contiguous() if have else torch.full((batch, groups, 2), float("nan"), dtype=torch.float64, device="cuda")
            scale, shift = torch.empty(batch, c, device="cuda"), torch.empty(batch, c, device="cuda")
            _lib.check(L.mf_groupnorm_forward(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), C.byref(g), C.byref(g), batch, groups, eps, silu, have,
                                              st.data_ptr(), scale.data_ptr(), shift.data_ptr(), _lib.PRECISIONS[prec], full.data_ptr(), None))
            assert_poison_outside(full, g, prec)
            err = (y.cpu().double() - want).abs()
            k = _needed(err, unit, rest)
            worst = max(worst, k)
            assert bool((err <= K_GN * unit + rest).all()), (silu, have, float((err / (K_GN * unit + rest)).max()))
            if not have:
                # a thread adds at most 64 pixels in fp32 before the fp64 bins: 64 x 2^-24 of the sum of magnitudes
                mag = N.gn_stats64(xs.abs(), groups)
                assert bool(((st.cpu() - sums).abs() <= 64 * F32 * mag + 1e-300).all()), "statistics"
            # mf_groupnorm_affine: scale = rstd gamma, shift = beta - mean scale
            mean_c = (sums[..., 0] / (T * (c // groups))).repeat_interleave(c // groups, 1)
            e_sc = (K_GN * F32 * (1 + R[:, 0] ** 2) + 2 * F32) * sc64.abs()
            assert bool(((scale.cpu().double() - sc64).abs() <= e_sc + N.TINY).all()), "affine scale"
            assert bool(((shift.cpu().double() - sh64).abs() <= mean_c.abs() * e_sc + 2 * F32 * (beta.double().abs() + (mean_c * sc64).abs()) + N.TINY).all()), "affine shift"
    print(f"[groupnorm C {c} groups {groups} {h}x{w} halo {halo} batch {batch} {prec}] K needed {worst:.2f} (K_GN {K_GN})")


# every relation of the 8-channel chunks to the groups (a group per chunk, per channel, 8 | cpg, cpg = 3 and 10 that do not divide 8, 16 | cpg, the second
# column block from C > 2048), maps of 1 token, 35 tokens against the 6 token lanes of C = 320 and against other lane counts, 256 tokens
GN_CASES = [(8, 1, 1, 1, 1), (8, 8, 5, 7, 3), (32, 32, 5, 7, 1), (64, 32, 16, 16, 3), (96, 32, 5, 7, 3), (320, 32, 7, 5, 3), (320, 32, 16, 16, 1), (512, 32, 5, 7, 1),
            (2560, 32, 5, 7, 3), (2560, 32, 1, 1, 1), (4096, 64, 5, 7, 1), (4096, 64, 16, 16, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "c%d_g%d_%dx%d_b%d" % c)
def test_groupnorm_chunk_to_group_relations(lib_built, prec, case):
    c, groups, h, w, batch = case
    _check_gn(c, groups, h, w, (c // 8) % 2, batch, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_groupnorm_view_inside_a_wider_buffer(lib_built, prec):
    _check_gn(320, 32, 7, 5, 1, 3, prec, cbuf=336, coff=8)


# k_gn_apply<4> from batch * T * C/8 >= 2^20: 2 x 13120 x 40 = 1049600 and 1 x 2048 x 512 = 2^20 take it, the same 320-channel tensor at batch 1 does not
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [(320, 32, 82, 160, 2), (320, 32, 82, 160, 1), (4096, 64, 32, 64, 1)], ids=lambda c: "c%d_g%d_%dx%d_b%d" % c)
def test_groupnorm_four_token_variant_and_its_threshold(lib_built, prec, case):
    c, groups, h, w, batch = case
    _check_gn(c, groups, h, w, 1, batch, prec)


@pytest.mark.gpu
def test_groupnorm_rejects_more_groups_than_bins(lib_built):
    _lib, L = _L()
    g = _geom(520, 0, 520, 2, 2, 1)
    x, y, v = torch.zeros(1, 4, 520, device="cuda"), torch.zeros(1, 4, 520, device="cuda"), torch.zeros(520, device="cuda")
    rc = L.mf_groupnorm_forward(x.data_ptr(), v.data_ptr(), v.data_ptr(), y.data_ptr(), C.byref(g), C.byref(g), 1, 65, 1e-6, 0, 0, None, None, None, 1, None, None)
    with pytest.raises(RuntimeError, match="groups=65"):
        _lib.check(rc)


# ---- GEMM with a device-packed operand ------------------------------------------------------------------------------------------------------------------------
def _gemm_inputs(T, n, k, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(T, k, generator=gen) * torch.linspace(0.5, 1.5, k) + 0.05 * torch.arange(k) / k
    b = torch.randn(n, k, generator=gen) * torch.linspace(1.5, 0.5, k) + torch.linspace(-0.3, 0.3, n)[:, None]
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layout", ["keys", "v_transposed"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 50, 1500])
def test_gemm_with_device_packed_operand(lib_built, prec, layout, n):
    _lib, L = _L()
    n8 = (n + 7) // 8 * 8
    for k in (8, 24, 64, 72, 512):
        for T in (1, 77):
            a, b = _gemm_inputs(T, n, k, n * 31 + k + T)
            a_s, b_s = N.stored_t(a, prec), N.stored_t(b, prec)
            if layout == "keys":                                      # b stored [n][k]
                src, rows, cols, sn, sk = b, n, k, k, 1
            else:                                                     # b stored [k][n]: V transposed
                src, rows, cols, sn, sk = b.t().contiguous(), k, n, 1, n
            ad, bd = a.cuda(), src.cuda()
            for pn, pk in ((n, k), ((n + 1) // 2, k - 3 if k > 8 else k)):
                out, full = torch.empty(T, n, device="cuda"), torch.empty(1, 3, T + 2, n8, device="cuda")
                _lib.check(L.mf_gemm_bt_forward(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), T, n, k, rows, cols, sn, sk, pn, pk, _lib.PRECISIONS[prec],
                                                full.data_ptr(), None))
                # mf_conv_launch's contract: the epilogue stores channel quads, so a width that is no multiple of 4 spills zero-weight channels up to the next one
                n4 = (n + 3) // 4 * 4
                assert_poison_outside(full, _geom(n8, 0, n4, 1, T, 1), prec)
                assert np.all(_bits(full[0, 1, 1:T + 1, n:n4].cpu().numpy()) == 0)
                bz = torch.zeros_like(b_s)
                bz[:pn, :pk] = b_s[:pn, :pk]                           # what the second, smaller pack must leave: zeros elsewhere
                want = N.gemm_bt64(a_s, bz)
                err = (out.cpu().double() - want).abs()
                bound = N.gemm_bound(a_s.double(), bz.double(), want, prec)
                assert bool((err <= bound + N.TINY).all()), (k, T, pn, pk, float((err / (bound + N.TINY)).max()))
                assert np.all(_bits(out.cpu()[:, pn:].numpy()) == 0)


# ---- composite attention ----------------------------------------------------------------------------------------------------------------------------------------
def _composite(q, k, v, heads, prec):
    _lib, L = _L()
    b, tq, c = q.shape
    out = torch.empty(b, tq, c, device="cuda")
    qd, kd, vd = (t.contiguous().cuda() for t in (q, k, v))
    _lib.check(L.mf_attention_composite_forward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(),
                                                b, tq, k.shape[1], heads, c // heads, _lib.PRECISIONS[prec], None, None))
    return out.cpu()


ATT_CASES = [(dh, tk, tq) for dh in (8, 24, 128, 512) for tk in (1, 63, 64, 65, 129, 1024) for tq in (1, 77)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dh,tk,tq", ATT_CASES, ids=lambda v: str(v))
def test_composite_attention_rows(lib_built, prec, dh, tk, tq):
    """q = 0 returns the mean of the valid v rows, one-hot rows return the hot v row, randn rows match float64: at every key count around the 64-wide
    padding of the weights, for one and two heads, batch 1 and 3"""
    heads, batch = ((1, 1), (2, 3))[(ATT_CASES.index((dh, tk, tq)) // 2) % 2]
    gen = torch.Generator().manual_seed(dh * 3 + tk)
    v = torch.randn(batch, tk, heads * dh, generator=gen) * 2 + 0.5
    k = torch.randn(batch, tk, heads * dh, generator=gen)
    got = _composite(torch.zeros(batch, tq, heads * dh), k, v, heads, prec)
    vs = N.stored_t(v, prec)
    want = vs.double().mean(1, keepdim=True).expand(batch, tq, heads * dh)
    err = float((got.double() - want).abs().max() / vs.abs().max())
    print(f"[composite uniform dh {dh} tk {tk} tq {tq} {prec}] L-inf / max|v| {err:.2e} (bound {2 * N.REPR[prec]:.2e})")
    assert err <= N.attention_unit(0.0, 1.0, prec), err                 # the weights and the output each pass through the planes

    hot = sorted({0, min(64, tk - 1), tk - 1})[:dh - 1]
    q, k, v, _ = N._one_hot_qkv(batch, tq, tk, heads, dh, hot, seed=dh + tk)
    got = _composite(q, k, v, heads, prec)
    want = N._one_hot_qkv(batch, tq, tk, heads, dh, hot, seed=dh + tk)[3]
    want = N.stored_t(want, prec)
    rel = float(((got - want).abs() / want.abs().clamp_min(1e-6)).max())
    print(f"[composite one-hot dh {dh} tk {tk} tq {tq} hot {hot} {prec}] max relative error {rel:.2e} (bound {N.REPR[prec]:.2e})")
    assert rel <= N.REPR[prec], rel

    q, k, v = (N.stored_t(t, prec) for t in N._qkv(batch, tq, tk, heads, dh, dh + tk))
    want, zmax = N.attention64(q, k, v, heads)
    err = float((_composite(q, k, v, heads, prec).double() - want).abs().max())
    unit = N.attention_unit(zmax, float(v.abs().max()), prec)
    print(f"[composite randn dh {dh} tk {tk} tq {tq} {prec}] L-inf {err:.2e} K needed {err / unit:.3f} (K_ATT {K_ATT})")
    assert err <= K_ATT * unit, err / unit


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("temp", [8, 24, 64])
@pytest.mark.parametrize("dh,tk", [(8, 1024), (24, 129), (128, 65), (512, 1024)])
def test_composite_attention_temperature_sweep(lib_built, prec, temp, dh, tk):
    heads, tq = 2, 77
    q, k, v = N._qkv(1, tq, tk, heads, dh, 3 * dh + tk)
    zmax = N.attention64(q, k, v, heads)[1]
    s = (temp / zmax) ** 0.5
    q, k, v = N.stored_t(q * s, prec), N.stored_t(k * s, prec), N.stored_t(v, prec)
    want, zmax = N.attention64(q, k, v, heads)
    err = float((_composite(q, k, v, heads, prec).double() - want).abs().max())
    unit = N.attention_unit(zmax, float(v.abs().max()), prec)
    print(f"[composite temperature {temp} dh {dh} tk {tk} {prec}] L-inf {err:.2e} K needed {err / unit:.3f} (K_ATT {K_ATT})")
    assert err <= K_ATT * unit, err / unit


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dh", [40, 64, 80, 160])
def test_composite_and_fused_attention_agree(lib_built, prec, dh):
    from test_attention import _hip_attention
    for tk in (63, 129):
        q, k, v = (N.stored_t(t, prec) for t in N._qkv(2, 77, tk, 2, dh, dh + tk))
        zmax = N.attention64(q, k, v, 2)[1]
        fused_bound = 2e-4 if prec == "bf16x3" else 8e-2              # test_attention.py::test_hip_attention_matches_oracle
        diff = float((_composite(q, k, v, 2, prec) - _hip_attention(q, k, v, 2, prec)).abs().max())
        assert diff <= fused_bound + K_ATT * N.attention_unit(zmax, float(v.abs().max()), prec), diff


# ---- uint8 tail -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("h,w", [(5, 7), (64, 64)])
@pytest.mark.parametrize("cbuf,coff", [(3, 0), (8, 2)])
def test_vae_post_u8(lib_built, prec, h, w, cbuf, coff):
    _lib, L = _L()
    batch = 3
    x = torch.from_numpy(_u8_inputs(prec, h * w * 3 * batch).copy()).view(batch, h * w, 3)
    g = _geom(cbuf, coff, 3, h, w, 1)
    dst, xd = torch.zeros(batch, h, w, 3, dtype=torch.uint8, device="cuda"), x.cuda()
    _lib.check(L.mf_vae_post_u8_forward(xd.data_ptr(), dst.data_ptr(), C.byref(g), batch, _lib.PRECISIONS[prec], None))
    got = dst.cpu().numpy().reshape(batch, h * w, 3)
    xs = N.stored(x.numpy(), prec)
    assert np.array_equal(got, N.post_u8_f32(xs)), "differs from the float32 evaluation of the same expression"       # BGR: post_u8_* reverse the channels
    f64, dist = N.post_u8_64(xs)
    near = dist <= 2.0 ** -14
    assert np.array_equal(got[~near], f64[~near])
    assert near.mean() <= 0.01
