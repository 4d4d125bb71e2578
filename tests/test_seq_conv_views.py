"""The conv engine and the fused attention kernel launched the way the sequence models launch them: (1 x k) layers on H == 1 buffers, token prefixes,
channel-slice views of shared buffers, residuals from another buffer, packed q | k | v -- one op at a time, through mf_conv_view_forward and
mf_attention_view_forward (csrc/mf_nn_api.hip).

Seams.  Both own their buffers per call and fill them with the poison of test_nn_ops first: the conv's input buffer then gets a zero halo ring (what a
network's allocation holds there) and the input view loaded over the poison, the output and residual buffers stay poisoned outside the loaded views, and
`y_full` hands the whole padded output buffer back.  A write outside the view -- rows past a prefix, a neighbouring group's channels, the ring -- changes
bits that assert_poison_outside compares exactly.

Conv comparisons are gated at conv_numerics.conv_bound (derivation: test_conv_configs.py) with the true K = taps x cin, inputs exact in the storage
format; the worst error of every comparison is printed in units of U A.  Attention on views is compared bit for bit with mf_attention_forward on the same
tensors: the kernel's arithmetic does not depend on addresses, so a pitch, offset or batch stride taken from the wrong tensor is the only way to differ."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_numerics import U, conv_bound, conv_ref, exact, gelu64, grouped_seq_ref
from nn_numerics import POISON, _qkv
from test_attention import KT, _hip_attention
from test_conv_configs import FAMILY, STATS, _kt_min, _note
from test_nn_ops import _bits, assert_poison_outside

PRECS = ["bf16x3", "bf16"]
BATCH = 3


def _d(cin, cout, k, s, p, w, act=0, residual=0):
    """a (1 x k) layer on a sequence of w positions"""
    return dict(cin=cin, cout=cout, kh=1, kw=k, stride_h=1, stride_w=s, pad_h=0, pad_w=p, act=act, residual=residual, in_h=1, in_w=w)


def _out_w(d):
    return (d["in_w"] + 2 * d["pad_w"] - d["kw"]) // d["stride_w"] + 1


def _halo_need(d):
    """mf_conv_plan_create's in_halo_need for a (1 x k) layer"""
    over = (_out_w(d) - 1) * d["stride_w"] + d["kw"] - 1 - d["pad_w"] - (d["in_w"] - 1)
    return max(d["pad_w"], over, 0)


# (name, desc, separate residual): Whisper's two convolutions (conv2's residual is the positional table: another buffer, added after the GELU), the same with
# cin % 64 == 0 (the tap-grouped K ordering, with 3 taps), wav2vec2's feature extractor (no padding; cin = 1 padded to 8; a length the stride does not divide)
SEQ_CASES = [
    ("whisper conv1", _d(80, 72, 3, 1, 1, 131, act=3), False),
    ("whisper conv2", _d(72, 72, 3, 2, 1, 131, act=3, residual=2), True),
    ("whisper conv2 cin 64", _d(64, 72, 3, 2, 1, 131, act=3, residual=2), True),
    ("wav2vec2 conv0", _d(1, 40, 10, 5, 0, 400), False),
    ("wav2vec2 k3 s2", _d(40, 40, 3, 2, 0, 79), False),
    ("wav2vec2 k2 s2", _d(40, 40, 2, 2, 0, 39), False),
    ("wav2vec2 k2 s2 odd remainder", _d(40, 40, 2, 2, 0, 40), False),
]
# the linear forms of the encoders (1 x 1 on T = 77): plain, residual before the activation from another buffer, GELU, cout % 4 != 0 (lm_head)
LINEAR_CASES = [
    ("linear", _d(136, 72, 1, 1, 0, 77), False),
    ("linear residual", _d(136, 72, 1, 1, 0, 77, residual=1), True),
    ("linear gelu", _d(136, 72, 1, 1, 0, 77, act=3), False),
    ("linear cout 30", _d(136, 30, 1, 1, 0, 77), False),
]
CONV2 = SEQ_CASES[1][1]
CONV1 = SEQ_CASES[0][1]
LINEAR = LINEAR_CASES[0][1]


# ---- CPU: the references ---------------------------------------------------------------------------------------------------------------------------
REF_CASES = SEQ_CASES + LINEAR_CASES + [
    ("whisper conv2, residual before the activation", dict(CONV2, residual=1), True),
    ("linear, residual after the activation", dict(LINEAR, act=3, residual=2), True),
    ("k3 s2 p1, residual is the input", _d(24, 24, 3, 1, 1, 17, act=3, residual=2), False),
]


@pytest.mark.parametrize("case", REF_CASES, ids=[c[0] for c in REF_CASES])
def test_conv_ref_is_torch_conv1d(case):
    """conv_ref with a (1 x k) descriptor and a residual operand of its own, against torch.nn.Conv1d in float64: stride, padding, GELU, the residual before
    and after the activation"""
    name, d, sep = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(2, d["cin"], d["in_w"], generator=g, dtype=torch.float64)
    m = nn.Conv1d(d["cin"], d["cout"], d["kw"], stride=d["stride_w"], padding=d["pad_w"]).double()
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64))
        m.bias.copy_(torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
        pre = m(x)
        assert pre.shape[-1] == _out_w(d)
        r = torch.randn(pre.shape, generator=g, dtype=torch.float64) if sep else x
        if d["residual"] == 1:
            pre = pre + r
        want = F.gelu(pre) if d["act"] == 3 else pre
        if d["residual"] == 2:
            want = want + r
        got, mag = conv_ref(x[:, :, None], m.weight.detach()[:, :, None], m.bias.detach(), d, res=r[:, :, None] if sep else None)
    assert got.shape == want[:, :, None].shape
    assert torch.allclose(got[:, :, 0], want, rtol=1e-12, atol=1e-12)
    assert torch.all(mag["pre"][:, :, 0] >= pre.abs() - 1e-12)
    if d["residual"] == 2:
        assert torch.equal(mag["res"][:, :, 0], r.abs())              # the separate operand's magnitude, not the input's


POS_GROUPS = [(3, 64), (2, 40)]           # (G, gc): cin_pad % 64 == 0 (tap-grouped K ordering) and the other ordering
POS_K = [128, 16, 4]


def _pos_lengths(K):
    return [K // 2 - 1, K // 2, min(K + 5, 160)]


def _pos_weights(G, gc, K, seed, dtype=np.float64):
    """weight_norm(dim = 2) parameters of a grouped Conv1d(G gc, G gc, K, groups = G) folded as mf_wav2vec2_create folds them (g v / |v|, the norm over
    dims 0 and 1 per tap), and the per-group (K + 1)-tap weights with the zero tap appended: (w [G gc, gc, K], wg [G, gc, gc, 1, K + 1], bias [G gc])"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((G * gc, gc, K))
    gk = rng.uniform(0.5, 2.0, K) * math.sqrt(G * gc * gc) / math.sqrt(gc * K)
    w = gk[None, None, :] * v / np.sqrt((v * v).sum(axis=(0, 1)))[None, None, :]
    wg = np.zeros((G, gc, gc, 1, K + 1))
    wg[:, :, :, 0, :K] = w.reshape(G, gc, gc, K)
    b = 0.5 * rng.standard_normal(G * gc)
    return (w.astype(dtype), wg.astype(dtype), b.astype(dtype)), (v, gk)


def _pos_desc(gc, K, T):
    return _d(gc, gc, K + 1, 1, K // 2, T, act=3, residual=2)


@pytest.mark.parametrize("G,gc", POS_GROUPS)
@pytest.mark.parametrize("K", POS_K)
def test_grouped_seq_ref_is_the_samepad_positional_conv(G, gc, K):
    """grouped_seq_ref on the launches mf_wav2vec2::body makes -- one symmetric pad-K/2 layer of K + 1 taps (the last zero) per channel group, GELU, + the
    hidden state -- against Wav2Vec2PositionalConvEmbedding in float64: weight-normed grouped Conv1d(padding = K / 2), SamePad drops the last output of
    the even kernel, GELU, + x; for sequences shorter than, equal to and longer than the padding"""
    (w, wg, b), (v, gk) = _pos_weights(G, gc, K, seed=G * 1000 + K)
    wn = torch._weight_norm(torch.from_numpy(v), torch.from_numpy(gk).view(1, 1, K), 2)
    assert torch.allclose(wn, torch.from_numpy(w), rtol=1e-13, atol=1e-13)               # the fold is torch's weight_norm over dim 2
    for T in _pos_lengths(K):
        x = torch.randn(2, G * gc, T, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
        conv = F.conv1d(x, torch.from_numpy(w), torch.from_numpy(b), padding=K // 2, groups=G)[..., :-1]
        want = F.gelu(conv) + x
        d = _pos_desc(gc, K, T)
        assert _out_w(d) == T and _halo_need(d) == K // 2
        got, mag = grouped_seq_ref(x[:, :, None], torch.from_numpy(wg), torch.from_numpy(b).view(G, gc), d)
        assert got.shape == (2, G * gc, 1, T)
        assert torch.allclose(got[:, :, 0], want, rtol=1e-12, atol=1e-12), (T, float((got[:, :, 0] - want).abs().max()))
        assert torch.all(mag["pre"][:, :, 0] >= conv.abs() - 1e-12) and torch.equal(mag["res"][:, :, 0], x.abs())


def test_grouped_seq_ref_takes_a_separate_residual():
    d = _d(8, 8, 3, 1, 1, 9, act=3, residual=1)
    g = torch.Generator().manual_seed(3)
    x, r = torch.randn(2, 16, 1, 9, generator=g, dtype=torch.float64), torch.randn(2, 16, 1, 9, generator=g, dtype=torch.float64)
    w, b = torch.randn(2, 8, 8, 1, 3, generator=g, dtype=torch.float64), torch.randn(2, 8, generator=g, dtype=torch.float64)
    got, mag = grouped_seq_ref(x, w, b, d, res=r)
    for k in range(2):
        one, m1 = conv_ref(x[:, 8 * k:8 * k + 8], w[k], b[k], d, res=r[:, 8 * k:8 * k + 8])
        assert torch.equal(got[:, 8 * k:8 * k + 8], one) and torch.equal(mag["pre"][:, 8 * k:8 * k + 8], m1["pre"])


# ---- GPU plumbing ------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from mere_fusion_amd import _lib
    _lib.init_device(0)
    return _lib, _lib.lib()


def _geom(cbuf, coff, c, w, halo, h=1):
    from mere_fusion_amd import _lib
    return _lib.MfRowsGeom(cbuf, coff, c, h, w, halo)


def _rows(t):
    """[B, C, 1, T] -> the [B, T, C] rows the seams take"""
    return t[:, :, 0].transpose(1, 2).contiguous()


def _nchw(rows):
    return rows.transpose(1, 2)[:, :, None]


def _r8(n):
    return (n + 7) // 8 * 8


class Seq:
    """one (1 x k) layer (or G of them, one per channel group) with seeded parameters and inputs exact in the storage format"""

    def __init__(self, d, prec, seed, batch=BATCH, groups=1, sep_res=False, weights=None):
        self.d, self.prec, self.B, self.G = d, prec, batch, groups
        rng = np.random.default_rng(seed)
        ci, co, k = d["cin"], d["cout"], d["kw"]
        if weights is None:
            self.w = (rng.standard_normal((groups, co, ci, 1, k)) / math.sqrt(ci * k)).astype(np.float32)
            self.b = (0.5 * rng.standard_normal((groups, co))).astype(np.float32)
        else:
            self.w, self.b = weights
        self.cin_pad = _r8(ci)
        x = np.zeros((batch, groups * self.cin_pad, 1, d["in_w"]), np.float32)           # the padding channels hold zero, as in the networks
        for g in range(groups):
            x[:, g * self.cin_pad:g * self.cin_pad + ci] = exact(rng, (batch, ci, 1, d["in_w"]), prec)
        self.x = torch.from_numpy(x)
        self.res = torch.from_numpy(exact(rng, (batch, groups * co, 1, _out_w(d)), prec)) if sep_res else None
        self.ow = _out_w(d)

    def geoms(self, in_cbuf=None, in_coff=0, out_cbuf=None, out_coff=0, res_cbuf=None, res_coff=0, in_halo=None, out_halo=1):
        cin, cout = self.G * self.cin_pad, self.G * self.d["cout"]
        gx = _geom(in_cbuf or cin, in_coff, cin, self.d["in_w"], max(1, _halo_need(self.d)) if in_halo is None else in_halo)
        gy = _geom(out_cbuf or _r8(cout), out_coff, cout, self.ow, out_halo)
        gr = _geom(res_cbuf or cout, res_coff, cout, self.ow, 1) if self.res is not None else None
        return gx, gy, gr

    def run(self, gx, gy, gr, tokens=0, pin=None, only=-1):
        """-> (y [B, cout, 1, Wo] on the CPU, y_full on the CPU, the configuration that ran)"""
        _lib, L = _L()
        f = dict(transposed=0, output_padding=0, upsample=0, pad_hi=0)
        f.update(self.d)
        cd = _lib.MfConv2dDesc(**{k: f[k] for k, _ in _lib.MfConv2dDesc._fields_})
        xd = _rows(self.x).cuda()
        rd = _rows(self.res).cuda() if self.res is not None else None
        y = torch.full((self.B, self.ow, gy.c), float("nan"), device="cuda")
        full = torch.full((self.B, gy.h + 2 * gy.halo, gy.w + 2 * gy.halo, gy.cbuf), float("nan"), device="cuda")
        info = (C.c_int * 11)()
        pins = (C.c_int * 6)(*(pin[0] + (pin[1], pin[2]))) if pin else None
        w, b = np.ascontiguousarray(self.w, np.float32), np.ascontiguousarray(self.b, np.float32)
        rc = L.mf_conv_view_forward(C.byref(cd), w.ctypes.data, b.ctypes.data, xd.data_ptr(), rd.data_ptr() if rd is not None else None, y.data_ptr(),
                                    C.byref(gx), C.byref(gy), C.byref(gr) if gr is not None else None, self.B, tokens, self.G, only, pins, info,
                                    _lib.PRECISIONS[self.prec], full.data_ptr(), None)
        _lib.check(rc, "conv_view_forward")
        v = list(info)
        cfg = dict(family=FAMILY[v[0]], tile=tuple(v[1:5]), split=v[5], ld=v[6], bk=v[7], nphase=v[8], stats=STATS[v[9]], pinned=v[10])
        return _nchw(y.cpu()), full.cpu(), cfg

    def reference(self):
        ci, co = self.d["cin"], self.d["cout"]
        x = torch.cat([self.x[:, g * self.cin_pad:g * self.cin_pad + ci] for g in range(self.G)], 1)
        want, mag = grouped_seq_ref(x, torch.from_numpy(self.w), torch.from_numpy(self.b), self.d, res=self.res)
        return want, mag, conv_bound(want, mag, self.d, self.prec, ci)

    def check(self, y, what, tokens=0, ref=None, channels=None):
        """rows < tokens (all: 0) of y within the bound, NaN and poison included in the failures; -> the worst error in units of U A"""
        want, mag, bound = ref or self.reference()
        n = tokens or self.ow
        sl = (slice(None), channels or slice(None), slice(None), slice(0, n))
        got, want, bound, A = y.double()[sl], want[sl], bound[sl], (mag["pre"] + mag["res"])[sl]
        err = (got - want).abs()
        ok = err <= bound
        if not bool(ok.all()):
            bad = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements over the bound; first at {bad}: got {got[tuple(bad)].item():.6e} "
                                 f"want {want[tuple(bad)].item():.6e} bound {bound[tuple(bad)].item():.3e}")
        return float((err / (U[self.prec] * A + 1e-300)).max())


def _poison_geom(gy, coff=None, c=None):
    """the part of the output buffer a launch may write: the view, its channel count rounded up to the quad the epilogue stores (cout % 4 != 0: up to 3
    zero-weight channels behind the view, which the launch requires the buffer to have)"""
    coff, c = gy.coff if coff is None else coff, gy.c if c is None else c
    return _geom(gy.cbuf, coff, (c + 3) // 4 * 4, gy.w, gy.halo, gy.h)


def _clamped_split(d, split):
    f = dict(d, upsample=0, transposed=0)
    return 1 if d["cout"] % 4 else max(1, min(split, _kt_min(f)))


# ---- a. sequence geometries, whole-buffer views ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", SEQ_CASES + LINEAR_CASES, ids=[c[0] for c in SEQ_CASES + LINEAR_CASES])
def test_sequence_layers_vs_fp64(lib_built, prec, case):
    """every (1 x k) geometry of the Whisper and wav2vec2 encoders and each of their linear forms at batch 3 (tiles straddle samples), on whole-buffer
    views, against float64 at the derived bound; nothing outside the view is written"""
    name, d, sep = case
    lay = Seq(d, prec, seed=sum(map(ord, name)), sep_res=sep)
    gx, gy, gr = lay.geoms()
    y, full, cfg = lay.run(gx, gy, gr)
    assert cfg["family"] == "igemm", (name, cfg)
    _note("igemm", prec, lay.check(y, f"{name} {prec} {cfg}"))
    assert_poison_outside(full, _poison_geom(gy), prec)


# ---- b. pinned split-K on sequences ----------------------------------------------------------------------------------------------------------------------
PIN_LAYERS = [("whisper conv2", CONV2, True), ("linear", LINEAR, False)]
SEQ_PINS = [((64, 64, 2, 2), 1, -1), ((64, 64, 2, 2), 3, -1), ((128, 64, 2, 2), 2, -1)]
PIN3 = SEQ_PINS[1]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layer", PIN_LAYERS, ids=[c[0] for c in PIN_LAYERS])
def test_pinned_split_k_on_sequences(lib_built, prec, layer):
    name, d, sep = layer
    lay = Seq(d, prec, seed=sum(map(ord, name)) + 1, sep_res=sep)
    gx, gy, gr = lay.geoms()
    ref = lay.reference()
    for pin in SEQ_PINS:
        y, full, cfg = lay.run(gx, gy, gr, pin=pin)
        assert cfg["family"] == "igemm" and cfg["pinned"] == 1 and cfg["tile"] == pin[0], (name, pin, cfg)
        assert cfg["split"] == _clamped_split(d, pin[1]), (name, pin, cfg)
        _note("igemm", prec, lay.check(y, f"{name} {prec} pin {pin} {cfg}", ref=ref))
        assert_poison_outside(full, _poison_geom(gy), prec)


# ---- c. token prefixes ---------------------------------------------------------------------------------------------------------------------------------
PREFIX_LAYERS = PIN_LAYERS + [("whisper conv1", CONV1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pinned", [False, True], ids=["unpinned", "split-3 pin"])
@pytest.mark.parametrize("layer", PREFIX_LAYERS, ids=[c[0] for c in PREFIX_LAYERS])
def test_token_prefixes(lib_built, prec, layer, pinned):
    """the `tokens` argument of mf_conv_launch: rows < tokens of every sample within the bound, every row >= tokens and everything else outside the view
    still the poison, bit for bit.  The prefixes are t in {1, 37, W_out - 1, W_out} of the layer; Whisper's conv1 gets the prefix the encoder derives from its
    conv2's t (W_out = 66): min(2 t + 2, W)."""
    name, d, sep = layer
    lay = Seq(d, prec, seed=sum(map(ord, name)) + 2, sep_res=sep)
    gx, gy, gr = lay.geoms()
    ref = lay.reference()
    wo = lay.ow
    prefixes = [1, 37, wo - 1, wo] if d is not CONV1 else sorted({min(2 * t + 2, wo) for t in (1, 37, _out_w(CONV2) - 1, _out_w(CONV2))})
    for t in prefixes:
        y, full, cfg = lay.run(gx, gy, gr, tokens=t, pin=PIN3 if pinned else None)
        assert cfg["family"] == "igemm" and cfg["pinned"] == int(pinned), (name, t, cfg)
        if pinned:
            assert cfg["tile"] == PIN3[0] and cfg["split"] > 1, (name, t, cfg)           # (the launch re-balances a prefix's split; these stay split)
        _note("igemm", prec, lay.check(y, f"{name} {prec} tokens {t} {cfg}", tokens=t, ref=ref))
        assert_poison_outside(full, _poison_geom(gy), prec, tokens=t)
        assert np.all(_bits(y[:, :, :, t:].numpy()) == _bits(POISON[prec]))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_token_prefix_refusals(lib_built, prec):
    """a prefix longer than the sequence, on a 2-D layer and on a halo-family layer: refused with a message, nothing launched"""
    lay = Seq(CONV2, prec, seed=5, sep_res=True)
    with pytest.raises(RuntimeError, match="token prefix"):
        lay.run(*lay.geoms(), tokens=lay.ow + 1)
    _lib, L = _L()
    for hw in (8, 20):                                          # 3x3 s1 p1: implicit GEMM on the 8 x 8 map, the halo tile on 20 x 20
        d = dict(cin=40, cout=64, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=1, residual=0, in_h=hw, in_w=hw, transposed=0, output_padding=0,
                 upsample=0, pad_hi=0)
        cd = _lib.MfConv2dDesc(**{k: d[k] for k, _ in _lib.MfConv2dDesc._fields_})
        gx, gy = _geom(40, 0, 40, hw, 1, h=hw), _geom(64, 0, 64, hw, 1, h=hw)
        w, b = np.zeros((64, 40, 3, 3), np.float32), np.zeros(64, np.float32)
        x, y = torch.zeros(1, hw * hw, 40, device="cuda"), torch.zeros(1, hw * hw, 64, device="cuda")
        info = (C.c_int * 11)()
        args = lambda t: (C.byref(cd), w.ctypes.data, b.ctypes.data, x.data_ptr(), None, y.data_ptr(), C.byref(gx), C.byref(gy), None, 1, t, 1, -1, None, info,
                          _lib.PRECISIONS[prec], None, None)
        _lib.check(L.mf_conv_view_forward(*args(0)))
        assert FAMILY[info[0]] == ("igemm" if hw == 8 else "halo")
        with pytest.raises(RuntimeError, match="token prefix"):
            _lib.check(L.mf_conv_view_forward(*args(5)))


# ---- d. output and residual views ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout,act,residual", [(40, 0, 1), (48, 3, 2), (20, 3, 1)])
def test_output_and_residual_views(lib_built, prec, cout, act, residual):
    """the 1 x 1 layer into channels [coff, coff + cout) of a wider buffer -- coff 0 and 8 may take the 16-byte epilogue stores, 4 and 12 take the narrow
    ones -- with the residual from channels [8, 8 + cout) of a buffer of another width: within the bound, and not one bit outside the view"""
    lay = Seq(dict(LINEAR, cout=cout, act=act, residual=residual), prec, seed=cout, sep_res=True)
    ref = lay.reference()
    for coff in (0, 8, 4, 12):
        gx, gy, gr = lay.geoms(out_cbuf=cout + 24, out_coff=coff, res_cbuf=cout + 16, res_coff=8)
        y, full, cfg = lay.run(gx, gy, gr)
        assert cfg["family"] == "igemm", cfg
        _note("igemm", prec, lay.check(y, f"cout {cout} coff {coff} {prec} {cfg}", ref=ref))
        inside = assert_poison_outside(full, gy, prec)
        assert np.array_equal(_bits(inside), _bits(_rows(y).numpy()).ravel())          # y_full's view is the y handed back


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin,residual", [(136, 0), (40, 1)])
def test_whole_buffer_view_is_mf_conv2d_forward_bit_for_bit(lib_built, prec, cin, residual):
    """coff 0, whole buffers: the view seam and mf_conv2d_forward build the same plan from the same descriptor and neither looks the tuning table up, so
    both report the cost model's configuration for M = 3 x 77 rows, and the outputs agree bit for bit (residual 1: mf_conv2d_forward adds the layer's
    input, the view seam is given the same tensor in a buffer of its own)"""
    from test_conv_configs import Layer
    d = dict(LINEAR, cin=cin, cout=40, act=3, residual=residual)
    ref = Layer(d, prec, seed=cin)
    try:
        assert not ref.rc, ref.err
        lay = Seq(d, prec, seed=cin, weights=(ref.w[None], ref.b[None]))
        if residual:
            lay.res = lay.x.clone()
        gx, gy, gr = lay.geoms()
        y, full, cfg = lay.run(gx, gy, gr)
        _note("igemm", prec, lay.check(y, f"whole buffer cin {cin} {prec} {cfg}"))
        assert_poison_outside(full, gy, prec)
        cfg2 = ref.config(BATCH)
        assert cfg2 == cfg, (cfg, cfg2)
        y2, _ = ref.forward(lay.x.cuda())
        assert np.array_equal(_bits(y2.cpu().numpy()), _bits(y.numpy()))
    finally:
        ref.close()


# ---- e. grouped positional convolution ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K", POS_K)
@pytest.mark.parametrize("G,gc", POS_GROUPS)
def test_grouped_positional_conv(lib_built, prec, G, gc, K):
    """wav2vec2's positional convolution as mf_wav2vec2::body launches it: per channel group one (K + 1)-tap pad-K/2 layer whose input, output and residual
    are channel slices of shared buffers (the residual is the input's own slice, added after the GELU), for sequences shorter than, equal to and longer
    than the padding.  Then group 1 alone: the other groups' output channels stay poison."""
    (_, wg, b), _ = _pos_weights(G, gc, K, seed=G * 1000 + K, dtype=np.float32)
    t0 = time.time()
    for T in _pos_lengths(K):
        d = _pos_desc(gc, K, T)
        lay = Seq(d, prec, seed=K + T, batch=2, groups=G, weights=(wg, b.reshape(G, gc)))
        gx, gy, gr = lay.geoms(in_halo=K // 2)
        ref = lay.reference()
        y, full, cfg = lay.run(gx, gy, gr)
        assert cfg["family"] == "igemm", cfg
        _note("igemm", prec, lay.check(y, f"positional G {G} gc {gc} K {K} T {T} {prec} {cfg}", ref=ref))
        assert_poison_outside(full, gy, prec)
        only = 1 if G > 2 else 0
        y, full, cfg = lay.run(gx, gy, gr, only=only)
        _note("igemm", prec, lay.check(y, f"positional group {only} alone, G {G} gc {gc} K {K} T {T} {prec}", ref=ref, channels=slice(only * gc, (only + 1) * gc)))
        assert_poison_outside(full, _poison_geom(gy, only * gc, gc), prec)
        if T == K // 2:
            with pytest.raises(RuntimeError, match="halo"):
                lay.run(*lay.geoms(in_halo=K // 2 - 1))
    print(f"[positional G {G} gc {gc} K {K} {prec}] {time.time() - t0:.1f} s")


# ---- f. attention on views ---------------------------------------------------------------------------------------------------------------------------
def _attn_view(q, k, v, gq, gk, gv, go, packing, heads, prec, tq=0, tk=0):
    """-> (out [B, Tq, C] on the CPU, y_full on the CPU)"""
    _lib, L = _L()
    B = q.shape[0]
    qd, kd, vd = (t.contiguous().cuda() for t in (q, k, v))
    out = torch.full((B, go.h * go.w, go.c), float("nan"), device="cuda")
    full = torch.full((B, go.h + 2 * go.halo, go.w + 2 * go.halo, go.cbuf), float("nan"), device="cuda")
    _lib.check(L.mf_attention_view_forward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), C.byref(gq), C.byref(gk), C.byref(gv), C.byref(go),
                                           packing, B, heads, tq, tk, _lib.PRECISIONS[prec], full.data_ptr(), None), "attention_view_forward")
    return out.cpu(), full.cpu()


def _same_bits(a, b):
    return np.array_equal(_bits(a.numpy()), _bits(b.numpy()))


FP64_GATE = {"bf16x3": 2e-4, "bf16": 8e-2}            # test_hip_attention_matches_oracle's, at _qkv inputs
HEADS = 2


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dh", [40, 64, 80, 160])
def test_packed_self_attention(lib_built, prec, dh):
    """q | k | v at channels 0, C, 2C of one buffer (row pitch 3C, and 3C + 8), sequence buffers with halo 0 and 1, the output at channel 8 of a C + 16
    buffer: bit-identical to mf_attention_forward, nothing outside the output view written"""
    from oracle import musetalk_ref as R
    Cc, T = HEADS * dh, 77
    q, k, v = _qkv(2, T, T, HEADS, dh, dh + 1)
    want = _hip_attention(q, k, v, HEADS, prec)
    err = float((want.double() - R.attention_core(q.double(), k.double(), v.double(), HEADS)).abs().max())
    print(f"[attention fp64 packed dh {dh} {prec}] L-inf {err:.3e} (gate {FP64_GATE[prec]})")
    assert err <= FP64_GATE[prec]
    for cbuf in (3 * Cc, 3 * Cc + 8):
        for halo in (0, 1):
            gq, gk, gv = (_geom(cbuf, i * Cc, Cc, T, halo) for i in range(3))
            go = _geom(Cc + 16, 8, Cc, T, halo)
            got, full = _attn_view(q, k, v, gq, gk, gv, go, 2, HEADS, prec)
            assert _same_bits(got, want), (cbuf, halo, float((got - want).abs().max()))
            assert_poison_outside(full, go, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dh", [40, 64, 80, 160])
def test_cross_attention_views(lib_built, prec, dh):
    """q at channel 8 of its own buffer, k and v at channels 16 and 16 + C of one wider buffer (the UNet's kv_all), Tk one past a key tile, the output at
    channel 8 of a third width; then k and v in buffers of their own, so that all four row pitches and batch strides differ (with k and v in one buffer
    the two share theirs: a V load addressed with K's pitch would pass there).  Bit-identical to mf_attention_forward."""
    from oracle import musetalk_ref as R
    Cc, Tq, Tk = HEADS * dh, 77, KT[dh] + 1
    q, k, v = _qkv(2, Tq, Tk, HEADS, dh, dh + 2)
    want = _hip_attention(q, k, v, HEADS, prec)
    err = float((want.double() - R.attention_core(q.double(), k.double(), v.double(), HEADS)).abs().max())
    print(f"[attention fp64 cross dh {dh} {prec}] L-inf {err:.3e} (gate {FP64_GATE[prec]})")
    assert err <= FP64_GATE[prec]
    gq, go = _geom(Cc + 8, 8, Cc, Tq, 0), _geom(Cc + 16, 8, Cc, Tq, 0)
    layouts = [(1, _geom(2 * Cc + 24, 16, Cc, Tk, 0), _geom(2 * Cc + 24, 16 + Cc, Cc, Tk, 0)),
               (0, _geom(Cc + 24, 16, Cc, Tk, 1), _geom(Cc + 32, 8, Cc, Tk, 0))]
    for packing, gk, gv in layouts:
        got, full = _attn_view(q, k, v, gq, gk, gv, go, packing, HEADS, prec)
        assert _same_bits(got, want), (packing, float((got - want).abs().max()))
        assert_poison_outside(full, go, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("dh", [40, 64, 80, 160])
def test_attention_prefixes(lib_built, prec, dh):
    """tq / tk on packed 150-token buffers.  Keys past the prefix are 50 q[0] with values of 1000: one that the kernel read would dominate every row.
    Bit-identical to mf_attention_forward on the sliced tensors; output rows >= tq stay poison."""
    Cc, T = HEADS * dh, 150
    q, k, v = _qkv(2, T, T, HEADS, dh, dh + 3)
    gq, gk, gv = (_geom(3 * Cc, i * Cc, Cc, T, 1) for i in range(3))
    go = _geom(Cc + 16, 8, Cc, T, 1)
    for tq, tk in [(20, 0), (0, 70), (20, 70), (1, 1), (150, 150)]:
        nq, nk = tq or T, tk or T
        kk, vv = k.clone(), v.clone()
        kk[:, nk:] = 50 * q[:, :1]
        vv[:, nk:] = 1000.0
        want = _hip_attention(q[:, :nq], kk[:, :nk], vv[:, :nk], HEADS, prec)
        assert float(want.abs().max()) < 100                                                   # (the reference never saw the trap)
        got, full = _attn_view(q, kk, vv, gq, gk, gv, go, 2, HEADS, prec, tq=tq, tk=tk)
        assert _same_bits(got[:, :nq], want), (tq, tk, float((got[:, :nq] - want).abs().max()))
        assert_poison_outside(full, go, prec, tokens=tq)
        assert np.all(_bits(got[:, nq:].numpy()) == _bits(POISON[prec]))


@pytest.mark.gpu
def test_attention_view_refusals(lib_built):
    q, k, v = _qkv(1, 77, 77, HEADS, 64, 0)
    g = [_geom(384, i * 128, 128, 77, 1) for i in range(3)]
    go = _geom(128, 0, 128, 77, 1)
    with pytest.raises(RuntimeError, match="prefix"):
        _attn_view(q, k, v, *g, go, 2, HEADS, "bf16x3", tq=78)
    with pytest.raises(RuntimeError, match="prefix"):
        _attn_view(q, k, v, *g, go, 2, HEADS, "bf16x3", tk=78)
    g2 = [_geom(384, i * 128, 128, 11, 1, h=7) for i in range(3)]                                # a 7 x 11 map with a halo: rows are not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        _attn_view(q, k, v, *g2, _geom(128, 0, 128, 11, 1, h=7), 2, HEADS, "bf16x3")
    with pytest.raises(RuntimeError, match="same one"):
        _attn_view(q, k, v, g[0], g[1], _geom(392, 256, 128, 77, 1), go, 2, HEADS, "bf16x3")


@pytest.mark.gpu
def test_attention_views_on_the_wide_query_tile(lib_built):
    """8 x 8 heads x 1024 queries of head dim 40: 64 groups x 8 tiles of 128 queries >= 512, launch_qb's rule for 32 queries per wave (QB = 2).  q in a
    buffer of its own, k and v sharing one; both precisions, bit-identical to mf_attention_forward."""
    B, heads, dh, Tq, Tk = 8, 8, 40, 1024, 129
    assert B * heads * ((Tq + 127) // 128) >= 512
    Cc = heads * dh
    q, k, v = _qkv(B, Tq, Tk, heads, dh, 9)
    gq, go = _geom(Cc + 8, 8, Cc, Tq, 1), _geom(Cc + 16, 8, Cc, Tq, 0)
    gk, gv = _geom(2 * Cc + 24, 16, Cc, Tk, 1), _geom(2 * Cc + 24, 16 + Cc, Cc, Tk, 1)
    for prec in PRECS:
        want = _hip_attention(q, k, v, heads, prec)
        got, full = _attn_view(q, k, v, gq, gk, gv, go, 1, heads, prec)
        assert _same_bits(got, want), (prec, float((got - want).abs().max()))
        assert_poison_outside(full, go, prec)
