"""float64 references, storage-format emulation and error bounds shared by the token-sequence op tests (test_nn_ops.py, test_attention.py).

- split / join: the exact (hi, lo) round-to-nearest-even bf16 planes of an fp32 value and the fp32 a kernel reads back (k_rows_from_f32 / k_rows_to_f32).
- layernorm64, softmax64, groupnorm64 (+ statistics and the per-channel affine), gemm_bt64, attention64, post_u8_64 / post_u8_f32: plain float64 (and, for
  the uint8 tail, the fp32 expression of the kernel in the kernel's order).  test_nn_ops.py pins them to torch.nn.functional on the CPU.
- *_bound: |got - want| allowed per element.  Every GPU comparison evaluates the reference on the values the planes hold (stored(x)), so a bound has two
  parts: the representation of the RESULT (REPR: 2^-16 relative for a (hi, lo) pair, 2^-8 for one bf16 plane) and the fp32 arithmetic in between, whose form
  follows the kernel and whose constant K is measured (3 x the worst first measurement on an MI355X, written beside each gate in test_nn_ops.py).
- _qkv, _one_hot_qkv: the attention input builders of test_attention.py, shared with the composite-attention cases.
"""
import math

import numpy as np
import torch

from conv_numerics import F32, bf16_rne, conv_bound, gelu64

REPR = {"bf16x3": 2.0 ** -16, "bf16": 2.0 ** -8}
POISON = {"bf16x3": np.float32(-1231.375), "bf16": np.float32(-1232.0)}      # MF_NN_POISON_* of include/merefusion.h
TINY = 1e-37                                                                 # results below fp32's normal range may flush to zero


# ---- storage --------------------------------------------------------------------------------------------------------------------------------------
def split(x, prec):
    """fp32 x -> (hi, lo) planes as fp32 arrays: hi = rne_bf16(x), lo = rne_bf16(x - hi) with the subtraction in fp32 (bf16: lo is None)"""
    x = np.ascontiguousarray(x, np.float32)
    hi = bf16_rne(x)
    return hi, (bf16_rne(x - hi) if prec == "bf16x3" else None)


def join(hi, lo):
    """what a kernel's load gives: hi + lo in fp32"""
    return hi if lo is None else (hi + lo).astype(np.float32)


def stored(x, prec):
    return join(*split(x, prec))


def stored_t(x, prec):
    """torch fp32 tensor -> the values its planes hold (fp32 tensor)"""
    return torch.from_numpy(stored(x.detach().cpu().numpy(), prec).copy()).reshape(x.shape)


# ---- float64 references ------------------------------------------------------------------------------------------------------------------------------
def layernorm64(x, gamma, beta, eps, act=0):
    """x [..., C] -> (y, pre, sigma): y = act(pre), pre = (x - mean) / sqrt(var + eps) * gamma + beta (biased variance), sigma = sqrt(var + eps) [..., 1]"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    sigma = torch.sqrt(var + eps)
    pre = (x - mean) / sigma * gamma + beta
    return (gelu64(pre) if act == 3 else pre), pre, sigma


def softmax64(s, scale, n_keys):
    """s [..., >= n_keys] -> (p [..., n_keys], scaled logits)"""
    z = s.double()[..., :n_keys] * float(np.float32(scale))
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True), z


def gn_stats64(x, groups):
    """x [B, T, C] -> float64 [B, groups, 2]: (sum, sum of squares) over (T x C/groups)"""
    B, T, C = x.shape
    g = x.double().view(B, T, groups, C // groups)
    return torch.stack([g.sum((1, 3)), (g * g).sum((1, 3))], -1)


def groupnorm64(x, gamma, beta, groups, eps, silu):
    """x [B, T, C] (channels last) -> (y, pre, R [B, 1, C], scale [B, C], shift [B, C]): R = |group mean| / sqrt(var + eps) per channel's group,
    pre = x * scale + shift the normalised value before the optional SiLU"""
    B, T, C = x.shape
    cpg = C // groups
    st = gn_stats64(x, groups)
    n = T * cpg
    mean = st[..., 0] / n
    var = (st[..., 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)          # [B, C]
    scale = rstd_c * gamma.double()
    shift = beta.double() - mean_c * scale
    pre = x.double() * scale[:, None] + shift[:, None]
    y = pre * torch.sigmoid(pre) if silu else pre
    return y, pre, (mean_c.abs() * rstd_c)[:, None], scale, shift


def gemm_bt64(a, b):
    return a.double() @ b.double().transpose(-1, -2)


def attention64(q, k, v, heads):
    """softmax(q k^T / sqrt(dh)) v per head on [B, T, heads * dh] -> (out, largest |logit|)"""
    B, tq, C = q.shape
    dh = C // heads
    h = lambda t: t.double().view(B, t.shape[1], heads, dh).transpose(1, 2)
    z = h(q) @ h(k).transpose(-1, -2) / math.sqrt(dh)
    out = torch.softmax(z, -1) @ h(v)
    return out.transpose(1, 2).reshape(B, tq, C), float(z.abs().max())


def post_u8_f32(x):
    """k_vae_post in numpy fp32, operation by operation: x / 2 + 0.5, clamp, * 255, round half to even; x [..., 3] RGB -> uint8 [..., 3] BGR"""
    x = np.asarray(x, np.float32)
    v = x / np.float32(2) + np.float32(0.5)
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(1))
    return np.rint(v * np.float32(255)).astype(np.uint8)[..., ::-1]


def post_u8_64(x):
    """the same in float64 -> (uint8 BGR, distance of 255 v from the nearest rounding boundary k + 1/2)"""
    v = np.clip(np.asarray(x, np.float64) / 2 + 0.5, 0.0, 1.0) * 255.0
    return np.rint(v).astype(np.uint8)[..., ::-1], np.abs(v - np.floor(v) - 0.5)[..., ::-1]


# ---- bounds (per element, K = 1 unless given; see the module docstring) ----------------------------------------------------------------------------
LIP = {0: 1.0, 3: 1.13}          # Lipschitz constants of the epilogue: none, GELU (conv_numerics.LIPSCHITZ)


def _act_terms(pre, y, act, prec, lip):
    # the last fp32 operation rounds relative to its result; GELU / SiLU: erff / __expf + v_rcp to a few ulp and the fp32 products (conv_numerics.conv_bound)
    return lip * 2 * F32 * pre.abs() + (8 * F32 * pre.abs() if act else 0.0) + REPR[prec] * y.abs() + TINY


def layernorm_terms(x, gamma, y, pre, sigma, act, prec):
    """(unit, rest): |got - want| <= K * unit + rest.  unit = 2^-24 (1 + max|x| / sigma_token) |gamma_c|: the fp32 mean and the centred values carry
    2^-24 max|x| absolute, divided by sigma; the variance and rsqrt a few 2^-24 relative on values of size |x - mean| / sigma <= max|x| / sigma."""
    unit = LIP[act] * F32 * (1.0 + x.double().abs().amax(-1, keepdim=True) / sigma) * gamma.double().abs()
    return unit, _act_terms(pre, y, act, prec, LIP[act])


def groupnorm_terms(gamma, y, pre, R, silu, prec):
    """unit = 2^-24 (1 + R^2) |gamma_c|: the variance is E[x^2] - mean^2 from fp32 per-thread partial sums, so its relative error is 2^-24 (1 + R^2)
    (cancellation against mean^2), and it scales the normalised value.  SiLU's Lipschitz constant is 1.1."""
    lip = 1.13 if silu else 1.0
    unit = lip * F32 * (1.0 + R * R) * gamma.double().abs()
    return unit, _act_terms(pre, y, 4 if silu else 0, prec, lip)


def softmax_terms(p, z, prec):
    """unit = 2^-24 (1 + max|logit|) p: exp's argument z - max rounds to 2^-24 |z - max| <= 2^-23 max|z| absolute, which is relative in p"""
    unit = F32 * (1.0 + z.abs().amax(-1, keepdim=True)) * p
    return unit, REPR[prec] * p + TINY


def gemm_bound(a, b, want, prec):
    """conv_numerics.conv_bound of the 1 x 1 convolution with these operand magnitudes"""
    d = {"kh": 1, "kw": 1, "stride_h": 1, "stride_w": 1, "act": 0}
    mag = {"pre": gemm_bt64(a.abs(), b.abs()), "res": torch.zeros((), dtype=torch.float64)}
    return conv_bound(want, mag, d, prec, a.shape[-1])


def attention_unit(zmax, vmax, prec):
    """The composite attention's error against float64 for logits up to zmax and |v| <= vmax, K = 1: the scores go through the planes (REPR relative, so
    delta = REPR zmax absolute on a logit, every weight off by a factor within e^(+-2 delta)), then the weights and the output do (REPR each)."""
    delta = REPR[prec] * zmax
    return (math.expm1(2 * delta) + 2 * REPR[prec]) * vmax


# ---- attention inputs (test_attention.py, test_nn_ops.py) ----------------------------------------------------------------------------------------------
def _qkv(b, tq, tk, heads, dh, seed):
    g = torch.Generator().manual_seed(seed)
    c = heads * dh
    # non-symmetric, per-channel scaled inputs: an operand transpose or a head / channel mix-up changes the answer
    ramp = torch.linspace(0.5, 1.5, c)
    q = torch.randn(b, tq, c, generator=g) * ramp
    k = torch.randn(b, tk, c, generator=g) * ramp.flip(0)
    v = torch.randn(b, tk, c, generator=g) + torch.arange(c) * 0.01
    return q, k, v


def _one_hot_qkv(b, tq, tk, heads, dh, hot_keys, seed, margin=200.0):
    """q, k, v and, per (batch, query, head), the key whose logit (q.k / sqrt(dh)) sits >= `margin` - ~10 above every other key's.  Hot key i of `hot_keys` is
    A e_i in its head; the other keys are N(0, 1) in the head dims >= len(hot_keys) (orthogonal to every hot key); query r of head h points at hot key
    (r + h) % len(hot_keys), with N(0, 1) noise in the same dims as the ordinary keys."""
    g = torch.Generator().manual_seed(seed)
    n = len(hot_keys)
    amp = (margin * dh ** 0.5) ** 0.5
    k = torch.randn(b, tk, heads, dh, generator=g)
    k[..., :n] = 0
    q = torch.randn(b, tq, heads, dh, generator=g)
    q[..., :n] = 0
    pick = (torch.arange(tq)[:, None] + torch.arange(heads)[None, :]) % n            # [tq, heads]
    for i, key in enumerate(hot_keys):
        k[:, key] = 0
        k[:, key, :, i] = amp
    q.scatter_(-1, pick[None, :, :, None].expand(b, tq, heads, 1), amp)
    v = torch.randn(b, tk, heads, dh, generator=g) * 2 + torch.linspace(-1, 1, dh)
    want = torch.stack([v[:, hot_keys[int(pick[r, h])], h] for r in range(tq) for h in range(heads)], 1).reshape(b, tq, heads, dh)
    return q.reshape(b, tq, -1), k.reshape(b, tk, -1), v.reshape(b, tk, -1), want.reshape(b, tq, -1)
