"""Fused attention kernel (mf_attn.hip) vs the oracle's attention core, through the C ABI.

The oracle core is oracle/musetalk_ref.py::attention_core (softmax(q k^T / sqrt(dh)) v per head, the arithmetic of the
diffusers Attention that musetalk/models/unet.py:36-47 instantiates and of whisper/model.py:82-93)."""
import ctypes as C

import numpy as np
import pytest
import torch

from nn_numerics import _one_hot_qkv, _qkv
from oracle import musetalk_ref as R


def test_oracle_attention_core_matches_dense_softmax():
    q, k, v = _qkv(2, 5, 7, 2, 8, 0)
    got = R.attention_core(q, k, v, 2)
    qh = q.view(2, 5, 2, 8).permute(0, 2, 1, 3).double()
    kh = k.view(2, 7, 2, 8).permute(0, 2, 1, 3).double()
    vh = v.view(2, 7, 2, 8).permute(0, 2, 1, 3).double()
    w = torch.softmax(qh @ kh.transpose(-1, -2) / np.sqrt(8.0), -1)
    want = (w @ vh).permute(0, 2, 1, 3).reshape(2, 5, 16)
    assert (got.double() - want).abs().max() < 1e-6


def _hip_attention(q, k, v, heads, precision):
    from mere_fusion_amd import _lib
    L = _lib.lib()
    _lib.init_device(0)
    b, tq, c = q.shape
    tk = k.shape[1]
    qd, kd, vd = (t.contiguous().cuda() for t in (q, k, v))
    out = torch.empty(b, tq, c, device="cuda")
    _lib.check(L.mf_attention_forward(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), b, tq, tk, heads, c // heads,
                                      _lib.PRECISIONS[precision], None))
    return out.cpu()


# (batch, tq, tk, heads, dh): the UNet's self / cross shapes, Whisper's, ragged tails, fewer queries than one wave
CASES = [
    (2, 1024, 1024, 8, 40), (2, 1024, 50, 8, 40), (2, 256, 256, 8, 80), (2, 256, 50, 8, 80),
    (2, 64, 64, 8, 160), (2, 64, 50, 8, 160), (1, 16, 16, 8, 160), (1, 16, 50, 8, 160),
    (1, 1500, 1500, 6, 64), (1, 100, 37, 2, 40), (3, 70, 129, 1, 80), (1, 1, 1, 1, 64), (8, 1024, 1024, 8, 40),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_q%d_k%d_h%d_d%d" % c)
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_hip_attention_matches_oracle(lib_built, case, precision):
    b, tq, tk, heads, dh = case
    q, k, v = _qkv(b, tq, tk, heads, dh, tq * 7 + tk)
    want = R.attention_core(q, k, v, heads)
    got = _hip_attention(q, k, v, heads, precision)
    err = (got - want).abs().max().item()
    # outputs are convex combinations of v (|v| <~ 8): x3 carries ~16 mantissa bits end to end, bf16 8
    tol = 2e-4 if precision == "bf16x3" else 8e-2
    assert err <= tol, f"L_inf {err:.3e} > {tol}"


@pytest.mark.gpu
def test_hip_attention_rejects_unsupported_head_dim(lib_built):
    q, k, v = _qkv(1, 8, 8, 1, 24, 0)
    with pytest.raises(RuntimeError, match="head_dim"):
        _hip_attention(q, k, v, 1, "bf16x3")


# ---- softmax edge cases: where an online softmax goes wrong and randn inputs never look ----
# The kernel walks the keys in tiles of KT (64 for head dims 40 / 64 / 80, 32 for 160) with a running max, an exp2 rescale of the accumulator (alpha) when a later
# tile raises the max, and masking of the keys past Tk in the last tile.  The bounds below are the representation error of v: the (hi, lo) pair carries ~16 bits
# (bf16x3), one bf16 8.
KT = {40: 64, 64: 64, 80: 64, 160: 32}
REPR = {"bf16x3": 2.0 ** -16, "bf16": 2.0 ** -8}
EDGE_CASES = [(dh, tk) for dh in (40, 64, 80, 160) for tk in (KT[dh] - 1, KT[dh], KT[dh] + 1, 2 * KT[dh] + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dh,tk", EDGE_CASES, ids=lambda x: str(x))
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_hip_attention_one_hot_rows_return_the_hot_value(lib_built, dh, tk, precision):
    """Every query row has one key >= ~190 logit units above all others, at key 0, at the first key after a tile boundary or at the last valid key of a partial
    last tile (rows of one workgroup point at different ones): the output is that key's v row to within the representation error of v.  A kernel that does not
    rescale its accumulator when a later tile raises the row max, or that lets a masked key in, fails here by O(|v|).  77 queries: a ragged query tile."""
    heads, tq = 2, 77
    hot = sorted({0, min(KT[dh], tk - 1), tk - 1})
    q, k, v, want = _one_hot_qkv(2, tq, tk, heads, dh, hot, seed=dh + tk)
    got = _hip_attention(q, k, v, heads, precision)
    rel = float(((got - want).abs() / want.abs().clamp_min(1e-6)).max())
    print(f"[one-hot dh {dh} tk {tk} hot {hot} {precision}] max relative error vs the hot v row {rel:.2e} (bound {REPR[precision]:.2e})")
    assert rel <= REPR[precision], rel


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_hip_attention_one_hot_rows_on_the_wide_query_tiles(lib_built, precision):
    """The same on 8 x 8 heads x 1024 queries: the launch takes 32 queries per wave (QB = 2) there, 16 in the cases above."""
    q, k, v, want = _one_hot_qkv(8, 1024, 129, 8, 40, [0, 64, 128], seed=5)
    got = _hip_attention(q, k, v, 8, precision)
    rel = float(((got - want).abs() / want.abs().clamp_min(1e-6)).max())
    print(f"[one-hot wide tiles {precision}] max relative error {rel:.2e}")
    assert rel <= REPR[precision], rel


@pytest.mark.gpu
@pytest.mark.parametrize("dh,tk", EDGE_CASES, ids=lambda x: str(x))
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_hip_attention_uniform_rows_and_tile_edges(lib_built, dh, tk, precision):
    """q = 0: every logit is 0 and the output is the mean of the tk valid v rows (a masked key counted, or one dropped, moves it by ~max|v| / tk).  Then randn
    inputs at the same key counts against the fp64 attention core, with the gates of test_hip_attention_matches_oracle."""
    heads, tq = 2, 77
    g = torch.Generator().manual_seed(dh * 3 + tk)
    v = torch.randn(2, tk, heads * dh, generator=g) * 2 + 0.5
    k = torch.randn(2, tk, heads * dh, generator=g)
    got = _hip_attention(torch.zeros(2, tq, heads * dh), k, v, heads, precision)
    want = v.double().mean(1, keepdim=True).expand(2, tq, heads * dh)
    err = float((got.double() - want).abs().max() / v.abs().max())
    print(f"[uniform dh {dh} tk {tk} {precision}] L-inf / max|v| {err:.2e} (bound {REPR[precision]:.2e})")
    assert err <= REPR[precision], err
    q, k, v = _qkv(2, tq, tk, heads, dh, dh + tk)
    want = R.attention_core(q.double(), k.double(), v.double(), heads)
    err = float((_hip_attention(q, k, v, heads, precision).double() - want).abs().max())
    assert err <= (2e-4 if precision == "bf16x3" else 8e-2), err


# Temperature sweep: q and k scaled so that the largest |logit| (q.k / sqrt(dh)) is about 8, 24 and 64 -- trained attention is this peaked, randn inputs
# (largest logit ~4) are not.  L-inf relative to max|v| against the fp64 core.  Gates at ~3 x the first MI355X measurement (worst of the four shapes), bf16x3
# never above the 1e-3 bound: bf16x3 5.5e-6 / 1.4e-5 / 4.4e-5 at 8 / 24 / 64, bf16 3.7e-3 / 7.9e-3 / 2.9e-2 -- the error grows with the logit range (an error
# of the logits themselves moves the weights by that much), nothing jumps.  The one-hot and uniform rows above measured at most 7.6e-6 relative (bf16x3).
TEMP_GATES = {("bf16x3", 8): 2e-5, ("bf16x3", 24): 5e-5, ("bf16x3", 64): 1.5e-4, ("bf16", 8): 1.2e-2, ("bf16", 24): 2.5e-2, ("bf16", 64): 9e-2}


@pytest.mark.gpu
@pytest.mark.parametrize("dh,tk", [(40, 1024), (80, 50), (160, 129), (64, 1500)])
@pytest.mark.parametrize("temp", [8, 24, 64])
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_hip_attention_temperature_sweep(lib_built, dh, tk, temp, precision):
    heads, tq = 2, 200
    q, k, v = _qkv(1, tq, tk, heads, dh, 3 * dh + tk)
    qh, kh = q.double().view(1, tq, heads, dh).transpose(1, 2), k.double().view(1, tk, heads, dh).transpose(1, 2)
    s = (temp / float((qh @ kh.transpose(-1, -2)).abs().max() * dh ** -0.5)) ** 0.5
    q, k = (q * s).float(), (k * s).float()
    want = R.attention_core(q.double(), k.double(), v.double(), heads)
    got = _hip_attention(q, k, v, heads, precision)
    err = float((got.double() - want).abs().max() / v.abs().max())
    print(f"[temperature {temp} dh {dh} tk {tk} {precision}] L-inf / max|v| {err:.2e} (gate {TEMP_GATES[(precision, temp)]:.1e})")
    assert err <= TEMP_GATES[(precision, temp)], err
