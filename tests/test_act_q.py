"""The producers of the MF_PREC_F16Q activation format (csrc/mf_aux.hip), byte for byte against the host model tests/act_q_ref.py, through the C-ABI seam
mf_act_q_encode (csrc/mf_nn_api.hip):

  mode 0   k_nchw_to_act_q            the conv seam's software encoder
  mode 1   k_affine_silu_to_q         per-thread parameters, maps that are not a multiple of 64 pixels (hardware FP6 conversions)
           k_affine_silu_to_q_u       wave-uniform parameters, what the VAE decoder runs (plain and XCD-ordered wave walk)
  mode 2   k_affine_silu_to_q_u<GN>   GroupNorm affine formed in the kernel        mode 3   mf_groupnorm_affine + the array form

The CPU tests pin the model to the OCP MX definition of FP6 E2M3 and to the emulation the format study used.  The GPU tests use one content for every
shape (`content`): random values with per-channel scales over four decades plus hand-built edge blocks whose values the (hi, lo) bf16 planes hold exactly.

The fp32 evaluation allowance `d` of the SiLU chain t = fma(x, scale, shift); y = post * t * rcp(1 + exp(-t)), per element, in units of 2^-24 (`silu_allowance`):
  fma               one rounding, 1/2 ulp of t; SiLU's Lipschitz constant is 1.1                              1.1 |t|
  __expf(-t)        v_exp_f32 of fl(-t * log2 e): the product's rounding and the constant's move the argument by 1.5 * 2^-24 |t| log2 e, which is
                    1.5 * 2^-24 |t| relative in e^-t; the instruction is documented to 1 ulp (2^-23)              (2 + 1.5 |t|) |y|
  1 + e             one rounding; the error of e enters 1 + e scaled by e / (1 + e) <= 1                         1 |y|
  v_rcp_f32         documented to 1 ulp                                                                          2 |y|
  t * rcp           one rounding (the product with the power of two `post` is exact)                            1 |y|
so d = 2^-24 |post| (1.1 |t| + (6 + 1.5 |t|) |y|) -- at most 30 * 2^-24 |y| + 1.1 * 2^-24 |t| for |t| <= 16.  The GroupNorm routes add the term of
nn_numerics.groupnorm_terms with the K_GN test_nn_ops.py holds the same scale / shift computation to."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import act_q_ref as Q
import conv_numerics as CN
import nn_numerics as N
from conftest import ROOT

E2M3_VALUES = [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
               2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5]          # OCP MX v1.0, table of FP6 E2M3 magnitudes


# ---- CPU: the model ----------------------------------------------------------------------------------------------------------------------------------
def test_decode_table():
    codes = np.arange(64)
    want = np.float64(E2M3_VALUES + [-v for v in E2M3_VALUES])
    assert np.array_equal(Q.dec_e2m3(codes), want)
    assert Q.dec_e2m3(0) == 0 and Q.dec_e2m3(0x20) == 0 and np.signbit(Q.dec_e2m3(0x20)) and not np.signbit(Q.dec_e2m3(0))


def test_round_trip_of_every_code():
    codes = np.arange(64, dtype=np.uint8)
    assert np.array_equal(Q.enc_e2m3(Q.dec_e2m3(codes)), codes)
    assert Q.enc_e2m3(0.0) == 0 and Q.enc_e2m3(-0.0) == 0x20


def test_midpoints_round_to_the_even_code_and_the_top_saturates():
    v = np.float64(E2M3_VALUES)
    mid = (v[:-1] + v[1:]) / 2
    even = np.where(np.arange(31) % 2 == 0, np.arange(31), np.arange(31) + 1)       # of the neighbours k, k + 1 the one with a zero last bit
    assert np.array_equal(Q.enc_e2m3(mid), even)
    assert np.array_equal(Q.enc_e2m3(-mid), even | 0x20)
    eps = 2.0 ** -30
    assert np.array_equal(Q.enc_e2m3(mid - eps), np.arange(31)) and np.array_equal(Q.enc_e2m3(mid + eps), np.arange(31) + 1)
    top = np.float64([7.5 + eps, 7.75, 7.75 + eps, 7.9999, np.nextafter(8.0, 0), 8.0, 100.0])
    assert np.all(Q.enc_e2m3(top) == 31) and np.all(Q.enc_e2m3(-top) == 63)


def test_packing_round_trips_and_straddles_words():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 64, (1000, 32), dtype=np.uint8)
    b = Q.pack6(codes)
    assert b.shape == (1000, 24) and b.dtype == np.uint8
    assert np.array_equal(Q.unpack6(b), codes)
    words = b.view("<u4").astype(np.uint64)                                         # [1000, 6]
    straddlers = [t for t in range(32) if (6 * t) % 32 > 26]
    assert straddlers == [5, 10, 21, 26]
    for row in range(8):
        whole = sum(int(words[row, j]) << (32 * j) for j in range(6))              # (python ints: 192 bits)
        assert [(whole >> (6 * t)) & 63 for t in range(32)] == codes[row].tolist()
    for t in straddlers:                                                             # the two words of a straddling code, each side alone
        sh = (6 * t) % 32
        assert np.array_equal((words[:, 6 * t // 32] >> sh) | ((words[:, 6 * t // 32 + 1] << (32 - sh)) & 63), codes[:, t])
    one = np.zeros((1, 32), np.uint8)
    one[0, 5] = 0x3F                                                                 # bits 30 .. 35: two in word 0, four in word 1
    w = Q.pack6(one).view("<u4")[0]
    assert w[0] == 0xC0000000 and w[1] == 0x0000000F and not w[2:].any()


def test_scale_rule():
    for k in (-20, -3, 0, 5, 14):
        m = np.float32(4 * 2.0 ** k)
        below = np.nextafter(m, np.float32(0))
        sb, sb_below = int(Q.block_scale(m)), int(Q.block_scale(below))
        assert sb == 127 + k and sb_below == sb - 1                                  # 4 * 2^k / 2^k = 4: the lower edge of the top binade
        assert float(m) / Q.scale_value(sb) == 4.0 and 7.99 < float(below) / Q.scale_value(sb_below) < 8.0
    assert int(Q.block_scale(np.float32(0))) == 0 and int(Q.block_scale(np.float32(1e-45))) == 0
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((4096, 32)) * 10.0 ** rng.uniform(-6, 4, (4096, 1))).astype(np.float32)
    m = np.abs(v).max(-1)
    top = m.astype(np.float64) / Q.scale_value(Q.block_scale(m))
    assert np.all((top >= 4) & (top < 8))
    half = Q.encode_half(v)
    assert np.array_equal(half[:, 24], Q.block_scale(m)) and not half[:, 25:].any()
    assert np.all(np.abs(Q.dec_e2m3(Q.unpack6(half[:, :24]))).max(-1) >= 4)


def test_model_agrees_with_the_format_study_emulation():
    """tools/numerics_split_study.py q_f6 (the emulation tests/test_numerics_formats.py runs) and the model decode to the same values"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import numerics_split_study as S
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((2048, 32)) * 10.0 ** rng.uniform(-3, 3, (2048, 32))).astype(np.float32)
    half = Q.encode_half(v)
    mine = Q.dec_e2m3(Q.unpack6(half[:, :24])) * Q.scale_value(half[:, 24])[:, None]
    theirs = S.q_f6(torch.from_numpy(v).double(), 1).numpy()
    assert np.array_equal(mine, theirs)
    h, r = Q.split_f16(v)
    hi, lo = Q.encode_block(v)
    dh, r_hat, h_hat, sl, sh = Q.decode_planes(hi, lo)
    assert np.array_equal(dh, h.astype(np.float64))
    assert np.array_equal(r_hat, S.q_f6(torch.from_numpy(r).double(), 1).numpy()) and np.array_equal(h_hat, S.q_f6(torch.from_numpy(h.astype(np.float64)), 1).numpy())
    assert np.array_equal(h.astype(np.float32) + r, v)                               # the split loses nothing


# ---- the content of every GPU case -------------------------------------------------------------------------------------------------------------------
def stored_t(x):
    """conv_numerics.stored(x, "bf16x3") as torch casts (both round to nearest even)"""
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def edge_blocks():
    """[n, 32] fp32 blocks built as v = h + r: h an f16 value 2^e (1 + m / 16), r = k * 2^(e - 19) with |k| <= 255 -- below half an f16 spacing (256 units), 8
    significant bits -- so that f16(v) == h, v - h == r, and both fp32 and the (hi, lo) bf16 pair hold v exactly.  A block's residual scale is 32 units when
    its largest |k| lies in [128, 256): a scaled residual is then k / 32, and every e2m3 midpoint is an integer k."""
    rng = np.random.default_rng(7)
    blocks, names = [], []

    def hv(e, m):
        return np.ldexp(1.0 + np.asarray(m) / 16.0, e)

    def add(name, h, k, e):
        v = np.float64(h) + np.float64(k) * 2.0 ** (e - 19)
        blocks.append(v)
        names.append(name)

    m = rng.integers(1, 16, 32)
    # block maximum exactly 4 * 2^k in both halves: h = 8 in one channel, the others in [2, 4); residual maximum 128 units -> 4.0 at scale 32
    h = hv(1, m); h[3] = 8.0
    k = rng.integers(-100, 101, 32); k[3] = 0; k[9] = 128
    add("max_pow2", h, k, 1)
    # ... and one step below: h = nextafter_f16(8, 0) (11 significant bits, residual 0), residual maximum 127.5 units -> 7.97 at scale 16, saturates
    h = hv(1, m); h[3] = 8.0 * (1 - 2.0 ** -11)
    k = rng.integers(-100, 101, 32).astype(np.float64); k[3] = 0; k[9] = 127.5
    add("max_below_pow2", h, k, 1)
    # every e2m3 midpoint as a scaled residual: k / 32 in {odd / 16 below 2, odd / 8 in [2, 4), odd / 4 in [4, 7.5)}, the maximum 7.5 itself
    mids = [2 * t for t in range(1, 32, 2)] + [4 * t for t in range(17, 32, 2)] + [8 * t for t in range(17, 30, 2)] + [240]
    assert len(mids) == 32 and np.array_equal(Q.enc_e2m3(np.float64(mids[:-1]) / 32), Q.enc_e2m3(np.float64(mids[:-1]) / 32) & 0x1E)
    add("ties_pos", hv(0, m), np.float64(mids), 0)
    add("ties_neg", hv(-3, m), -np.float64(mids), -3)
    # scaled maximum in (7.75, 8): saturates at 7.5
    k = rng.integers(-120, 121, 32); k[[2, 17, 30]] = [249, -252, 255]
    add("saturate", hv(2, m), k, 2)
    add("zero", np.zeros(32), np.zeros(32), 0)
    for slot in (0, 5, 15, 16, 31):
        h = np.zeros(32); k = np.zeros(32)
        h[slot] = hv(-1, 11); k[slot] = 77 if slot % 2 else -201
        add(f"single_{slot}", h, k, -1)
    # f16-exact values: a zero residual block beside a non-zero hi block
    add("f16_exact", hv(rng.integers(-6, 7, 32), rng.integers(0, 16, 32)) * rng.choice([-1.0, 1.0], 32), np.zeros(32), 0)
    # negative values only
    k = rng.integers(-255, 256, 32)
    blocks.append(-(hv(4, m) + k * 2.0 ** (4 - 19))); names.append("negative")
    # wholly in the f16-subnormal range (6e-8 .. 6e-5): h = j * 2^-24, residuals below half of that spacing
    j = rng.integers(1, 32, 32) * 2.0 ** rng.integers(0, 6, 32)
    j[0] = 1; j[1] = 1023 - 31
    blocks.append(j * 2.0 ** -24 + rng.integers(-255, 256, 32) * 2.0 ** -33); names.append("f16_subnormal")
    # |v| up to 6e4
    k = rng.integers(-255, 256, 32)
    big = m.copy(); big[7] = 15
    blocks.append((hv(15, big) + k * 2.0 ** (15 - 19)) * rng.choice([-1.0, 1.0], 32)); names.append("large")
    v = np.stack(blocks)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "an edge value is not an fp32 value"
    assert np.array_equal(CN.stored(v32, "bf16x3"), v32), "an edge value does not survive the (hi, lo) bf16 planes"
    sub = np.abs(v32[names.index("f16_subnormal")].astype(np.float16))
    assert np.abs(v32).max() > 6e4 and np.all((sub > 0) & (sub < 2.0 ** -14)) and sub.min() == 2.0 ** -24 and sub.max() > 5.9e-5
    return v32, names


def content(B, C, H, W, seed=1234):
    """fp32 NCHW [B, C, H, W], C a multiple of 32: values the (hi, lo) bf16 planes hold exactly.  Edge block i sits at pixel 2 i (flattened over the batch), channel
    block i % (C / 32); the last one (|v| up to 6e4) at the very last pixel, last block."""
    g = torch.Generator().manual_seed(seed)
    chs = 10.0 ** (torch.rand(C, generator=g) * 4 - 2)
    x = stored_t(torch.randn(B, H, W, C, generator=g) * chs)
    e, _ = edge_blocks()
    nblk = C // 32
    xv = x.view(B * H * W, nblk, 32)
    assert 2 * len(e) <= B * H * W
    for i in range(len(e) - 1):
        xv[2 * i, i % nblk] = torch.from_numpy(e[i])
    xv[-1, -1] = torch.from_numpy(e[-1])
    return x.permute(0, 3, 1, 2).contiguous()


def test_edge_blocks_are_the_edges_they_are_built_for():
    """CPU: the model on the hand-built blocks -- exact power-of-two maxima, ties, saturation, zero halves, f16 subnormals"""
    e, names = edge_blocks()
    h, r = Q.split_f16(e)
    hi, lo = Q.encode_block(e)
    dh, r_hat, h_hat, sl, sh = Q.decode_planes(hi, lo)
    rs = r.astype(np.float64) / Q.scale_value(sl)[:, None]                            # scaled residuals
    hs = h.astype(np.float64) / Q.scale_value(sh)[:, None]
    codes_l, codes_h = Q.unpack6(lo[:, :24]), Q.unpack6(lo[:, 32:56])
    i = names.index("max_pow2")
    assert np.abs(rs[i]).max() == 4.0 and np.abs(hs[i]).max() == 4.0 and codes_l[i, 9] == 24 and codes_h[i, 3] == 24
    j = names.index("max_below_pow2")
    assert sl[j] == sl[i] - 1 and sh[j] == sh[i] - 1 and 7.96 < rs[j, 9] < 8 and 7.99 < hs[j, 3] < 8 and codes_l[j, 9] == 31 and codes_h[j, 3] == 31
    for name, sign in (("ties_pos", 0), ("ties_neg", 0x20)):
        i = names.index(name)
        mag = np.abs(rs[i, :31])
        assert np.all(Q.dec_e2m3(Q.enc_e2m3(mag - 2.0 ** -20)) != Q.dec_e2m3(Q.enc_e2m3(mag + 2.0 ** -20))), "not a midpoint"
        assert np.all(codes_l[i, :31] & 1 == 0) and np.all(codes_l[i] & 0x20 == sign) and codes_l[i, 31] & 0x1F == 31 and abs(rs[i, 31]) == 7.5
    i = names.index("saturate")
    assert np.all((np.abs(rs[i, [2, 17, 30]]) > 7.75) & (np.abs(rs[i, [2, 17, 30]]) < 8)) and np.all(codes_l[i, [2, 17, 30]] & 0x1F == 31)
    i = names.index("zero")
    assert not hi[i].any() and not lo[i].any()
    for slot in (0, 5, 15, 16, 31):
        i = names.index(f"single_{slot}")
        assert np.flatnonzero(codes_l[i]).tolist() == [slot] and np.flatnonzero(codes_h[i]).tolist() == [slot] and 4 <= abs(rs[i, slot]) < 8
    i = names.index("f16_exact")
    assert not lo[i, :32].any() and sh[i] != 0 and np.abs(Q.dec_e2m3(codes_h[i])).max() >= 4
    i = names.index("negative")
    assert np.all(e[i] < 0) and np.all(codes_h[i] & 0x20 == 0x20)
    i = names.index("f16_subnormal")
    assert np.all(np.abs(h[i].astype(np.float64)) < 2.0 ** -14) and r[i].any() and np.abs(hs[i]).max() >= 4 and sl[i] > 0
    assert np.array_equal(h.astype(np.float32) + r, e)


# ---- the seam ----------------------------------------------------------------------------------------------------------------------------------------
CASES = {   # B, C, H, W, source cbuf / coff / halo, destination halo
    "a": (1, 32, 8, 8, 32, 0, 0, 1),
    "b": (2, 96, 16, 12, 112, 8, 1, 2),
    "c": (1, 96, 7, 10, 96, 0, 1, 1),
    "d": (3, 128, 9, 9, 144, 16, 2, 1),
    "e": (3, 160, 264, 272, 160, 0, 1, 1),
}
POISON_HI, POISON_LO = 0xC49A, 0x3F20            # MF_ACT_Q_POISON_* of include/merefusion.h
UNTOUCHED = 0x5A5A                                # what the output tensors hold before a call


def _i16(v):
    return v - 0x10000 if v >= 0x8000 else v


class Out:
    pass


def encode(x, geom, dst_halo, mode, dst_c=None, silu=0, scale=None, shift=None, post=None, gamma=None, beta=None, groups=0, eps=1e-6, want_src=True, expect=0):
    """x: device fp32 [B, C, H, W]; geom (cbuf, coff, halo) of the source.  Returns the planes as int16 [B, Hp, Wp, Cd], their 64-word tails, the source buffer."""
    from mere_fusion_amd import _lib
    L = _lib.lib()
    B, Cx, H, W = x.shape
    cbuf, coff, halo = geom
    dst_c = dst_c or Cx
    g = _lib.MfRowsGeom(cbuf, coff, Cx, H, W, halo)
    Hp, Wp = H + 2 * dst_halo, W + 2 * dst_halo
    n = B * Hp * Wp * dst_c
    o = Out()
    hi = torch.full((n + 64,), _i16(UNTOUCHED), dtype=torch.int16, device="cuda")
    lo = torch.full((n + 64,), _i16(UNTOUCHED), dtype=torch.int16, device="cuda")
    ns = B * (H + 2 * halo) * (W + 2 * halo) * cbuf
    src = torch.full((ns + 64,), 7.0, device="cuda") if (want_src and mode) else None
    p = lambda t: None if t is None else t.data_ptr()
    keep = [t.contiguous() if t is not None else None for t in (x, scale, shift, post, gamma, beta)]
    rc = L.mf_act_q_encode(p(keep[0]), C.byref(g), B, dst_c, dst_halo, mode, silu, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), p(keep[5]), groups, eps,
                           hi.data_ptr(), lo.data_ptr(), p(src), None)
    torch.cuda.synchronize()
    o.rc, o.error = rc, L.mf_last_error().decode() if rc else ""
    if expect:
        assert rc == expect, (rc, o.error)
        assert bool((hi == _i16(UNTOUCHED)).all()) and bool((lo == _i16(UNTOUCHED)).all()), "a refused call wrote to its outputs"
        assert src is None or bool((src == 7.0).all())
        return o
    _lib.check(rc, "act_q_encode")
    o.hi, o.lo = hi[:n].view(B, Hp, Wp, dst_c), lo[:n].view(B, Hp, Wp, dst_c)
    o.tail_hi, o.tail_lo = hi[n:], lo[n:]
    o.halo, o.shape = dst_halo, (B, dst_c, H, W)
    o.src = None if src is None else src[:ns].view(B, H + 2 * halo, W + 2 * halo, cbuf)
    o.src_tail = None if src is None else src[ns:]
    return o


def interior(o):
    """the written view as bytes: (hi [B, H, W, nblk, 64], lo [B, H, W, nblk, 64]) device uint8"""
    B, Cd, H, W = o.shape
    h = o.halo
    cut = lambda t: t[:, h:h + H, h:h + W].contiguous().view(torch.uint8).view(B, H, W, Cd // 32, 64)
    return cut(o.hi), cut(o.lo)


def assert_nothing_outside(o, x=None, geom=None):
    """assertion 7: the destination's halo ring and tail still hold the poison; the source buffer holds x in its slice and the poison everywhere else"""
    B, Cd, H, W = o.shape
    h = o.halo
    for plane, tail, word in ((o.hi, o.tail_hi, POISON_HI), (o.lo, o.tail_lo, POISON_LO)):
        ring = plane.clone()
        ring[:, h:h + H, h:h + W] = _i16(word)
        assert bool((ring == _i16(word)).all()), "a producer wrote into the destination's halo ring"
        assert bool((tail == _i16(word)).all()), "a producer wrote past the destination's last pixel"
    if o.src is not None:
        cbuf, coff, sh = geom
        want = torch.full_like(o.src, float(N.POISON["bf16x3"]))
        want[:, sh:sh + H, sh:sh + W, coff:coff + x.shape[1]] = x.permute(0, 2, 3, 1)
        assert torch.equal(o.src.view(torch.int32), want.view(torch.int32)), "the source buffer changed (or did not hold x exactly)"
        assert bool((o.src_tail == float(N.POISON["bf16x3"])).all())


def blocks_of(v_nchw):
    """[B, C, H, W] -> numpy [B, H, W, C / 32, 32]"""
    B, Cx, H, W = v_nchw.shape
    return v_nchw.permute(0, 2, 3, 1).reshape(B, H, W, Cx // 32, 32).cpu().numpy()


def assert_bytes_equal(hi, lo, want_hi, want_lo, what):
    """both planes, byte for byte.  A half (residual or hi block) that is all zero is the one exception: its codes must be zero and its scale byte finite
    (not the E8M0 NaN 255), whatever it is -- the software encoder writes 127 there, the hardware path 0; the pad bytes are zero everywhere."""
    hi, lo, want_hi, want_lo = (np.asarray(t.cpu() if torch.is_tensor(t) else t).reshape(-1, 64) for t in (hi, lo, want_hi, want_lo))
    bad = np.flatnonzero((hi != want_hi).any(-1))
    assert bad.size == 0, f"{what}: {bad.size} blocks with wrong f16 words, first {bad[0]}: {hi[bad[0]].view(np.float16)} != {want_hi[bad[0]].view(np.float16)}"
    for half, off in (("residual", 0), ("hi", 32)):
        g, w = lo[:, off:off + 32], want_lo[:, off:off + 32]
        zero = ~(w[:, :24] & Q.pack6(np.full(32, 0x1F))).any(-1)                   # expected codes all +-0
        bad = np.flatnonzero((g != w).any(-1) & ~zero)
        assert bad.size == 0, (f"{what}: {bad.size} {half} blocks differ, first {bad[0]}: codes {Q.unpack6(g[bad[0], :24])} scale {g[bad[0], 24]} pad {g[bad[0], 25:]}"
                               f" != codes {Q.unpack6(w[bad[0], :24])} scale {w[bad[0], 24]}")
        assert not (g[zero, :24] & Q.pack6(np.full(32, 0x1F))).any() and np.all(g[zero, 24] != 255) and not g[zero, 25:].any(), f"{what}: an all-zero {half} block"
    return lo[:, 24], lo[:, 56]


def case_inputs(name):
    B, Cx, H, W, cbuf, coff, halo, dh = CASES[name]
    return content(B, Cx, H, W).cuda(), (cbuf, coff, halo), dh


def ones(B, Cx, v=1.0):
    return torch.full((B, Cx), v, device="cuda")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_identity_is_bit_exact_in_all_three_implementations(lib_built, name):
    """Assertion 1 (and 7).  Software encoder (mode 0), hardware conversions (mode 1 with scale 1, shift 0: k_affine_silu_to_q_u on a and b, k_affine_silu_to_q on
    c and d) and the model write the same bytes for the same values: f16 words, 24 code bytes, scale byte, zero pad.  An all-zero half block: scale byte 127 from
    the software path and 0 from the hardware path (asserted here), all codes zero from both.
    The f16-subnormal block needs no special case: the hardware conversions take f16 subnormals as values (no flush), as the model does."""
    x, geom, dh = case_inputs(name)
    B, Cx, H, W = x.shape
    want_hi, want_lo = Q.encode_block(blocks_of(x))
    sw = encode(x, geom, dh, 0)
    hw = encode(x, geom, dh, 1, scale=ones(B, Cx), shift=ones(B, Cx, 0.0))
    got = {}
    for tag, o in (("software", sw), ("hardware", hw)):
        assert_nothing_outside(o, x, geom)
        hi, lo = interior(o)
        got[tag] = (hi.cpu().numpy(), lo.cpu().numpy())
        sl, sh = assert_bytes_equal(hi, lo, want_hi, want_lo, f"case {name} {tag} vs model")
        zero_l = ~want_lo.reshape(-1, 64)[:, :24].any(-1)
        assert zero_l.any() and np.all(sl[zero_l] == (127 if tag == "software" else 0)), f"{tag}: scale byte of an all-zero block {set(sl[zero_l].tolist())}"
    assert_bytes_equal(*got["software"], *got["hardware"], f"case {name} software vs hardware")
    e, names = edge_blocks()
    i = names.index("f16_subnormal")
    hi, lo = (t.reshape(-1, Cx // 32, 64)[2 * i, i % (Cx // 32)] for t in got["hardware"])
    h, r_hat, h_hat, sl, sh = Q.decode_planes(hi, lo)
    print(f"[act_q {name}] f16-subnormal block: hi scale byte {sh}, largest |h| {np.abs(h).max():.3e}, decoded FP6 copy off by at most {np.abs(h_hat - h).max():.2e}, "
          f"residual scale byte {sl}; identical to the model (no flush of f16 subnormals)")


@pytest.mark.gpu
def test_software_encoder_pads_missing_channels_with_zero(lib_built):
    """Assertion 1, case f: 40 channels into a 64-channel destination (mode 0 only): channels 40 .. 63 encode as zero and take no part in block 1's maximum"""
    x = content(2, 64, 8, 8)[:, :40].contiguous().cuda()
    o = encode(x, (40, 0, 0), 1, 0, dst_c=64)
    full = torch.zeros(2, 64, 8, 8, device="cuda")
    full[:, :40] = x
    want_hi, want_lo = Q.encode_block(blocks_of(full))
    assert_bytes_equal(*interior(o), want_hi, want_lo, "case f")
    assert_nothing_outside(o)


def affine_params(B, Cx, seed):
    """scale, shift [B, C] with at most 8 significant bits, post [C] in 2^-3 .. 2^3.  |scale| < 2^-4 keeps post * (scale * 6e4 + shift) inside f16."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (B, Cx), generator=g) * 2.0 - 1
    scale = sign * (1 + torch.randint(0, 128, (B, Cx), generator=g) / 128.0) * 2.0 ** -5
    shift = torch.randint(-128, 129, (B, Cx), generator=g) / 64.0
    post = 2.0 ** torch.randint(-3, 4, (Cx,), generator=g).float()
    return scale.cuda(), shift.cuda(), post.cuda()


def affine64(x, scale, shift):
    """x * scale + shift per (sample, channel) in float64, checked to be exact there: the product has at most 32 significant bits; the sum's rounding error
    (TwoSum) is zero everywhere.  float32() of it is then what one fused multiply-add returns."""
    a = x.double().cpu().numpy() * scale.double().cpu().numpy()[:, :, None, None]
    b = np.broadcast_to(shift.double().cpu().numpy()[:, :, None, None], a.shape)
    s = a + b
    bb = s - a
    assert not ((a - (s - bb)) + (b - bb)).any(), "the float64 affine is not exact"
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("name,with_post", [("b", False), ("b", True), ("c", False), ("c", True)])
def test_affine_and_post_are_bit_exact(lib_built, name, with_post):
    """Assertion 2 (and 7): v = fma(x, scale, shift) [* post] without SiLU is one rounding of an exact float64 expression, so the bytes are the model's of
    float32(x * scale + shift) * post -- on k_affine_silu_to_q_u (b) and on the fallback (c), whose `v * sck + shk` must contract to the same single fma."""
    x, geom, dh = case_inputs(name)
    B, Cx, H, W = x.shape
    scale, shift, post = affine_params(B, Cx, 11)
    v = torch.from_numpy(affine64(x, scale, shift).astype(np.float32))
    if with_post:
        v = v * post.cpu()[None, :, None, None]
    assert float(v.abs().max()) < 65504
    o = encode(x, geom, dh, 1, scale=scale, shift=shift, post=post if with_post else None)
    want_hi, want_lo = Q.encode_block(blocks_of(v))
    assert_bytes_equal(*interior(o), want_hi, want_lo, f"case {name} affine post={with_post}")
    assert_nothing_outside(o, x, geom)


@pytest.mark.gpu
@pytest.mark.parametrize("with_post", [False, True])
def test_fallback_and_uniform_kernel_agree_bit_for_bit_with_silu(lib_built, with_post):
    """Assertion 3: case b's first 64 pixel vectors as an 8 x 8 map (k_affine_silu_to_q_u) and as the first 64 pixels of a 7 x 10 map (k_affine_silu_to_q), same
    per-channel parameters, SiLU on: the bytes of those pixels are identical -- the contraction choices of the two kernels (default against contract(off)) agree."""
    xb, geom, dh = case_inputs("b")
    Cx = xb.shape[1]
    px = xb[0].reshape(Cx, -1)                                                       # [C, 192], pixels row-major
    x_u = px[:, :64].reshape(1, Cx, 8, 8).contiguous()
    x_f = px[:, :70].reshape(1, Cx, 7, 10).contiguous()
    scale, shift, post = silu_params(x_f, 5)
    kw = dict(scale=scale, shift=shift, post=post if with_post else None, silu=1)
    u, f = encode(x_u, geom, dh, 1, **kw), encode(x_f, geom, dh, 1, **kw)
    hu, lu = (t.reshape(64, -1) for t in interior(u))
    hf, lf = (t.reshape(70, -1)[:64] for t in interior(f))
    assert torch.equal(hu, hf), "the f16 planes of the two kernels differ"
    assert torch.equal(lu, lf), "the FP6 planes of the two kernels differ"
    assert_nothing_outside(u, x_u, geom)
    assert_nothing_outside(f, x_f, geom)


def silu_params(x, seed):
    """per-(sample, channel) scale (either sign, a full fp32 mantissa: x * scale is not exact, so one fused multiply-add and a rounded product differ) and shift
    in [-2, 2] with |scale * x + shift| <= 12 * 1.125 + 2 < 16, post [C] in 2^-3 .. 2^3"""
    B, Cx = x.shape[:2]
    g = torch.Generator().manual_seed(seed)
    amax = x.abs().amax((2, 3)).cpu().clamp_min(1e-3)
    scale = 2.0 ** torch.floor(torch.log2(12.0 / amax)).clamp(max=1) * (torch.randint(0, 2, (B, Cx), generator=g) * 2.0 - 1)
    scale = scale * (1 + torch.rand(B, Cx, generator=g) / 8)
    shift = torch.rand(B, Cx, generator=g) * 4 - 2
    post = 2.0 ** torch.randint(-3, 4, (Cx,), generator=g).float()
    return scale.cuda(), shift.cuda(), post.cuda()


def silu_allowance(t, y, post):
    """d of the module docstring: t, y float64 (the pre-activation and post * silu(t)), post broadcastable"""
    return 2.0 ** -24 * (1.1 * np.abs(t) * np.abs(post) + (6 + 1.5 * np.abs(t)) * np.abs(y))


def half_step(a):
    """half the e2m3 spacing around the scaled magnitude a (in units of the block scale); past 7.5 the distance to 7.5: saturation, up to 0.5 -- a block's
    largest value stays below 8"""
    return np.where(a < 2, 0.0625, np.where(a < 4, 0.125, np.where(a <= 7.5, 0.25, np.clip(a - 7.5, 0.25, 0.5))))


def ulp_f16(v):
    """spacing of f16 at |v| (2^-24 in the subnormal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return np.exp2(e - 10)


def assert_decoded_within_bounds(o, v64, d, what):
    """Assertion 4 on the interior of `o` against v64 [B, C, H, W] float64 with the per-element allowance d; prints worst error / bound"""
    hi, lo = interior(o)
    h, r_hat, h_hat, sl, sh = Q.decode_planes(hi.cpu().numpy(), lo.cpu().numpy())
    want = blocks_of(torch.from_numpy(v64))
    d = blocks_of(torch.from_numpy(np.array(np.broadcast_to(d, v64.shape))))
    assert np.isfinite(h).all() and np.all(sl != 255) and np.all(sh != 255)
    e_h, b_h = np.abs(h - want), ulp_f16(want) / 2 + d
    s_l, s_h = Q.scale_value(sl)[..., None], Q.scale_value(sh)[..., None]
    e_v, b_v = np.abs(h + r_hat - want), half_step(np.abs(want - h) / s_l) * s_l + d
    e_q, b_q = np.abs(h_hat - h), half_step(np.abs(h) / s_h) * s_h
    print(f"[act_q {what}] worst error / bound: f16 plane {np.max(e_h / b_h):.3f}, f16 + FP6 residual {np.max(e_v / b_v):.3f}, FP6 copy of the f16 plane "
          f"{np.max(e_q / np.maximum(b_q, 1e-300)):.3f}; largest d / (FP6 half step) {np.max(d / (half_step(np.abs(want - h) / s_l) * s_l)):.3f}")
    assert np.all(e_h <= b_h), f"{what}: f16 plane off by {np.max(e_h / b_h):.3f} of the bound"
    assert np.all(e_v <= b_v), f"{what}: h + r_hat off by {np.max(e_v / b_v):.3f} of the bound"
    assert np.all(e_q <= b_q), f"{what}: FP6 copy of the f16 plane off by {np.max(e_q / np.maximum(b_q, 1e-300)):.3f} of the bound"
    # the block-maximum invariant from the bytes alone: a block with any non-zero value has a code of magnitude >= 4 (its maximum sits in the top binade)
    lob = lo.cpu().numpy()
    cl, ch = np.abs(Q.dec_e2m3(Q.unpack6(lob[..., 0:24]))), np.abs(Q.dec_e2m3(Q.unpack6(lob[..., 32:56])))
    assert np.all(cl.max(-1)[cl.any(-1)] >= 4), f"{what}: a residual block whose largest code is below 4"
    assert np.all(ch.max(-1)[(h != 0).any(-1)] >= 4), f"{what}: a hi block whose largest code is below 4"


def silu64(x, scale, shift, post):
    t = x.double().cpu().numpy() * scale.double().cpu().numpy()[:, :, None, None] + shift.double().cpu().numpy()[:, :, None, None]
    p = np.ones(x.shape[1]) if post is None else post.double().cpu().numpy()
    p = p[None, :, None, None]
    y = p * t / (1 + np.exp(-t))
    assert np.abs(t).max() <= 16
    return t, y, p


@pytest.mark.gpu
@pytest.mark.parametrize("name,with_post", [("a", True), ("b", False), ("b", True), ("c", False), ("c", True), ("d", True)])
def test_silu_against_float64(lib_built, name, with_post):
    """Assertion 4 (and 7): post * silu(scale * x + shift) decoded from the bytes against float64, within the f16 / FP6 rounding plus the fp32 allowance d"""
    x, geom, dh = case_inputs(name)
    scale, shift, post = silu_params(x, 3)
    post = post if with_post else None
    o = encode(x, geom, dh, 1, silu=1, scale=scale, shift=shift, post=post)
    t, y, p = silu64(x, scale, shift, post)
    assert_decoded_within_bounds(o, y, silu_allowance(t, y, p), f"silu case {name} post={with_post}")
    assert_nothing_outside(o, x, geom)


K_GN = 11.0         # test_nn_ops.py: the GroupNorm scale / shift computation (k_gn_stats, mf_gn_affine_pair) against nn_numerics.groupnorm_terms


def gn_inputs(name, B=None):
    _, Cx, H, W, cbuf, coff, halo, dh = CASES[name]
    B = B or CASES[name][0]
    x = content(B, Cx, H, W).clamp(-50, 50)            # (GroupNorm over a group that holds the 6e4 block would flatten everything else to zero)
    x = stored_t(x).cuda()
    g = torch.Generator().manual_seed(9)
    gamma = (torch.rand(Cx, generator=g) + 0.5) * (torch.randint(0, 2, (Cx,), generator=g) * 2.0 - 1)
    beta = torch.rand(Cx, generator=g) * 2 - 1
    post = 2.0 ** torch.randint(-3, 4, (Cx,), generator=g).float()
    return x, (cbuf, coff, halo), dh, gamma.cuda(), beta.cuda(), post.cuda()


def gn_reference(x, gamma, beta, post, groups, eps):
    B, Cx, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(B, H * W, Cx).cpu()
    y, pre, R, sc, sh = N.groupnorm64(rows, gamma.cpu(), beta.cpu(), groups, eps, True)
    unit, _ = N.groupnorm_terms(gamma.cpu(), y, pre, R, True, "bf16x3")
    nchw = lambda t: t.expand(B, H * W, Cx).reshape(B, H, W, Cx).permute(0, 3, 1, 2).numpy()
    p = post.double().cpu().numpy()[None, :, None, None]
    t, y = nchw(pre), nchw(y) * p
    return y, silu_allowance(t, y, p) + K_GN * nchw(unit) * np.abs(p), float(pre.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,groups", [("b", 2, 3), ("b", 2, 8), ("a", 2, 8)])
def test_groupnorm_routes_agree_and_match_float64(lib_built, name, B, groups):
    """Assertion 5 (and 7): the in-kernel affine (mode 2, mf_gn_affine_pair per lane) and the two-launch route (mode 3, k_gn_affine + the array form) write the
    same bytes, and both decode to float64 GroupNorm + SiLU * post within assertion 4's bounds plus the GroupNorm term.  groups = 8: 12-channel groups (C 96) or
    4-channel groups (C 32) inside a 32-channel block; groups = 3 on C 96: one group per block."""
    x, geom, dh, gamma, beta, post = gn_inputs(name, B)
    kw = dict(gamma=gamma, beta=beta, post=post, groups=groups, eps=1e-6)
    fused, two = encode(x, geom, dh, 2, **kw), encode(x, geom, dh, 3, **kw)
    assert torch.equal(fused.hi, two.hi) and torch.equal(fused.lo, two.lo), "the in-kernel affine and k_gn_affine disagree"
    y, d, tmax = gn_reference(x, gamma, beta, post, groups, 1e-6)
    assert tmax <= 16
    assert_decoded_within_bounds(fused, y, d, f"groupnorm case {name} B={B} groups={groups}")
    for o in (fused, two):
        assert_nothing_outside(o, x, geom)


@pytest.mark.gpu
def test_groupnorm_group_count_must_divide_the_channels(lib_built):
    """Assertion 5 names case a (32 channels) with 3 groups: no GroupNorm of this library (or torch) has that shape -- the call is refused and writes nothing"""
    x, geom, dh, gamma, beta, post = gn_inputs("a", 2)
    for mode in (2, 3):
        o = encode(x, geom, dh, mode, gamma=gamma, beta=beta, groups=3, expect=-1)
        assert "group count that divides C" in o.error


@pytest.mark.gpu
def test_groupnorm_on_a_ragged_map(lib_built):
    """Assertion 5, case c (70 pixels): the in-kernel affine is refused by name and nothing is written; the two-launch route runs the fallback within the bounds"""
    x, geom, dh, gamma, beta, post = gn_inputs("c")
    kw = dict(gamma=gamma, beta=beta, post=post, groups=8, eps=1e-6)
    o = encode(x, geom, dh, 2, expect=-1, **kw)
    assert "multiple of 64 pixels" in o.error
    two = encode(x, geom, dh, 3, **kw)
    y, d, tmax = gn_reference(x, gamma, beta, post, 8, 1e-6)
    assert tmax <= 16
    assert_decoded_within_bounds(two, y, d, "groupnorm case c (two launches)")
    assert_nothing_outside(two, x, geom)


@pytest.mark.gpu
def test_xcd_ordered_walk_covers_every_chunk_once(lib_built):
    """Assertion 6 (and 7), case e: one call at B = 3 (16830 waves: XCD-ordered, 3366 chunks, 3366 % 8 = 6) against three calls at B = 1 (5610 waves each: plain
    order) -- the same bytes everywhere -- and 4096 random blocks of it against the model (identity mode)."""
    x, geom, dh = case_inputs("e")
    B, Cx, H, W = x.shape
    one, zero = ones(B, Cx), ones(B, Cx, 0.0)
    whole = encode(x, geom, dh, 1, scale=one, shift=zero)
    assert_nothing_outside(whole, x, geom)
    for b in range(B):
        part = encode(x[b:b + 1].contiguous(), geom, dh, 1, scale=one[:1], shift=zero[:1], want_src=False)
        assert torch.equal(part.hi[0], whole.hi[b]) and torch.equal(part.lo[0], whole.lo[b]), f"image {b}: the XCD-ordered walk and the plain walk differ"
        del part
    hi, lo = interior(whole)
    g = torch.Generator().manual_seed(4)
    nblk = Cx // 32
    pick = torch.randint(0, B * H * W * nblk, (4096,), generator=g)
    pick[0], pick[1] = 0, B * H * W * nblk - 1
    pick = pick.cuda()
    vals = x.permute(0, 2, 3, 1).reshape(-1, 32)[pick].cpu().numpy()
    want_hi, want_lo = Q.encode_block(vals)
    assert_bytes_equal(hi.view(-1, 64)[pick], lo.view(-1, 64)[pick], want_hi, want_lo, "case e spot check")


@pytest.mark.gpu
def test_seam_refuses_bad_arguments(lib_built):
    """null pointers and bad geometry come back as MF_ERR_INVALID before anything is launched or written"""
    from mere_fusion_amd import _lib
    L = _lib.lib()
    x, geom, dh = case_inputs("a")
    s = ones(1, 32)
    encode(x, (32, 8, 0), dh, 1, scale=s, shift=s, expect=-1)                        # the slice leaves the buffer
    encode(x, (40, 4, 0), dh, 1, scale=s, shift=s, expect=-1)                        # a slice that does not start at a multiple of 8
    encode(x, geom, dh, 1, scale=s, shift=None, expect=-1)
    encode(x, geom, dh, 1, scale=s, shift=s, dst_c=64, expect=-1)                    # the producers need dst_c == C
    encode(x, geom, dh, 0, dst_c=48, expect=-1)
    encode(x, geom, dh, 4, scale=s, shift=s, expect=-1)
    encode(x, geom, dh, 2, gamma=None, beta=None, groups=8, expect=-1)
    g = _lib.MfRowsGeom(32, 0, 32, 8, 8, 0)
    assert L.mf_act_q_encode(None, C.byref(g), 1, 32, 1, 0, 0, None, None, None, None, None, 0, 0.0, None, None, None, None) == -1
    assert "null" in L.mf_last_error().decode()
