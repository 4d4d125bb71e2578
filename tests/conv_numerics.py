"""Storage-format emulation and float64 references shared by the conv tests (test_net_ops.py, test_conv_configs.py, test_seq_conv_views.py).

- U[prec]: relative rounding of one stored value; F32: fp32 unit roundoff.  `stored` / `exact` emulate the (hi, lo) bf16 planes and bf16 alone.
- conv_ref: the full mf_conv2d_desc in float64 -- Conv2d or ConvTranspose2d (output_padding), pad_hi, nearest-2x upsample, eval BatchNorm folded into the
  conv, residual before (1) or after (2) the activation, acts 0-5 (GEGLU: x[:, :c/2] * gelu(x[:, c/2:])) -- with the magnitudes an error bound needs.
  test_conv_configs.py::test_conv_ref_is_torch_nn pins it to torch.nn modules.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# relative rounding of one stored value.  bf16 keeps 8 significant bits: RNE is within half a spacing, 2^-8 |x| (reached just above a
# power of two).  hi + lo: the residual x - hi is at most half of hi's spacing, 2^(e-8) for x in [2^e, 2^(e+1)), and the lo plane rounds it
# to 8 bits, within 2^(e-17) <= 2^-17 |x|.  test_net_ops.py::test_stored_matches_the_format_rounding checks both.
U = {"bf16x3": 2.0 ** -17, "bf16": 2.0 ** -8}
F32 = 2.0 ** -24                      # fp32 unit roundoff: every op computes in fp32 between a load and a store


def bf16_rne(x):
    """fp32 -> bf16 -> fp32, round to nearest even: Pl::st's nfb() and the hardware conversion of k_nchw_to_act (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def stored(x, prec):
    """what a buffer gives back for fp32 x: hi = rne(x), lo = rne(x - hi) in fp32 (bf16x3), read as hi + lo in fp32"""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    if prec == "bf16":
        return hi
    lo = bf16_rne(x - hi)
    return hi + lo


def exact(rng, shape, prec, scale=1.0, offset=0.0):
    """random values the storage format holds exactly: stored() of an fp32 draw (hi + lo needs <= 17 significant bits, so it is an fp32 sum
    without rounding, and storing it again splits it into the same value)"""
    return stored((offset + scale * rng.standard_normal(shape)).astype(np.float32), prec)


def bn_fold(w, b, gamma, beta, mean, var, eps=1e-5):
    """eval-mode BatchNorm2d after a conv, as one conv: (w', b')"""
    sc = gamma / np.sqrt(var + eps)
    return w * sc.reshape(-1, 1, 1, 1), (b - mean) * sc + beta


# ---- the full layer in float64 ----------------------------------------------------------------------------------------------------------------
def gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def act64(t, act):
    if act == 0:
        return t
    if act == 1:
        return torch.relu(t)
    if act == 2:
        return torch.sigmoid(t)
    if act == 3:
        return gelu64(t)
    if act == 4:
        return t * torch.sigmoid(t)
    raise ValueError(act)


def max_phase_taps(d):
    """the largest number of kernel taps one output pixel sums (ConvTranspose / upsample phases: per phase); K = that x cin"""
    kh, kw = d["kh"], d["kw"]
    if d.get("upsample"):
        return 4                                    # 2 x 2 pre-summed taps per phase
    if d.get("transposed"):
        sh, sw = d["stride_h"], d["stride_w"]
        return math.ceil(kh / sh) * math.ceil(kw / sw)
    return kh * kw


def conv_ref(x, w, b, d, bn=None, res=None):
    """float64 forward of one mf_conv2d_desc `d` (dict with the desc's field names) -> (want, mag) where
         want  the layer's output,
         mag   {"pre": conv(|x|, |w'|) + |b'| (+ |r| for residual 1) of the pre-activation, "res": |r| added after the activation (residual 2) or 0,
                "v", "u": GEGLU only, the value and gate halves of the pre-activation, "mv", "mu": their magnitudes},
         r     the residual operand: `res` ([B, cout, Ho, Wo], a tensor of its own, as a network hands a layer the positional table or another branch), or x.
    x: [B, cin, H, W]; w: [cout, cin, kh, kw] (Conv2d) or [cin, cout, kh, kw] (ConvTranspose2d); b: [cout] or None; bn: (gamma, beta, mean, var) or None.
    Tensors of any device; computed in float64 there."""
    dev = x.device if torch.is_tensor(x) else "cpu"
    t = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float64, device=dev)
    x, w = t(x), t(w)
    cout = w.shape[1] if d.get("transposed") else w.shape[0]
    b = t(b) if b is not None else torch.zeros(cout, dtype=torch.float64, device=dev)
    if bn is not None:
        g, be, m, v = (t(a) for a in bn)
        sc = g / torch.sqrt(v + 1e-5)
        w = w * (sc.view(1, -1, 1, 1) if d.get("transposed") else sc.view(-1, 1, 1, 1))
        b = (b - m) * sc + be
    st, pad = (d["stride_h"], d["stride_w"]), (d["pad_h"], d["pad_w"])

    def lin(xx, ww, bb):
        if d.get("transposed"):
            return F.conv_transpose2d(xx, ww, bb, stride=st, padding=pad, output_padding=d.get("output_padding", 0))
        if d.get("upsample"):
            xx = F.interpolate(xx, scale_factor=2.0, mode="nearest")
        if d.get("pad_hi"):
            xx = F.pad(xx, (0, d["pad_hi"], 0, d["pad_hi"]))
        return F.conv2d(xx, ww, bb, stride=st, padding=pad)

    pre, mpre = lin(x, w, b), lin(x.abs(), w.abs(), b.abs())
    r = x if res is None else t(res)
    res = d.get("residual", 0)
    if res == 1:
        pre, mpre = pre + r, mpre + r.abs()
    mag = {"pre": mpre, "res": r.abs() if res == 2 else torch.zeros((), dtype=torch.float64, device=dev)}
    if d["act"] == 5:
        h = cout // 2
        v, u = pre[:, :h], pre[:, h:]
        mag.update(v=v, u=u, mv=mpre[:, :h], mu=mpre[:, h:])
        return v * gelu64(u), mag
    want = act64(pre, d["act"])
    if res == 2:
        want = want + r
    return want, mag


def grouped_seq_ref(x, w, b, d, res=None):
    """G layers of desc `d`, one per channel group, side by side: group g reads channels [g cin, (g + 1) cin) of x [B, G cin, H, W] with w[g] ([G, cout, cin,
    kh, kw]) and b[g] ([G, cout] or None) and writes channels [g cout, (g + 1) cout) -- conv_ref per group, the outputs and magnitudes concatenated.  The
    residual of group g is its slice of `res` ([B, G cout, Ho, Wo]) or, without one, of x: the form of wav2vec2's positional convolution (one launch per group
    of a grouped Conv1d, GELU, then + the hidden state the layer read)."""
    G, cin, cout = len(w), d["cin"], d["cout"]
    wants, pres, ress = [], [], []
    for g in range(G):
        want, mag = conv_ref(x[:, g * cin:(g + 1) * cin], w[g], None if b is None else b[g], d,
                             res=None if res is None else res[:, g * cout:(g + 1) * cout])
        wants.append(want)
        pres.append(mag["pre"])
        ress.append(mag["res"].expand_as(want))
    return torch.cat(wants, 1), {"pre": torch.cat(pres, 1), "res": torch.cat(ress, 1)}


# Lipschitz constants of the activations (act 0 .. 4): GELU's derivative peaks at 1.1289 (t = sqrt(2)), SiLU's at 1.0998 (t = 2.3994), sigmoid's at 1/4
LIPSCHITZ = {0: 1.0, 1: 1.0, 2: 0.25, 3: 1.13, 4: 1.13}


def conv_bound(want, mag, d, prec, cin):
    """|got - want| allowed per element for a layer with inputs exact in the format and weights rounded to it (derivation: test_conv_configs.py)."""
    u = U[prec]
    K = max_phase_taps(d) * cin
    lin = 2 * u + (K + 8) * F32                               # relative to the magnitude of the pre-activation
    act = d["act"]
    if act == 5:
        # y = v * gelu(u): |dy| <= |gelu(u)| |dv| + 1.13 |v| |du| + 1.13 |dv| |du|; gelu by erf_as (|erf error| <= 1.5e-7: 0.75e-7 |u| absolute)
        # plus a few fp32 roundings of the product, then the store
        ev, eu = lin * mag["mv"], lin * mag["mu"]
        gu = gelu64(mag["u"]).abs()
        return (gu * ev + 1.13 * mag["v"].abs() * eu + 1.13 * ev * eu + (0.75e-7 + 8 * F32) * mag["v"].abs() * mag["u"].abs()
                + 8 * F32 * want.abs() + 2 * u * want.abs())
    A = mag["pre"]
    e = LIPSCHITZ[act] * lin * A
    if act == 2:                                              # sigmoid via __expf: exp's argument rounds (|t| log2(e) F32), exp2 to a few ulp
        e = e + (4 + 0.4 * A) * F32
    elif act == 3:                                            # erff to a few ulp and the fp32 products of 0.5 t (1 + erf)
        e = e + 8 * F32 * A
    elif act == 4:                                            # t * sigmoid(t): the sigmoid's error above times |t|
        e = e + (8 + 0.4 * A) * F32 * A
    # residual after the activation: one more fp32 add of |act(pre)| + |x| (|act(t)| <= |t| + 1 for every act here)
    e = e + F32 * (A + 1.0 + mag["res"])
    return e + 2 * u * want.abs()
