"""NumPy model of the Wav2Lip and VAE edge kernels of csrc/mf_aux.hip (k_faces_u8, k_faces_u8_rows, k_vae_image_u8, k_head<32>), shared by
test_aux_kernels.py's host and GPU tests.  No torch.

- split: the (hi, lo) bf16 planes of an fp32 value, hi = rne(v), lo = rne(v - fp32(hi)) with the subtraction in fp32.  hi + lo is exact in fp32 (v - hi is
  exact, lo keeps its leading 8 bits, none of them below v's last bit), so a buffer read back as fp32(hi + lo) names one (hi, lo) pair's sum without rounding.
- faces_value / vae_value: the pixel arithmetic in the kernels' own formats -- fp32(u8) / fp32(255) for the faces; fp32(fp64(u8) / 255.0), the optional
  mask, then (f - 0.5f) / 0.5f in fp32 for the VAE image.
- faces_channels / vae_channels: the 8 channels of every pixel; rows y >= H // 2 are the masked ones (y < H // 2 is kept).
- padded: channels-last values placed at [b][y + halo][x + halo][c] of a poisoned buffer of batch + `spare` items with the allocation's tail.
- head64: the 32-channel 1 x 1 conv + sigmoid in float64 over the values the planes hold, with the magnitude sum the rounding bound needs.
"""
import numpy as np

POISON_HI = np.uint16(0xC49A)            # -1232        (csrc/mf_nn_api.hip)
POISON_LO = np.uint16(0x3F20)            # 0.625: hi + lo = -1231.375 = MF_NN_POISON_X3; the hi plane alone MF_NN_POISON_BF16
TAIL = 64                                # elements every allocation carries behind its last item
U32 = 2.0 ** -24                         # fp32 unit roundoff


def bf16_rne(x):
    """fp32 -> bf16 -> fp32, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_bits(x):
    """the 16-bit pattern of a value that is a bf16"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def from_bits(h):
    return (np.asarray(h, np.uint32) << 16).view(np.float32)


def split(v, prec):
    """(hi, lo) planes as fp32 arrays; lo is None in bf16 mode"""
    v = np.ascontiguousarray(v, np.float32)
    hi = bf16_rne(v)
    return hi, (bf16_rne(v - hi) if prec == "bf16x3" else None)


def faces_value(u8):
    return np.asarray(u8, np.uint8).astype(np.float32) / np.float32(255)


def vae_unit(u8):
    """fp32(fp64(u8) / 255.0): numpy's double division, rounded once"""
    return (np.asarray(u8, np.uint8).astype(np.float64) / 255.0).astype(np.float32)


def vae_normalise(f):
    return (np.asarray(f, np.float32) - np.float32(0.5)) / np.float32(0.5)


def vae_value(u8):
    return vae_normalise(vae_unit(u8))


def keep_rows(H):
    """[H] bool: the rows the half mask keeps"""
    return np.arange(H) < H // 2


def faces_channels(faces):
    """uint8 [B, H, W, 3] -> fp32 [B, H, W, 8]: 0-2 the face with rows >= H // 2 zeroed, 3-5 the whole face, 6-7 zero"""
    B, H, W, _ = faces.shape
    f = faces_value(faces)
    v = np.zeros((B, H, W, 8), np.float32)
    v[..., 0:3] = np.where(keep_rows(H)[None, :, None, None], f, np.float32(0))
    v[..., 3:6] = f
    return v


def vae_channels(img_bgr, half_mask):
    """uint8 BGR [B, H, W, 3] -> fp32 [B, H, W, 8]: R, G, B normalised (masked rows hold (0 - 0.5) / 0.5 = -1), 3-7 zero"""
    B, H, W, _ = img_bgr.shape
    f = vae_unit(img_bgr[..., ::-1])
    if half_mask:
        f = np.where(keep_rows(H)[None, :, None, None], f, np.float32(0))
    v = np.zeros((B, H, W, 8), np.float32)
    v[..., 0:3] = vae_normalise(f)
    return v


def padded(v, halo, prec, spare=1, tail=TAIL):
    """channels-last fp32 v [B, H, W, C] -> (want, written): the flat fp32 image (hi + lo) of a poisoned buffer of B + spare items [H + 2 halo][W + 2 halo][C]
    plus `tail` elements with split(v) stored at [b][y + halo][x + halo][c], and the bool mask of the elements that were stored"""
    B, H, W, Cn = v.shape
    Hp, Wp = H + 2 * halo, W + 2 * halo
    hi, lo = split(v, prec)
    n = (B + spare) * Hp * Wp * Cn
    ph = np.full(n + tail, from_bits(POISON_HI), np.float32)
    pl = np.full(n + tail, from_bits(POISON_LO) if prec == "bf16x3" else np.float32(0), np.float32)
    written = np.zeros(n + tail, bool)
    for plane, src in ((ph, hi), (pl, lo)):
        if src is not None:
            plane[:n].reshape(B + spare, Hp, Wp, Cn)[:B, halo:halo + H, halo:halo + W] = src
    written[:n].reshape(B + spare, Hp, Wp, Cn)[:B, halo:halo + H, halo:halo + W] = True
    return ph + pl, written                  # (exact: see the module docstring; the poison pair sums exactly too)


def head64(xs, w, b):
    """xs [B, T, 32]: the values the planes hold; w [3, 32], b [3] fp32.  -> float64 (s, z, A) [B, 3, T]: s = sigmoid(z), z = b + sum_c w[k, c] xs[c],
    A = |b| + sum_c |w[k, c] xs[c]| (what 32 chained fp32 FMAs round against)"""
    x, w, b = np.asarray(xs, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    z = np.einsum("btc,kc->bkt", x, w) + b[None, :, None]
    A = np.einsum("btc,kc->bkt", np.abs(x), np.abs(w)) + np.abs(b)[None, :, None]
    with np.errstate(over="ignore"):
        s = np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))
    return s, z, A


def head_gate_terms(z, A):
    """the derivation of test_aux_kernels.py's head gate, per element: (logit term, evaluation term).
    logit: k_head forms z with 32 chained fp32 FMAs from the bias, each rounding a partial sum bounded by A: |dz| <= 32 u A; the sigmoid's slope
    s (1 - s) is at most 1/4 and at most e^-|z|.  evaluation: expf within 1 ulp = 2 u relative, the rounding of 1 + e (u), a division within 2.5 ulp = 5 u,
    all relative to s <= 1, and one more rounding (u) for the product with 255 in the other layout: 9 u."""
    return np.minimum(0.25, np.exp(-np.abs(z))) * 32 * U32 * A, 9 * U32
