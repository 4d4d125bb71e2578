"""Host model of the MF_PREC_F16Q activation format (numpy only, no device): what a producer has to write for a 32-channel block of fp32 values.

Per pixel and 32-channel block the first plane holds the 32 f16 words h = f16(v) and the second 64 bytes [q6(v - h) | q6(h)].  Each half: 24 bytes of e2m3
codes (channel t of the block in bits [6t, 6t + 6), little endian), one E8M0 scale byte and 7 zero bytes.  The block scale is 2^(floor(log2 max|.|) - 2): the
largest value of the block divided by it lies in [4, 8), the top binade of e2m3 (OCP Microscaling Formats v1.0, FP6 E2M3: sign, 2 exponent bits of bias 1,
3 mantissa bits, subnormal step 0.125, largest value 7.5, no infinities or NaNs; conversion rounds to nearest even and saturates).
"""
import numpy as np

E2M3_MAX = 7.5


def split_f16(v):
    """h = float16(v) (round to nearest even) as float16, r = float32(v) - float32(h) in fp32 (exact: Sterbenz, or h == 0)"""
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    return h, v - h.astype(np.float32)


def block_scale(m):
    """E8M0 byte of a block whose largest magnitude is the fp32 m: max(biased exponent of m, 2) - 2 = 127 + floor(log2 m) - 2 (zeros and denormals: 0)"""
    e = (np.asarray(m, np.float32).view(np.uint32) >> 23) & 0xFF
    return (np.maximum(e, 2) - 2).astype(np.uint8)


def scale_value(byte):
    """the float64 value 2^(byte - 127) of an E8M0 byte"""
    return np.ldexp(1.0, np.asarray(byte).astype(np.int64) - 127)


def dec_e2m3(c):
    """float64 value of the 6-bit code"""
    c = np.asarray(c).astype(np.int64)
    e, m = (c >> 3) & 3, c & 7
    mag = np.where(e == 0, m * 0.125, (1 + m * 0.125) * np.exp2(np.maximum(e, 1) - 1))
    return np.where(c & 0x20, -mag, mag)


def enc_e2m3(y):
    """6-bit code of y (already divided by the block scale): round to nearest, ties to the even code, saturate at 7.5; the sign bit of y is kept (-0 -> 0x20)"""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), E2M3_MAX)
    e = np.clip(np.floor(np.log2(np.maximum(a, 1.0))), 0, 2)                 # binade 1, 2 or 4; below 1 the subnormal step equals binade 1's
    step = np.exp2(e) * 0.125
    k = np.rint(a / step).astype(np.int64)                                   # a / step is exact (a power of two); rint: half to even.  0 .. 16
    code = np.where(e == 0, k, ((e.astype(np.int64) + 1) << 3) + (k - 8))    # k == 16 carries into the next exponent: the same bit pattern
    code = np.minimum(code, 0x1F)
    return (code | np.where(np.signbit(y), 0x20, 0)).astype(np.uint8)


def pack6(codes):
    """[..., 32] codes -> [..., 24] bytes: code t in bits [6t, 6t + 6) of the 192-bit little-endian word"""
    c = np.asarray(codes).astype(np.uint8)
    bits = (c[..., :, None] >> np.arange(6, dtype=np.uint8)) & 1
    return np.packbits(bits.reshape(*c.shape[:-1], 192), axis=-1, bitorder="little")


def unpack6(b):
    """[..., 24] bytes -> [..., 32] codes"""
    bits = np.unpackbits(np.asarray(b, np.uint8), axis=-1, bitorder="little").reshape(*np.shape(b)[:-1], 32, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(-1).astype(np.uint8)


def encode_half(v):
    """[..., 32] fp32 -> [..., 32] bytes: 24 code bytes, the scale byte, 7 zero bytes"""
    v = np.asarray(v, np.float32)
    sb = block_scale(np.abs(v).max(-1))
    codes = enc_e2m3(v.astype(np.float64) / scale_value(sb)[..., None])
    out = np.zeros(v.shape[:-1] + (32,), np.uint8)
    out[..., :24] = pack6(codes)
    out[..., 24] = sb
    return out


def encode_block(v32):
    """[..., 32] fp32 -> (hi bytes [..., 64]: the f16 words, little endian;  lo bytes [..., 64]: [q6(residual) | q6(h)])"""
    h, r = split_f16(v32)
    hi = np.ascontiguousarray(h).view(np.uint8).reshape(h.shape[:-1] + (64,))
    return hi, np.concatenate([encode_half(r), encode_half(h.astype(np.float32))], -1)


def decode_planes(hi_bytes, lo_bytes):
    """[..., 64] + [..., 64] bytes -> h, r_hat, h_hat ([..., 32] float64) and the scale bytes of the residual and of the hi block ([...] uint8)"""
    hi_bytes, lo_bytes = np.ascontiguousarray(hi_bytes, np.uint8), np.ascontiguousarray(lo_bytes, np.uint8)
    h = hi_bytes.view(np.float16).astype(np.float64)
    sl, sh = lo_bytes[..., 24], lo_bytes[..., 56]
    r_hat = dec_e2m3(unpack6(lo_bytes[..., 0:24])) * scale_value(sl)[..., None]
    h_hat = dec_e2m3(unpack6(lo_bytes[..., 32:56])) * scale_value(sh)[..., None]
    return h, r_hat, h_hat, sl, sh
