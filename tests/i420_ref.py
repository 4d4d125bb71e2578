"""The project's I420 definition in numpy, as tests/test_i420_host.py and tests/test_i420.py share it: the integer model the kernel must equal byte for byte
(csrc/mf_i420.hip states the same integers) and the float64 matrix it approximates."""
import numpy as np

KNOWN = {  # (R, G, B) -> (Y, Cb, Cr)
    (255, 255, 255): (235, 128, 128),
    (0, 0, 0): (16, 128, 128),
    (255, 0, 0): (81, 90, 240),
    (0, 255, 0): (145, 54, 34),
    (0, 0, 255): (41, 240, 110),
}


def _rgb_planes(frames, order):
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim == 4 and f.shape[3] == 3 and f.shape[1] % 2 == 0 and f.shape[2] % 2 == 0 and order in ("bgr", "rgb")
    c = (0, 1, 2) if order == "rgb" else (2, 1, 0)
    return [f[..., i].astype(np.int64) for i in c]


def _blocks(p):
    """sums over the 2 x 2 blocks of [B, H, W]"""
    B, H, W = p.shape
    return p.reshape(B, H // 2, 2, W // 2, 2).sum(axis=(2, 4))


def _pack(y, cb, cr):
    """the planes as bytes of one contiguous buffer per frame (H need not be a multiple of 4)"""
    B, H, W = y.shape
    return np.concatenate([y.reshape(B, -1), cb.reshape(B, -1), cr.reshape(B, -1)], axis=1).reshape(B, H * 3 // 2, W)


def i420_model(frames, order):
    """uint8 [B, H, W, 3] in `order` -> uint8 [B, H * 3 / 2, W]: 16.16 fixed point, chroma from the 2 x 2 sums, floor shifts"""
    r, g, b = _rgb_planes(frames, order)
    y = (16829 * r + 33039 * g + 6416 * b + (16 << 16) + 32768) >> 16
    sr, sg, sb = _blocks(r), _blocks(g), _blocks(b)
    cb = (-9714 * sr - 19070 * sg + 28784 * sb + (128 << 18) + (1 << 17)) >> 18
    cr = (28784 * sr - 24103 * sg - 4681 * sb + (128 << 18) + (1 << 17)) >> 18
    for p in (y, cb, cr):
        assert p.min() >= 0 and p.max() <= 255
    return _pack(y, cb, cr).astype(np.uint8)


def i420_float64(frames, order):
    """the BT.601 studio-swing matrix in float64, unrounded: (Y [B, H, W], Cb, Cr [B, H / 2, W / 2]), chroma of the 2 x 2 mean"""
    r, g, b = [p.astype(np.float64) for p in _rgb_planes(frames, order)]
    y = 16.0 + (0.299 * r + 0.587 * g + 0.114 * b) * 219.0 / 255.0
    mr, mg, mb = _blocks(r) / 4.0, _blocks(g) / 4.0, _blocks(b) / 4.0
    cb = 128.0 + (-0.168736 * mr - 0.331264 * mg + 0.5 * mb) * 224.0 / 255.0
    cr = 128.0 + (0.5 * mr - 0.418688 * mg - 0.081312 * mb) * 224.0 / 255.0
    return y, cb, cr


def planes(i420, H, W):
    """[B, H * 3 / 2, W] -> (Y [B, H, W], Cb [B, H / 2, W / 2], Cr)"""
    a = np.asarray(i420)
    B = a.shape[0]
    flat = a.reshape(B, -1)
    n = H * W
    return flat[:, :n].reshape(B, H, W), flat[:, n:n + n // 4].reshape(B, H // 2, W // 2), flat[:, n + n // 4:].reshape(B, H // 2, W // 2)


def primaries_frame(H, W, order):
    """uint8 [H, W, 3]: 2 x 2 blocks of white, black, red, green, blue, in turn"""
    cols = np.array(list(KNOWN), dtype=np.uint8)
    if order == "bgr":
        cols = cols[:, ::-1]
    by, bx = np.meshgrid(np.arange(H) // 2, np.arange(W) // 2, indexing="ij")
    return np.ascontiguousarray(cols[(by * (W // 2) + bx) % len(cols)])
