"""Test-side models of avatar preparation's box and crop steps (csrc/mf_crop_resize.hip), in numpy.

  lip_boxes            the integer model of genavatar.py:80-96 (first box, clip, int(), pads, clamp, get_smoothened_boxes): held to the reference's own outputs by
                       tests/golden/lip_boxes_golden.npz
  crop_linear          cv2.resize(frame[y1:y2, x1:x2], (dw, dh)): oracle.blend_ref.resize_linear_u8 on the cropped array
  crop_lanczos4        the integer two-pass on ops.lanczos4_tables (the wrapper's own builder), written row by row, independent of the kernel's tiling
  lanczos4_float64     the Lanczos-4 resample in float64 with exact weights sinc(t) sinc(t / 4) / sum: what the integer tables approximate
  lanczos4_bound       the per-pixel difference the tables allow between the two, computed from the tables"""
import numpy as np

from mere_fusion_amd.ops import lanczos4_tables
from oracle.blend_ref import resize_linear_u8

TAPS = 8


def _wrap32(v):
    """int64 -> the value a 32-bit two's complement accumulator holds"""
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)


def lip_boxes(det, counts, H, W, pads=(0, 10, 0, 0), nosmooth=False, T=5):
    """det: [n, >=4] first boxes (x1, y1, x2, y2, ...), counts [n] -> (coords int [n, 4] as (y1, y2, x1, x2), number of frames without a face)"""
    n = len(det)
    top, bottom, left, right = (int(p) for p in pads)
    b = [[0, 0, 0, 0] for _ in range(n)]                                     # x1, y1, x2, y2
    no_face = 0
    for i in range(n):
        if counts[i] < 1:
            no_face += 1
            continue
        rx1, ry1, rx2, ry2 = (int(max(float(v), 0.0)) for v in det[i][:4])
        b[i] = [max(0, rx1 - left), max(0, ry1 - top), min(W, rx2 + right), min(H, ry2 + bottom)]
    if not nosmooth:
        for i in range(n):
            if i + T > n:
                start = n - T
                if start < 0:
                    start = max(start + n, 0)
                lo, hi = start, n
            else:
                lo, hi = i, i + T
            b[i] = [_trunc_div(sum(b[j][e] for j in range(lo, hi)), hi - lo) for e in range(4)]         # np.mean -> int64: truncated quotient
    return np.array([(y1, y2, x1, x2) for x1, y1, x2, y2 in b], dtype=np.int64).reshape(n, 4), no_face


def _trunc_div(s, c):
    q = abs(s) // c
    return q if s >= 0 else -q


def crop_linear(frame, box, dw, dh):
    x1, y1, x2, y2 = box
    return resize_linear_u8(np.ascontiguousarray(frame[y1:y2, x1:x2]), dw, dh)


def crop_lanczos4(frame, box, dw, dh):
    x1, y1, x2, y2 = box
    crop = frame[y1:y2, x1:x2].astype(np.int64)
    ch, cw, _ = crop.shape
    xo, xc = lanczos4_tables(cw, dw)
    yo, yc = lanczos4_tables(ch, dh)
    rows = np.zeros((ch, dw, 3), dtype=np.int64)
    for k in range(TAPS):
        rows += crop[:, np.clip(xo.astype(np.int64) + k, 0, cw - 1)] * xc[:, k].astype(np.int64)[None, :, None]
    assert np.abs(rows).max() < (1 << 31)
    out = np.zeros((dh, dw, 3), dtype=np.int64)
    for k in range(TAPS):
        out = _wrap32(out + _wrap32(rows[np.clip(yo.astype(np.int64) + k, 0, ch - 1)] * yc[:, k].astype(np.int64)[:, None, None]))
    out = _wrap32(out + (1 << 21)) >> 22
    return np.clip(out, 0, 255).astype(np.uint8)


def _lanczos_weights(ssize, dsize):
    """float64: (first tap index [dsize], weights [dsize, 8]) at the un-rounded position"""
    pos = (np.arange(dsize, dtype=np.float64) + 0.5) * (np.float64(ssize) / np.float64(dsize)) - 0.5
    s = np.floor(pos)
    t = (pos - s)[:, None] - (np.arange(TAPS, dtype=np.float64) - 3)[None, :]            # distance of tap k (at s - 3 + k) from the position
    w = np.sinc(t) * np.sinc(t / 4)
    return (s - 3).astype(np.int64), w / w.sum(axis=1, keepdims=True)


def lanczos4_float64(frame, box, dw, dh):
    x1, y1, x2, y2 = box
    crop = frame[y1:y2, x1:x2].astype(np.float64)
    ch, cw, _ = crop.shape
    xo, wx = _lanczos_weights(cw, dw)
    yo, wy = _lanczos_weights(ch, dh)
    rows = np.zeros((ch, dw, 3))
    for k in range(TAPS):
        rows += crop[:, np.clip(xo + k, 0, cw - 1)] * wx[:, k][None, :, None]
    out = np.zeros((dh, dw, 3))
    for k in range(TAPS):
        out += rows[np.clip(yo + k, 0, ch - 1)] * wy[:, k][:, None, None]
    return np.clip(out, 0, 255)


def _axis_error(ssize, dsize):
    """per destination index: (sum |e|, sum |w|), e = table coefficient - 2048 w, both on the SAME source taps (a table whose float32 position fell on the other
    side of an integer has its taps shifted by one: the comparison is made on the union of the two windows)"""
    to, tc = lanczos4_tables(ssize, dsize)
    wo, w = _lanczos_weights(ssize, dsize)
    e_sum = np.zeros(dsize)
    for d in range(dsize):
        lo = min(int(to[d]), int(wo[d]))
        a, b = np.zeros(TAPS + 2), np.zeros(TAPS + 2)
        a[int(to[d]) - lo:int(to[d]) - lo + TAPS] = tc[d].astype(np.float64)
        b[int(wo[d]) - lo:int(wo[d]) - lo + TAPS] = 2048.0 * w[d]
        e_sum[d] = np.abs(a - b).sum()
    return e_sum, np.abs(w).sum(axis=1)


def lanczos4_bound(cw, ch, dw, dh):
    """[dh, dw]: 255 (sum|e_y| sum|w_x| + sum|e_x| sum|w_y|) / 2048 + 0.5"""
    ex, wx = _axis_error(cw, dw)
    ey, wy = _axis_error(ch, dh)
    return 255.0 * (ey[:, None] * wx[None, :] + ex[None, :] * wy[:, None]) / 2048.0 + 0.5
