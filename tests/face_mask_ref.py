"""TEST HELPER: numpy restatement of what surrounds BiSeNet in MuseTalk's mask preparation (face_parsing/__init__.py:38-50, musetalk/utils/blending.py:17-24, 62-86).

  resize_u8        Pillow's `Image.resize` for 8-bit pixels (src/libImaging/Resample.c): float64 coefficient tables rounded to 22-bit fixed point, a horizontal pass to a
                   uint8 intermediate, a vertical pass, `(acc + 2^21) >> 22` clipped to 0..255.  Pure integer numpy after the tables; tests/test_face_mask.py holds it
                   to Pillow itself with 0 differing values where Pillow imports, and to the golden file everywhere.
  crop_u8          `Image.crop`: black outside the image.
  window           the crop / paste / top-boundary statements of blending.py:74-82.
  gaussian_blur    cv2.GaussianBlur(mask, (k, k), 0) as OpenCV documents it (getGaussianKernel's sigma rule and taps, BORDER_REFLECT_101), evaluated in float64 and NOT
                   rounded: the yardstick of the device blur.  OpenCV is not available to the tests, so this is a restatement of the published algorithm, unpinned.
Never imported by the product."""
import numpy as np

PRECISION_BITS = 22
BILINEAR, BICUBIC = 0, 1
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}


def _filter(kind, x):
    x = np.abs(x)
    if kind == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def coeffs(in_size, out_size, kind):
    """precompute_coeffs + normalize_coeffs_8bpc for the box (0, in_size): (xmin [out], n [out], kk int64 [out, ksize])"""
    scale = float(np.float32(in_size) - np.float32(0)) / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[kind] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmin, num, kk = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = _filter(kind, (np.arange(n) + lo - center + 0.5) * ss)
        ww = 0.0
        for v in w:                                   # the C loop's order of additions
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        q = w * float(1 << PRECISION_BITS)
        kk[xx, :n] = np.where(w < 0, np.trunc(-0.5 + q), np.trunc(0.5 + q)).astype(np.int64)
        xmin[xx], num[xx] = lo, n
    return xmin, num, kk


def _pass(img, out_size, kind):
    """resample axis 1 of uint8 [h, w, c] to out_size"""
    xmin, num, kk = coeffs(img.shape[1], out_size, kind)
    src = img.astype(np.int64)
    acc = np.full((img.shape[0], out_size, img.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(kk.shape[1]):
        live = t < num
        idx = np.where(live, xmin + t, 0)
        acc += src[:, idx, :] * (kk[:, t] * live)[None, :, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_u8(img, size, kind):
    """Image.resize(size, kind) of a uint8 [h, w] or [h, w, c] array; size = (width, height).  An axis whose size does not change is skipped, as in Pillow."""
    a = img[:, :, None] if img.ndim == 2 else img
    if a.shape[1] != size[0]:
        a = _pass(a, size[0], kind)
    if a.shape[0] != size[1]:
        a = _pass(a.transpose(1, 0, 2), size[1], kind).transpose(1, 0, 2)
    a = np.ascontiguousarray(a)
    return a[:, :, 0] if img.ndim == 2 else a


def crop_u8(img, box):
    """Image.crop(box): pixels of the box outside the image are 0"""
    x0, y0, x1, y1 = box
    out = np.zeros((y1 - y0, x1 - x0) + img.shape[2:], img.dtype)
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x1, img.shape[1]), min(y1, img.shape[0])
    if sx1 > sx0 and sy1 > sy0:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return out


def get_crop_box(box, expand):
    x, y, x1, y1 = box
    x_c, y_c = (x + x1) // 2, (y + y1) // 2
    w, h = x1 - x, y1 - y
    s = int(max(w, h) // 2 * expand)
    return [x_c - s, y_c - s, x_c + s, y_c + s], s


def window(mask, face_box, crop_box, upper_boundary_ratio=0.5, top=None):
    """blending.py:74-82 on the crop-size mask: zero outside the face-box rectangle and above top_boundary (top: the boundary row itself, where a test sets one that
    no ratio gives)"""
    x, y, x1, y1 = face_box
    x_s, y_s = crop_box[:2]
    h, w = mask.shape
    out = np.zeros_like(mask)
    out[y - y_s:y1 - y_s, x - x_s:x1 - x_s] = mask[y - y_s:y1 - y_s, x - x_s:x1 - x_s]
    out[:int(h * upper_boundary_ratio) if top is None else top] = 0
    return out


def blur_kernel_size(width):
    return int(0.1 * width // 2 * 2) + 1


def gaussian_taps(k):
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = np.arange(k, dtype=np.float64)
    t = np.exp(-(i - (k - 1) / 2) ** 2 / (2 * sigma * sigma))
    return t / t.sum()


def reflect101(i, n):
    """BORDER_REFLECT_101 as the loop `while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i` states it, for an integer array i: bounces as often as needed"""
    i = np.array(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return i


def gaussian_blur(mask, k, index=None):
    """float64 [h, w], not rounded.  index(i, n): the border rule as a function of an index array and the axis length, in place of numpy's padding (reflect101 gives
    the same image; a test hands in a deliberately different rule to show that its comparison notices)"""
    taps, r = gaussian_taps(k), k // 2
    h, w = mask.shape
    if index is None:
        a = np.pad(mask.astype(np.float64), r, mode="reflect")   # numpy's "reflect" is BORDER_REFLECT_101
    else:
        a = mask.astype(np.float64)[index(np.arange(-r, h + r), h)][:, index(np.arange(-r, w + r), w)]
    tmp = sum(taps[t] * a[:, t:t + w] for t in range(k))
    return sum(taps[t] * tmp[t:t + h, :] for t in range(k))


def class_mask(logits):
    """face_parsing/__init__.py:47-49 on [19, H, W] logits"""
    p = logits.argmax(0)
    p[p > 13] = 0
    p[p >= 1] = 255
    return p.astype(np.uint8)


def near_tie(logits, eps):
    """pixels whose best class in 1..13 and best class in {0, 14..18} are closer than either side's logit error allows: gap <= 2 * eps"""
    fg = logits[1:14].max(0)
    bg = np.maximum(logits[0], logits[14:].max(0))
    return np.abs(fg - bg) <= 2 * eps


def dilate(mask, r):
    """square dilation by r pixels of a boolean [h, w] map"""
    h, w = mask.shape
    c = np.cumsum(np.pad(mask.astype(np.int64), ((r + 1, r), (r + 1, r))), 0).cumsum(1)
    s = c[2 * r + 1:, 2 * r + 1:] - c[:h, 2 * r + 1:] - c[2 * r + 1:, :w] + c[:h, :w]
    return s > 0
