"""DWPose (RTMPose-l whole-body, 384 x 288) restated in torch / numpy: the oracle of tests/test_dwpose*.py.

UNPINNED.  mmpose, mmdet, mmcv and OpenCV are not installed where this suite runs, so nothing here was compared against them: it is a restatement of the
published modules named by musetalk/utils/dwpose/rtmpose-l_8xb32-270e_coco-ubody-wholebody-384x288.py -- mmdet's CSPNeXt (P5, deepen 1, widen 1, expand 0.5,
channel attention, SiLU, out_indices (4,)), mmpose's RTMCCHead (7 x 7 final conv, ScaleNorm, Linear, one RTMCCBlock with s 128 / expansion 2 / SiLU / no
relative bias / no positional encoding, cls_x, cls_y), the SimCCLabel codec (split ratio 2) with flip_test=True, the top-down pipeline of `inference_topdown`
(whole-image box, GetBBoxCenterScale padding 1.25, TopdownAffine to 288 x 384, cv2.warpAffine INTER_LINEAR with a constant 0 border, PoseDataPreprocessor) --
and of musetalk/utils/preprocessing.py:96-131, which cannot be imported here.  state_dict keys are those of an mmpose checkpoint (dw-ll_ucoco_384.pth), so that
file loads with strict=True; no real checkpoint has been loaded.

Runs in fp32 or fp64 (`DWPoseRef(...).double()`)."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

INPUT_SIZE = (288, 384)                                   # (w, h) of the codec
MEAN = (123.675, 116.28, 103.53)                          # PoseDataPreprocessor, RGB order
STD = (58.395, 57.12, 57.375)
PADDING = 1.25                                            # GetBBoxCenterScale
SPLIT = 2.0                                               # simcc_split_ratio
# eval-mode BatchNorm.  eps 1e-3 (momentum 0.03, irrelevant in eval) is the default norm_cfg of mmdet's CSPNeXt; the config file passes norm_cfg=dict(type='SyncBN')
# of its own, so a loader of a real checkpoint must check which of the two its mmdet version ends up with -- it is an argument of DWPoseRef for that reason.
BN_EPS = 1e-3
ARCH_P5 = [[64, 128, 3, True, False], [128, 256, 6, True, False], [256, 512, 6, True, False], [512, 1024, 3, False, True]]
NUM_KEYPOINTS = 133
FACE = slice(23, 91)                                      # preprocessing.py:100


def flip_indices(K=NUM_KEYPOINTS):
    """COCO-WholeBody left/right pairs as the permutation `flip_indices` of the dataset meta: 17 body, 6 feet, 68 face, 2 x 21 hands"""
    p = list(range(133))

    def swap(a, b):
        p[a], p[b] = b, a
    for a in range(1, 17, 2):
        swap(a, a + 1)
    for a in (17, 18, 19):
        swap(a, a + 3)
    f = 23
    for i in range(8):
        swap(f + i, f + 16 - i)                           # jaw line
    for i in range(5):
        swap(f + 17 + i, f + 26 - i)                      # brows
    swap(f + 31, f + 35); swap(f + 32, f + 34)            # nostrils
    for a, b in ((36, 45), (37, 44), (38, 43), (39, 42), (40, 47), (41, 46)):
        swap(f + a, f + b)                                # eyes
    for a, b in ((48, 54), (49, 53), (50, 52), (55, 59), (56, 58), (60, 64), (61, 63), (65, 67)):
        swap(f + a, f + b)                                # mouth
    for i in range(21):
        swap(91 + i, 112 + i)                             # hands
    if K == 133:
        return p
    return [i + 1 if i % 2 == 0 and i + 1 < K else (i - 1 if i % 2 == 1 else i) for i in range(K)]   # reduced nets: neighbours swap, an odd last one stays


# ---- module tree ------------------------------------------------------------------------------------------------------------------------------
class ConvModule(nn.Module):
    """mmcv ConvModule with norm: conv (no bias) -> BatchNorm2d -> SiLU"""
    def __init__(self, cin, cout, k, stride=1, padding=0, groups=1, eps=BN_EPS):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, padding, groups=groups, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=eps, momentum=0.03)

    def forward(self, x):
        return F.silu(self.bn(self.conv(x)))


class DepthwiseSeparableConvModule(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0, eps=BN_EPS):
        super().__init__()
        self.depthwise_conv = ConvModule(cin, cin, k, stride, padding, groups=cin, eps=eps)
        self.pointwise_conv = ConvModule(cin, cout, 1, eps=eps)

    def forward(self, x):
        return self.pointwise_conv(self.depthwise_conv(x))


class ChannelAttention(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.fc = nn.Conv2d(channels, channels, 1, 1, 0, bias=True)

    def forward(self, x):
        return x * F.hardsigmoid(self.fc(x.mean((2, 3), keepdim=True)))


class CSPNeXtBlock(nn.Module):
    def __init__(self, cin, cout, add_identity, eps):
        super().__init__()
        self.conv1 = ConvModule(cin, cout, 3, 1, 1, eps=eps)                   # expansion 1.0 inside a CSPLayer
        self.conv2 = DepthwiseSeparableConvModule(cout, cout, 5, 1, 2, eps=eps)
        self.add_identity = add_identity and cin == cout

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return out + x if self.add_identity else out


class CSPLayer(nn.Module):
    def __init__(self, cin, cout, expand_ratio, num_blocks, add_identity, eps):
        super().__init__()
        mid = int(cout * expand_ratio)
        self.main_conv = ConvModule(cin, mid, 1, eps=eps)
        self.short_conv = ConvModule(cin, mid, 1, eps=eps)
        self.final_conv = ConvModule(2 * mid, cout, 1, eps=eps)
        self.blocks = nn.Sequential(*[CSPNeXtBlock(mid, mid, add_identity, eps) for _ in range(num_blocks)])
        self.attention = ChannelAttention(2 * mid)

    def forward(self, x):
        x_short = self.short_conv(x)
        x_main = self.blocks(self.main_conv(x))
        return self.final_conv(self.attention(torch.cat((x_main, x_short), dim=1)))


class SPPBottleneck(nn.Module):
    def __init__(self, cin, cout, eps, kernel_sizes=(5, 9, 13)):
        super().__init__()
        mid = cin // 2
        self.conv1 = ConvModule(cin, mid, 1, eps=eps)
        self.poolings = nn.ModuleList([nn.MaxPool2d(k, 1, k // 2) for k in kernel_sizes])
        self.conv2 = ConvModule(mid * (len(kernel_sizes) + 1), cout, 1, eps=eps)

    def forward(self, x):
        x = self.conv1(x)
        return self.conv2(torch.cat([x] + [p(x) for p in self.poolings], dim=1))


class CSPNeXt(nn.Module):
    def __init__(self, deepen=1.0, widen=1.0, expand_ratio=0.5, eps=BN_EPS):
        super().__init__()
        c = int(ARCH_P5[0][0] * widen)
        self.stem = nn.Sequential(ConvModule(3, c // 2, 3, 2, 1, eps=eps), ConvModule(c // 2, c // 2, 3, 1, 1, eps=eps), ConvModule(c // 2, c, 3, 1, 1, eps=eps))
        for i, (cin, cout, nb, add_identity, use_spp) in enumerate(ARCH_P5):
            cin, cout, nb = int(cin * widen), int(cout * widen), max(round(nb * deepen), 1)
            stage = [ConvModule(cin, cout, 3, 2, 1, eps=eps)]
            if use_spp:
                stage.append(SPPBottleneck(cout, cout, eps))
            stage.append(CSPLayer(cout, cout, expand_ratio, nb, add_identity, eps))
            setattr(self, f"stage{i + 1}", nn.Sequential(*stage))
        self.out_channels = int(ARCH_P5[-1][1] * widen)

    def forward(self, x):
        x = self.stem(x)
        for i in range(4):
            x = getattr(self, f"stage{i + 1}")(x)
        return x                                                                # out_indices (4,)


class ScaleNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.scale, self.eps = dim ** -0.5, eps
        self.g = nn.Parameter(torch.ones(1))

    def forward(self, x):
        norm = torch.linalg.norm(x, dim=-1, keepdim=True) * self.scale
        return x / norm.clamp(min=self.eps) * self.g


class Scale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.scale


class RTMCCBlock(nn.Module):
    """the gated attention unit, self-attention, shortcut, no relative bias, no positional encoding, dropout 0"""
    def __init__(self, dims, s=128, expansion_factor=2):
        super().__init__()
        self.s, self.e = s, int(dims * expansion_factor)
        self.o = nn.Linear(self.e, dims, bias=False)
        self.uv = nn.Linear(dims, 2 * self.e + s, bias=False)
        self.gamma = nn.Parameter(torch.rand(2, s))
        self.beta = nn.Parameter(torch.rand(2, s))
        self.ln = ScaleNorm(dims)
        self.res_scale = Scale(dims)
        self.sqrt_s = math.sqrt(s)

    def forward(self, inputs):
        x = self.ln(inputs)
        uv = F.silu(self.uv(x))
        u, v, base = torch.split(uv, [self.e, self.e, self.s], dim=2)
        base = base.unsqueeze(2) * self.gamma[None, None, :] + self.beta
        q, k = torch.unbind(base, dim=2)
        kernel = torch.square(F.relu(torch.bmm(q, k.permute(0, 2, 1)) / self.sqrt_s))
        return self.res_scale(inputs) + self.o(u * torch.bmm(kernel, v))


class RTMCCHead(nn.Module):
    def __init__(self, in_channels, out_channels, input_size, in_featuremap_size, hidden=256, s=128, final_kernel=7):
        super().__init__()
        flat = in_featuremap_size[0] * in_featuremap_size[1]
        self.final_layer = nn.Conv2d(in_channels, out_channels, final_kernel, 1, final_kernel // 2)
        self.mlp = nn.Sequential(ScaleNorm(flat), nn.Linear(flat, hidden, bias=False))
        self.gau = RTMCCBlock(hidden, s, 2)
        self.cls_x = nn.Linear(hidden, int(input_size[0] * SPLIT), bias=False)
        self.cls_y = nn.Linear(hidden, int(input_size[1] * SPLIT), bias=False)

    def tokens(self, maps):
        return self.gau(self.mlp(torch.flatten(maps, 2)))

    def forward(self, feats):
        t = self.tokens(self.final_layer(feats))
        return self.cls_x(t), self.cls_y(t)


class DWPoseRef(nn.Module):
    """TopdownPoseEstimator: backbone + head.  `reduced()` is the small configuration of the whole-path tests."""
    def __init__(self, deepen=1.0, widen=1.0, input_size=INPUT_SIZE, keypoints=NUM_KEYPOINTS, hidden=256, s=128, bn_eps=BN_EPS):
        super().__init__()
        self.input_size, self.keypoints = tuple(input_size), keypoints
        self.backbone = CSPNeXt(deepen, widen, 0.5, bn_eps)
        self.head = RTMCCHead(self.backbone.out_channels, keypoints, input_size, (input_size[0] // 32, input_size[1] // 32), hidden, s)
        self.eval()

    @classmethod
    def reduced(cls):
        return cls(deepen=1.0 / 3.0, widen=0.25, input_size=(64, 96))

    @torch.no_grad()
    def logits(self, x):
        """normalised RGB [B, 3, h, w] -> (simcc_x [B, K, 2w], simcc_y [B, K, 2h]) of the straight pass"""
        return self.head(self.backbone(x))


# ---- pre-processing ----------------------------------------------------------------------------------------------------------------------------
def bbox_center_scale(w, h, padding=PADDING, input_size=INPUT_SIZE):
    """the whole-image box [0, 0, w, h] (inference_topdown without boxes) -> GetBBoxCenterScale -> the aspect-ratio fix of TopdownAffine; float32 like mmpose"""
    box = np.array([0, 0, w, h], np.float32)
    center = (box[2:] + box[:2]) * np.float32(0.5)
    scale = (box[2:] - box[:2]) * np.float32(padding)
    aspect = np.float32(input_size[0] / input_size[1])
    bw, bh = scale
    scale = np.array([bw, bw / aspect], np.float32) if bw > bh * aspect else np.array([bh * aspect, bh], np.float32)
    return center, scale


def _third(a, b):
    d = a - b
    return b + np.array([-d[1], d[0]])


def warp_matrix(center, scale, output_size=INPUT_SIZE):
    """get_warp_matrix(center, scale, rot=0, output_size): cv2.getAffineTransform of three point pairs, solved in float64.  Returns the 2 x 3 source -> input map."""
    center, scale = np.asarray(center, np.float64), np.asarray(scale, np.float64)
    dw, dh = output_size
    src, dst = np.zeros((3, 2)), np.zeros((3, 2))
    src[0] = center
    src[1] = center + np.array([0.0, scale[0] * -0.5])
    src[2] = _third(src[0], src[1])
    dst[0] = [dw * 0.5, dh * 0.5]
    dst[1] = dst[0] + np.array([0.0, dw * -0.5])
    dst[2] = _third(dst[0], dst[1])
    A = np.hstack([src, np.ones((3, 1))])
    return np.linalg.solve(A, dst).T                                            # [2, 3]


def invert_affine(M):
    """cv2.invertAffineTransform in float64: the input -> source map warpAffine walks"""
    M = np.asarray(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[1, 1] * D, M[0, 0] * D, -M[0, 1] * D, -M[1, 0] * D
    return np.array([[A11, A12, -A11 * M[0, 2] - A12 * M[1, 2]], [A21, A22, -A21 * M[0, 2] - A22 * M[1, 2]]])


# The warp as an integer model: with Minv the float64 input -> source map,
#   X = (rint(Minv00 * x * 1024) + rint((Minv01 * y + Minv02) * 1024) + 16) >> 5     (likewise Y; rint = round half to even; products and the sum rounded
#                                                                                     one by one in float64, no fused multiply-add)
# is the source position in 1/32-pixel steps; sx = X >> 5, fx = X & 31.  The four taps (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1) carry the 15-bit
# weights (32 - fy)(32 - fx) * 32, (32 - fy) fx * 32, fy (32 - fx) * 32, fy fx * 32 (they sum to 32768 exactly); a tap outside the frame reads 0; the code is
# (sum + 16384) >> 15: one rounding.
def warp_affine_int(img, Minv, out_wh):
    img = np.asarray(img)
    H, W = img.shape[:2]
    ow, oh = out_wh
    Minv = np.asarray(Minv, np.float64)
    x, y = np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64)
    X = (np.rint(Minv[0, 0] * x * 1024.0)[None, :] + np.rint((Minv[0, 1] * y + Minv[0, 2]) * 1024.0)[:, None]).astype(np.int64) + 16 >> 5
    Y = (np.rint(Minv[1, 0] * x * 1024.0)[None, :] + np.rint((Minv[1, 1] * y + Minv[1, 2]) * 1024.0)[:, None]).astype(np.int64) + 16 >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.zeros((oh, ow, img.shape[2]), np.int64)
    for dy, dx, w in ((0, 0, (32 - fy) * (32 - fx)), (0, 1, (32 - fy) * fx), (1, 0, fy * (32 - fx)), (1, 1, fy * fx)):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        tap = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64) * ok[..., None]
        acc += tap * (w * 32)[..., None]
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_affine_f64(img, Minv, out_wh):
    """the same bilinear warp with exact float64 coordinates and weights, not rounded to codes"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    ow, oh = out_wh
    Minv = np.asarray(Minv, np.float64)
    x, y = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    X, Y = Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2], Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]
    sx, sy = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    fx, fy = X - sx, Y - sy
    acc = np.zeros((oh, ow, img.shape[2]))
    for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        acc += img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.float64) * (ok * w)[..., None]
    return acc


def normalise(warped_bgr_u8, mean=MEAN, std=STD):
    """PoseDataPreprocessor: BGR -> RGB, (x - mean) / std, one fp32 subtraction and one fp32 division; [h, w, 3] uint8 -> float32 [3, h, w]"""
    rgb = np.asarray(warped_bgr_u8)[..., ::-1].astype(np.float32)
    return np.ascontiguousarray(((rgb - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).transpose(2, 0, 1))


def preprocess(frame_bgr, input_size=INPUT_SIZE, mean=MEAN, std=STD):
    """one BGR uint8 frame -> (normalised fp32 [3, h, w], center, scale)"""
    H, W = frame_bgr.shape[:2]
    center, scale = bbox_center_scale(W, H, input_size=input_size)
    Minv = invert_affine(warp_matrix(center, scale, input_size))
    return normalise(warp_affine_int(frame_bgr, Minv, input_size), mean, std), center, scale


# ---- post-processing ----------------------------------------------------------------------------------------------------------------------------
def flip_average(x, y, xf, yf, pairs):
    """flip_test: flip_vectors of the flipped pass (keypoints swapped, the bin axis of simcc_x reversed), averaged with the straight pass; fp32 in, fp32 out"""
    pairs = np.asarray(pairs)
    xf, yf = xf[:, pairs][:, :, ::-1], yf[:, pairs]
    return (x + xf) * np.float32(0.5), (y + yf) * np.float32(0.5)


def simcc_maximum(x, y):
    """get_simcc_maximum: np.argmax takes the first maximum; score = the smaller maximum; location -1 where the score <= 0"""
    xl, yl = np.argmax(x, axis=-1), np.argmax(y, axis=-1)
    vals = np.minimum(np.max(x, axis=-1), np.max(y, axis=-1))
    locs = np.stack([xl, yl], axis=-1).astype(np.float32)
    locs[vals <= 0.0] = -1
    return locs, vals


def decode(x, y, center, scale, xf=None, yf=None, pairs=None, input_size=INPUT_SIZE):
    """SimCC logits [B, K, *] -> (keypoints fp32 [B, K, 2] in frame pixels, scores fp32 [B, K]).  The map back
    `keypoints / input_size * scale + center - 0.5 * scale` is taken in fp32, one rounding per operation in that order (mmpose mixes fp32 and fp64 here; the
    difference is far below the truncation to pixels that follows)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if xf is not None:
        x, y = flip_average(x, y, np.asarray(xf, np.float32), np.asarray(yf, np.float32), pairs)
    locs, vals = simcc_maximum(x, y)
    k = locs / np.float32(SPLIT)
    c, s, isz = np.asarray(center, np.float32), np.asarray(scale, np.float32), np.asarray(input_size, np.float32)
    return ((k / isz) * s + c) - s * np.float32(0.5), vals.astype(np.float32)


# ---- preprocessing.py:100-101, 113-131 -------------------------------------------------------------------------------------------------------------
COORD_PLACEHOLDER = (0.0, 0.0, 0.0, 0.0)
FLAG_PLACEHOLDER, FLAG_LANDMARK, FLAG_DETECTOR = 0, 1, 2


def landmark_boxes(keypoints, det_boxes, bbox_shift=0):
    """keypoints: [n, 133, 2]; det_boxes: per frame the detector's (x1, y1, x2, y2) ints or None.  Returns (coord_list, flags, (sum range_minus, sum range_plus,
    frames counted)): the loop of get_landmark_and_bbox with batch size 1."""
    coords, flags, minus, plus = [], [], [], []
    for kp, f in zip(keypoints, det_boxes):
        lm = np.asarray(kp)[FACE].astype(np.int32)                              # :100-101: truncation toward zero
        if f is None:
            coords.append(COORD_PLACEHOLDER); flags.append(FLAG_PLACEHOLDER)
            continue
        half = lm[29]                                                           # a view, as in the reference: the shift below moves row 29 of lm itself
        minus.append(int(lm[30][1] - lm[29][1]))
        plus.append(int(lm[29][1] - lm[28][1]))
        if bbox_shift != 0:
            half[1] = bbox_shift + half[1]
        half_face_dist = np.max(lm[:, 1]) - half[1]
        upper_bond = half[1] - half_face_dist
        x1, y1, x2, y2 = int(np.min(lm[:, 0])), int(upper_bond), int(np.max(lm[:, 0])), int(np.max(lm[:, 1]))
        if y2 - y1 <= 0 or x2 - x1 <= 0 or x1 < 0:
            coords.append(tuple(int(v) for v in f)); flags.append(FLAG_DETECTOR)
        else:
            coords.append((x1, y1, x2, y2)); flags.append(FLAG_LANDMARK)
    return coords, flags, (sum(minus), sum(plus), len(minus))


def range_text(n_frames, sums, bbox_shift=0):
    """:134 (the reference divides by the number of frames with a face; with none it raises ZeroDivisionError, here the range reads 0~0)"""
    sm, sp, cnt = sums
    a, b = (int(sm / cnt), int(sp / cnt)) if cnt else (0, 0)
    return f"Total frame:「{n_frames}」 Manually adjust range : [ -{a}~{b} ] , the current value: {bbox_shift}"


def detector_box(row, W, H):
    """face_detection/api.py:74-78 as avatar/prepare.py restates it: clipped at 0, truncated, clipped to the frame"""
    r = np.clip(np.asarray(row[:4], np.float32), 0, None)
    return (min(int(r[0]), W), min(int(r[1]), H), min(int(r[2]), W), min(int(r[3]), H))
