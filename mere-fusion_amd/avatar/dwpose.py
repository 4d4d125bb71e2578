"""DWPose, the whole-body landmark network of musetalk/utils/preprocessing.py:17-19 (`init_model(rtmpose-l_8xb32-270e_coco-ubody-wholebody-384x288.py,
dw-ll_ucoco_384.pth)`), and mmpose's `inference_topdown(model, frame)` around it, on the device.

    pose = DWPose(max_batch=8); pose.load_state_dict(torch.load("dw-ll_ucoco_384.pth")["state_dict"])
    kpts, scores = pose.keypoints(frames_u8)              # device fp32 [n, 133, 2] in frame pixels, [n, 133]

The module tree is mmdet's CSPNeXt (stem, four stages of conv / [SPP] / CSPLayer with channel attention) and mmpose's RTMCCHead; state-dict keys are those of the
mmpose checkpoint (`backbone.stage1.1.blocks.0.conv2.depthwise_conv.conv.weight`, `head.gau.uv.weight`, ...).  Width, depth and the head's sizes are read from the
tensors' shapes, so a reduced net loads the same way.  Top-down steps as mmpose runs them for a call without boxes: the whole-image box, GetBBoxCenterScale
(padding 1.25), the aspect-ratio fix, the three-point affine map, cv2.warpAffine as an integer model (mf_warp_affine_u8), both passes of flip_test, SimCC decode.
Parity is unpinned: mmpose / mmdet / OpenCV are not available to the tests, which hold this to a restatement of the published modules.  No CPU path."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .net import Net

INPUT_SIZE = (288, 384)                                   # (w, h)
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
PADDING = 1.25
ARCH_P5 = ((64, 128, 3, True, False), (128, 256, 6, True, False), (256, 512, 6, True, False), (512, 1024, 3, False, True))   # mmdet CSPNeXt.arch_settings['P5']


def flip_indices():
    """COCO-WholeBody's left / right permutation (dataset meta `flip_indices`): 17 body, 6 feet, 68 face, 2 x 21 hand keypoints"""
    p = list(range(133))
    pairs = [(a, a + 1) for a in range(1, 17, 2)] + [(17, 20), (18, 21), (19, 22)]
    pairs += [(23 + i, 39 - i) for i in range(8)] + [(40 + i, 49 - i) for i in range(5)] + [(54, 58), (55, 57)]
    pairs += [(59, 68), (60, 67), (61, 66), (62, 65), (63, 70), (64, 69)]
    pairs += [(71, 77), (72, 76), (73, 75), (78, 82), (79, 81), (83, 87), (84, 86), (88, 90)]
    pairs += [(91 + i, 112 + i) for i in range(21)]
    for a, b in pairs:
        p[a], p[b] = b, a
    return p


def topdown_affine(w, h, input_size=INPUT_SIZE, padding=PADDING):
    """(center fp32 [2], scale fp32 [2], Minv float64 [2, 3]) of the whole-image box of a w x h frame: bbox_xyxy2cs, TopdownAffine._fix_aspect_ratio,
    get_warp_matrix(rot=0) solved from its three point pairs in float64, and the inverse cv2.warpAffine walks (cv2.invertAffineTransform's formulas)"""
    box = np.array([0, 0, w, h], np.float32)
    center = (box[2:] + box[:2]) * np.float32(0.5)
    scale = (box[2:] - box[:2]) * np.float32(padding)
    aspect = np.float32(input_size[0] / input_size[1])
    bw, bh = scale
    scale = np.array([bw, bw / aspect], np.float32) if bw > bh * aspect else np.array([bh * aspect, bh], np.float32)

    def third(a, b):
        d = a - b
        return b + np.array([-d[1], d[0]])
    c64, s64 = center.astype(np.float64), scale.astype(np.float64)
    dw, dh = input_size
    src, dst = np.zeros((3, 2)), np.zeros((3, 2))
    src[0] = c64
    src[1] = c64 + np.array([0.0, s64[0] * -0.5])
    src[2] = third(src[0], src[1])
    dst[0] = [dw * 0.5, dh * 0.5]
    dst[1] = dst[0] + np.array([0.0, dw * -0.5])
    dst[2] = third(dst[0], dst[1])
    M = np.linalg.solve(np.hstack([src, np.ones((3, 1))]), dst).T
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[1, 1] * D, M[0, 0] * D, -M[0, 1] * D, -M[1, 0] * D
    Minv = np.array([[A11, A12, -A11 * M[0, 2] - A12 * M[1, 2]], [A21, A22, -A21 * M[0, 2] - A22 * M[1, 2]]])
    return center, scale, Minv


class DWPose:
    def __init__(self, precision="bf16x3", max_batch=1, device="cuda", input_size=INPUT_SIZE, bn_eps=1e-3):
        """bn_eps: 1e-3 is the default norm_cfg of mmdet's CSPNeXt (eval-mode BatchNorm; momentum plays no part)"""
        self.precision, self.max_batch, self.device, self.input_size, self.bn_eps = precision, int(max_batch), torch.device(device), tuple(input_size), float(bn_eps)
        self._sd, self._g, self._head = None, None, None

    def load_state_dict(self, sd, strict=True):
        """mmpose checkpoint keys.  strict: the key set and the shapes must be those of the net the tensors themselves describe (weights.dwpose_manifest for the width,
        depth and head sizes found), else a RuntimeError lists what is missing, unexpected or misshapen -- as nn.Module.load_state_dict does."""
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        if strict:
            self._check_keys(sd)
        self._sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
        self._drop()
        return self

    def _check_keys(self, sd):
        from ..weights import dwpose_manifest
        need = ("backbone.stem.2.conv.weight", "head.final_layer.weight", "head.mlp.1.weight", "head.gau.gamma")
        lost = [k for k in need if k not in sd]
        if lost:
            raise RuntimeError(f"DWPose.load_state_dict: missing key(s) {lost}")
        widen = sd["backbone.stem.2.conv.weight"].shape[0] / 64.0
        blocks = [len({k.split(".")[4] for k in sd if k.startswith(f"backbone.stage{i}.{2 if i == 4 else 1}.blocks.")}) for i in (1, 2, 3, 4)]
        deepen = blocks[1] / 6.0
        want = dict(dwpose_manifest(deepen=deepen, widen=widen, input_size=self.input_size, keypoints=sd["head.final_layer.weight"].shape[0],
                                    hidden=sd["head.mlp.1.weight"].shape[0], s=sd["head.gau.gamma"].shape[1]))
        missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
        shape = [k for k in want if k in sd and tuple(sd[k].shape) != tuple(want[k])]
        if missing or extra or shape:
            raise RuntimeError(f"DWPose.load_state_dict (strict): missing {missing[:8]}, unexpected {extra[:8]}, wrong shape {shape[:8]} "
                               f"(for widen {widen:g}, deepen {deepen:g}, input {self.input_size})")

    def _drop(self):
        if self._head:
            _lib.lib().mf_rtmcc_head_destroy(self._head)
        self._g, self._head = None, None

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def cuda(self):
        return self

    def to(self, device):
        return self

    def eval(self):
        return self

    # ---- module tree -> ops ---------------------------------------------------------------------------------------------------
    def _cm(self, n, p, x, y, stride=1, pad=0, **kw):
        """ConvModule: conv (no bias) + eval BatchNorm folded here in float64 (its eps is not the builder's) + SiLU"""
        sd = self._sd
        w = sd[p + ".conv.weight"].double()
        sc = sd[p + ".bn.weight"].double() / torch.sqrt(sd[p + ".bn.running_var"].double() + self.bn_eps)
        n.conv((w * sc.view(-1, 1, 1, 1)).float(), x, y, stride, pad, act=4, bias=(sd[p + ".bn.bias"].double() - sd[p + ".bn.running_mean"].double() * sc).float(), name=p, **kw)

    def _csp(self, n, p, x, c, nb, add_identity, h, w, out_halo):
        """CSPLayer: [blocks(main_conv(x)) | short_conv(x)] as channel slices of one buffer -> channel attention -> final_conv"""
        sd, mid = self._sd, c // 2
        cat = n.buffer(2 * mid, h, w, 0)
        self._cm(n, p + ".short_conv", x, cat, out_coff=mid)
        m = n.buffer(mid, h, w, 1)
        self._cm(n, p + ".main_conv", x, m)
        for b in range(nb):
            q = f"{p}.blocks.{b}"
            t, d = n.buffer(mid, h, w, 0), n.buffer(mid, h, w, 0)
            self._cm(n, q + ".conv1", m, t, 1, 1)
            dw = q + ".conv2.depthwise_conv"
            n.dwconv(sd[dw + ".conv.weight"], t, d, 1, act=4, bn=tuple(sd[f"{dw}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")), bn_eps=self.bn_eps)
            last = b == nb - 1
            o = cat if last else n.buffer(mid, h, w, 1)
            res = dict(res_buf=m, res_after_act=True) if add_identity else {}
            self._cm(n, q + ".conv2.pointwise_conv", d, o, **res)
            m = o
        pooled, att = n.buffer(2 * mid, 1, 1, 0), n.buffer(2 * mid, h, w, 0)
        n.global_avgpool(cat, 2 * mid, pooled)
        n.chan_attn(cat, 2 * mid, pooled, sd[p + ".attention.fc.weight"], sd[p + ".attention.fc.bias"], att)
        y = n.buffer(c, h, w, out_halo)
        self._cm(n, p + ".final_conv", att, y)
        return y

    def _spp(self, n, p, x, c, h, w):
        """SPPBottleneck, kernel sizes (5, 9, 13): a 9 (13) window max is two (three) 5 windows in a row, -inf padding included"""
        mid = c // 2
        cat = n.buffer(4 * mid, h, w, 0)
        t = n.buffer(mid, h, w, 0)
        self._cm(n, p + ".conv1", x, t)
        n.scale_add(t, mid, cat)
        for i in (1, 2, 3):
            nx = n.buffer(mid, h, w, 0)
            n.maxpool(t, nx, 5, 1, 2)
            n.scale_add(nx, mid, cat, out_coff=i * mid)
            t = nx
        y = n.buffer(c, h, w, 0)
        self._cm(n, p + ".conv2", cat, y)
        return y

    def _build(self):
        sd = self._sd
        W, H = self.input_size
        if W % 32 or H % 32:
            raise ValueError(f"DWPose: the input size {self.input_size} must be a multiple of 32")
        n = Net(2 * self.max_batch, self.precision, self.device)                # the straight images, then their mirrors
        g = dict(net=n)
        x = g["inp"] = n.buffer(3, H, W, 1)
        c = sd["backbone.stem.2.conv.weight"].shape[0]
        h, w = H // 2, W // 2
        a, b, y = n.buffer(c // 2, h, w, 1), n.buffer(c // 2, h, w, 1), n.buffer(c, h, w, 1)
        self._cm(n, "backbone.stem.0", x, a, 2, 1); self._cm(n, "backbone.stem.1", a, b, 1, 1); self._cm(n, "backbone.stem.2", b, y, 1, 1)
        x = y
        for i, (_, _, _, add_identity, spp) in enumerate(ARCH_P5, 1):
            p = f"backbone.stage{i}"
            c = sd[p + ".0.conv.weight"].shape[0]
            h, w = h // 2, w // 2
            y = n.buffer(c, h, w, 0)
            self._cm(n, p + ".0", x, y, 2, 1)
            j = 1
            if spp:
                y, j = self._spp(n, p + ".1", y, c, h, w), 2
            nb = len({k.split(".")[4] for k in sd if k.startswith(f"{p}.{j}.blocks.")})
            x = self._csp(n, f"{p}.{j}", y, c, nb, add_identity, h, w, 3 if i == 4 else 1)
        # RTMCCHead.final_layer (rows padded to a multiple of 4, like the parser's output conv)
        wf, bf = sd["head.final_layer.weight"], sd["head.final_layer.bias"]
        K = wf.shape[0]
        kp = (K + 3) // 4 * 4
        wp, bp = torch.zeros((kp,) + tuple(wf.shape[1:])), torch.zeros(kp)
        wp[:K], bp[:K] = wf, bf
        maps = g["maps"] = n.buffer(kp, h, w, 0)
        n.conv(wp, x, maps, 1, wf.shape[2] // 2, act=0, bias=bp, name="head.final_layer")
        hidden, s = sd["head.mlp.1.weight"].shape[0], sd["head.gau.gamma"].shape[1]
        if sd["head.mlp.1.weight"].shape[1] != h * w or sd["head.gau.uv.weight"].shape[0] != 4 * hidden + s:
            raise ValueError("DWPose: the head's tensors do not match the input size (flatten dims) or expansion factor 2")
        g.update(K=K, bx=sd["head.cls_x.weight"].shape[0], by=sd["head.cls_y.weight"].shape[0])
        t = {k: sd["head." + k].contiguous() for k in ("mlp.0.g", "mlp.1.weight", "gau.ln.g", "gau.uv.weight", "gau.gamma", "gau.beta", "gau.o.weight", "gau.res_scale.scale",
                                                       "cls_x.weight", "cls_y.weight")}
        hh = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_rtmcc_head_create(K, h * w, hidden, s, g["bx"], g["by"], *[C.c_void_p(v.data_ptr()) for v in t.values()], 2 * self.max_batch,
                                                       C.byref(hh)), "rtmcc_head_create")
        self._head, self._g = hh.value, g
        return g

    # ---- execution -------------------------------------------------------------------------------------------------------------
    def logits(self, frames_u8, flip=True):
        """uint8 BGR device frames [n, H, W, 3] -> (simcc_x [n, K, 2w], simcc_y [n, K, 2h], the two of the mirrored pass or None, None), fp32 on the device"""
        if self._sd is None:
            raise RuntimeError("DWPose: load_state_dict first (preprocessing.py:18-19)")
        fr = frames_u8
        if not (torch.is_tensor(fr) and fr.is_cuda and fr.dtype == torch.uint8 and fr.dim() == 4 and fr.shape[3] == 3):
            raise RuntimeError("DWPose needs uint8 [n, H, W, 3] frames on the HIP device; no CPU path exists here")
        n = int(fr.shape[0])
        if n < 1 or n > self.max_batch:
            raise ValueError(f"DWPose: {n} frames for max_batch {self.max_batch}")
        g = self._g or self._build()
        net, fr = g["net"], fr.contiguous()
        H, W = int(fr.shape[1]), int(fr.shape[2])
        _, _, Minv = topdown_affine(W, H, self.input_size)
        minv = torch.from_numpy(np.tile(Minv.reshape(1, 6), (n, 1))).to(self.device)
        B = 2 * n if flip else n
        lx = torch.empty((B, g["K"], g["bx"]), dtype=torch.float32, device=self.device)
        ly = torch.empty((B, g["K"], g["by"]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_warp_affine_u8(net._h, g["inp"], C.c_void_p(fr.data_ptr()), n, H, W, C.c_void_p(minv.data_ptr()), (C.c_float * 3)(*MEAN),
                                                    (C.c_float * 3)(*STD), 1, int(bool(flip)), _lib.stream_ptr(self.device)), "warp_affine_u8")
            net.run(B)
            _lib.check(_lib.lib().mf_rtmcc_head_forward(self._head, net._h, g["maps"], 0, B, C.c_void_p(lx.data_ptr()), C.c_void_p(ly.data_ptr()), _lib.stream_ptr(self.device)),
                       "rtmcc_head_forward")
        return (lx[:n], ly[:n], lx[n:], ly[n:]) if flip else (lx, ly, None, None)

    def decode(self, lx, ly, fx, fy, W, H):
        """mf_simcc_decode for frames of W x H: (kpts fp32 [n, K, 2], scores fp32 [n, K]) on the device, nothing synchronised"""
        center, scale, _ = topdown_affine(W, H, self.input_size)
        return simcc_decode(lx, ly, fx, fy, flip_indices() if fx is not None else None, self.input_size, center, scale)

    def keypoints(self, frames_u8):
        lx, ly, fx, fy = self.logits(frames_u8, flip=True)                      # test_cfg flip_test=True
        return self.decode(lx, ly, fx, fy, int(frames_u8.shape[2]), int(frames_u8.shape[1]))


def simcc_decode(lx, ly, fx, fy, pairs, input_size, center, scale):
    if not (torch.is_tensor(lx) and lx.is_cuda and lx.dtype == torch.float32 and lx.dim() == 3 and ly.shape[:2] == lx.shape[:2]):
        raise RuntimeError("simcc_decode needs fp32 [n, K, bins] logits on the HIP device; no CPU path exists here")
    lx, ly = lx.contiguous(), ly.contiguous()
    fx, fy = (None, None) if fx is None else (fx.contiguous(), fy.contiguous())
    n, K = int(lx.shape[0]), int(lx.shape[1])
    if pairs is not None and len(pairs) != K:
        raise ValueError(f"{len(pairs)} flip indices for {K} keypoints")
    kpts = torch.empty((n, K, 2), dtype=torch.float32, device=lx.device)
    scores = torch.empty((n, K), dtype=torch.float32, device=lx.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(lx.device):
        _lib.check(_lib.lib().mf_simcc_decode(p(lx), p(ly), p(fx), p(fy), (C.c_int * K)(*[int(v) for v in pairs]) if pairs is not None else None, n, K, int(lx.shape[2]),
                                              int(ly.shape[2]), int(input_size[0]), int(input_size[1]), (C.c_float * 2)(*[float(v) for v in center]),
                                              (C.c_float * 2)(*[float(v) for v in scale]), p(kpts), p(scores),
                                              _lib.stream_ptr(lx.device)), "simcc_decode")
    return kpts, scores
