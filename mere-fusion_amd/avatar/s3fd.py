"""`s3fd` drop-in (face_detection/detection/sfd/net_s3fd.py:22-129; identical copies under wav2lip/ and musetalk/utils/).

`SFDDetector.__init__` does `self.face_detector = s3fd(); .load_state_dict(weights); .to(device); .eval()` and `detect` / `batch_detect`
call `net(img)` on a float tensor [B, 3, H, W] (BGR minus the channel means, sfd/detect.py:19-33,54-66), reading back the list
[cls1, reg1, ..., cls6, reg6].  Same surface here; the 12 tensors stay on the device (the reference's softmax / threshold / decode /
nms code runs on them unchanged).  One graph per input size; conf and loc heads of a level share one convolution.

`detect` goes further and ends in boxes: uint8 frames in, the graph, then softmax / threshold / decode / NMS as HIP kernels on the head buffers
in place (csrc/mf_s3fd_detect.hip).  `face_detection.py` beside this file wraps it in the reference's `SFDDetector` / `FaceAlignment` surface."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .net import Net

_TRUNK = [("conv1_1", 3, 64), ("conv1_2", 64, 64), "pool", ("conv2_1", 64, 128), ("conv2_2", 128, 128), "pool",
          ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), "pool",
          ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512), "pool",
          ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512), "pool"]

CAND_THRESH, NMS_THRESH, FINAL_THRESH = 0.05, 0.3, 0.5       # sfd/detect.py:79, sfd_detector.py:43,45
MAX_CANDIDATES, MAX_DET = 4096, 256                          # per image; 4096 is what the NMS kernel's workgroup sorts in LDS
MEAN = (104.0, 117.0, 123.0)                                 # sfd/detect.py:59


class s3fd:
    def __init__(self, precision="bf16x3", max_batch=16, device="cuda"):
        self.precision, self.max_batch, self.device = precision, max_batch, torch.device(device)
        self._sd, self._nets = None, {}

    def load_state_dict(self, sd, strict=True):
        self._sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}
        self._nets = {}
        return self

    def to(self, device):
        return self

    def eval(self):
        return self

    def _build(self, H, W):
        sd = self._sd
        n = Net(self.max_batch, self.precision, self.device)
        g = dict(net=n, taps={})
        x = g["inp"] = n.buffer(3, H, W, 1)
        h, w = H, W
        for idx, item in enumerate(_TRUNK):
            if item == "pool":                                           # F.max_pool2d(h, 2, 2)
                h, w = h // 2, w // 2
                if h < 1 or w < 1:
                    raise ValueError(f"s3fd: a {H}x{W} image is too small for the five pooling stages")
                y = n.buffer(n.shape[x][0], h, w, 3 if idx == len(_TRUNK) - 1 else 1)        # fc6 pads by 3
                n.maxpool(x, y, 2, 2)
            else:
                name, ci, co = item
                y = n.buffer(co, h, w, 1)
                n.conv(sd[name + ".weight"], x, y, 1, 1, act=1, bias=sd[name + ".bias"], name=name)
                if name in ("conv3_3", "conv4_3", "conv5_3"):
                    g["taps"][name] = (y, co, h, w)
            x = y
        # fc6: Conv2d(512, 1024, 3, 1, 3) -- padding 3, so the map grows by 4 (the last pool's buffer carries a halo of 3)
        h, w = h + 4, w + 4
        y = n.buffer(1024, h, w, 1); n.conv(sd["fc6.weight"], x, y, 1, 3, act=1, bias=sd["fc6.bias"], name="fc6"); x = y
        y = n.buffer(1024, h, w, 1); n.conv(sd["fc7.weight"], x, y, 1, 0, act=1, bias=sd["fc7.bias"], name="fc7"); x = y
        feats = []
        for name, scale_key in (("conv3_3", "conv3_3_norm"), ("conv4_3", "conv4_3_norm"), ("conv5_3", "conv5_3_norm")):
            b, co, fh, fw = g["taps"][name]
            nb = n.buffer(co, fh, fw, 1)
            n.l2norm(b, nb, sd[scale_key + ".weight"], 1e-10)
            feats.append((scale_key, nb, fh, fw))
        feats.append(("fc7", x, h, w))
        y = n.buffer(256, h, w, 1); n.conv(sd["conv6_1.weight"], x, y, 1, 0, act=1, bias=sd["conv6_1.bias"], name="conv6_1"); x = y
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        y = n.buffer(512, h, w, 1); n.conv(sd["conv6_2.weight"], x, y, 2, 1, act=1, bias=sd["conv6_2.bias"], name="conv6_2"); x = y
        feats.append(("conv6_2", x, h, w))
        y = n.buffer(128, h, w, 1); n.conv(sd["conv7_1.weight"], x, y, 1, 0, act=1, bias=sd["conv7_1.bias"], name="conv7_1"); x = y
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        y = n.buffer(256, h, w, 1); n.conv(sd["conv7_2.weight"], x, y, 2, 1, act=1, bias=sd["conv7_2.bias"], name="conv7_2"); x = y
        feats.append(("conv7_2", x, h, w))
        # heads: conf | loc of one level as one 3x3 convolution with 8 output channels (conf padded to 4)
        g["heads"] = []
        for key, fb, fh, fw in feats:
            wc, bc = sd[key + "_mbox_conf.weight"], sd[key + "_mbox_conf.bias"]
            wl, bl = sd[key + "_mbox_loc.weight"], sd[key + "_mbox_loc.bias"]
            nc = wc.shape[0]
            wcat = torch.zeros((8,) + tuple(wc.shape[1:]))
            bcat = torch.zeros(8)
            wcat[:nc], wcat[4:8], bcat[:nc], bcat[4:8] = wc, wl, bc, bl
            ob = n.buffer(8, fh, fw, 0)
            n.conv(wcat, fb, ob, 1, 1, act=0, bias=bcat, name=key + "_mbox")
            g["heads"].append((ob, nc))
        return g

    def __call__(self, x):
        if self._sd is None:
            raise RuntimeError("s3fd: load_state_dict first (sfd_detector.py:27-28)")
        x = torch.as_tensor(x)
        B, Cn, H, W = x.shape
        if B > self.max_batch:
            raise ValueError(f"s3fd: batch {B} exceeds max_batch {self.max_batch}")
        g = self._nets.get((H, W))
        if g is None:
            g = self._nets[(H, W)] = self._build(H, W)
        n = g["net"]
        n.set_input(g["inp"], x)
        n.run(B)
        outs = []
        for i, (ob, nc) in enumerate(g["heads"]):
            cls = n.output(ob, nc, B, coff=0)
            if i == 0:                                                   # max-out background label (net_s3fd.py:123-126)
                c2 = torch.empty((B, 2) + tuple(cls.shape[2:]), dtype=torch.float32, device=cls.device)
                _lib.check(_lib.lib().mf_s3fd_maxout_bg(C.c_void_p(cls.data_ptr()), C.c_void_p(c2.data_ptr()), B, cls.shape[2] * cls.shape[3],
                                                        _lib.stream_ptr(cls.device)), "s3fd_maxout_bg")
                cls = c2
            outs += [cls, n.output(ob, 4, B, coff=4)]
        return outs

    forward = __call__

    # ---- boxes ---------------------------------------------------------------------------------------------------------------------
    def detect(self, images_u8, cand_thresh=CAND_THRESH, nms_thresh=NMS_THRESH, final_thresh=FINAL_THRESH, max_candidates=MAX_CANDIDATES, max_det=MAX_DET,
               reverse_channels=False, mean=MEAN):
        """uint8 [B, H, W, 3] frames (numpy or tensor) -> (boxes [B, max_det, 5] fp32, counts [B] int32, n_candidates [B] int32), all on the device and
        without a host sync: boxes[b, :counts[b]] are the rows (x1, y1, x2, y2, score) `SFDDetector.detect_from_batch` returns for image b, in its order.
        `check_counts` turns the two counters into the overflow errors; `boxes_to_lists` into the reference's lists."""
        if self._sd is None:
            raise RuntimeError("s3fd: load_state_dict first (sfd_detector.py:27-28)")
        x = torch.as_tensor(np.ascontiguousarray(images_u8) if isinstance(images_u8, np.ndarray) else images_u8)
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"s3fd.detect: uint8 [B, H, W, 3] frames expected, got {x.dtype} {tuple(x.shape)}")
        B, H, W, _ = x.shape
        if B > self.max_batch:
            raise ValueError(f"s3fd: batch {B} exceeds max_batch {self.max_batch}")
        g = self._nets.get((H, W))
        if g is None:
            g = self._nets[(H, W)] = self._build(H, W)
        n = g["net"]
        x = x.to(self.device).contiguous()
        n.set_input_u8(g["inp"], x, mean, reverse_channels)
        n.run(B)
        boxes, counts, ncand = _outputs(B, max_det, self.device)
        bufs = (C.c_int * 6)(*[ob for ob, _ in g["heads"]])
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mf_s3fd_detect(n._h, bufs, B, cand_thresh, nms_thresh, final_thresh, int(max_candidates), int(max_det), C.c_void_p(boxes.data_ptr()),
                                                 C.c_void_p(counts.data_ptr()), C.c_void_p(ncand.data_ptr()), n._stream()), "s3fd_detect")
        return boxes, counts, ncand


def _outputs(B, max_det, device):
    return (torch.zeros((B, int(max_det), 5), dtype=torch.float32, device=device), torch.zeros(B, dtype=torch.int32, device=device),
            torch.zeros(B, dtype=torch.int32, device=device))


def detect_from_heads(olist, cand_thresh=CAND_THRESH, nms_thresh=NMS_THRESH, final_thresh=FINAL_THRESH, max_candidates=MAX_CANDIDATES, max_det=MAX_DET):
    """The post-process alone, on the twelve tensors [cls1, reg1, ..., cls6, reg6] `s3fd.__call__` returns (device fp32): same outputs as `s3fd.detect`."""
    if len(olist) != 12:
        raise ValueError(f"detect_from_heads: 12 head tensors expected, got {len(olist)}")
    dev = olist[0].device
    if dev.type != "cuda":
        raise RuntimeError("detect_from_heads: the head tensors must be on a HIP device; no CPU path exists here")
    _lib.init_device(dev.index if dev.index is not None else torch.cuda.current_device())
    ts = [t.to(dev, torch.float32).contiguous() for t in olist]
    B = ts[0].shape[0]
    hw = []
    for l in range(6):
        c, r = ts[2 * l], ts[2 * l + 1]
        if c.dim() != 4 or tuple(c.shape[:2]) != (B, 2) or tuple(r.shape) != (B, 4) + tuple(c.shape[2:]):
            raise ValueError(f"detect_from_heads: level {l + 1} has cls {tuple(c.shape)} / reg {tuple(r.shape)}, expected [B, 2, h, w] / [B, 4, h, w]")
        hw += [c.shape[2], c.shape[3]]
    boxes, counts, ncand = _outputs(B, max_det, dev)
    lib = _lib.lib()
    ws = torch.empty(max(1, lib.mf_s3fd_detect_workspace_bytes(B, int(max_candidates))), dtype=torch.uint8, device=dev)
    heads = (C.c_void_p * 12)(*[t.data_ptr() for t in ts])
    with torch.cuda.device(dev):
        _lib.check(lib.mf_s3fd_detect_tensors(heads, (C.c_int * 12)(*hw), B, cand_thresh, nms_thresh, final_thresh, int(max_candidates), int(max_det),
                                              C.c_void_p(ws.data_ptr()), C.c_void_p(boxes.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(ncand.data_ptr()),
                                              _lib.stream_ptr(dev)), "s3fd_detect_tensors")
    return boxes, counts, ncand


def check_counts(counts, n_candidates, max_candidates=MAX_CANDIDATES, max_det=MAX_DET):
    """The one host sync of a detection: reads the counters, raises on a capacity overflow (no host fallback), returns counts as a list."""
    cn = torch.stack([counts, n_candidates]).cpu().numpy()
    for b in range(cn.shape[1]):
        if cn[1, b] > max_candidates:
            raise RuntimeError(f"s3fd detect: image {b} has {int(cn[1, b])} candidates, more than the capacity max_candidates = {int(max_candidates)}; "
                               "raise max_candidates (at most 4096) or cand_thresh")
        if cn[0, b] > max_det:
            raise RuntimeError(f"s3fd detect: image {b} keeps {int(cn[0, b])} boxes, more than the capacity max_det = {int(max_det)}")
    return [int(c) for c in cn[0]]


def boxes_to_lists(boxes, counts, n_candidates, max_candidates=MAX_CANDIDATES, max_det=MAX_DET):
    """-> per image a list of float32 [x1, y1, x2, y2, score] rows in keep order (what sfd_detector.py:41-47 returns)"""
    cnt = check_counts(counts, n_candidates, max_candidates, max_det)
    rows = boxes.cpu().numpy()
    return [[rows[b, i] for i in range(c)] for b, c in enumerate(cnt)]
