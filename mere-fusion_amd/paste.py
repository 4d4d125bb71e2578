"""Paste-back of generated faces into the cached full frames on the GPU: thin host side of `mf_paste_frames`.

The reference does this per frame on the host after a D2H of every generated face (lipreal.py:207-214; musereal.py:238-247 +
musetalk/utils/blending.py:103-125).  Here the avatar's full frames, bboxes and masks are cached on the device once and a batch of
generated faces is composed into a batch of uint8 BGR frames in one launch; results are bit-exact with OpenCV's 8-bit arithmetic
(csrc/mf_blend.hip).  There is no CPU path."""
import numpy as np
import torch

from . import _lib
from .ops import frames_to_i420, gather_frames                       # noqa: F401  (re-exported: the frames' last launches before the ring)


def _dev_u8(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != torch.uint8:
        raise RuntimeError(f"expected a uint8 image, got {t.dtype}")
    return t.to(device).contiguous()


class AvatarFrames:
    """Device-resident cache of one avatar's full frames and paste geometry.

    frames      : [n, H, W, 3] uint8 BGR        (frame_list_cycle, lipreal.py:174-179 / musereal.py:169-179)
    bboxes      : n x (x1, y1, x2, y2)           MuseTalk order (coords.pkl, musereal.py:239); for Wav2Lip avatars pass `lip_order=True`
                                                 and the reference's (y1, y2, x1, x2) tuples (lipreal.py:208)
    masks       : n uint8 [h_i, w_i, 3] BGR images (mask_list_cycle) or None (Wav2Lip: rectangle copy)
    crop_boxes  : n x (x_s, y_s, x_e, y_e)       mask_coords_list_cycle
    """

    def __init__(self, frames, bboxes, masks=None, crop_boxes=None, lip_order=False, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("AvatarFrames needs a HIP device; no CPU path exists here")
        self.device = torch.device(device)
        fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in frames])))
        self.frames = _dev_u8(fr, self.device)
        if self.frames.dim() != 4 or self.frames.shape[3] != 3:
            raise RuntimeError(f"frames must be [n, H, W, 3], got {tuple(self.frames.shape)}")
        self.n, self.H, self.W = self.frames.shape[0], self.frames.shape[1], self.frames.shape[2]
        self.bboxes = [(int(b[2]), int(b[0]), int(b[3]), int(b[1])) if lip_order else tuple(int(v) for v in b) for b in bboxes]
        if len(self.bboxes) != self.n:
            raise RuntimeError("one bbox per cached frame is required")
        self.masks = None if masks is None else [_dev_u8(m, self.device) for m in masks]
        self.crop_boxes = None if crop_boxes is None else [tuple(int(v) for v in c) for c in crop_boxes]
        if self.masks is not None:
            if self.crop_boxes is None or len(self.masks) != self.n or len(self.crop_boxes) != self.n:
                raise RuntimeError("masks need one crop box per cached frame")
            for m, (xs, ys, xe, ye) in zip(self.masks, self.crop_boxes):
                if tuple(m.shape) != (ye - ys, xe - xs, 3):
                    raise RuntimeError(f"mask shape {tuple(m.shape)} does not match its crop box {(xs, ys, xe, ye)}")

    def source(self, i):
        """the device view of cached full frame i, uint8 [H, W, 3]: what a listening session shows (`frame_list_cycle[idx]`, lipreal.py:205 / musereal.py:236) and
        what ops.gather_frames takes as a source"""
        if not 0 <= int(i) < self.n:
            raise RuntimeError(f"AvatarFrames.source: frame {i} of {self.n}")
        return self.frames[int(i)]

    def jobs(self, indices):
        arr = (_lib.MfPasteJob * len(indices))()
        for k, i in enumerate(indices):
            j = arr[k]
            j.frame_index = int(i)
            j.x1, j.y1, j.x2, j.y2 = self.bboxes[i]
            if self.masks is not None:
                j.cx1, j.cy1, j.cx2, j.cy2 = self.crop_boxes[i]
                j.mask = self.masks[i].data_ptr()
            else:
                j.mask = None
        return arr

    def paste(self, res, indices, out=None):
        """res: device [B, S, S', 3] uint8 (MuseTalk frames) or fp32 (Wav2Lip `pred * 255`); indices: the B cached-frame indices
        (mirror index of each result).  Returns uint8 [B, H, W, 3] on the device."""
        if not res.is_cuda:
            raise RuntimeError("paste needs the generated frames on the HIP device; no CPU path exists here")
        if res.dtype not in (torch.uint8, torch.float32) or res.dim() != 4 or res.shape[3] != 3 or res.shape[0] != len(indices):
            raise RuntimeError(f"res must be uint8 / float32 [B, h, w, 3] with B = {len(indices)}, got {res.dtype} {tuple(res.shape)}")
        res = res.contiguous()
        B = res.shape[0]
        if out is None:
            out = torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device=res.device)
        jobs = self.jobs(list(indices))
        with torch.cuda.device(res.device):
            _lib.check(_lib.lib().mf_paste_frames(res.data_ptr(), int(res.dtype == torch.float32), res.shape[1], res.shape[2], self.frames.data_ptr(),
                                                  self.n, self.H, self.W, jobs, B, out.data_ptr(),
                                                  _lib.stream_ptr(res.device)), "paste_frames")
        return out

    def paste_i420(self, res, indices, out=None):
        """paste() and the composed BGR frames as planar YUV 4:2:0, both launches on the caller's stream: uint8 [B, H * 3 / 2, W] (ops.frames_to_i420; H and W
        must be even).  out: the tensor of that shape to write."""
        if self.H % 2 or self.W % 2:
            raise RuntimeError(f"paste_i420: the avatar's frames are {self.H} x {self.W} (H x W); 4:2:0 needs even sizes")
        return frames_to_i420(self.paste(res, indices), order="bgr", out=out)


class CustomVideos:
    """Device-resident copy of a session's custom videos (basereal.py:52-68): cycles {audiotype: uint8 [n, H, W, 3] BGR} is `custom_img_cycle`, uploaded once;
    custom_index is the dict the deployment's `BaseReal` holds, taken BY REFERENCE -- the scheduler walks it (serving.choose_frames), the deployment resets it
    (`set_curr_state(audiotype, reinit=True)`, `init_customindex()`).  One dict per session, as one `BaseReal` per session holds one.

    lengths                {audiotype: n}
    source(audiotype, i)   the device view of frame i of that video, uint8 [H, W, 3]
    check_size(H, W, who)  refuses a video whose frames are not H x W: the reference would hand the encoder a frame of another size, a ring has fixed slots"""

    def __init__(self, cycles, custom_index, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("CustomVideos needs a HIP device; no CPU path exists here")
        if not isinstance(custom_index, dict):
            raise RuntimeError(f"CustomVideos: custom_index must be the dict the deployment holds, got {type(custom_index).__name__}")
        self.device, self.custom_index, self.cycles = torch.device(device), custom_index, {}
        for t, cyc in dict(cycles).items():
            fr = cyc if torch.is_tensor(cyc) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in cyc])))
            fr = _dev_u8(fr, self.device)
            if fr.dim() != 4 or fr.shape[3] != 3 or fr.shape[0] < 1:
                raise RuntimeError(f"CustomVideos: cycles[{t!r}] must be [n, H, W, 3] with n >= 1, got {tuple(fr.shape)}")
            self.cycles[t] = fr
        self.lengths = {t: int(fr.shape[0]) for t, fr in self.cycles.items()}

    def source(self, audiotype, i):
        fr = self.cycles.get(audiotype)
        if fr is None or not 0 <= int(i) < fr.shape[0]:
            raise RuntimeError(f"CustomVideos.source: frame {i} of custom video {audiotype!r} ({'no such video' if fr is None else f'{fr.shape[0]} frames'})")
        return fr[int(i)]

    def check_size(self, H, W, who="CustomVideos"):
        for t, fr in self.cycles.items():
            if (int(fr.shape[1]), int(fr.shape[2])) != (int(H), int(W)):
                raise RuntimeError(f"{who}: custom video {t!r} holds {fr.shape[1]} x {fr.shape[2]} frames (H x W), the avatar's frames are {H} x {W}; a ring's slots "
                                   f"have one size")


def resize_linear_u8(src, dw, dh):
    """cv2.resize(src, (dw, dh)) (INTER_LINEAR) for a uint8 [h, w, 3] device tensor."""
    if not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
        raise RuntimeError("resize_linear_u8 needs a uint8 [h, w, 3] HIP device tensor; no CPU path exists here")
    src = src.contiguous()
    dst = torch.empty((dh, dw, 3), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().mf_resize_linear_u8(src.data_ptr(), src.shape[0], src.shape[1], dst.data_ptr(), int(dh), int(dw),
                                                  _lib.stream_ptr(src.device)), "resize_linear_u8")
    return dst
