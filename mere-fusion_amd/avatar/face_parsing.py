"""`FaceParsing` drop-in (musetalk/utils/face_parsing/__init__.py:10-51) ending in a mask computed on the device, and `face_seg` (musetalk/utils/blending.py:17-24).

    from mere_fusion_amd.avatar.face_parsing import FaceParsing      # instead of `from face_parsing import FaceParsing`

The reference resizes with Pillow, normalises with torchvision, copies the [19, 512, 512] logits to the host and takes the argmax in numpy.  Here the crop box of a
uint8 device frame goes through csrc/mf_face_mask.hip: a resampler that reproduces Pillow's 8-bit `Image.resize` bit for bit, the normalisation fused into its vertical
pass, the BiSeNet graph, and one kernel for upsampling + argmax + class remap.  `parse` never leaves the device; `__call__` keeps the reference's surface.  There is no
CPU path, and a geometry the kernels cannot serve raises a RuntimeError naming the limit."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .bisenet import BiSeNet

MEAN = (0.485, 0.456, 0.406)               # face_parsing/__init__.py:31
STD = (0.229, 0.224, 0.225)
SIZE = (512, 512)


def _ints(rows):
    flat = [int(v) for r in rows for v in r]
    return (C.c_int * len(flat))(*flat)


def workspace_bytes(finish, box_sizes, mask_h, mask_w):
    n = _lib.lib().mf_face_mask_workspace_bytes(int(finish), _ints(box_sizes), len(box_sizes), int(mask_h), int(mask_w))
    if n == 0:                             # refused: let the entry point say why
        return 256
    return n


def blur_kernel_size(width):
    """blending.py:84"""
    return int(0.1 * width // 2 * 2) + 1


def finish_masks(masks, jobs, blur=True, want_pre_blur=False):
    """mf_face_mask_finish.  masks: device uint8 [n, S_h, S_w]; jobs: n x (w, h, rx0, ry0, rx1, ry1, top).  Returns the list of device uint8 [h, w] masks (blurred, or the
    windowed resize when blur is False), and with want_pre_blur the list of windowed resizes as well."""
    if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.shape[0] == len(jobs)):
        raise RuntimeError("finish_masks needs one uint8 [S, S] mask per job on the HIP device; no CPU path exists here")
    masks = masks.contiguous()
    dev = masks.device
    sizes = [(j[0], j[1]) for j in jobs]
    total = sum(max(int(w), 0) * max(int(h), 0) for w, h in sizes)
    ws = torch.empty(workspace_bytes(1, sizes, masks.shape[1], masks.shape[2]), dtype=torch.uint8, device=dev)
    pre = torch.empty(max(total, 1), dtype=torch.uint8, device=dev) if (want_pre_blur or not blur) else None
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev) if blur else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mf_face_mask_finish(masks.data_ptr(), masks.shape[1], masks.shape[2], _ints(jobs), len(jobs), int(bool(blur)), ws.data_ptr(), ws.numel(),
                                                  None if pre is None else pre.data_ptr(), None if out is None else out.data_ptr(),
                                                  _lib.stream_ptr(dev)), "face_mask_finish")

    def split(flat):
        res, o = [], 0
        for w, h in sizes:
            res.append(flat[o:o + w * h].view(h, w))
            o += w * h
        return res

    if not blur:
        return split(pre)
    return (split(out), split(pre)) if want_pre_blur else split(out)


class FaceParsing:
    def __init__(self, resnet_path=None, model_pth=None, state_dict=None, precision="bf16x3", max_batch=8, device="cuda"):
        """resnet_path is accepted and unused, as in the reference once the full state dict is loaded (face_parsing/__init__.py:19-22)."""
        if state_dict is None:
            if model_pth is None:
                raise ValueError("FaceParsing: give model_pth (the reference's 79999_iter.pth) or state_dict; nothing is downloaded here")
            state_dict = torch.load(model_pth, map_location="cpu")
        self.device, self.max_batch = torch.device(device), int(max_batch)
        self.net = BiSeNet(resnet_path, precision=precision, max_batch=self.max_batch, device=device)
        self.net.load_state_dict(state_dict)
        self.net.eval()

    def _graph(self, size):
        W, H = size
        g = self.net._nets.get((H, W))
        if g is None:
            g = self.net._nets[(H, W)] = self.net._build(H, W)
        return g

    def parse(self, frames_u8, crop_boxes, frame_indices=None, reverse_channels=True, size=SIZE):
        """frames_u8: uint8 [n, H, W, 3] on the device (BGR frames with reverse_channels, the `image[:, :, ::-1]` of blending.py:63; RGB without); crop_boxes: B x
        (x_s, y_s, x_e, y_e), box i cut from frame frame_indices[i] (default i), black outside the frame.  Returns uint8 [B, 512, 512] on the device: 255 on classes
        1..13.  Nothing is copied to the host and nothing waits for the device."""
        if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3):
            raise RuntimeError("parse needs uint8 [n, H, W, 3] frames on the HIP device; no CPU path exists here")
        frames_u8 = frames_u8.contiguous()
        idx = list(range(len(crop_boxes))) if frame_indices is None else [int(i) for i in frame_indices]
        if len(idx) != len(crop_boxes):
            raise ValueError("parse: one frame index per crop box")
        g = self._graph(size)
        n = g["net"]
        dev = frames_u8.device
        out = torch.empty((len(idx), size[1], size[0]), dtype=torch.uint8, device=dev)
        mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        for i in range(0, len(idx), self.max_batch):
            boxes = [tuple(int(v) for v in b) for b in crop_boxes[i:i + self.max_batch]]
            jobs = [(f,) + b for f, b in zip(idx[i:i + self.max_batch], boxes)]
            ws = torch.empty(workspace_bytes(0, [(b[2] - b[0], b[3] - b[1]) for b in boxes], size[1], size[0]), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mf_face_mask_parse(n._h, g["inp"], g["out"], self.net.n_classes, frames_u8.data_ptr(), frames_u8.shape[0], frames_u8.shape[1],
                                                         frames_u8.shape[2], int(bool(reverse_channels)), _ints(jobs), len(jobs), mean, std, ws.data_ptr(), ws.numel(),
                                                         out[i:i + len(jobs)].data_ptr(), _lib.stream_ptr(dev)), "face_mask_parse")
        return out

    @staticmethod
    def _rgb_array(image):
        if isinstance(image, str):
            from PIL import Image
            image = Image.open(image)
        if not isinstance(image, (np.ndarray, torch.Tensor)):
            image = np.array(image.convert("RGB") if hasattr(image, "convert") else image)
        image = torch.as_tensor(np.array(image) if isinstance(image, np.ndarray) else image)      # (a copy: the caller's array may be read-only)
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
            raise ValueError(f"FaceParsing: an RGB uint8 [h, w, 3] image expected, got {image.dtype} {tuple(image.shape)}")
        return image

    @staticmethod
    def _to_pil(mask):
        a = mask.cpu().numpy()
        try:
            from PIL import Image
        except ImportError:
            return a
        return Image.fromarray(a)

    def __call__(self, image, size=SIZE):
        """face_parsing/__init__.py:34-51: a PIL image, a path or an RGB uint8 array -> the 512 x 512 mask (a PIL `L` image when Pillow imports, else the array)."""
        rgb = self._rgb_array(image).to(self.device)
        h, w = rgb.shape[:2]
        return self._to_pil(self.parse(rgb[None], [(0, 0, w, h)], reverse_channels=False, size=size)[0])

    def face_seg(self, image):
        """blending.py:17-24: the mask resized back to the image's size (Image.resize's default filter for mode L: BICUBIC)."""
        rgb = self._rgb_array(image).to(self.device)
        h, w = rgb.shape[:2]
        m = self.parse(rgb[None], [(0, 0, w, h)], reverse_channels=False)
        return self._to_pil(finish_masks(m, [(w, h, 0, 0, w, h, 0)], blur=False)[0])
