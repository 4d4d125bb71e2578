"""`musetalk.utils.blending` drop-in, hot-path subset (musetalk/utils/blending.py:8-14, 103-125).

`get_image_blending(image, face, face_box, mask_array, crop_box)` keeps the reference's signature and its in-place contract: numpy
arrays in, the modified `image` back.  The arithmetic (BGR2GRAY, / 255, cv2.blendLinear) runs in `mf_paste_frames` on the GPU, bit-exact
with OpenCV's 8-bit algorithms.  Called this way every frame crosses PCIe twice, like any other use of the GPU from process_frames; the
route that pays is `mere_fusion_amd.muse_driver.MuseBatcher(paste=...)`, which composes the frames before they ever leave HBM."""
import numpy as np
import torch

from ...paste import AvatarFrames


def get_crop_box(box, expand):
    """blending.py:8-14."""
    x, y, x1, y1 = box
    x_c, y_c = (x + x1) // 2, (y + y1) // 2
    w, h = x1 - x, y1 - y
    s = int(max(w, h) // 2 * expand)
    return [x_c - s, y_c - s, x_c + s, y_c + s], s


def get_image_blending(image, face, face_box, mask_array, crop_box):
    """blending.py:103-125.  `face` is the generator's frame already resized to the bbox (musereal.py:241); a face of another size is
    resized exactly as cv2.resize would."""
    if not torch.cuda.is_available():
        raise RuntimeError("get_image_blending needs a HIP device; no CPU path exists here")
    mask = np.asarray(mask_array)
    if mask.ndim == 2:
        raise RuntimeError("mask_array must be the 3-channel image cv2.imread returns (blending.py:110 converts it with COLOR_BGR2GRAY)")
    av = AvatarFrames(np.asarray(image)[None], [face_box], [mask], [crop_box])
    out = av.paste(torch.from_numpy(np.ascontiguousarray(face))[None].cuda(), [0])
    image[...] = out[0].cpu().numpy()
    return image


# ---- mask preparation on the device (blending.py:17-24, 62-86; csrc/mf_face_mask.hip) ---------------------------------------------------------------------------
_fp = None


def _default_fp():
    """the module-level `fp = FaceParsing()` of blending.py:7, built on first use with the reference's default checkpoint path"""
    global _fp
    if _fp is None:
        from ...avatar.face_parsing import FaceParsing
        _fp = FaceParsing(model_pth="./models/face-parse-bisent/79999_iter.pth")
    return _fp


def prepare_materials(frames, face_boxes, fp=None, upper_boundary_ratio=0.5, expand=1.2, want_pre_blur=False):
    """`get_image_prepare_material` for a batch, without leaving the device.  frames: n BGR uint8 frames of one size ([n, H, W, 3] array / tensor, or a list);
    face_boxes: n x (x, y, x1, y1).  Returns (masks, crop_boxes): masks[i] a uint8 [h_i, w_i] device tensor, crop_boxes[i] the reference's list
    [x_s, y_s, x_e, y_e].  `mask_planes` turns the masks into what `paste.AvatarFrames` takes."""
    from ...avatar.face_parsing import finish_masks
    if not torch.cuda.is_available():
        raise RuntimeError("prepare_materials needs a HIP device; no CPU path exists here")
    fp = fp if fp is not None else _default_fp()
    fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in frames])))
    fr = fr.to(fp.device)
    if len(face_boxes) != fr.shape[0]:
        raise ValueError("prepare_materials: one face box per frame")
    crop_boxes, jobs = [], []
    for box in face_boxes:
        x, y, x1, y1 = (int(v) for v in box)
        crop_box, _ = get_crop_box((x, y, x1, y1), expand)
        x_s, y_s, x_e, y_e = crop_box
        w, h = x_e - x_s, y_e - y_s
        crop_boxes.append(crop_box)
        jobs.append((w, h, x - x_s, y - y_s, x1 - x_s, y1 - y_s, int(h * upper_boundary_ratio)))       # blending.py:74-82
    masks512 = fp.parse(fr, crop_boxes, reverse_channels=True)
    return finish_masks(masks512, jobs, blur=True, want_pre_blur=want_pre_blur), crop_boxes


def get_image_prepare_material(image, face_box, upper_boundary_ratio=0.5, expand=1.2, fp=None):
    """blending.py:62-86: (mask_array uint8 [h, w], crop_box), computed on the device."""
    masks, crop_boxes = prepare_materials(np.asarray(image)[None], [face_box], fp, upper_boundary_ratio, expand)
    return masks[0].cpu().numpy(), crop_boxes[0]


def mask_planes(masks):
    """Single-plane device masks -> the 3-channel images `paste.AvatarFrames` (and `get_image_blending`) expect: what cv2.imread returns for the PNG that
    mere_musetalk.py:311 writes.  BGR2GRAY of three equal planes is the plane itself, so the blend is unchanged."""
    return [m[:, :, None].expand(-1, -1, 3).contiguous() for m in masks]
