"""Generates tests/golden/face_mask_golden.npz by CALLING the reference's own `get_image_prepare_material` (musetalk/utils/blending.py:62-86), which runs its own
`face_seg` and its own `FaceParsing.__call__` (face_parsing/__init__.py:34-51) around its own BiSeNet module, with Pillow doing every resize, crop and paste (build
container only: the two modules are imported from /root/reference).  cv2 and torchvision are absent and stubbed (`load_reference`): the cv2 stub's GaussianBlur records
the mask it is handed and returns it, so the golden ends at the mask before the blur, and the blur is held to tests/face_mask_ref.py's float64 evaluation.  The
intermediates come from hooks and wrappers, not from restated code.

Weights: mere_fusion_amd.weights.make_bisenet_state_dict(SEED) with a recorded change to the 19 x 256 matrix of conv_out.conv_out.  With the plain seeded weights one
background class wins nearly everywhere (foreground share 4-6 %), and any rescaling that balances the classes leaves a logit field so flat against max|logit| that
3-4 % of the pixels are near ties.  So the head gets contrast: d = the first principal direction of the head's input features over the golden's own crops, with the
mean feature projected out; rows of the mask classes 1..13 get + k d, rows of {0, 14..18} get - k d, k = HEAD_CONTRAST x (std of the logits) / (std of d . features).
On the two-tone frames d separates the tones, the mask follows the image's regions and the near ties shrink to their borders.  The changed matrix is stored in the
golden file (19 KB); tests/test_face_mask.py puts it into the seeded state dict.

Only data is stored: the frames and face boxes, the changed head matrix, the 512 x 512 crops, one job's conv_out head logits [20, 64, 64] (forward hook), the 512 x 512 class masks, the crop-size
masks before the blur, the packed near-tie bitmaps and the settings.  The generator refuses to write unless every 512 x 512 mask has a foreground share of 20-80 % and
at most 1 % of its pixels are near ties.

    python tests/golden/make_face_mask_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import face_mask_ref as R   # noqa: E402

REF_UTILS = "/root/reference/musetalk/utils"
SEED = 0
HEAD_CONTRAST = 3.0
BG_CLASSES = [0, 14, 15, 16, 17, 18]
LOGIT_GATE = 2e-3                         # tests/test_avatar.py: BiSeNet logits within 2e-3 x max|logit|
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UPPER, EXPAND = 0.5, 1.2
# (frame, face box): an upscaled crop, a crop box that leaves the frame (other size), a downscaled crop
JOBS = [("A", (60, 50, 135, 140)), ("A", (150, 110, 236, 196)), ("B", (85, 95, 595, 605))]
# resample-only cases (no network) on a frame of small colour blocks: frame, box, channel reversal -- a non-square box read without the reversal, a box that leaves
# the frame on two sides, a box whose width is already 512 (Pillow skips the horizontal pass)
RESAMPLE = [("C", (10, 20, 167, 131), False), ("C", (-20, 60, 100, 230), True), ("B", (100, 50, 612, 350), True)]


def blocks(rng, h, w, bs):
    """random colour blocks under a diagonal sawtooth: edges, flats and ramps for the resampler, and little entropy for the file"""
    pal = rng.integers(0, 256, (12, 3), dtype=np.uint8)
    idx = rng.integers(0, 12, ((h + bs - 1) // bs, (w + bs - 1) // bs))
    img = pal[np.kron(idx, np.ones((bs, bs), int))[:h, :w]]
    yy, xx = np.mgrid[:h, :w]
    ramp = ((xx * 3 + yy * 2) // 8 % 32).astype(np.int64)
    return np.clip(img.astype(np.int64) + ramp[..., None] - 16, 0, 255).astype(np.uint8)


def two_tone(rng, h, w, bs):
    """large dark and bright regions under a faint sawtooth: the image's regions are what the mask should follow"""
    idx = rng.integers(0, 2, ((h + bs - 1) // bs, (w + bs - 1) // bs))
    img = np.array([[20, 20, 20], [235, 235, 235]], dtype=np.uint8)[np.kron(idx, np.ones((bs, bs), int))[:h, :w]]
    yy, xx = np.mgrid[:h, :w]
    ramp = ((xx * 3 + yy * 2) // 8 % 16).astype(np.int64)
    return np.clip(img.astype(np.int64) + ramp[..., None] - 8, 0, 255).astype(np.uint8)


def state_dict(conv_out_weight=None, seed=SEED):
    from mere_fusion_amd import weights as W
    sd = W.make_bisenet_state_dict(int(seed))
    if conv_out_weight is not None:
        sd["conv_out.conv_out.weight"] = torch.as_tensor(conv_out_weight).float().reshape(sd["conv_out.conv_out.weight"].shape).clone()
    return sd


def contrast_head(net, sd, crops512, mean, std):
    """the changed conv_out.conv_out matrix (module docstring); net: the reference's BiSeNet holding `sd`"""
    feat = {}
    hook = net.conv_out.conv_out.register_forward_hook(lambda m, i, o: feat.__setitem__("v", i[0].detach()))
    x = torch.stack([(torch.from_numpy(c.transpose(2, 0, 1).copy()).float().div(255) - mean) / std for c in crops512])
    with torch.no_grad():
        net(x)
    hook.remove()
    fm = feat["v"].double().permute(1, 0, 2, 3).reshape(feat["v"].shape[1], -1)
    mu = fm.mean(1)
    d = torch.linalg.svd(fm - mu[:, None], full_matrices=False)[0][:, 0]
    d = d - (d @ mu) / (mu @ mu) * mu
    w = sd["conv_out.conv_out.weight"].double()[:, :, 0, 0]
    k = HEAD_CONTRAST * (w @ (fm - mu[:, None])).std().item() / (d @ fm).std().item()
    sign = torch.ones(w.shape[0], dtype=torch.double)
    sign[BG_CLASSES] = -1
    return (w + k * sign[:, None] * d[None, :]).float()[:, :, None, None]


class Taps:
    """what the stubs and wrappers around the reference's modules saw during one call"""
    def __init__(self):
        self.v = {}

    def keep(self, name, value):
        self.v[name] = value
        return value


def load_reference(taps, sd):
    """Imports the reference's own `face_parsing` package and `blending` module (musetalk/utils) with the two libraries that are absent here stubbed:
      cv2                     GaussianBlur records its arguments and returns the image unchanged: the golden ends where the reference hands over to OpenCV
      torchvision.transforms  Compose / ToTensor / Normalize with torchvision's documented arithmetic (x / 255 in CHW, then (x - mean) / std); ToTensor records the image
    `torch.load` returns the seeded state dict while `blending` builds its module-level `fp = FaceParsing()`; Resnet18.init_weight (the ImageNet file) is skipped as in
    make_avatar_golden.py.  The module's `fp` and `face_seg` are wrapped so that their results are recorded."""
    import importlib
    import types
    cv2 = types.ModuleType("cv2")
    cv2.GaussianBlur = lambda img, ksize, sigma: taps.keep("blur_args", (np.array(img), tuple(ksize), sigma))[0]
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class ToTensor:
        def __call__(self, pic):
            a = taps.keep("crop512", np.array(pic))
            return torch.from_numpy(a.transpose(2, 0, 1).copy()).float().div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean)[:, None, None], torch.tensor(std)[:, None, None]

        def __call__(self, t):
            return (t - self.mean) / self.std

    tr.Compose, tr.ToTensor, tr.Normalize = Compose, ToTensor, Normalize
    tv.transforms = tr
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tr})
    sys.path.insert(0, REF_UTILS)
    real_load = torch.load
    try:
        resnet = importlib.import_module("face_parsing.resnet")
        resnet.Resnet18.init_weight = lambda self, path: None
        torch.load = lambda *a, **k: sd
        blending = importlib.import_module("blending")
    finally:
        torch.load = real_load
        sys.path.remove(REF_UTILS)
    fp, face_seg = blending.fp, blending.face_seg
    fp.net.register_forward_hook(lambda m, i, o: taps.v.__setitem__("logits", o[0].detach().numpy()[0]))     # (a hook that returns a value replaces the output)
    fp.net.conv_out.conv_out.register_forward_hook(lambda m, i, o: taps.v.__setitem__("head", o.detach().numpy()[0]))
    blending.fp = lambda image, *a, **k: taps.keep("mask512_image", fp(image, *a, **k))
    blending.face_seg = lambda image: taps.keep("seg_image", face_seg(image))
    return blending, fp


def main():
    from PIL import Image
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rng = np.random.default_rng(0)
    frames = {"A": two_tone(rng, 200, 240, 45), "B": two_tone(rng, 680, 680, 260), "C": blocks(rng, 200, 240, 12)}          # BGR, as cv2.imread returns them
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
    taps = Taps()
    blending, fp = load_reference(taps, state_dict())
    crops = []
    for f, face_box in JOBS:                                  # first with the plain seeded weights: the crops the head's contrast direction is taken from
        blending.get_image_prepare_material(frames[f], face_box, UPPER, EXPAND)
        crops.append(taps.v["crop512"])
    conv_out_weight = contrast_head(fp.net, state_dict(), crops, mean, std)
    fp.net.load_state_dict(state_dict(conv_out_weight), strict=True)
    out = {"settings": np.array([SEED, HEAD_CONTRAST, LOGIT_GATE, UPPER, EXPAND]), "bg_classes": np.array(BG_CLASSES), "conv_out_weight": conv_out_weight.numpy(),
           "frame_A": frames["A"], "frame_B": frames["B"], "frame_C": frames["C"], "job_frame": np.array([f for f, _ in JOBS]), "face_boxes": np.array([b for _, b in JOBS])}
    for k, (f, face_box) in enumerate(JOBS):
        taps.v.clear()
        mask_array, crop_box = blending.get_image_prepare_material(frames[f], face_box, UPPER, EXPAND)       # the reference's own function, blending.py:62-86
        pre, ksize, sigma = taps.v["blur_args"]
        logits, mask512 = taps.v["logits"], np.array(taps.v["mask512_image"])
        assert mask_array is pre or np.array_equal(mask_array, pre)
        assert ksize == (R.blur_kernel_size(pre.shape[1]),) * 2 and sigma == 0 and list(crop_box) == R.get_crop_box(face_box, EXPAND)[0]
        eps = LOGIT_GATE * float(np.abs(logits).max())
        tie = R.near_tie(logits, eps)
        share, tie_share = float((mask512 > 0).mean()), float(tie.mean())
        print(f"job {k}: crop box {list(crop_box)} ({pre.shape[1]} x {pre.shape[0]}), blur kernel {ksize}, foreground {share:.1%}, near ties {tie_share:.2%}, "
              f"max|logit| {np.abs(logits).max():.1f}, classes {np.unique(logits.argmax(0)).tolist()}, pre-blur mask mean {pre.mean():.1f}")
        if not 0.2 <= share <= 0.8:
            raise SystemExit(f"job {k}: foreground share {share:.1%} outside 20-80 %: not written")
        if tie_share > 0.01:
            raise SystemExit(f"job {k}: {tie_share:.2%} near-tie pixels, the cap is 1 %: not written")
        out[f"crop_box{k}"] = np.array(crop_box)
        out[f"crop512_{k}"] = taps.v["crop512"]
        out[f"mask512_{k}"] = mask512
        out[f"seg_{k}"] = np.array(taps.v["seg_image"])
        out[f"preblur_{k}"] = pre
        out[f"near_tie{k}"] = np.packbits(tie)
        out[f"logit_max{k}"] = np.array(np.abs(logits).max())
        if k == 0:
            out["head_logits0"] = taps.v["head"]              # [19, 64, 64] (the device buffer pads to 20); one job only, to keep the file small
    for k, (f, box, rev) in enumerate(RESAMPLE):
        src = frames[f][:, :, ::-1] if rev else frames[f]
        out[f"rs_box{k}"] = np.array(box)
        out[f"rs_rev{k}"] = np.array(rev)
        out[f"rs_frame{k}"] = np.array(f)
        out[f"rs_crop512_{k}"] = np.asarray(Image.fromarray(np.ascontiguousarray(src)).crop(box).resize((512, 512), Image.BILINEAR))
    path = os.path.join(ROOT, "tests", "golden", "face_mask_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
