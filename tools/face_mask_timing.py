"""One batch of 720p frames through `prepare_materials` (all on the device) against the host route on the same machine: per frame Pillow's crop + BILINEAR resize,
ToTensor + Normalize, BiSeNet.__call__, the D2H copy of the [19, 512, 512] logits, numpy argmax and remap, Pillow's BICUBIC resize back and the window.  That is the
host figure.  cv2 is not installed, so the host route's blur is not part of it: a float64 numpy blur produces the masks the device is compared with and is timed on its
own (`host_blur_standin_ms`; the real cv2.GaussianBlur would cost far less).  Where Pillow does not import, tests/face_mask_ref.py's resampler stands in and the output
says so.  Prints one JSON line.

    python tools/face_mask_timing.py [--batch 8] [--repeats 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import face_mask_ref as R   # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None


def host_route(fp, frames, face_boxes, blur=True):
    from mere_fusion_amd.avatar.face_parsing import MEAN, STD
    mean, std = torch.tensor(MEAN)[:, None, None], torch.tensor(STD)[:, None, None]
    out = []
    for image, face_box in zip(frames, face_boxes):
        crop_box, _ = R.get_crop_box(face_box, 1.2)
        w, h = crop_box[2] - crop_box[0], crop_box[3] - crop_box[1]
        if Image is not None:
            c512 = np.asarray(Image.fromarray(image[:, :, ::-1]).crop(crop_box).resize((512, 512), Image.BILINEAR))
        else:
            c512 = R.resize_u8(R.crop_u8(image[:, :, ::-1], crop_box), (512, 512), R.BILINEAR)
        x = (torch.from_numpy(c512.transpose(2, 0, 1).copy()).float().div(255) - mean) / std
        logits = fp.net(x[None].cuda())[0][0].cpu().numpy()                     # the 20 MB copy
        m512 = R.class_mask(logits)
        seg = np.asarray(Image.fromarray(m512).resize((w, h))) if Image is not None else R.resize_u8(m512, (w, h), R.BICUBIC)
        pre = R.window(seg, face_box, crop_box)
        if not blur:
            out.append(pre)
            continue
        out.append(np.clip(np.rint(R.gaussian_blur(pre, R.blur_kernel_size(w))), 0, 255).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.avatar import FaceParsing
    from mere_fusion_amd.musetalk.utils import blending
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (a.batch, 720, 1280, 3), dtype=np.uint8)
    face_boxes = [(500 + 7 * i, 200 + 5 * i, 760 + 9 * i, 520 + 6 * i) for i in range(a.batch)]     # crop boxes of 384, 386, 388 and 390 pixels, each twice
    fp = FaceParsing(state_dict=W.make_bisenet_state_dict(0), max_batch=a.batch)
    dev_frames = torch.from_numpy(frames).cuda()

    def device_route():
        masks, _ = blending.prepare_materials(dev_frames, face_boxes, fp)
        torch.cuda.synchronize()
        return masks

    got, want = device_route(), host_route(fp, frames, face_boxes)                                   # warm-up of both routes (graphs at B and at 1)
    diff = max(int(np.abs(g.cpu().numpy().astype(int) - w.astype(int)).max()) for g, w in zip(got, want))
    t_dev, t_host, t_blur = [], [], []
    for _ in range(a.repeats):
        t = time.perf_counter(); device_route(); t_dev.append(time.perf_counter() - t)
    for _ in range(max(2, a.repeats // 3)):
        t = time.perf_counter(); pre = host_route(fp, frames, face_boxes, blur=False); t_host.append(time.perf_counter() - t)
        t = time.perf_counter(); [R.gaussian_blur(p, R.blur_kernel_size(p.shape[1])) for p in pre]; t_blur.append(time.perf_counter() - t)
    print(json.dumps({"batch": a.batch, "frame": [720, 1280], "device_ms": round(1e3 * float(np.median(t_dev)), 2), "host_ms": round(1e3 * float(np.median(t_host)), 2),
                      "ratio": round(float(np.median(t_host) / np.median(t_dev)), 1), "host_blur_standin_ms": round(1e3 * float(np.median(t_blur)), 2), "host_resampler": "Pillow" if Image is not None else "tests/face_mask_ref.py (Pillow absent)",
                      "max_level_difference_between_routes": diff}))


if __name__ == "__main__":
    main()
