"""Times face detection for B = 8 frames of 720 x 1280 through two routes (avatar preparation):

  device   SFDDetector.detect_from_batch: uint8 frames -> graph -> softmax / threshold / decode / NMS kernels -> one read-back of counters and boxes
  host     the route before the detect kernels: float frames -> graph -> twelve NCHW tensors -> the reference-shaped host post-process, restated below
           (sfd/detect.py:70-94 batch_detect, bbox.py:44-64 nms, sfd_detector.py:41-47)

Seeded weights; the conf biases are shifted so that, as with trained weights on a real frame, a few hundred positions per image pass 0.05 (the host loop's cost is
per passing position).  Warm-up, then the median of 20 runs, one sync per call.

    python tools/s3fd_detect_timing.py
"""
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))
from mere_fusion_amd import weights as W                      # noqa: E402
from mere_fusion_amd.avatar import SFDDetector                # noqa: E402

SHIFT = (-3.45, -3.1, -2.8, -1e4, -1e4, -1e4)
NAMES = ["conv3_3_norm", "conv4_3_norm", "conv5_3_norm", "fc7", "conv6_2", "conv7_2"]


def host_nms(dets, thresh):
    if 0 == len(dets):
        return []
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = scores.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(0.0, xx2 - xx1 + 1), np.maximum(0.0, yy2 - yy1 + 1)
        ovr = w * h / (areas[i] + areas[order[1:]] - w * h)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return keep


def host_route(net, imgs):
    x = torch.from_numpy((imgs - np.array([104, 117, 123])).transpose(0, 3, 1, 2)).float().cuda()
    olist = net(x)
    BB = x.shape[0]
    for i in range(6):
        olist[i * 2] = F.softmax(olist[i * 2], dim=1)
    olist = [o.cpu() for o in olist]
    rows = []
    for i in range(6):
        ocls, oreg = olist[i * 2], olist[i * 2 + 1]
        stride = 2 ** (i + 2)
        for _, h, w in zip(*np.where(ocls[:, 1, :, :] > 0.05)):
            pri = torch.Tensor([[stride / 2 + w * stride, stride / 2 + h * stride, stride * 4.0, stride * 4.0]]).view(1, 1, 4)
            loc = oreg[:, :, h, w].contiguous().view(BB, 1, 4)
            box = torch.cat((pri[:, :, :2] + loc[:, :, :2] * 0.1 * pri[:, :, 2:], pri[:, :, 2:] * torch.exp(loc[:, :, 2:] * 0.2)), 2)
            box[:, :, :2] -= box[:, :, 2:] / 2
            box[:, :, 2:] += box[:, :, :2]
            rows.append(torch.cat([box[:, 0], ocls[:, 1, h, w].unsqueeze(1)], 1).numpy())
    bl = np.array(rows) if rows else np.zeros((1, BB, 5))
    keeps = [host_nms(bl[:, i, :], 0.3) for i in range(BB)]
    return [[r for r in bl[k, i, :] if r[-1] > 0.5] for i, k in enumerate(keeps)], len(rows)


def median_ms(fn, warmup=3, runs=20):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                     # both routes end in host data: their own read-back is the one sync
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    sd = W.make_s3fd_state_dict(0)
    for n, s in zip(NAMES, SHIFT):
        sd[n + "_mbox_conf.bias"] = sd[n + "_mbox_conf.bias"].clone()
        sd[n + "_mbox_conf.bias"][-1] += s
    B, H, Wd = 8, 720, 1280
    imgs = np.random.default_rng(0).integers(0, 256, (B, H, Wd, 3), dtype=np.uint8)
    det = SFDDetector(device="cuda", state_dict=sd, max_batch=B)
    b, c, n = det.face_detector.detect(imgs)
    torch.cuda.synchronize()
    _, host_rows = host_route(det.face_detector, imgs)
    print(f"candidates per image above 0.05 (device): {n.cpu().tolist()}; positions the host loop visits: {host_rows}; boxes kept: {c.cpu().tolist()}")
    dev_ms = median_ms(lambda: det.detect_from_batch(imgs))
    host_ms = median_ms(lambda: host_route(det.face_detector, imgs))
    print(f"B = {B}, {H} x {Wd}: device route {dev_ms:.2f} ms, host post-process route {host_ms:.2f} ms, ratio {host_ms / dev_ms:.2f} (medians of 20)")


if __name__ == "__main__":
    main()
