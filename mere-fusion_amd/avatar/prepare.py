"""Building a Wav2Lip or MuseTalk avatar on the device: uploaded frames in, what `LipSession` / `MuseSession` take out.

    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar, prepare_muse_avatar

`prepare_lip_avatar` is wav2lip/genavatar.py:61-122 without its files: detection over slices of the frames, the pads / clamp / temporal smoothing of the boxes
(mf_avatar_lip_boxes) and the crop + cv2.resize to 96 x 96 (mf_crop_resize_u8, linear) are enqueued back to back; the host waits once, for the counter of frames
without a face and the coords.  `prepare_muse_avatar` is musetalk/mere_musetalk.py:284-310: crop + INTER_LANCZOS4 resize to 256 x 256, both VAE encoder passes on the
device crop, and the blend masks of `prepare_materials`; with `pose=` (the `DWPose` drop-in, avatar/dwpose.py) the landmark boxes of
musetalk/utils/preprocessing.py:96-131 are built on the device too (`muse_landmark_boxes`: detector, landmark network, mf_muse_landmark_boxes, one read-back).  Image and video
files, and the coords.pkl / latents.pt / PNG trees the reference writes, are the caller's.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

from .. import _lib, ops
from ..paste import AvatarFrames
from .s3fd import MAX_CANDIDATES, MAX_DET, check_counts

NO_FACE = "Face not detected! Ensure the video contains a face in all the frames."          # genavatar.py:85
COORD_PLACEHOLDER = (0.0, 0.0, 0.0, 0.0)                                                    # mere_musetalk.py:288
SMOOTH_T = 5                                                                                # genavatar.py:95


def _device_frames(frames, device):
    fr = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in frames])))
    if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3 or fr.shape[0] < 1:
        raise ValueError(f"avatar frames must be uint8 [n, H, W, 3] (BGR, one size), got {fr.dtype} {tuple(fr.shape)}")
    return fr.to(device).contiguous()


def _detect(fa, fr, det_batch):
    """the detector over det_batch-sized slices (genavatar.py:70-71), nothing read back: (boxes [n, max_det, 5], counts [n], n_candidates [n]) on the device"""
    det = fa.face_detector
    step = min(int(det_batch), det.face_detector.max_batch)
    if step < 1:
        raise ValueError(f"det_batch must be positive, got {det_batch}")
    parts = [det.face_detector.detect(fr[i:i + step], max_candidates=det.max_candidates, max_det=det.max_det, reverse_channels=True)      # api.py:65
             for i in range(0, fr.shape[0], step)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3)), det.max_candidates, det.max_det


def lip_boxes(boxes, counts, H, W, pads=(0, 10, 0, 0), nosmooth=False, T=SMOOTH_T):
    """mf_avatar_lip_boxes on the detector's device outputs -> (coords int32 [n, 4] as (y1, y2, x1, x2), jobs int32 [n, 5] for ops.crop_resize_u8, n_no_face int32 [1]),
    all on the device, nothing synchronised."""
    if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[2] == 5):
        raise RuntimeError("lip_boxes needs the detector's fp32 [n, max_det, 5] boxes on the HIP device; no CPU path exists here")
    n = int(boxes.shape[0])
    if not (torch.is_tensor(counts) and counts.device == boxes.device and counts.dtype == torch.int32 and tuple(counts.shape) == (n,)):
        raise RuntimeError(f"lip_boxes: counts must be int32 [{n}] on {boxes.device}")
    if len(pads) != 4:
        raise ValueError("pads are (top, bottom, left, right)")
    boxes, counts, dev = boxes.contiguous(), counts.contiguous(), boxes.device
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    jobs = torch.empty((n, 5), dtype=torch.int32, device=dev)
    no_face = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mf_avatar_lip_boxes(boxes.data_ptr(), counts.data_ptr(), n, int(boxes.shape[1]), int(H), int(W), (C.c_int * 4)(*[int(p) for p in pads]),
                                                  0 if nosmooth else int(T), coords.data_ptr(), jobs.data_ptr(), no_face.data_ptr(),
                                                  _lib.stream_ptr(dev)), "avatar_lip_boxes")
    return coords, jobs, no_face


def prepare_lip_avatar(frames, fa, pads=(0, 10, 0, 0), nosmooth=False, img_size=96, det_batch=16, detections=None):
    """genavatar.py:61-122 for frames already in memory.  frames: n BGR uint8 frames of one size ([n, H, W, 3] array / tensor, or a list); fa: the `FaceAlignment`
    drop-in (unused when `detections` is given); detections: the (boxes, counts, n_candidates) device triple of `s3fd.detect` for all n frames, for a caller with its
    own detector run.  Returns (faces_u8, coords): faces_u8 uint8 [n, img_size, img_size, 3] on the device (face_imgs), coords the reference's list of
    (y1, y2, x1, x2) (coords.pkl) -- what `LipSession(model, faces_u8, AvatarFrames(frames, coords, lip_order=True))` takes.  One host sync, at the end.
    Raises the reference's ValueError when a frame has no face, and the detector's RuntimeError when a capacity overflowed."""
    if not torch.cuda.is_available():
        raise RuntimeError("prepare_lip_avatar needs a HIP device; no CPU path exists here")
    dev = torch.device(fa.device if fa is not None else "cuda")
    if torch.is_tensor(frames) and frames.is_cuda:
        dev = frames.device
    fr = _device_frames(frames, dev)
    n, H, W = (int(v) for v in fr.shape[:3])
    if detections is None:
        (boxes, counts, ncand), max_cand, max_det = _detect(fa, fr, det_batch)
    else:
        boxes, counts, ncand = detections
        max_cand, max_det = MAX_CANDIDATES, int(boxes.shape[1])
    if int(boxes.shape[0]) != n:
        raise ValueError(f"{int(boxes.shape[0])} detections for {n} frames")
    coords, jobs, no_face = lip_boxes(boxes, counts, H, W, pads, nosmooth)
    faces = ops.crop_resize_u8(fr, jobs, int(img_size), mode="linear")
    # the one sync: counters and coords in one transfer
    host = torch.cat([no_face, counts.to(torch.int32), ncand.to(torch.int32), coords.reshape(-1)]).cpu().numpy()
    check_counts(torch.from_numpy(host[1:1 + n]), torch.from_numpy(host[1 + n:1 + 2 * n]), max_cand, max_det)
    if host[0] > 0:
        raise ValueError(NO_FACE)
    c = host[1 + 2 * n:].reshape(n, 4)
    return faces, [tuple(int(v) for v in row) for row in c]


def landmark_boxes_device(kpts, boxes, counts, H, W, bbox_shift=0):
    """mf_muse_landmark_boxes on device keypoints [n, K, 2] and the detector's device outputs -> (coords int32 [n, 4] as (x1, y1, x2, y2), flags int32 [n]: 0 no face /
    1 landmark box / 2 detector's box, range sums int32 [3]), all on the device, nothing synchronised"""
    if not (torch.is_tensor(kpts) and kpts.is_cuda and kpts.dtype == torch.float32 and kpts.dim() == 3 and kpts.shape[2] == 2):
        raise RuntimeError("landmark_boxes_device needs fp32 [n, K, 2] keypoints on the HIP device; no CPU path exists here")
    n, dev = int(kpts.shape[0]), kpts.device
    if not (torch.is_tensor(boxes) and boxes.device == dev and boxes.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[0] == n and boxes.shape[2] == 5):
        raise RuntimeError(f"landmark_boxes_device: boxes must be the detector's fp32 [{n}, max_det, 5] on {dev}")
    if not (torch.is_tensor(counts) and counts.device == dev and counts.dtype == torch.int32 and tuple(counts.shape) == (n,)):
        raise RuntimeError(f"landmark_boxes_device: counts must be int32 [{n}] on {dev}")
    kpts, boxes, counts = kpts.contiguous(), boxes.contiguous(), counts.contiguous()
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty(3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mf_muse_landmark_boxes(kpts.data_ptr(), int(kpts.shape[1]), boxes.data_ptr(), counts.data_ptr(), n, int(boxes.shape[1]), int(H), int(W),
                                                     int(bbox_shift), coords.data_ptr(), flags.data_ptr(), sums.data_ptr(),
                                                     _lib.stream_ptr(dev)), "muse_landmark_boxes")
    return coords, flags, sums


def range_text(n_frames, sums, bbox_shift=0):
    """preprocessing.py:134 (with no face in any frame the reference divides by zero; here the range reads 0~0)"""
    sm, sp, cnt = (int(v) for v in sums)
    a, b = (int(sm / cnt), int(sp / cnt)) if cnt else (0, 0)
    return f"Total frame:「{n_frames}」 Manually adjust range : [ -{a}~{b} ] , the current value: {bbox_shift}"


def muse_landmark_boxes(frames, pose, fa, bbox_shift=0, det_batch=16):
    """get_landmark_and_bbox (preprocessing.py:84-136) for frames already in memory: the detector, the landmark network and the box statements run back to back on the
    device, one read-back.  Returns (coord_list, range_text): one (x1, y1, x2, y2) tuple of ints per frame, `(0.0, 0.0, 0.0, 0.0)` where no face was detected."""
    if not torch.cuda.is_available():
        raise RuntimeError("muse_landmark_boxes needs a HIP device; no CPU path exists here")
    dev = frames.device if torch.is_tensor(frames) and frames.is_cuda else pose.device
    fr = _device_frames(frames, dev)
    n, H, W = (int(v) for v in fr.shape[:3])
    (b, counts, ncand), max_cand, max_det = _detect(fa, fr, det_batch)
    kp = torch.cat([pose.keypoints(fr[i:i + pose.max_batch])[0] for i in range(0, n, pose.max_batch)])
    coords, flags, sums = landmark_boxes_device(kp, b, counts, H, W, bbox_shift)
    host = torch.cat([counts.to(torch.int32), ncand.to(torch.int32), flags, sums, coords.reshape(-1)]).cpu().numpy()      # the one sync
    check_counts(torch.from_numpy(host[:n]), torch.from_numpy(host[n:2 * n]), max_cand, max_det)
    fl, c = host[2 * n:3 * n], host[3 * n + 3:].reshape(n, 4)
    return [tuple(int(v) for v in row) if f else COORD_PLACEHOLDER for row, f in zip(c, fl)], range_text(n, host[3 * n:3 * n + 3], bbox_shift)


def prepare_muse_avatar(frames, vae, fp, boxes=None, fa=None, generator=None, det_batch=16, pose=None, bbox_shift=0):
    """mere_musetalk.py:284-310 for frames already in memory.  frames: n BGR uint8 frames of one size; vae: the `VAE` drop-in (with encoder weights); fp: the
    `FaceParsing` drop-in; boxes: the reference's coord_list -- one (x1, y1, x2, y2) per frame from the caller's landmark step (DWPose,
    musetalk/utils/preprocessing.py:96-131), `(0.0, 0.0, 0.0, 0.0)` where it found no face.  boxes=None takes the DETECTOR's first box of `fa` instead (clipped to
    the frame) when `pose` is None too; with pose (the `DWPose` drop-in) and fa it builds the landmark boxes itself (`muse_landmark_boxes`, bbox_shift as in
    get_landmark_and_bbox).  The detector's box is what preprocessing.py:126-128 falls back to when the landmark box is unusable: it is NOT the landmark box -- it is not cut at the
    half-face line and is wider -- so an avatar built this way differs from one built from landmarks.
    Frames with the placeholder are skipped, as mere_musetalk.py:291 skips them for the latents; here the frame leaves the avatar altogether, so that latents,
    frames, boxes and masks stay one per cached frame (what `MuseSession` requires).
    Returns (latents, avatar): latents a list of fp32 [1, 8, 32, 32] device tensors (latents.pt: [masked | reference], the noise drawn from `generator` frame by
    frame in the reference's order), avatar the `AvatarFrames` of the kept frames with their boxes, blend masks and crop boxes -- `MuseSession(latents, avatar)`."""
    from ..musetalk.utils.blending import mask_planes, prepare_materials
    if not torch.cuda.is_available():
        raise RuntimeError("prepare_muse_avatar needs a HIP device; no CPU path exists here")
    dev = frames.device if torch.is_tensor(frames) and frames.is_cuda else vae.device
    fr = _device_frames(frames, dev)
    n, H, W = (int(v) for v in fr.shape[:3])
    if boxes is None and pose is not None:
        if fa is None:
            raise ValueError("prepare_muse_avatar: the landmark boxes need the detector too (fa), as preprocessing.py:104 does")
        boxes, _ = muse_landmark_boxes(fr, pose, fa, bbox_shift, det_batch)
    if boxes is None:
        if fa is None:
            raise ValueError("prepare_muse_avatar: give the landmark boxes, or fa to fall back on the detector's boxes")
        (b, counts, ncand), max_cand, max_det = _detect(fa, fr, det_batch)
        host = torch.cat([counts.to(torch.float32), ncand.to(torch.float32), b[:, 0, :4].reshape(-1)]).cpu().numpy()
        cnt = check_counts(torch.from_numpy(host[:n].astype(np.int32)), torch.from_numpy(host[n:2 * n].astype(np.int32)), max_cand, max_det)
        rows = np.clip(host[2 * n:].reshape(n, 4), 0, None)                                   # api.py:74-78: clipped at 0, truncated
        boxes = [(min(int(r[0]), W), min(int(r[1]), H), min(int(r[2]), W), min(int(r[3]), H)) if c > 0 else COORD_PLACEHOLDER for r, c in zip(rows, cnt)]
    if len(boxes) != n:
        raise ValueError(f"{len(boxes)} boxes for {n} frames")
    keep = [i for i, b in enumerate(boxes) if tuple(b) != COORD_PLACEHOLDER]
    if not keep:
        raise ValueError(NO_FACE)
    kept = [tuple(int(v) for v in boxes[i]) for i in keep]
    crops = ops.crop_resize_u8(fr, kept, 256, mode="lanczos4", frame_indices=keep)
    latents = [vae.get_latents_for_unet(crops[k:k + 1], generator) for k in range(len(keep))]
    kept_frames = fr if len(keep) == n else fr[torch.tensor(keep, device=dev)]
    masks, crop_boxes = prepare_materials(kept_frames, kept, fp)
    return latents, AvatarFrames(kept_frames, kept, mask_planes(masks), crop_boxes, device=dev)
