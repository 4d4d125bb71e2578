"""`face_detection` drop-in: `SFDDetector` (face_detection/detection/sfd/sfd_detector.py:16-59) and the part of `FaceAlignment` that avatar preparation
calls (face_detection/api.py:46-79; genavatar.py:62-71, musetalk/utils/preprocessing.py:23,63,104), ending in boxes computed on the device.

    from mere_fusion_amd.avatar.face_detection import FaceAlignment, LandmarksType      # instead of `from face_detection import ...`

The network and its post-process run as HIP kernels (avatar/s3fd.py `s3fd.detect`); the host reads back the counters and the kept rows only.  A list that
outgrows a capacity raises a RuntimeError naming the capacity and the count; nothing falls back to the host."""
from enum import Enum

import numpy as np
import torch

from .s3fd import MAX_CANDIDATES, MAX_DET, boxes_to_lists, s3fd


class LandmarksType(Enum):                 # api.py:17-27 (the callers pass `_2D`; no landmark network is built here)
    _2D = 1
    _2halfD = 2
    _3D = 3


class NetworkSize(Enum):                   # api.py:30-42
    LARGE = 4

    def __int__(self):
        return self.value


class SFDDetector:
    def __init__(self, device="cuda", path_to_detector=None, verbose=False, state_dict=None, precision="bf16x3", max_batch=16,
                 max_candidates=MAX_CANDIDATES, max_det=MAX_DET):
        if state_dict is None:
            if path_to_detector is None:
                raise ValueError("SFDDetector: give path_to_detector (the reference's s3fd.pth) or state_dict; nothing is downloaded here")
            state_dict = torch.load(path_to_detector, map_location="cpu")
        self.device, self.verbose = device, verbose
        self.max_candidates, self.max_det = int(max_candidates), int(max_det)
        self.face_detector = s3fd(precision=precision, max_batch=max_batch, device=device)
        self.face_detector.load_state_dict(state_dict)
        self.face_detector.to(device)
        self.face_detector.eval()

    def _detect(self, images, reverse_channels):
        """-> (boxes, counts, n_candidates) host arrays for any batch size (chunks of max_batch); one sync per chunk"""
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if images.dtype != torch.uint8:
            raise ValueError(f"SFDDetector: uint8 [B, H, W, 3] frames expected, got {images.dtype}")
        out, mb = [], self.face_detector.max_batch
        for i in range(0, images.shape[0], mb):
            b, c, n = self.face_detector.detect(images[i:i + mb], max_candidates=self.max_candidates, max_det=self.max_det, reverse_channels=reverse_channels)
            out += boxes_to_lists(b, c, n, self.max_candidates, self.max_det)
        return out

    def detect_from_batch(self, images, reverse_channels=False):
        """uint8 [B, H, W, 3] -> per image the list of float32 [x1, y1, x2, y2, score] rows, in keep order (score descending)"""
        return self._detect(images, reverse_channels)

    def detect_from_image(self, image):
        image = torch.as_tensor(np.ascontiguousarray(image) if isinstance(image, np.ndarray) else image)
        return self._detect(image[None], False)[0]

    @property
    def reference_scale(self):
        return 195

    @property
    def reference_x_shift(self):
        return 0

    @property
    def reference_y_shift(self):
        return 0


FaceDetector = SFDDetector                 # face_detection/detection/sfd/__init__.py


class FaceAlignment:
    def __init__(self, landmarks_type=LandmarksType._2D, network_size=NetworkSize.LARGE, device="cuda", flip_input=False, face_detector="sfd", verbose=False, **detector_kw):
        if face_detector != "sfd":
            raise ValueError(f"FaceAlignment: only the 'sfd' detector exists here, not {face_detector!r}")
        self.device, self.flip_input, self.landmarks_type, self.verbose = device, flip_input, landmarks_type, verbose
        self.face_detector = SFDDetector(device=device, verbose=verbose, **detector_kw)

    def get_detections_for_batch(self, images):
        """api.py:64-79: channels flipped (on the device, while the frame is converted), first box, clipped at 0, truncated to int; None where no face"""
        results = []
        for d in self.face_detector.detect_from_batch(images, reverse_channels=True):
            if len(d) == 0:
                results.append(None)
                continue
            d = np.clip(d[0], 0, None)
            x1, y1, x2, y2 = map(int, d[:-1])
            results.append((x1, y1, x2, y2))
        return results
