"""`musetalk.utils.preprocessing` (musetalk/utils/preprocessing.py): `get_landmark_and_bbox`, `get_bbox_range` and `coord_placeholder` for frames already in memory.

The reference builds its two models at import time (`model = init_model(config, 'dw-ll_ucoco_384.pth')`, `fa = FaceAlignment(...)`, :16-23).  Here they are the module
attributes `model` (the `DWPose` drop-in, avatar/dwpose.py) and `fa` (the `FaceAlignment` drop-in), set by the deployment once its checkpoints are loaded:

    from mere_fusion_amd.musetalk.utils import preprocessing
    preprocessing.model, preprocessing.fa = pose, fa
    coord_list, frames = preprocessing.get_landmark_and_bbox(frames)

Detector, landmark network and the box statements run on the device (avatar/prepare.py `muse_landmark_boxes`); image files are not read here."""
import numpy as np

from mere_fusion_amd.avatar.prepare import COORD_PLACEHOLDER, muse_landmark_boxes

model = None
fa = None
coord_placeholder = COORD_PLACEHOLDER                                          # :26


def _frames(img_list, who):
    if any(isinstance(f, (str, bytes)) or hasattr(f, "__fspath__") for f in img_list):
        raise RuntimeError(f"{who}: reading image files (cv2.imread) stays with the reference; pass the BGR frames")
    if model is None or fa is None:
        raise RuntimeError(f"{who}: set musetalk.utils.preprocessing.model (DWPose) and .fa (FaceAlignment) first; the reference builds them at import (:16-23)")
    return [np.asarray(f) for f in img_list]


def get_landmark_and_bbox(img_list, upperbondrange=0):
    """:84-136 -> (coords_list, frames); prints the adjustment range as the reference does"""
    frames = _frames(img_list, "get_landmark_and_bbox")
    coords, text = muse_landmark_boxes(frames, model, fa, int(upperbondrange))
    print("********************************************bbox_shift parameter adjustment**********************************************************")
    print(text)
    print("*************************************************************************************************************************************")
    return coords, frames


def get_bbox_range(img_list, upperbondrange=0):
    """:43-81 -> the range text"""
    frames = _frames(img_list, "get_bbox_range")
    return muse_landmark_boxes(frames, model, fa, int(upperbondrange))[1]
