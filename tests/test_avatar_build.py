"""GPU tier of avatar/prepare.py: one call from frames to what LipSession / MuseSession take, against the reference's recorded boxes (tests/golden/lip_boxes_golden.npz)
and the integer resampling models of tests/crop_resize_ref.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import crop_resize_ref as R
from mere_fusion_amd import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
LEVEL_NAMES = ["conv3_3_norm", "conv4_3_norm", "conv5_3_norm", "fc7", "conv6_2", "conv7_2"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "lip_boxes_golden.npz"))


def _detections(det, counts=None, max_det=4):
    """the device triple of s3fd.detect holding `det` as every frame's first kept box (a second, different box behind it)"""
    n = len(det)
    boxes = torch.zeros((n, max_det, 5), dtype=torch.float32)
    boxes[:, 0] = torch.from_numpy(np.asarray(det, dtype=np.float32))
    boxes[:, 1] = boxes[:, 0] + 7.0
    counts = torch.full((n,), 2, dtype=torch.int32) if counts is None else torch.tensor(counts, dtype=torch.int32)
    return boxes.cuda(), counts.cuda(), torch.zeros(n, dtype=torch.int32).cuda()


def _frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _check_faces(frames, coords, faces, size=96):
    faces = faces.cpu().numpy()
    for i, (y1, y2, x1, x2) in enumerate(coords):
        assert y2 > y1 and x2 > x1
        assert np.array_equal(faces[i], R.crop_linear(frames[i], (x1, y1, x2, y2), size, size)), f"face {i}"          # cv2.resize(frame[y1:y2, x1:x2], (96, 96))


def test_lip_avatar_coords_equal_the_reference_and_faces_the_integer_model(lib_built, golden):
    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar
    for k, name in enumerate(str(n) for n in golden["names"]):
        det, (H, Wd) = golden[f"det_{name}"], (int(v) for v in golden[f"hw_{name}"])
        frames = _frames(len(det), H, Wd, k)
        faces, coords = prepare_lip_avatar(frames, None, pads=tuple(int(p) for p in golden[f"pads_{name}"]), nosmooth=bool(golden[f"nosmooth_{name}"]),
                                           detections=_detections(det))
        assert coords == [tuple(int(v) for v in row) for row in golden[f"coords_{name}"]], name
        assert all(type(v) is int for c in coords for v in c)
        assert faces.is_cuda and faces.dtype == torch.uint8 and tuple(faces.shape) == (len(det), 96, 96, 3)
        _check_faces(frames, coords, faces)


def test_lip_avatar_other_size_and_device_frames(lib_built, golden):
    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar
    det = golden["det_n9"]
    frames = _frames(9, 72, 88, 3)
    faces, coords = prepare_lip_avatar(torch.from_numpy(frames).cuda(), None, detections=_detections(det), img_size=48)
    assert coords == [tuple(int(v) for v in row) for row in golden["coords_n9"]] and tuple(faces.shape) == (9, 48, 48, 3)
    _check_faces(frames, coords, faces, 48)


def test_lip_avatar_raises_the_references_error_without_a_face(lib_built, golden):
    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar
    det = golden["det_n6"]
    with pytest.raises(ValueError, match="Face not detected! Ensure the video contains a face in all the frames."):
        prepare_lip_avatar(_frames(6, 72, 88, 0), None, detections=_detections(det, counts=[1, 1, 0, 1, 1, 1]))
    with pytest.raises(ValueError, match="6 detections for 5 frames"):
        prepare_lip_avatar(_frames(5, 72, 88, 0), None, detections=_detections(det))


def test_lip_avatar_feeds_lip_session(lib_built, golden, gpu_model_factory):
    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar
    from mere_fusion_amd.lip_driver import LipSession
    from mere_fusion_amd.paste import AvatarFrames
    frames = _frames(6, 72, 88, 4)
    faces, coords = prepare_lip_avatar(frames, None, detections=_detections(golden["det_n6"]))
    av = AvatarFrames(frames, coords, lip_order=True)
    assert av.bboxes == [(x1, y1, x2, y2) for (y1, y2, x1, x2) in coords]
    sess = LipSession(gpu_model_factory("bf16"), faces, av)
    assert sess.length == 6 and sess.faces.data_ptr() == faces.data_ptr()
    mel, _, _ = W.make_lip_inputs(2, 0)
    out, idx = sess.step_pasted(mel.cuda())
    out = out.cpu().numpy()
    assert idx == [0, 1] and out.shape == (2, 72, 88, 3)
    y1, y2, x1, x2 = coords[0]
    outside = np.ones((72, 88), dtype=bool)
    outside[y1:y2, x1:x2] = False
    assert np.array_equal(out[0][outside], frames[0][outside])


def _shifted_state_dict(g):
    """tests/test_s3fd_detect.py's detector: seeded weights whose face logits are shifted so that the seeded images of the committed golden hold faces"""
    sd = W.make_s3fd_state_dict(0)
    for n, s in zip(LEVEL_NAMES, g["E_bias_shift"]):
        sd[n + "_mbox_conf.bias"] = sd[n + "_mbox_conf.bias"].clone()
        sd[n + "_mbox_conf.bias"][-1] += float(s)
    return sd


def test_lip_avatar_through_the_detector_equals_the_stepwise_route(lib_built):
    """the one-enqueue route against get_detections_for_batch + the numpy models, step by step, on the seeded detector and images of s3fd_detect_golden.npz
    (96 x 128: images 1 and 2 hold a face, 0 and 3 none)"""
    from mere_fusion_amd.avatar import FaceAlignment
    from mere_fusion_amd.avatar.prepare import prepare_lip_avatar
    g = np.load(os.path.join(ROOT, "tests", "golden", "s3fd_detect_golden.npz"))
    assert list(g["F_has_box"]) == [False, True, True, False]
    fa = FaceAlignment(device="cuda", state_dict=_shifted_state_dict(g), max_batch=4)
    frames = np.ascontiguousarray(g["E_images"][[1, 2, 2, 1, 1, 2]])
    H, Wd = frames.shape[1:3]
    faces, coords = prepare_lip_avatar(frames, fa, det_batch=4)
    rects = [r for i in range(0, 6, 4) for r in fa.get_detections_for_batch(frames[i:i + 4])]
    assert all(r is not None for r in rects)
    want, no_face = R.lip_boxes(rects, [1] * 6, H, Wd)
    assert no_face == 0 and coords == [tuple(int(v) for v in row) for row in want]
    _check_faces(frames, coords, faces)
    with_flat = np.ascontiguousarray(g["E_images"][[1, 3, 2]])
    assert fa.get_detections_for_batch(with_flat)[1] is None                     # genavatar.py:83-85 raises on it
    with pytest.raises(ValueError, match="Face not detected!"):
        prepare_lip_avatar(with_flat, fa)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_muse_avatar_latents_masks_and_session(lib_built):
    from mere_fusion_amd.avatar import FaceParsing
    from mere_fusion_amd.avatar.prepare import COORD_PLACEHOLDER, prepare_muse_avatar
    from mere_fusion_amd.muse_driver import MuseSession
    from mere_fusion_amd.musetalk.config import vae_config_json
    from mere_fusion_amd.musetalk.models.vae import VAE
    from mere_fusion_amd.musetalk.utils import blending
    from oracle import musetalk_ref
    g = np.load(os.path.join(ROOT, "tests", "golden", "face_mask_golden.npz"))
    gen = _load(os.path.join(ROOT, "tests", "golden", "make_face_mask_golden.py"), "make_face_mask_golden")
    fp = FaceParsing(state_dict=gen.state_dict(g["conv_out_weight"]), max_batch=4)
    cfg = musetalk_ref.MUSETALK_SMALL
    sd = dict(W.make_musetalk_vae_state_dict(cfg, 0))
    sd.update(W.make_musetalk_vae_encoder_state_dict(cfg, 0))
    vae = VAE(config=vae_config_json(cfg["vae"]), state_dict=sd, max_batch=2)
    frames = np.stack([g["frame_A"], g["frame_C"], g["frame_A"], g["frame_C"]])                   # 200 x 240
    b0, b1 = (tuple(int(v) for v in g["face_boxes"][k]) for k in range(2))
    boxes = [b0, COORD_PLACEHOLDER, b1, (100, 20, 141, 199)]
    keep = [0, 2, 3]
    latents, avatar = prepare_muse_avatar(frames, vae, fp, boxes=boxes, generator=torch.Generator(device="cuda").manual_seed(11))
    assert len(latents) == 3 and avatar.n == 3 and avatar.bboxes == [boxes[i] for i in keep]
    assert torch.equal(avatar.frames.cpu(), torch.from_numpy(frames[keep]))
    gen2 = torch.Generator(device="cuda").manual_seed(11)
    for lat, i in zip(latents, keep):
        crop = R.crop_lanczos4(frames[i], boxes[i], 256, 256)                                     # cv2.resize(frame[y1:y2, x1:x2], (256, 256), INTER_LANCZOS4)
        want = vae.get_latents_for_unet(crop, gen2)
        assert tuple(lat.shape) == (1, 8, 32, 32) and lat.is_cuda and torch.equal(lat, want)
    # a batch of device crops in one call: the same rows, the same noise order
    crops = torch.from_numpy(np.stack([R.crop_lanczos4(frames[i], boxes[i], 256, 256) for i in keep])).cuda()
    batch = vae.get_latents_for_unet(crops, torch.Generator(device="cuda").manual_seed(11))
    assert torch.equal(batch, torch.cat(latents))
    masks, crop_boxes = blending.prepare_materials(frames[keep], [boxes[i] for i in keep], fp)
    assert avatar.crop_boxes == [tuple(c) for c in crop_boxes]
    for m, got in zip(masks, avatar.masks):
        assert tuple(got.shape) == tuple(m.shape) + (3,) and all(torch.equal(got[:, :, c], m) for c in range(3))
    sess = MuseSession(latents, avatar)
    assert sess.length == 3 and torch.equal(sess.latents, torch.cat(latents))
    with pytest.raises(ValueError, match="Face not detected!"):
        prepare_muse_avatar(frames[:1], vae, fp, boxes=[COORD_PLACEHOLDER])
    with pytest.raises(ValueError, match="landmark boxes, or fa"):
        prepare_muse_avatar(frames[:1], vae, fp)
