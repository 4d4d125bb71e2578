"""The DWPose landmark path end to end on the device (avatar/dwpose.py, avatar/prepare.py) against the UNPINNED oracle of tests/dwpose_ref.py (a restatement of
the published mmdet / mmpose modules; the seeded weights are random, no real checkpoint has been loaded)."""
import os

import numpy as np
import pytest
import torch

import dwpose_ref as R
from mere_fusion_amd import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
REDUCED = dict(deepen=1.0 / 3.0, widen=0.25, input_size=(64, 96))
BOUND = {"bf16x3": 2e-3}                                                       # tests/test_avatar.py's bound for S3FD and BiSeNet
SEED = 0                                                                       # weights
FRAME_SEED = 6                                                                 # frames of the reduced net's tests: chosen on the CPU (test_landmarks_end_to_end)


def _frames(n, H, W, seed):
    """smooth synthetic frames (random low-frequency colour fields), not noise: the warp halves noise away"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W, 3))
    for i in range(n):
        for c in range(3):
            for _ in range(6):
                fx, fy, ph, a = rng.uniform(0.5, 6) / W, rng.uniform(0.5, 6) / H, rng.uniform(0, 6.28), rng.uniform(10, 40)
                out[i, :, :, c] += a * np.sin(6.28 * (fx * x + fy * y) + ph)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def reduced():
    """the reduced net's seeded weights, frames and the fp64 oracle's logits of both passes, computed once"""
    sd = W.make_dwpose_state_dict(SEED, **REDUCED)
    ref = R.DWPoseRef.reduced().double()
    ref.load_state_dict(sd)
    frames = _frames(2, 120, 90, FRAME_SEED)
    pre = [R.preprocess(f, (64, 96)) for f in frames]
    x = torch.from_numpy(np.stack([p[0] for p in pre])).double()
    lx, ly = ref.logits(x)
    fx, fy = ref.logits(x.flip(-1))
    return dict(sd=sd, frames=frames, center=pre[0][1], scale=pre[0][2], want=[t.numpy() for t in (lx, ly, fx, fy)])


def _pose(sd, prec, max_batch, input_size):
    from mere_fusion_amd.avatar.dwpose import DWPose
    return DWPose(precision=prec, max_batch=max_batch, input_size=input_size).load_state_dict(sd)


def _rel(got, want):
    return max(float(np.abs(g.cpu().numpy() - w[:g.shape[0]]).max() / np.abs(w).max()) for g, w in zip(got, want))


@pytest.mark.parametrize("batch", [1, 2])
def test_reduced_net_logits(lib_built, reduced, batch):
    """widen 0.25, deepen 1/3, input 96 x 64: the SimCC logits of the straight and the mirrored pass against the fp64 oracle, max|d| / max|oracle| <= 2e-3 in bf16x3;
    bf16's error must be at least 10 x bf16x3's, which shows that the comparison sees a precision loss"""
    fr = torch.from_numpy(reduced["frames"][:batch]).cuda()
    err = {}
    for prec in ("bf16x3", "bf16"):
        got = _pose(reduced["sd"], prec, 2, (64, 96)).logits(fr)
        assert tuple(got[0].shape) == (batch, 133, 128) and tuple(got[1].shape) == (batch, 133, 192)
        err[prec] = _rel(got, reduced["want"])
        print(f"dwpose reduced, batch {batch}, {prec}: max|d| / max|oracle| = {err[prec]:.3e}")
    assert err["bf16x3"] <= BOUND["bf16x3"]
    assert err["bf16"] >= 10 * err["bf16x3"]


def test_full_size_net_logits(lib_built):
    """rtmpose-l at 384 x 288, once, batch 1, bf16x3, straight pass, same bound"""
    sd = W.make_dwpose_state_dict(SEED)
    ref = R.DWPoseRef().double()
    ref.load_state_dict(sd)
    frames = _frames(1, 240, 320, 2)
    x = torch.from_numpy(R.preprocess(frames[0])[0][None]).double()
    want = [t.numpy() for t in ref.logits(x)]
    got = _pose(sd, "bf16x3", 1, R.INPUT_SIZE).logits(torch.from_numpy(frames).cuda(), flip=False)
    assert tuple(got[0].shape) == (1, 133, 576) and tuple(got[1].shape) == (1, 133, 768)
    err = _rel(got[:2], want)
    print(f"dwpose full size, bf16x3: max|d| / max|oracle| = {err:.3e}")
    assert err <= BOUND["bf16x3"]


def _margins(l):
    """top bin minus the best bin more than one away, per keypoint axis"""
    top = l.argmax(-1)
    idx = np.arange(l.shape[-1])
    far = np.abs(idx[None, None, :] - top[..., None]) > 1
    return l.max(-1) - np.where(far, l, -np.inf).max(-1)


def test_landmarks_end_to_end(lib_built, reduced):
    """(a) mf_simcc_decode on the device's own logits equals the oracle's decode of those logits copied back, exactly.  (b) Against the fp64 oracle's own logits the
    face keypoint axes are compared where the oracle's margin (top bin minus the best bin more than one away) exceeds four times the logit bound; there the device's
    coordinate is within one bin (half an input pixel, mapped back).  Weights seed 0, frames _frames(2, 120, 90, 6), picked on the CPU among frame seeds 1-8 (shares left out 8.1 % to 15.1 %): 8.1 % of the 2 x 68 x 2 face
    axes are left out (cap 10 %, asserted), and the fp32 oracle's keypoints equal the fp64 oracle's on every axis kept (asserted here as well, on the CPU)."""
    pose = _pose(reduced["sd"], "bf16x3", 2, (64, 96))
    fr = torch.from_numpy(reduced["frames"]).cuda()
    lx, ly, fx, fy = pose.logits(fr)
    kp, sc = pose.decode(lx, ly, fx, fy, 90, 120)
    c, s, pairs = reduced["center"], reduced["scale"], R.flip_indices()
    want_k, want_s = R.decode(lx.cpu().numpy(), ly.cpu().numpy(), c, s, fx.cpu().numpy(), fy.cpu().numpy(), pairs, (64, 96))
    assert np.array_equal(kp.cpu().numpy().view(np.uint32), want_k.view(np.uint32)) and np.array_equal(sc.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
    w = [a.astype(np.float32) for a in reduced["want"]]
    ax, ay = R.flip_average(w[0], w[1], w[2], w[3], pairs)
    ok_k, _ = R.decode(w[0], w[1], c, s, w[2], w[3], pairs, (64, 96))
    keep = np.stack([_margins(ax) > 4 * BOUND["bf16x3"] * np.abs(ax).max(), _margins(ay) > 4 * BOUND["bf16x3"] * np.abs(ay).max()], -1)[:, R.FACE]
    share = 1.0 - keep.mean()
    print(f"dwpose landmarks: {share:.1%} of the face axes left out")
    assert share <= 0.10
    r32 = R.DWPoseRef.reduced()
    r32.load_state_dict(reduced["sd"])
    x32 = torch.from_numpy(np.stack([R.preprocess(f, (64, 96))[0] for f in reduced["frames"]]))
    v = [t.numpy() for t in (*r32.logits(x32), *r32.logits(x32.flip(-1)))]
    k32, _ = R.decode(v[0], v[1], c, s, v[2], v[3], pairs, (64, 96))
    assert (k32[:, R.FACE][keep] == ok_k[:, R.FACE][keep]).all()
    bin_px = s / np.array([64, 96], np.float32) / 2                             # one bin in frame pixels
    d = np.abs(kp.cpu().numpy()[:, R.FACE] - ok_k[:, R.FACE])
    assert (d[keep] <= np.broadcast_to(bin_px * 1.001, d.shape)[keep]).all()


def _shifted_detector():
    from test_avatar_build import _shifted_state_dict
    from mere_fusion_amd.avatar import FaceAlignment
    g = np.load(os.path.join(ROOT, "tests", "golden", "s3fd_detect_golden.npz"))
    return FaceAlignment(device="cuda", state_dict=_shifted_state_dict(g), max_batch=4), np.ascontiguousarray(g["E_images"][[1, 3, 2]])


def test_muse_landmark_boxes_one_read_back(lib_built, monkeypatch):
    """3 frames of the committed detector golden (96 x 128), the middle one without a face: the boxes equal the oracle's box statements run on the device's own
    keypoints and the detector's rectangles; the host reads back once (every Tensor.cpu() of a device tensor during the call is counted)"""
    from mere_fusion_amd.avatar.prepare import COORD_PLACEHOLDER, muse_landmark_boxes
    fa, frames = _shifted_detector()
    pose = _pose(W.make_dwpose_state_dict(SEED, **REDUCED), "bf16x3", 2, (64, 96))
    fr = torch.from_numpy(frames).cuda()
    kp = torch.cat([pose.keypoints(fr[:2])[0], pose.keypoints(fr[2:])[0]]).cpu().numpy()
    rects = fa.get_detections_for_batch(frames)
    assert rects[1] is None and rects[0] is not None and rects[2] is not None
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (calls.append(1) if t.is_cuda else None, real(t, *a, **k))[1])
    for shift in (0, 3):
        calls.clear()
        coords, text = muse_landmark_boxes(fr, pose, fa, shift)
        assert len(calls) == 1
        want, flags, sums = R.landmark_boxes(kp, rects, shift)
        assert coords == [tuple(c) for c in want] and coords[1] == COORD_PLACEHOLDER and text == R.range_text(3, sums, shift)
        assert all(type(v) is int for i in (0, 2) for v in coords[i])


def _muse_models():
    """the face parser and the reduced VAE of tests/test_avatar_build.py::test_muse_avatar_latents_masks_and_session"""
    from test_avatar_build import _load
    from mere_fusion_amd.avatar import FaceParsing
    from mere_fusion_amd.musetalk.config import vae_config_json
    from mere_fusion_amd.musetalk.models.vae import VAE
    from oracle import musetalk_ref
    g = np.load(os.path.join(ROOT, "tests", "golden", "face_mask_golden.npz"))
    gen = _load(os.path.join(ROOT, "tests", "golden", "make_face_mask_golden.py"), "make_face_mask_golden")
    fp = FaceParsing(state_dict=gen.state_dict(g["conv_out_weight"]), max_batch=4)
    cfg = musetalk_ref.MUSETALK_SMALL
    sd = dict(W.make_musetalk_vae_state_dict(cfg, 0))
    sd.update(W.make_musetalk_vae_encoder_state_dict(cfg, 0))
    return fp, VAE(config=vae_config_json(cfg["vae"]), state_dict=sd, max_batch=2)


def _centred_state_dict(seed):
    """seeded reduced-net weights whose SimCC bins outside the middle of each axis are switched off (zero rows of cls_x / cls_y give logit 0, below the largest
    of the random logits left), so that the random landmarks fall inside a 96 x 128 frame and give a landmark box; with the plain seeded weights the landmarks
    spread over the padded box, x1 < 0 and every frame falls back to the detector's box, which on the detector golden is too small for the blend-mask step"""
    sd = dict(W.make_dwpose_state_dict(seed, **REDUCED))
    wx, wy = sd["head.cls_x.weight"].clone(), sd["head.cls_y.weight"].clone()
    wx[:20] = 0; wx[108:] = 0; wy[:62] = 0; wy[130:] = 0
    sd["head.cls_x.weight"], sd["head.cls_y.weight"] = wx, wy
    return sd


PREP_SEED = 10            # picked on the CPU with the fp32 oracle among seeds 0-39: landmark boxes (9, 13, 117, 89) and (9, 22, 117, 80), inside the frame, at shift 0 and -2


def test_prepare_muse_avatar_from_landmarks(lib_built, monkeypatch):
    """prepare_muse_avatar(frames, vae, fp, pose=..., fa=...) on 3 frames of the detector golden, the middle one without a face: its boxes are the oracle's box
    statements run on the device's keypoints, the frame without a face leaves the avatar, the result equals prepare_muse_avatar(..., boxes=those) tensor for tensor,
    and the host reads back exactly once (every Tensor.cpu() / .item() / .tolist() of a device tensor during the call is counted)."""
    from mere_fusion_amd.avatar.prepare import COORD_PLACEHOLDER, prepare_muse_avatar
    fa, frames = _shifted_detector()
    fp, vae = _muse_models()
    pose = _pose(_centred_state_dict(PREP_SEED), "bf16x3", 2, (64, 96))
    fr = torch.from_numpy(frames).cuda()
    kp = torch.cat([pose.keypoints(fr[:2])[0], pose.keypoints(fr[2:])[0]]).cpu().numpy()
    rects = fa.get_detections_for_batch(frames)
    assert rects[1] is None
    with pytest.raises(ValueError, match="need the detector too"):
        prepare_muse_avatar(fr, vae, fp, pose=pose)
    for shift in (0, -2):
        want, flags, _ = R.landmark_boxes(kp, rects, shift)
        want = [tuple(c) for c in want]
        assert want[1] == COORD_PLACEHOLDER and flags == [1, 0, 1]
        calls = []
        with monkeypatch.context() as mp:
            for name in ("cpu", "item", "tolist"):
                real = getattr(torch.Tensor, name)
                mp.setattr(torch.Tensor, name, lambda t, *a, _real=real, **k: (calls.append(1) if t.is_cuda else None, _real(t, *a, **k))[1])
            latents, avatar = prepare_muse_avatar(fr, vae, fp, pose=pose, fa=fa, bbox_shift=shift, generator=torch.Generator(device="cuda").manual_seed(5))
        assert len(calls) == 1, f"{len(calls)} host read-backs"
        assert avatar.n == 2 and avatar.bboxes == [want[0], want[2]] and len(latents) == 2
        lat2, av2 = prepare_muse_avatar(fr, vae, fp, boxes=want, generator=torch.Generator(device="cuda").manual_seed(5))
        assert av2.bboxes == avatar.bboxes and av2.crop_boxes == avatar.crop_boxes
        assert all(torch.equal(a, b) for a, b in zip(latents, lat2)) and torch.equal(avatar.frames, av2.frames)
        assert torch.equal(avatar.frames.cpu(), torch.from_numpy(frames[[0, 2]]))
        assert len(avatar.masks) == len(av2.masks) == 2 and all(torch.equal(a, b) for a, b in zip(avatar.masks, av2.masks))


def test_preprocessing_module_refuses_paths_and_unset_models(lib_built):
    """mere_fusion_amd.musetalk.utils.preprocessing: the reference's names, file paths refused with VAE.preprocess_img's sentence.  (It is not re-exported under
    dropin/: tests/test_blend.py pins that `musetalk.utils.preprocessing` falls through to the reference there.)"""
    from mere_fusion_amd.musetalk.utils import preprocessing as mod
    assert mod.coord_placeholder == (0.0, 0.0, 0.0, 0.0)
    for fn in (mod.get_landmark_and_bbox, mod.get_bbox_range):
        with pytest.raises(RuntimeError, match=r"reading image files \(cv2.imread\) stays with the reference"):
            fn(["./results/lyria/00000.png"])
        with pytest.raises(RuntimeError, match="set musetalk.utils.preprocessing.model"):
            fn([np.zeros((8, 8, 3), np.uint8)])


def test_preprocessing_module_builds_the_boxes(lib_built):
    from mere_fusion_amd.avatar.prepare import muse_landmark_boxes
    from mere_fusion_amd.musetalk.utils import preprocessing as mod
    fa, frames = _shifted_detector()
    pose = _pose(W.make_dwpose_state_dict(SEED, **REDUCED), "bf16x3", 4, (64, 96))
    mod.model, mod.fa = pose, fa
    try:
        coords, got_frames = mod.get_landmark_and_bbox(list(frames), 2)
        want, text = muse_landmark_boxes(frames, pose, fa, 2)
        assert coords == want and len(got_frames) == 3 and mod.get_bbox_range(list(frames), 2) == text
    finally:
        mod.model, mod.fa = None, None
