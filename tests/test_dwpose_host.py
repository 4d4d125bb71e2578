"""Host tier of the DWPose landmark path: the oracle (tests/dwpose_ref.py) against itself and against hand-derived answers.  No GPU.
The oracle is UNPINNED: a restatement of the published mmdet / mmpose modules and of musetalk/utils/preprocessing.py:96-131, never compared with those packages."""
import numpy as np
import torch

import dwpose_ref as R
from mere_fusion_amd import weights as W

REDUCED = dict(deepen=1.0 / 3.0, widen=0.25, input_size=(64, 96))


def test_manifest_is_the_mmpose_checkpoint_layout():
    """key names, shapes and the parameter count of rtmpose-l whole-body 384 x 288; the generator's manifest is the oracle module tree's state_dict, key for key"""
    m = R.DWPoseRef()
    sd = m.state_dict()
    man = W.dwpose_manifest()
    assert [k for k, _ in man] == list(sd.keys())
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in man)
    assert len(man) == 470
    assert sum(p.numel() for p in m.parameters()) == 33_610_919            # backbone 26 138 912 + head 7 472 007 (the 7 x 7 final conv alone: 6 673 541)
    pinned = {"backbone.stem.0.conv.weight": (32, 3, 3, 3), "backbone.stem.2.bn.running_var": (64,), "backbone.stage1.1.main_conv.conv.weight": (64, 128, 1, 1),
              "backbone.stage1.1.blocks.0.conv2.depthwise_conv.conv.weight": (64, 1, 5, 5), "backbone.stage2.1.blocks.5.conv2.pointwise_conv.conv.weight": (128, 128, 1, 1),
              "backbone.stage3.1.attention.fc.weight": (512, 512, 1, 1), "backbone.stage3.1.attention.fc.bias": (512,), "backbone.stage4.1.conv2.conv.weight": (1024, 2048, 1, 1),
              "backbone.stage4.2.final_conv.conv.weight": (1024, 1024, 1, 1), "backbone.stage4.2.blocks.2.conv1.bn.num_batches_tracked": (),
              "head.final_layer.weight": (133, 1024, 7, 7), "head.final_layer.bias": (133,), "head.mlp.0.g": (1,), "head.mlp.1.weight": (256, 108),
              "head.gau.uv.weight": (1152, 256), "head.gau.o.weight": (256, 512), "head.gau.gamma": (2, 128), "head.gau.beta": (2, 128), "head.gau.ln.g": (1,),
              "head.gau.res_scale.scale": (256,), "head.cls_x.weight": (576, 256), "head.cls_y.weight": (768, 256)}
    shapes = dict(man)
    for k, s in pinned.items():
        assert tuple(shapes[k]) == s, k
    assert not any("stage4.2.blocks.3" in k or "stage1.1.blocks.3" in k or "stage2.1.blocks.6" in k for k in shapes)      # 3, 6, 6, 3 blocks
    m.load_state_dict(W.make_dwpose_state_dict(0), strict=True)
    r = R.DWPoseRef.reduced()
    r.load_state_dict(W.make_dwpose_state_dict(0, **REDUCED), strict=True)
    assert W.make_dwpose_state_dict(0, shapes_only=True, **REDUCED)["head.mlp.1.weight"] == (256, 6)


def test_flip_indices_are_an_involution_and_the_products():
    from mere_fusion_amd.avatar.dwpose import flip_indices
    p = R.flip_indices()
    assert sorted(p) == list(range(133)) and all(p[p[i]] == i for i in range(133))
    assert [i for i in range(133) if p[i] == i] == [0, 31, 50, 51, 52, 53, 56, 74, 80, 85, 89]      # nose; chin, nose ridge and tip, lip mid-points
    assert p == flip_indices()


def test_oracle_fp32_against_fp64_on_the_reduced_net():
    """the fp32 oracle differs from the fp64 oracle by fp32 rounding only: 1e-4 of the largest logit is three orders above what some hundred fp32 operations in a
    row leave and three below a wrong layer"""
    sd = W.make_dwpose_state_dict(0, **REDUCED)
    a, b = R.DWPoseRef.reduced(), R.DWPoseRef.reduced().double()
    a.load_state_dict(sd); b.load_state_dict(sd)
    x = torch.from_numpy(np.stack([R.preprocess(f, (64, 96))[0] for f in np.random.default_rng(0).integers(0, 256, (2, 120, 90, 3), dtype=np.uint8)]))
    for got, want in zip(a.logits(x), b.logits(x.double())):
        assert want.abs().max() > 1 and (got.double() - want).abs().max() / want.abs().max() < 1e-4


def test_product_affine_is_the_oracles():
    from mere_fusion_amd.avatar.dwpose import topdown_affine
    for w, h in ((640, 480), (90, 120), (17, 31), (1920, 1080), (288, 384)):
        c, s, minv = topdown_affine(w, h)
        rc, rs = R.bbox_center_scale(w, h)
        assert np.array_equal(c, rc) and np.array_equal(s, rs) and c.dtype == np.float32
        assert np.array_equal(minv, R.invert_affine(R.warp_matrix(rc, rs)))
        assert abs(s[0] / s[1] - 0.75) < 1e-6 and s[0] >= 1.25 * w - 1e-3 and s[1] >= 1.25 * h - 1e-3


def test_affine_by_hand():
    """derived by hand, independent of both restatements.  A 640 x 480 frame: box [0, 0, 640, 480], centre (320, 240), scale 1.25 x = (800, 600); 800 > 600 * 0.75, so
    the height grows to 800 / 0.75 = 1066.67.  The map is a uniform zoom by 288 / 800 about the centre, so its inverse is x_src = 800 / 288 * (x - 144) + 320 =
    2.7778 x - 80 and y_src = 2.7778 (y - 192) + 240 = 2.7778 y - 293.33.  A 90 x 120 frame: scale (112.5, 150) has the input's aspect already; zoom 288 / 112.5."""
    from mere_fusion_amd.avatar.dwpose import topdown_affine
    for fn in (lambda w, h: topdown_affine(w, h), lambda w, h: (*R.bbox_center_scale(w, h), R.invert_affine(R.warp_matrix(*R.bbox_center_scale(w, h))))):
        c, s, minv = fn(640, 480)
        assert c.tolist() == [320.0, 240.0] and s[0] == 800.0 and abs(s[1] - 3200.0 / 3.0) < 1e-4
        assert np.allclose(minv, [[800.0 / 288.0, 0.0, -80.0], [0.0, 800.0 / 288.0, 240.0 - 192.0 * 800.0 / 288.0]], rtol=0, atol=1e-9)
        c, s, minv = fn(90, 120)
        assert c.tolist() == [45.0, 60.0] and s.tolist() == [112.5, 150.0]
        assert np.allclose(minv, [[112.5 / 288.0, 0.0, 45.0 - 144.0 * 112.5 / 288.0], [0.0, 112.5 / 288.0, 60.0 - 192.0 * 112.5 / 288.0]], rtol=0, atol=1e-9)


def test_strict_loading_names_what_is_wrong():
    from mere_fusion_amd.avatar.dwpose import DWPose
    import pytest
    sd = W.make_dwpose_state_dict(0, **REDUCED)
    DWPose(input_size=(64, 96)).load_state_dict(sd, strict=True)
    DWPose(input_size=(64, 96)).load_state_dict({"state_dict": sd})                       # a checkpoint file's wrapper
    less = {k: v for k, v in sd.items() if k != "backbone.stage2.1.attention.fc.bias"}
    with pytest.raises(RuntimeError, match=r"missing \['backbone.stage2.1.attention.fc.bias'\]"):
        DWPose(input_size=(64, 96)).load_state_dict(less)
    with pytest.raises(RuntimeError, match=r"unexpected \['head.extra'\]"):
        DWPose(input_size=(64, 96)).load_state_dict(dict(sd, **{"head.extra": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"wrong shape \['head.mlp.1.weight', 'head.cls_x.weight', 'head.cls_y.weight'\]"):
        DWPose(input_size=(288, 384)).load_state_dict(sd)                                  # flatten dims of another input size
    DWPose(input_size=(64, 96)).load_state_dict(less, strict=False)


def test_warp_integer_model_against_float64():
    rng = np.random.default_rng(1)
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    img = rng.integers(0, 256, (384, 288, 3), dtype=np.uint8)
    assert np.array_equal(R.warp_affine_int(img, ident, R.INPUT_SIZE), img)                                      # identity: byte-equal
    for H, Wd in ((480, 640), (31, 17), (100, 60)):                                                                  # the last two are smaller than 288 x 384
        img = rng.integers(0, 256, (H, Wd, 3), dtype=np.uint8)
        c, s = R.bbox_center_scale(Wd, H)
        for m in (R.invert_affine(R.warp_matrix(c, s)), np.array([[0.5371, 0.031, 2.3], [-0.027, 0.4412, 1.9]]) * (Wd / 288.0)):
            a, b = R.warp_affine_int(img, m, R.INPUT_SIZE).astype(np.float64), R.warp_affine_f64(img, m, R.INPUT_SIZE)
            # 1/32-pixel positions move a tap weight by at most 1/64 per axis; neighbours in random noise differ by up to 255, so the bound of "one code" holds for the
            # warp's own rounding only on smooth images: compare on a smooth image, and on noise bound by the position quantisation
            assert np.abs(a - b).max() <= 0.5 + 255 * (2 / 64 + 1e-9)
        y, x = np.mgrid[0:H, 0:Wd]
        smooth = np.stack([x * 200.0 / Wd, y * 200.0 / H, (x + y) * 100.0 / (H + Wd)], -1).round().astype(np.uint8)
        m = R.invert_affine(R.warp_matrix(c, s))
        a, b = R.warp_affine_int(smooth, m, R.INPUT_SIZE).astype(np.float64), R.warp_affine_f64(smooth, m, R.INPUT_SIZE)
        ox, oy = np.meshgrid(np.arange(R.INPUT_SIZE[0], dtype=np.float64), np.arange(R.INPUT_SIZE[1], dtype=np.float64))
        X, Y = m[0, 0] * ox + m[0, 1] * oy + m[0, 2], m[1, 0] * ox + m[1, 1] * oy + m[1, 2]
        inner = (X >= 0.05) & (X <= Wd - 1.05) & (Y >= 0.05) & (Y <= H - 1.05)                                       # all four taps inside the frame in both models
        assert inner.sum() > 1000 and np.abs(a - b)[inner].max() <= 1.0                                              # within one code


def test_decode_known_answers():
    K, bx, by = 4, 24, 32
    c, s = np.array([12.0 / 2, 16.0 / 2], np.float32), np.array([12.0, 16.0], np.float32)                    # input 12 x 16 mapped onto itself
    x, y = np.full((1, K, bx), -1, np.float32), np.full((1, K, by), -1, np.float32)
    x[0, 0, 7] = 3; y[0, 0, 9] = 2                                                                            # one-hot at bin k -> k / 2
    x[0, 1, 5] = x[0, 1, 11] = 4; y[0, 1, 3] = y[0, 1, 30] = 4                                                # a tie takes the first maximum
    x[0, 2, 6] = 0; y[0, 2, 6] = 5                                                                            # a non-positive smaller maximum -> -1 (-0.5 after / 2)
    x[0, 3, 23] = 1; y[0, 3, 0] = 6
    kp, sc = R.decode(x, y, c, s, input_size=(12, 16))
    assert kp[0].tolist() == [[3.5, 4.5], [2.5, 1.5], [-0.5, -0.5], [11.5, 0.0]] and sc[0].tolist() == [2.0, 4.0, 0.0, 1.0]
    # flip pair (0, 1): the flipped pass saw keypoint 1 at mirrored bin (bx - 1 - 7): averaged, the peak stays at bin 7 with the mean height
    xf, yf = np.full((1, K, bx), -1, np.float32), np.full((1, K, by), -1, np.float32)
    xf[0, 1, bx - 1 - 7] = 5; yf[0, 1, 9] = 4
    kp, sc = R.decode(x, y, c, s, xf, yf, [1, 0, 2, 3], (12, 16))
    assert kp[0, 0].tolist() == [3.5, 4.5] and sc[0, 0] == 3.0                                                # min((3 + 5) / 2, (2 + 4) / 2)


def _face():
    lm = np.zeros((133, 2), np.float32)
    face = np.stack([np.linspace(100.4, 180.9, 68), np.linspace(50.2, 140.8, 68)], 1).astype(np.float32)
    face[28, 1], face[29, 1], face[30, 1] = 80.9, 95.9, 107.2
    lm[R.FACE] = face
    return lm


def test_landmark_box_statements_by_hand():
    det = (90, 40, 200, 160)
    # a normal face: x 100..180, max y 140; half = 95; upper = 95 - (140 - 95) = 50
    coords, flags, sums = R.landmark_boxes([_face()], [det])
    assert coords == [(100, 50, 180, 140)] and flags == [1] and sums == (107 - 95, 95 - 80, 1)
    # bbox_shift +10: half 105, upper 105 - 35 = 70; -10: half 85, upper 85 - 55 = 30; the ranges are taken before the shift
    assert R.landmark_boxes([_face()], [det], 10)[0] == [(100, 70, 180, 140)]
    assert R.landmark_boxes([_face()], [det], -10)[0] == [(100, 30, 180, 140)]
    assert R.landmark_boxes([_face()], [det], -10)[2] == (12, 15, 1)
    # a shift that pushes row 29 below every other landmark moves the maximum too (half_face_coord is a view): max y = 95 + 60 = 155 = half -> y2 - y1 = 0 -> detector
    assert R.landmark_boxes([_face()], [det], 60)[:2] == ([det], [2])
    # each fallback condition alone
    flat = _face(); flat[R.FACE, 1] = 77.7                                   # y2 - y1 = 77 - (77 - 0) = 0
    thin = _face(); thin[R.FACE, 0] = 120.3                                  # x2 - x1 = 0
    left = _face(); left[23, 0] = -1.2                      # x1 = -1 < 0
    for kp in (flat, thin, left):
        assert R.landmark_boxes([kp], [det])[:2] == ([det], [2])
    # truncation, not floor: -0.9 -> 0, the landmark box stays
    trunc = _face(); trunc[23, 0] = -0.9
    assert R.landmark_boxes([trunc], [det])[:2] == ([(0, 50, 180, 140)], [1])
    # no face: the placeholder, and nothing enters the range sums
    coords, flags, sums = R.landmark_boxes([_face(), _face()], [None, det])
    assert coords == [R.COORD_PLACEHOLDER, (100, 50, 180, 140)] and flags == [0, 1] and sums == (12, 15, 1)
    assert R.range_text(2, sums, 3) == "Total frame:「2」 Manually adjust range : [ -12~15 ] , the current value: 3"
    assert R.detector_box([-3.2, 10.9, 700.5, 470.2, 0.9], 640, 480) == (0, 10, 640, 470)


def test_product_range_text_is_the_oracles():
    from mere_fusion_amd.avatar.prepare import range_text
    for sums in ((12, 15, 1), (-7, 100, 3), (0, 0, 0)):
        assert range_text(5, sums, -2) == R.range_text(5, sums, -2)
