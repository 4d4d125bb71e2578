"""MuseTalk's blend masks on the device (csrc/mf_face_mask.hip, avatar/face_parsing.py, musetalk/utils/blending.py `prepare_materials`).

Golden = the reference's own statements around the reference's own BiSeNet, Pillow doing the resizes (tests/golden/make_face_mask_golden.py -> face_mask_golden.npz).
The resizes are integer arithmetic and held to 0 differing values.  The class mask is held to the reference on every pixel that is not a near tie: a pixel is flagged
when the best class in 1..13 and the best class in {0, 14..18} are within 2 x 2e-3 x max|logit|, the BiSeNet logit gate of tests/test_avatar.py spent by both sides.
The blur has no pinned reference (no OpenCV here): it is held to tests/face_mask_ref.py's float64 evaluation of the published formulas -- within 1 level everywhere, and
equal to round(float64) wherever the float64 value is farther than 1e-2 from a rounding boundary (the fp32 error of two passes of <= 151 taps is bounded by
2 x 151 x 2^-24 x 255 ~ 5e-3)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import face_mask_ref as R

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW_SYMBOLS = ["mf_face_mask_parse", "mf_face_mask_finish", "mf_face_mask_workspace_bytes"]
SIZES = [(90, 90), (300, 300), (613, 613), (1024, 1024), (257, 401)]          # (width, height)
N_JOBS, N_RS = 3, 3


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "face_mask_golden.npz"))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_face_mask_golden", os.path.join(ROOT, "tests", "golden", "make_face_mask_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)                      # the reference is only imported inside its main()
    return m


def _frame(golden, k):
    return golden["frame_" + str(golden["job_frame"][k])]


def _tie(golden, k):
    return np.unpackbits(golden[f"near_tie{k}"])[:512 * 512].reshape(512, 512).astype(bool)


def _geometry(golden, k, upper=0.5, expand=1.2):
    x, y, x1, y1 = (int(v) for v in golden["face_boxes"][k])
    (x_s, y_s, x_e, y_e), _ = R.get_crop_box((x, y, x1, y1), expand)
    w, h = x_e - x_s, y_e - y_s
    return (w, h, x - x_s, y - y_s, x1 - x_s, y1 - y_s, int(h * upper))


def _normalise(crop512):
    """ToTensor + Normalize on the host (face_parsing/__init__.py:29-33), [h, w, 3] uint8 -> [3, h, w] fp32"""
    t = torch.from_numpy(np.ascontiguousarray(crop512.transpose(2, 0, 1))).float().div(255)
    return (t - torch.tensor([0.485, 0.456, 0.406])[:, None, None]) / torch.tensor([0.229, 0.224, 0.225])[:, None, None]


def _tie_in_crop(tie512, w, h, k):
    """near-tie pixels carried to the crop-size mask: every crop pixel whose bicubic window or blur window can see one"""
    ys, xs = np.nonzero(tie512)
    m = np.zeros((h, w), bool)
    m[np.minimum(ys * h // 512, h - 1), np.minimum(xs * w // 512, w - 1)] = True
    return R.dilate(m, int(np.ceil(2 * max(max(w, h) / 512, 1))) + 1 + k // 2)


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------------------------
def test_ref_resampler_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    for w, h in SIZES + [(512, 300), (512, 512)]:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_u8(a, (512, 512), R.BILINEAR), np.asarray(Image.fromarray(a).resize((512, 512), Image.BILINEAR))), (w, h)
        m = (rng.integers(0, 2, (512, 512)) * 255).astype(np.uint8)
        assert np.array_equal(R.resize_u8(m, (w, h), R.BICUBIC), np.asarray(Image.fromarray(m).resize((w, h)))), (w, h)       # the default filter of mode L


def test_ref_equals_golden(golden):
    for k in range(N_JOBS):
        frame, box = _frame(golden, k), [int(v) for v in golden[f"crop_box{k}"]]
        assert box == R.get_crop_box([int(v) for v in golden["face_boxes"][k]], 1.2)[0]
        assert np.array_equal(R.resize_u8(R.crop_u8(frame[:, :, ::-1], box), (512, 512), R.BILINEAR), golden[f"crop512_{k}"])
        w, h = box[2] - box[0], box[3] - box[1]
        seg = R.resize_u8(golden[f"mask512_{k}"], (w, h), R.BICUBIC)
        assert np.array_equal(seg, golden[f"seg_{k}"])
        assert np.array_equal(R.window(seg, [int(v) for v in golden["face_boxes"][k]], box), golden[f"preblur_{k}"])
    assert any(b[0] < 0 or b[1] < 0 or b[2] > f.shape[1] or b[3] > f.shape[0] for b, f in ((golden[f"crop_box{k}"], _frame(golden, k)) for k in range(N_JOBS)))
    for k in range(N_RS):
        frame = golden["frame_" + str(golden[f"rs_frame{k}"])]
        src = frame[:, :, ::-1] if bool(golden[f"rs_rev{k}"]) else frame
        assert np.array_equal(R.resize_u8(R.crop_u8(src, [int(v) for v in golden[f"rs_box{k}"]]), (512, 512), R.BILINEAR), golden[f"rs_crop512_{k}"])
    # the head logits of job 0, upsampled and classified on the host, give the stored mask wherever the pixel is not a near tie
    up = torch.nn.functional.interpolate(torch.from_numpy(golden["head_logits0"])[None], (512, 512), mode="bilinear", align_corners=True)[0].numpy()
    assert np.array_equal(R.class_mask(up)[~_tie(golden, 0)], golden["mask512_0"][~_tie(golden, 0)])


def test_generator_conditions_hold_on_committed_golden(golden, gen):
    assert tuple(golden["settings"]) == (gen.SEED, gen.HEAD_CONTRAST, gen.LOGIT_GATE, gen.UPPER, gen.EXPAND) and gen.LOGIT_GATE == 2e-3
    assert golden["head_logits0"].shape == (19, 64, 64)
    for k in range(N_JOBS):
        share, ties = float((golden[f"mask512_{k}"] > 0).mean()), float(_tie(golden, k).mean())
        assert 0.2 <= share <= 0.8 and ties <= 0.01, (k, share, ties)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "face_mask_golden.npz")) < 1 << 20


def test_new_symbols_in_header_exports_and_ctypes_table(lib_built):
    import ctypes as C
    from mere_fusion_amd import _lib
    declared = set(_lib.HEADER.functions)
    lib = C.CDLL(lib_built)
    for n in NEW_SYMBOLS:
        assert n in declared and hasattr(lib, n) and n in _lib.SIGNATURES, n
    l = _lib.lib()
    assert l.mf_abi_version() == 4                                            # symbols were only added
    sizes = (C.c_int * 2)(108, 108)
    assert l.mf_face_mask_workspace_bytes(0, sizes, 1, 512, 512) > 108 * 512 * 3 and l.mf_face_mask_workspace_bytes(1, sizes, 1, 512, 512) > 108 * 108 * 5
    # argument checks that need no device: a null pointer, and the two geometry limits by name
    assert l.mf_face_mask_finish(None, 512, 512, None, 1, 1, None, 0, None, None, None) == -1 and b"null" in l.mf_last_error()
    dummy = C.c_void_p(256)                                                   # never dereferenced: the geometry is refused before any launch
    wide = (C.c_int * 7)(1600, 1600, 0, 0, 1600, 1600, 800)
    assert l.mf_face_mask_finish(dummy, 512, 512, wide, 1, 1, dummy, 1 << 40, None, dummy, None) == -1
    assert b"161-tap blur" in l.mf_last_error() and b"MF_FM_BLUR_MAX_K = 151" in l.mf_last_error()
    tiny = (C.c_int * 7)(20, 20, 0, 0, 20, 20, 10)
    assert l.mf_face_mask_finish(dummy, 512, 512, tiny, 1, 1, dummy, 1 << 40, None, dummy, None) == -1 and b"MF_FM_MAX_TAPS = 64" in l.mf_last_error()
    assert l.mf_face_mask_workspace_bytes(1, (C.c_int * 2)(1600, 1600), 1, 512, 512) == 0


def test_blur_ref_properties():
    from mere_fusion_amd.avatar.face_parsing import blur_kernel_size
    assert [blur_kernel_size(w) for w in (102, 108, 612, 1500)] == [R.blur_kernel_size(w) for w in (102, 108, 612, 1500)] == [11, 11, 61, 151]
    assert abs(R.gaussian_taps(61).sum() - 1) < 1e-15
    flat = np.full((40, 50), 200, np.uint8)
    assert np.abs(R.gaussian_blur(flat, 11) - 200).max() < 1e-10            # REFLECT_101 keeps a flat image flat


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp(lib_built, golden, gen):
    from mere_fusion_amd.avatar import FaceParsing
    return FaceParsing(state_dict=gen.state_dict(golden["conv_out_weight"]), max_batch=4)


def _cases(golden):
    """(name, frame, crop box, channel reversal, Pillow's 512 x 512 crop)"""
    out = [(f"job{k}", _frame(golden, k), [int(v) for v in golden[f"crop_box{k}"]], True, golden[f"crop512_{k}"]) for k in range(N_JOBS)]
    return out + [(f"rs{k}", golden["frame_" + str(golden[f"rs_frame{k}"])], [int(v) for v in golden[f"rs_box{k}"]], bool(golden[f"rs_rev{k}"]), golden[f"rs_crop512_{k}"])
                  for k in range(N_RS)]


@pytest.mark.gpu
def test_resample_and_fused_normalisation_bit_equal(fp, golden):
    """upscale, downscale, a non-square box, boxes that leave the frame, a source read with and without the channel reversal, an axis Pillow skips: the parser's input
    planes after the device resample are bit-equal to set_input of the host-normalised Pillow crop, i.e. 0 differing 8-bit values and the same normalisation"""
    g = fp._graph((512, 512))
    n = g["net"]
    for name, frame, box, rev, crop512 in _cases(golden):
        x = _normalise(crop512)[None]
        n.set_input(g["inp"], x)
        want = n.output(g["inp"], 8, 1).cpu()
        n.set_input(g["inp"], torch.zeros_like(x))
        fp.parse(torch.from_numpy(frame)[None].cuda(), [box], reverse_channels=rev)
        got = n.output(g["inp"], 8, 1).cpu()
        # the normalisation is injective on 0..255 at the planes' precision, so a differing plane value is a differing 8-bit value
        differing = int((got[:, :3].view(torch.int32) != want[:, :3].view(torch.int32)).sum())
        print(f"[face mask resample {name}] box {box} reverse {rev}: {differing} differing 8-bit values of {crop512.size}")
        assert differing == 0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        assert not got[:, 3:].any()


@pytest.mark.gpu
def test_parse_bit_equal_to_host_argmax_over_bisenet_call(fp, golden):
    """B = 3 with three crop sizes in one call, and B = 1: the fused upsample + argmax + remap equals numpy's over BiSeNet.__call__ of the same handle and input"""
    frames = torch.from_numpy(np.stack([golden["frame_A"], golden["frame_C"]])).cuda()
    boxes = [[int(v) for v in golden["crop_box0"]], [int(v) for v in golden["crop_box1"]], [int(v) for v in golden["rs_box1"]]]
    crops = [golden["crop512_0"], golden["crop512_1"], golden["rs_crop512_1"]]
    for sel in ([0, 1, 2], [1]):
        got = fp.parse(frames, [boxes[i] for i in sel], frame_indices=[[0, 0, 1][i] for i in sel]).cpu().numpy()
        logits = fp.net(torch.stack([_normalise(crops[i]) for i in sel]))[0].cpu().numpy()
        assert logits.shape == (len(sel), 19, 512, 512)
        for b in range(len(sel)):
            want = R.class_mask(logits[b])
            assert np.array_equal(got[b], want), f"batch {len(sel)}, item {b}: {(got[b] != want).sum()} pixels differ"
            assert 0.05 < (want > 0).mean() < 0.95


@pytest.mark.gpu
def test_parse_matches_reference_golden(fp, golden):
    for k in range(N_JOBS):
        got = fp.parse(torch.from_numpy(_frame(golden, k))[None].cuda(), [[int(v) for v in golden[f"crop_box{k}"]]])[0].cpu().numpy()
        want, tie = golden[f"mask512_{k}"], _tie(golden, k)
        wrong = int((got != want)[~tie].sum())
        print(f"[face mask parse job {k}] pixels that differ outside the {tie.sum()} near ties: {wrong}; agreement on the near ties: {(got == want)[tie].mean():.1%}")
        assert wrong == 0


@pytest.mark.gpu
def test_finish_stages_on_golden_masks(lib_built, golden):
    from mere_fusion_amd.avatar import finish_masks
    masks = torch.from_numpy(np.stack([golden[f"mask512_{k}"] for k in range(N_JOBS)])).cuda()
    jobs = [_geometry(golden, k) for k in range(N_JOBS)]
    blurred, pre = finish_masks(masks, jobs, want_pre_blur=True)
    only_pre = finish_masks(masks, jobs, blur=False)
    seg = finish_masks(masks, [(j[0], j[1], 0, 0, j[0], j[1], 0) for j in jobs], blur=False)       # face_seg alone: the bicubic resize
    for k in range(N_JOBS):
        assert np.array_equal(seg[k].cpu().numpy(), golden[f"seg_{k}"]), f"job {k}: bicubic mask-back resize"
        assert np.array_equal(pre[k].cpu().numpy(), golden[f"preblur_{k}"]) and torch.equal(pre[k], only_pre[k]), f"job {k}: windowed mask"
        ksz = R.blur_kernel_size(jobs[k][0])
        f64 = R.gaussian_blur(golden[f"preblur_{k}"], ksz)
        got = blurred[k].cpu().numpy().astype(np.float64)
        want = np.clip(np.rint(f64), 0, 255)
        clear = np.abs(f64 - np.floor(f64) - 0.5) > 1e-2
        print(f"[face mask blur job {k}] k = {ksz}: max |device - float64| {np.abs(got - f64).max():.4f} (gate: within 1 level of round), "
              f"{int((got != want)[clear].sum())} of {int(clear.sum())} clear pixels differ from round(float64), {int((got != want).sum())} of all {got.size}")
        assert np.abs(got - want).max() <= 1
        assert np.array_equal(got[clear], want[clear])
        assert 5 < got.mean() < 250 and len(np.unique(got)) > 50                                      # a real blur of a real mask


@pytest.mark.gpu
def test_get_image_prepare_material_end_to_end(fp, golden):
    from mere_fusion_amd.musetalk.utils import blending
    from mere_fusion_amd.paste import AvatarFrames
    for k in range(N_JOBS):
        face_box = tuple(int(v) for v in golden["face_boxes"][k])
        mask, crop_box = blending.get_image_prepare_material(_frame(golden, k), face_box, fp=fp)
        assert isinstance(mask, np.ndarray) and mask.dtype == np.uint8 and isinstance(crop_box, list)
        assert crop_box == [int(v) for v in golden[f"crop_box{k}"]]
        w, h = crop_box[2] - crop_box[0], crop_box[3] - crop_box[1]
        ksz = R.blur_kernel_size(w)
        f64 = R.gaussian_blur(golden[f"preblur_{k}"], ksz)
        want = np.clip(np.rint(f64), 0, 255)
        near = _tie_in_crop(_tie(golden, k), w, h, ksz) | (np.abs(f64 - np.floor(f64) - 0.5) <= 1e-2)
        held = ~near
        wrong = int((mask != want)[held].sum())
        edge, full = int(((want > 0) & (want < 255) & held).sum()), int(((want == 255) & held).sum())
        print(f"[face mask end to end job {k}] {mask.shape}: {wrong} pixels differ outside the {near.mean():.1%} of the mask near a tie; {int((mask != want).sum())} of all; "
              f"held pixels: {int(held.sum())}, of them {edge} on a blurred edge and {full} at 255")
        assert mask.shape == (h, w) and wrong == 0
        # what the exclusion leaves is fixed by the committed golden (44.0 %, 51.7 %, 33.1 % excluded): it must keep blurred edges and full mask, not only the trivial zeros
        assert near.mean() <= (0.45, 0.52, 0.34)[k] and edge >= (300, 600, 13000)[k] and full >= (1500, 1250, 16000)[k]
    # the batched route hands device masks to AvatarFrames without a PNG round trip
    masks, boxes = blending.prepare_materials(np.stack([golden["frame_B"]]), [tuple(int(v) for v in golden["face_boxes"][2])], fp)
    assert masks[0].is_cuda and masks[0].dtype == torch.uint8
    av = AvatarFrames(golden["frame_B"][None], [tuple(int(v) for v in golden["face_boxes"][2])], blending.mask_planes(masks), boxes)
    assert tuple(av.masks[0].shape) == tuple(masks[0].shape) + (3,) and torch.equal(av.masks[0][:, :, 1], masks[0])
    with pytest.raises(RuntimeError, match="3-channel"):                                              # the existing contract of get_image_blending stays
        blending.get_image_blending(golden["frame_B"].copy(), np.zeros((510, 510, 3), np.uint8), golden["face_boxes"][2], masks[0].cpu().numpy(), boxes[0])


@pytest.mark.gpu
def test_repeatable_and_batch_order_free(fp, golden):
    from mere_fusion_amd.musetalk.utils import blending
    frames = np.stack([golden["frame_A"], golden["frame_A"], golden["frame_C"]])
    boxes = [tuple(int(v) for v in golden["face_boxes"][0]), tuple(int(v) for v in golden["face_boxes"][1]), (40, 30, 150, 170)]
    first, crop = blending.prepare_materials(frames, boxes, fp)
    first = [m.cpu() for m in first]
    assert len({tuple(m.shape) for m in first}) == 3
    for _ in range(3):
        again, _ = blending.prepare_materials(frames, boxes, fp)
        assert all(torch.equal(a.cpu(), f) for a, f in zip(again, first))
    perm = [2, 0, 1]
    shuffled, crop2 = blending.prepare_materials(frames[perm], [boxes[i] for i in perm], fp)
    assert all(torch.equal(shuffled[j].cpu(), first[i]) for j, i in enumerate(perm)) and crop2 == [crop[i] for i in perm]
    one, _ = blending.prepare_materials(frames[1:2], boxes[1:2], fp)                                  # alone == inside a batch
    assert torch.equal(one[0].cpu(), first[1])


@pytest.mark.gpu
def test_call_and_face_seg_surface(fp, golden):
    rgb = np.ascontiguousarray(golden["frame_C"][:, :, ::-1])
    seg512, seg = fp(rgb), fp.face_seg(rgb)
    a512, a = np.asarray(seg512), np.asarray(seg)
    assert a512.shape == (512, 512) and a512.dtype == np.uint8 and set(np.unique(a512)) <= {0, 255}
    assert a.shape == rgb.shape[:2] and np.array_equal(a, R.resize_u8(a512, (rgb.shape[1], rgb.shape[0]), R.BICUBIC))
    try:
        from PIL import Image
    except ImportError:
        return
    assert isinstance(seg512, Image.Image) and seg512.mode == "L" and seg.size == (rgb.shape[1], rgb.shape[0])
    assert np.array_equal(np.asarray(fp(Image.fromarray(rgb))), a512)
