"""GPU tier of mf_crop_resize_u8: byte-equal to the integer models of tests/crop_resize_ref.py (linear: oracle.blend_ref.resize_linear_u8 on the cropped array; lanczos4:
the two-pass on ops.lanczos4_tables), for every crop shape at which the kernels take another path."""
import numpy as np
import pytest
import torch

import crop_resize_ref as R

pytestmark = pytest.mark.gpu


def _frames(reps=(1, 1)):
    """3 frames of 72 x 88 (noise, a gradient, hard edges), optionally tiled for the crops larger than a frame"""
    rng = np.random.default_rng(7)
    fr = rng.integers(0, 256, (3, 72, 88, 3), dtype=np.uint8)
    y, x = np.mgrid[0:72, 0:88]
    fr[1] = ((x * 3 + y * 2)[:, :, None] + np.array([0, 85, 170])) % 256
    fr[2, 20:50, 30:60] = (255, 0, 255)
    fr[2, 50:, :20] = 0
    return np.ascontiguousarray(np.tile(fr, (1, reps[0], reps[1], 1)))


@pytest.fixture(scope="module")
def small(lib_built):
    fr = _frames()
    return fr, torch.from_numpy(fr).cuda()


@pytest.fixture(scope="module")
def tiled(lib_built):
    fr = _frames((4, 4))                                 # 288 x 352: the 200 x 260 of the large linear crops and the 300 x 280 Lanczos crop both fit
    return fr, torch.from_numpy(fr).cuda()


def _check(frames, dev, boxes, idx, size, mode):
    from mere_fusion_amd import ops
    dw, dh = (size, size) if isinstance(size, int) else size
    got = ops.crop_resize_u8(dev, boxes, size, mode=mode, frame_indices=idx).cpu().numpy()
    model = R.crop_linear if mode == "linear" else R.crop_lanczos4
    assert got.shape == (len(boxes), dh, dw, 3)
    for k, (b, f) in enumerate(zip(boxes, idx)):
        want = model(frames[f], b, dw, dh)
        assert np.array_equal(got[k], want), f"{mode} job {k}: box {b} of frame {f}: {int((got[k] != want).sum())} bytes differ"
    return got


def test_linear_to_96_byte_equal(small, tiled):
    fr, dev = tiled
    # 192 x 192 (area path), 191 x 192 and 192 x 191 (not the area path), 96 x 96 (copy), all inside the 200 x 260 corner of the tiled frames
    _check(fr, dev, [(5, 3, 197, 195), (5, 3, 196, 195), (5, 3, 197, 194), (60, 100, 156, 196), (68, 8, 260, 200)], [0, 1, 2, 1, 2], 96, "linear")
    fr, dev = small
    # 40 x 33 (upscale), 1 pixel wide, 1 pixel tall, one crop on each frame edge, the corners, the whole frame
    boxes = [(11, 9, 51, 42), (30, 5, 31, 60), (5, 30, 60, 31), (0, 10, 25, 50), (60, 10, 88, 50), (20, 0, 70, 30), (20, 40, 70, 72), (0, 0, 9, 9), (80, 64, 88, 72),
             (0, 0, 88, 72)]
    _check(fr, dev, boxes, [0, 1, 2, 0, 1, 2, 0, 1, 2, 1], 96, "linear")


def test_lanczos_to_256_byte_equal(small, tiled):
    fr, dev = small
    # 37 x 53, 5 x 5 (every tap clamps), one crop on each frame edge, the whole frame
    boxes = [(10, 7, 47, 60), (40, 30, 45, 35), (0, 10, 25, 50), (60, 10, 88, 50), (20, 0, 70, 30), (20, 40, 70, 72), (0, 0, 88, 72), (87, 71, 88, 72)]
    _check(fr, dev, boxes, [0, 1, 2, 0, 1, 2, 1, 0], 256, "lanczos4")
    fr, dev = tiled
    # 256 x 256 (identity), 300 x 280 (downscale: taps skip rows), the whole 352 x 288 frame
    got = _check(fr, dev, [(33, 17, 289, 273), (3, 2, 303, 282), (0, 0, 352, 288)], [2, 1, 0], 256, "lanczos4")
    assert np.array_equal(got[0], fr[2, 17:273, 33:289])


def test_lanczos_strong_decimation_takes_the_row_chunks(tiled):
    """288 rows -> 16: a destination tile's rows spread over more source rows than the kernel's LDS block holds, so the tile is taken in chunks"""
    fr, dev = tiled
    _check(fr, dev, [(0, 0, 352, 288), (10, 0, 300, 288)], [1, 2], (40, 16), "lanczos4")
    _check(fr, dev, [(0, 0, 352, 288)], [0], (33, 3), "lanczos4")


@pytest.mark.parametrize("mode", ["linear", "lanczos4"])
def test_batch_of_37_shuffled_and_one_alone(small, mode):
    """37 jobs in shuffled frame order at a destination of 75 x 41: more than one workgroup per axis, and a remainder on both axes of the Lanczos tile (32 x 16) and
    of the linear kernel's 256-pixel groups"""
    from mere_fusion_amd import ops
    fr, dev = small
    rng = np.random.default_rng(37)
    boxes, idx = [], []
    for _ in range(37):
        x1, y1 = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        boxes.append((x1, y1, int(rng.integers(x1 + 1, 89)), int(rng.integers(y1 + 1, 73))))
        idx.append(int(rng.integers(0, 3)))
    assert len(set(idx)) == 3 and idx != sorted(idx)
    got = _check(fr, dev, boxes, idx, (75, 41), mode)
    for k in (0, 19, 36):
        alone = ops.crop_resize_u8(dev, [boxes[k]], (75, 41), mode=mode, frame_indices=[idx[k]]).cpu().numpy()
        assert np.array_equal(alone[0], got[k])


@pytest.mark.parametrize("mode,size", [("linear", 96), ("lanczos4", (75, 41))])
def test_dst_view_leaves_its_surroundings_untouched(small, mode, size):
    from mere_fusion_amd import ops
    fr, dev = small
    dw, dh = (size, size) if isinstance(size, int) else size
    block = torch.full((5, dh, dw, 3), 0xA5, dtype=torch.uint8, device="cuda")
    boxes, idx = [(10, 7, 47, 60), (0, 0, 88, 72)], [2, 0]
    out = ops.crop_resize_u8(dev, boxes, size, mode=mode, frame_indices=idx, out=block[2:4])
    assert out.data_ptr() == block[2].data_ptr()
    host = block.cpu().numpy()
    assert (host[:2] == 0xA5).all() and (host[4:] == 0xA5).all()
    model = R.crop_linear if mode == "linear" else R.crop_lanczos4
    for k in range(2):
        assert np.array_equal(host[2 + k], model(fr[idx[k]], boxes[k], dw, dh))


def test_device_job_table_and_rows_the_kernel_refuses(small):
    """a table the host never saw: valid rows are byte-equal to the model, rows that are empty, outside the frame or of a missing frame give a zeroed crop"""
    from mere_fusion_amd import ops
    fr, dev = small
    rows = [(1, 10, 7, 47, 60), (0, 5, 5, 5, 20), (2, 0, 0, 88, 72), (3, 0, 0, 10, 10), (0, 0, 0, 0, 0), (1, 80, 60, 89, 72), (2, -1, 0, 10, 10), (0, 0, 30, 88, 31)]
    jobs = torch.tensor(rows, dtype=torch.int32, device="cuda")
    got = ops.crop_resize_u8(dev, jobs, 96, mode="linear").cpu().numpy()
    for k, (f, x1, y1, x2, y2) in enumerate(rows):
        if k in (0, 2, 7):
            assert np.array_equal(got[k], R.crop_linear(fr[f], (x1, y1, x2, y2), 96, 96)), k
        else:
            assert not got[k].any(), k
    with pytest.raises(RuntimeError, match="host list"):
        ops.crop_resize_u8(dev, jobs, 256, mode="lanczos4")


@pytest.mark.parametrize("mode", ["linear", "lanczos4"])
def test_every_argument_error_is_refused_before_a_launch(small, mode):
    """host-side argument checks: each returns MF_ERR_INVALID with its message, nothing is launched, and the next valid call is served"""
    from mere_fusion_amd import ops
    fr, dev = small
    for boxes, idx, size, msg in [([(10, 10, 10, 40)], [0], 96, r"job 0: crop \(10, 10, 10, 40\) is empty"),
                                  ([(0, 0, 8, 8), (10, 40, 30, 40)], [0, 1], 96, r"job 1: crop .* is empty"),
                                  ([(30, 10, 20, 40)], [0], 96, "is empty"),
                                  ([(0, 0, 89, 72)], [0], 96, r"outside the 88 x 72 frame"),
                                  ([(0, -1, 40, 40)], [0], 96, "outside"),
                                  ([(0, 0, 40, 73)], [2], 96, "outside"),
                                  ([(0, 0, 40, 40)], [3], 96, r"frame index 3 out of range \(3 frames\)"),
                                  ([(0, 0, 40, 40)], [-1], 96, "frame index -1 out of range"),
                                  ([(0, 0, 40, 40)], [0], (0, 96), "destination 96 x 0"),
                                  ([(0, 0, 40, 40)], [0], (96, 0), "destination 0 x 96")]:
        with pytest.raises(RuntimeError, match=msg):
            ops.crop_resize_u8(dev, boxes, size, mode=mode, frame_indices=idx)
    with pytest.raises(RuntimeError, match="mode must be"):
        ops.crop_resize_u8(dev, [(0, 0, 8, 8)], 96, mode="cubic")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.crop_resize_u8(torch.from_numpy(fr), [(0, 0, 8, 8)], 96, mode=mode)
    size = 96 if mode == "linear" else (75, 41)
    _check(fr, dev, [(10, 7, 47, 60)], [1], size, mode)
    torch.cuda.synchronize()
