"""CPU: the host side of `mere_fusion_amd.nerf_driver.NerfSession` -- the loader's index arithmetic against hand-written sequences, the constructor's
refusals, and the three symbols the session needs in header, exports and ctypes table (tests/test_abi.py covers the last for every symbol; it is restated
here so that this file fails without the feature)."""
import ctypes as C

import pytest
import torch

import nerf_session_ref as ref

NEW_SYMBOLS = ("mf_nerf_frame_background", "mf_nerf_frame_out", "mf_nerf_head_set_aabb")


def test_loader_indices_against_hand_written_sequences():
    from mere_fusion_amd.nerf_driver import loader_indices
    # 5 poses, 12 frames: forwards, backwards (the loader's 2 * 5 indices), then the loader starts again
    audio = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 1]
    mirrored = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 0, 1]
    assert [loader_indices(5, k) for k in range(12)] == list(zip(audio, mirrored))
    assert ref.loader_sequence(5, 12) == list(zip(audio, mirrored))
    # one pose: every index is 0; three poses over two wraps
    assert [loader_indices(1, k) for k in range(5)] == [(0, 0), (1, 0), (0, 0), (1, 0), (0, 0)]
    assert [loader_indices(3, k)[1] for k in range(14)] == [0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]


class _NoModel:
    torso = False


def _args(n=5, H=8, W=6, device="cpu"):
    poses = torch.eye(4, device=device).repeat(n, 1, 1)
    return dict(model=_NoModel(), poses=poses, intrinsics=(10.0, 10.0, 3.0, 4.0), H=H, W=W, get_rays=lambda *a, **k: None)


def test_custom_index_arithmetic_and_switching():
    """nerfreal.py:98-102 on the host: both audio types non-zero and a cycle registered for the first; the custom cycle ping-pongs on its own counter while the
    loader keeps advancing.  (The custom branch needs no device work until the frame is formed: frame_out is replaced by a recorder.)"""
    from mere_fusion_amd import nerf_driver
    kw = _args()
    cycle = torch.arange(3 * 2 * 2 * 3, dtype=torch.uint8).reshape(3, 2, 2, 3)
    s = nerf_driver.NerfSession.__new__(nerf_driver.NerfSession)
    s.size, s.index, s.custom_img_cycle, s.custom_index = 5, 0, {2: cycle}, {2: 0}
    seen = []
    s.frame_out = lambda image, body=None: seen.append(int(body[0, 0, 0]) // 12) or "frame"
    s.poses = kw["poses"]
    for k in range(7):
        assert s.step(None, audiotype=(2, 2)) == "frame"
    assert seen == [0, 1, 2, 2, 1, 0, 0] and s.custom_index[2] == 7 and s.index == 7 and s.last_index == 3 and s.last_audio_index == 6
    # a type without a registered cycle, or one silent chunk, is a rendered frame: no custom image, the counter stays
    for at in ((3, 3), (2, 0), (0, 2), (0, 0)):
        assert s.next_custom(at) is None
    assert s.custom_index[2] == 7
    assert int(s.next_custom((2, 1))[0, 0, 0]) // 12 == 1 and s.custom_index[2] == 8      # the FIRST type chooses the cycle (nerfreal.py:98-99)


def test_constructor_refusals_by_name():
    from mere_fusion_amd.nerf_driver import NerfSession
    kw = _args()
    with pytest.raises(RuntimeError, match=r"4 torso images for 5 poses"):
        NerfSession(**kw, torso_imgs=torch.zeros(4, 8, 6, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"a 6 x 8 frame at \(3, 0\) leaves the 8 x 20 body frame"):
        NerfSession(**kw, fullbody_frames=torch.zeros(5, 20, 8, 3, dtype=torch.uint8), fullbody_offset=(3, 0))
    with pytest.raises(RuntimeError, match=r"a 12 x 9 frame at \(0, 0\) leaves the 11 x 9 body frame"):
        NerfSession(**kw, fullbody_frames=torch.zeros(5, 9, 11, 3, dtype=torch.uint8), gui_size=(9, 12))
    with pytest.raises(RuntimeError, match=r"3 body frames for 5 poses"):
        NerfSession(**kw, fullbody_frames=torch.zeros(3, 20, 20, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"poses must be a CUDA tensor \(there is no CPU path\)"):
        NerfSession(**kw)
    with pytest.raises(RuntimeError, match=r"torso_imgs must be uint8 RGBA \[N, 8, 6, 4\]"):
        NerfSession(**kw, torso_imgs=torch.zeros(5, 8, 6, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"bg must be an image, 'white' or 'black'"):
        NerfSession(**kw, bg="green")
    with pytest.raises(RuntimeError, match=r"eye_area holds 4 values for 5 poses"):
        NerfSession(**kw, eye_area=torch.zeros(4, 1))


def test_new_symbols_in_header_exports_and_ctypes_table(lib_built):
    from mere_fusion_amd import _lib
    lib = C.CDLL(lib_built)
    for name in NEW_SYMBOLS:
        assert name in _lib.HEADER.functions, f"{name} is not declared in merefusion.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not in the ctypes table"
    l = _lib.lib()
    # null arguments are refused by name before any launch (the paste-rectangle refusal takes real buffers: tests/test_nerf_session.py)
    assert l.mf_nerf_frame_background(None, None, 0.0, 4, 4, 0, None, None) == -1 and b"nerf_frame_background" in l.mf_last_error()
    assert l.mf_nerf_head_set_aabb(None, None) == -1 and b"null handle" in l.mf_last_error()
    assert l.mf_nerf_frame_out(None, 4, 4, 6, 5, None, 10, 10, 0, 0, 0, None, None) == -1 and b"nerf_frame_out" in l.mf_last_error()
