"""CPU: the lip-sync scorer's host side -- the golden against the real reference module, the state-dict surface and refusals of SyncNet_color, the argument checks
of the two new entry points, the / 255 rule, the window arithmetic, the monitor's ring and the curve reduction.  The device side is tests/test_sync_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import sync_ref as SR
from serving_fakes import FakeBatcher


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "syncnet_golden.npz")))


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------
def test_golden_regenerates_from_the_reference(golden):
    """bit for bit from the reference's own SyncNet_color in float64 (where the reference checkout is present: the build container)"""
    if not os.path.isdir("/root/reference/wav2lip"):
        pytest.skip("the reference checkout is not on this machine")
    import subprocess
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_syncnet_golden.py"), "--check"], capture_output=True, text=True)   # (its own process: the
    assert run.returncode == 0 and "identical" in run.stdout, run.stdout + run.stderr                    # reference's top-level `wav2lip` package stays out of this one)
    assert len(golden) >= 25


def test_golden_separates_its_windows(golden):
    """the condition on the fixture: embeddings of different windows lie at least 10 x the GPU test's embedding gate apart, face and audio alike"""
    for name in ("face", "audio"):
        e = golden[f"{name}_embedding"]
        d = min(np.linalg.norm(e[i] - e[j]) for i in range(len(e)) for j in range(i))
        assert abs(d - float(golden[f"{name}_distance"])) <= 1e-12
        assert d >= 10 * SR.TOL_X3, (name, d)
        assert np.allclose(np.linalg.norm(e, axis=1), 1.0, atol=1e-12)
    assert golden["frames"].shape == (6, 96, 96, 3) and golden["pcm"].shape == (3840,) and golden["mel_windows"].shape == (2, 1, 80, 16)
    assert np.array_equal(golden["frames"], SR.golden_frames()) and np.array_equal(golden["pcm"], SR.golden_pcm())
    assert np.array_equal(SR.face_windows(golden["frames"], golden["frame_starts"]), golden["face_windows_u8"] / 255.0)
    sim, curve, counts = SR.sync_score_ref(golden["face_embedding"], golden["audio_embedding"], int(golden["max_shift"]))
    assert np.abs(sim - golden["sim"]).max() <= 1e-12 and np.abs(curve - golden["curve"]).max() <= 1e-12 and np.array_equal(counts, golden["counts"])


# ---- the module's surface ------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_refusals():
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.wav2lip.models import SyncNet_color
    sd = W.syncnet_state_dict(0)
    assert len(sd) == 217
    assert sum(v.numel() for k, v in sd.items() if k.endswith((".weight", ".bias"))) == 16_435_072
    m = SyncNet_color()
    missing, unexpected = m.load_state_dict(sd)
    assert not missing and not unexpected
    back = m.state_dict()
    assert list(back.keys()) == list(sd.keys())
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    short = {k: v for k, v in sd.items() if k != "face_encoder.1.conv_block.0.weight"}
    short["extra.weight"] = torch.zeros(1)
    missing, unexpected = m.load_state_dict(short, strict=False)
    assert missing == ["face_encoder.1.conv_block.0.weight"] and unexpected == ["extra.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(short)
    assert m.eval() is m and m.to("cpu") is m
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 1, 80, 16), torch.zeros(1, 15, 48, 96))
    m.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        m(torch.zeros(1, 1, 80, 16), torch.zeros(1, 15, 48, 96))


def test_dropin_keeps_the_reference_discriminators():
    """the new class lives under the project's package only: the drop-in's wav2lip.models does not export it"""
    import mere_fusion_amd.wav2lip.models as M
    assert hasattr(M, "SyncNet_color")
    text = open(os.path.join(ROOT, "mere-fusion_amd", "dropin", "wav2lip", "models", "__init__.py")).read()
    assert "SyncNet" not in text.split('"""')[2]


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(lib_built):
    from mere_fusion_amd import _lib
    l = _lib.lib()
    one = (C.c_int * 1)(0)
    assert l.mf_net_set_input_u8_windows(None, 0, None, 5, 96, 96, one, 1, 5, 48, 48, None) == -1
    assert b"null" in l.mf_last_error()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert l.mf_sync_score(None, None, 1, 4, 0, None, None, None, None) == -1 and b"null" in l.mf_last_error()
    for W, dim, S, word in ((0, 4, 0, b"W = 0"), (1, 6, 0, b"dim 6"), (1, 0, 0, b"dim 0"), (1, 1028, 0, b"dim 1028"), (1, 4, -1, b"max_shift -1"), (1, 4, 65, b"max_shift 65")):
        assert l.mf_sync_score(p, p, W, dim, S, p, p, p, None) == -1, (W, dim, S)
        assert word in l.mf_last_error(), l.mf_last_error()
    assert l.mf_abi_version() == 4


def test_division_by_255_agrees_for_all_codes():
    """upstream divides in float64 and casts; the kernel divides in fp32: the same value for every one of the 256 codes, so no table is needed"""
    codes = np.arange(256, dtype=np.uint8)
    upstream = (codes / 255.0).astype(np.float32)
    kernel = codes.astype(np.float32) / np.float32(255.0)
    assert kernel.dtype == np.float32 and np.array_equal(upstream.view(np.uint32), kernel.view(np.uint32))


# ---- the window arithmetic ----------------------------------------------------------------------------------------------------------------------------------
def test_window_starts_hand_derived():
    from mere_fusion_amd.sync_score import window_starts
    # fps 25, 6 frames, 3840 samples: 1 + 3840 // 200 = 20 mel columns; windows at frames 0 and 1, mel columns int(3.2 i) = 0 and 3; 3 + 16 = 19 <= 20
    assert window_starts(6, 3840, 25) == [(0, 0), (1, 3)]
    assert window_starts(6, 3840, 25) == SR.window_starts(6, 3840, 25)
    assert window_starts(4, 3840, 25) == []                                   # fewer than 5 frames
    # the drop rule: 3799 samples give 19 columns, window 1 would need [3, 19) -- still inside; 3599 give 18: dropped
    assert window_starts(6, 3799, 25) == [(0, 0), (1, 3)]
    assert window_starts(6, 3599, 25) == [(0, 0)]
    assert window_starts(6, 2999, 25) == []                                   # 15 columns: not one window
    # 4 s: 100 frames, 64000 samples, 321 columns: 96 windows by the frames, the last at int(80 * 95 / 25) = 304, 304 + 16 = 320 <= 321
    w = window_starts(100, 64000, 25)
    assert len(w) == 96 and w[-1] == (95, 304) and w[5] == (5, 16)
    # fps 30: int(80 * i / 30) = 0, 2, 5, 8
    assert [m for _, m in window_starts(8, 16000, 30)] == [0, 2, 5, 8]
    # audio shorter than the frames: the mel ends first and the later windows go with it
    assert len(window_starts(100, 32000, 25)) == 46                           # 161 columns: int(3.2 i) + 16 <= 161 for i <= 45


def test_offset_confidence_and_ties():
    from mere_fusion_amd.sync_score import reduce_curve
    S = 2
    score, off, conf = reduce_curve([0.1, 0.5, 0.2, 0.3, 0.0], [3, 4, 5, 4, 3], S)
    assert score == 0.2 and off == -1 and conf == pytest.approx(0.5 - 0.2)
    # a tie goes to the smaller |shift| ...
    assert reduce_curve([0.7, 0.1, 0.2, 0.7 - 0.0, 0.1], [1, 1, 1, 1, 1], S)[1] == 1
    assert reduce_curve([0.1, 0.4, 0.4, 0.1, 0.4], [1, 1, 1, 1, 1], S)[1] == 0
    # ... and shifts without a valid window do not vote, however large their (zero-filled) entry
    score, off, conf = reduce_curve([9.0, -0.2, -0.3, -0.1, 9.0], [0, 1, 2, 1, 0], S)
    assert score == -0.3 and off == 1 and conf == pytest.approx(-0.1 - -0.2)
    assert reduce_curve([0.25], [1], 0) == (0.25, 0, 0.0)
    score, off, conf = reduce_curve([0.0, 0.5, 0.0], [0, 1, 0], 1)           # W = 1: only the centre
    assert (score, off, conf) == (0.5, 0, 0.0)
    # an even number of valid shifts: the median is the mean of the middle two
    assert reduce_curve([0.0, 0.1, 0.2, 0.4, 0.8], [0, 1, 1, 1, 1], S)[2] == pytest.approx(0.8 - 0.3)


# ---- the monitor's rings --------------------------------------------------------------------------------------------------------------------------------------
def test_ring_spans():
    from mere_fusion_amd.sync_score import ring_spans
    assert ring_spans(0, 4, 10) == [(0, 0, 4)]
    assert ring_spans(8, 2, 10) == [(8, 0, 2)]
    assert ring_spans(8, 5, 10) == [(8, 0, 2), (0, 2, 3)]
    assert ring_spans(3, 10, 10) == [(3, 0, 7), (0, 7, 3)]
    assert ring_spans(3, 0, 10) == [(3, 0, 0)]
    with pytest.raises(ValueError):
        ring_spans(10, 1, 10)


def test_monitor_ring_indices_on_the_host():
    """SyncMonitor over a FakeBatcher's steps on CPU tensors: every frame carries its index, its PCM the index too; after any number of steps the monitor holds
    the newest `capacity` frames in order, and the scorer is handed exactly those"""
    from mere_fusion_amd.sync_score import SyncMonitor
    seen = []
    scorer = type("S", (), {"fps": 25, "score": lambda self, fr, pcm: seen.append((fr.clone(), pcm.clone())) or "report"})()
    mon = SyncMonitor(scorer, seconds=0.4, face_size=(4, 4), device="cpu")     # 10 frames
    assert mon.capacity == 10 and mon.frames.shape == (10, 4, 4, 3) and mon.pcm.shape == (6400,)
    ptrs = (mon.frames.data_ptr(), mon.pcm.data_ptr(), mon._lin_frames.data_ptr(), mon._lin_pcm.data_ptr())
    fb = FakeBatcher(1, 1, batch_size=3)
    with pytest.raises(ValueError, match="a window needs 5"):
        mon.report()
    total = 0
    for step in range(9):                                                       # 27 frames through a ring of 10: wraps at several phases
        _, idx = fb.step([object()], only=[0])[0]
        fr = torch.stack([torch.full((4, 4, 3), i % 256, dtype=torch.uint8) for i in idx])
        pcm = torch.cat([torch.full((640,), float(i)) for i in idx])
        mon.push(fr, pcm)
        total += len(idx)
        assert mon.count == min(10, total) and mon.head == total % 10
        hf, hp = mon.held()
        want = list(range(total - mon.count, total))
        assert hf[:, 0, 0, 0].tolist() == want and hp[::640].tolist() == [float(i) for i in want] and hp[639::640].tolist() == [float(i) for i in want]
        if mon.count >= 5:
            assert mon.report() == "report"
            assert seen[-1][0][:, 0, 0, 0].tolist() == want and seen[-1][1].shape == (640 * len(want),)
    assert ptrs == (mon.frames.data_ptr(), mon.pcm.data_ptr(), mon._lin_frames.data_ptr(), mon._lin_pcm.data_ptr())     # allocated once
    mon.push(torch.stack([torch.full((4, 4, 3), i, dtype=torch.uint8) for i in range(100, 112)]), torch.zeros(12 * 640))   # a step larger than the ring
    assert mon.held()[0][:, 0, 0, 0].tolist() == list(range(102, 112))
    with pytest.raises(ValueError, match="samples"):
        mon.push(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros(640))
    with pytest.raises(ValueError, match="frames expected"):
        mon.push(torch.zeros((2, 5, 4, 3), dtype=torch.uint8), torch.zeros(1280))
