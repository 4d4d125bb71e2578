"""CPU: the host side of I420 delivery -- the integer arithmetic the kernel restates (csrc/mf_i420.hip) against the float64 matrix, the ring's slot shape, and
what serving.PipelinedScheduler does with frame_format="i420" before any frame exists: it refuses a ring of packed slots, and silent batches stay None."""
import numpy as np
import pytest

import i420_ref as R
from mere_fusion_amd import serving as S
from mere_fusion_amd import transport as T
from serving_fakes import FakeBatcher, FakeRing, fake_cuda_events

B = 2


@pytest.mark.parametrize("order", ["bgr", "rgb"])
def test_integer_model_against_the_float64_matrix(order):
    """0.51 code: half a code of rounding plus the 16.16 coefficients' own error (at most 3 x 0.5 / 65536 x 255 = 0.006 for luma, the same over the block mean
    for chroma).  Seeded random [4, 64, 72, 3] plus the five primaries as 2 x 2 blocks."""
    rng = np.random.default_rng(420)
    frames = rng.integers(0, 256, (4, 64, 72, 3), dtype=np.uint8)
    frames[3] = R.primaries_frame(64, 72, order)
    got = R.planes(R.i420_model(frames, order), 64, 72)
    want = R.i420_float64(frames, order)
    for name, g, w in zip(("Y", "Cb", "Cr"), got, want):
        err = float(np.abs(g.astype(np.float64) - w).max())
        print(f"{order} {name}: max |integer - float64| = {err:.4f} code")
        assert err <= 0.51, (name, err)


def test_known_answers():
    for (r, g, b), want in R.KNOWN.items():
        for order, px in (("rgb", (r, g, b)), ("bgr", (b, g, r))):
            frame = np.broadcast_to(np.array(px, np.uint8), (1, 2, 2, 3)).copy()
            out = R.i420_model(frame, order)
            assert out.shape == (1, 3, 2)
            y, cb, cr = R.planes(out, 2, 2)
            assert (set(y.ravel().tolist()), int(cb[0, 0, 0]), int(cr[0, 0, 0])) == ({want[0]}, want[1], want[2]), ((r, g, b), order)
    grey = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], (1, 2, 256, 3)))   # both chroma rows sum to zero
    _, cb, cr = R.planes(R.i420_model(grey, "rgb"), 2, 256)
    assert set(cb.ravel().tolist()) == set(cr.ravel().tolist()) == {128}


def test_i420_shape():
    assert T.i420_shape(720, 1280) == (1080, 1280)
    assert T.i420_shape(2, 2) == (3, 2)
    assert T.i420_shape(6, 10) == (9, 10)                                  # H no multiple of 4: the planes are bytes of one buffer
    assert T.i420_shape(30, 40) == (45, 40)
    for hw in ((3, 4), (4, 3), (0, 2), (2, 0), (-2, 2)):
        with pytest.raises(ValueError, match="even and positive"):
            T.i420_shape(*hw)
    ring = T.FrameRing(2, T.i420_shape(6, 10))
    try:
        assert ring.frame_shape == (9, 10) and ring.slot_bytes == 90         # 1.5 bytes per pixel
    finally:
        ring.close()


def test_abi_refusals_name_the_value_and_launch_nothing(lib_built):
    """every refusal comes before the launch, so none needs a device; the pointers are never read"""
    import ctypes as C
    from mere_fusion_amd import _lib
    l = _lib.lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    for args, text in (((None, 1, 4, 4, 0, p), b"frames is a null pointer"), ((p, 1, 4, 4, 0, None), b"out is a null pointer"),
                       ((p, 0, 4, 4, 0, p), b"n_frames 0"), ((p, -2, 4, 4, 0, p), b"n_frames -2"), ((p, 1, 0, 4, 0, p), b"frame size 0 x 4"),
                       ((p, 1, 4, -4, 0, p), b"frame size 4 x -4"), ((p, 1, 5, 4, 0, p), b"H 5 is odd"), ((p, 1, 4, 7, 1, p), b"W 7 is odd"),
                       ((p, 1, 4, 4, 2, p), b"rgb_order 2")):
        assert l.mf_frames_to_i420(*args, None) == -1, args
        assert text in l.mf_last_error(), (args, l.mf_last_error())
    assert bytes(buf) == bytes(64)


class _ShapedRing(FakeRing):
    def __init__(self, places, frame_shape):
        super().__init__(places)
        self.frame_shape = tuple(frame_shape)


class _BgrBatcher(FakeBatcher):
    frame_order = "bgr"                                                     # its frames are [B, 4, 4, 3]


def test_scheduler_refuses_a_packed_ring_with_frame_format_i420():
    bat = _BgrBatcher(2, 2, batch_size=B)
    good, packed = _ShapedRing(2 * B, T.i420_shape(4, 4)), _ShapedRing(2 * B, (4, 4, 3))
    with pytest.raises(RuntimeError, match=r"ring 1 has slots of shape \(4, 4, 3\)"):
        S.PipelinedScheduler(bat, rings=[good, packed], single_stream=True, frame_format="i420")
    with pytest.raises(RuntimeError, match="frame_format must be one of"):
        S.PipelinedScheduler(bat, rings=[good, good], single_stream=True, frame_format="nv12")
    with pytest.raises(RuntimeError, match="without rings"):
        S.PipelinedScheduler(bat, single_stream=True, frame_format="i420")
    with pytest.raises(RuntimeError, match="does not state its frames' channel order"):
        S.PipelinedScheduler(FakeBatcher(2, 2, batch_size=B), rings=[good, good], single_stream=True, frame_format="i420")
    bat.frame_hw = lambda k: (8, 4)                                         # a batcher that knows its frame size: the ring must hold exactly that
    with pytest.raises(RuntimeError, match=r"need \(12, 4\)"):
        S.PipelinedScheduler(bat, rings=[good, good], single_stream=True, frame_format="i420")
    bat.frame_hw = lambda k: (4, 4)
    S.PipelinedScheduler(bat, rings=[good, good], single_stream=True, frame_format="i420").close()
    # the default format looks at no ring
    S.PipelinedScheduler(FakeBatcher(2, 2, batch_size=B), rings=[packed, FakeRing(2 * B)], single_stream=True).close()


def test_silent_batches_pass_through_as_none_with_frame_format_i420(monkeypatch):
    fake_cuda_events(monkeypatch)
    rings = [_ShapedRing(2 * B, T.i420_shape(4, 4)) for _ in range(2)]
    bat = _BgrBatcher(2, 2, batch_size=B)
    with S.PipelinedScheduler(bat, rings=rings, clock=lambda: 1.0, hold_s=0.0, single_stream=True, frame_format="i420") as sch:
        sch.submit(0, None, 0.5, pairs=[("a", 1)] * (2 * B))                 # the default stage: the payload is the batcher's input; None is a silent batch
        sch.submit(1, None, 0.6, pairs=[("b", 1)] * (2 * B))
        done = sch.run_once() + sch.drain()
    assert sorted(k for k, *_ in done) == [0, 1] and all(fr is None for _, fr, _, _ in done)
    assert bat.steps == [([0, 1], [None, None])] and bat.index == [B, B]
    for k, ring in enumerate(rings):                                         # B (None, idx, audio pair) tuples per session, nothing left open
        assert ring.msgs == [(None, i, [("ab"[k], 1)] * 2) for i in range(B)] and not ring.open and not ring.aborted
