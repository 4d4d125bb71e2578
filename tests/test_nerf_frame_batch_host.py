"""CPU: the host side of the frame-indexed launches around the batched ER-NeRF head render (csrc/mf_nerf_frame_batch.hip) -- the five symbols in header, exports
and ctypes table, every argument refusal by name before anything touches a device (the handle allocates its descriptor ring at the first accepted call, so it
exists on a box without a GPU), and `NerfBatcher`'s grouping: frames of unequal size never share a call, and a size's frames fill neighbouring slots of one
block.  The bits are tests/test_nerf_frame_batch.py's business."""
import ctypes as C

import pytest
import torch

import nerf_serving_util as U  # noqa: F401  (the serving tests' shared helpers live on the same path)

NEW_SYMBOLS = ("mf_nerf_frame_batch_create", "mf_nerf_frame_batch_destroy", "mf_nerf_frame_batch_background", "mf_nerf_torso_forward_batch",
               "mf_nerf_frame_batch_out")
B = 2


def test_new_symbols_in_header_exports_and_ctypes_table(lib_built):
    from mere_fusion_amd import _lib
    declared = _lib.HEADER.functions
    lib = C.CDLL(lib_built)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in merefusion.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not in the ctypes table"
    # the declared argument lists, against the ctypes table: as many arguments, and the descriptor tables typed
    for name, n_args in (("mf_nerf_frame_batch_create", 3), ("mf_nerf_frame_batch_destroy", 1), ("mf_nerf_frame_batch_background", 6),
                         ("mf_nerf_torso_forward_batch", 6), ("mf_nerf_frame_batch_out", 12)):
        assert len(declared[name][1]) == n_args == len(_lib.SIGNATURES[name][1]), (name, declared[name])
    assert _lib.SIGNATURES["mf_nerf_frame_batch_background"][1][1] is C.POINTER(_lib.MfNerfBgDesc)
    assert _lib.SIGNATURES["mf_nerf_torso_forward_batch"][1][2] is C.POINTER(_lib.MfNerfTorsoDesc)
    assert _lib.SIGNATURES["mf_nerf_frame_batch_out"][1][1] is C.POINTER(_lib.MfNerfOutDesc)
    # the descriptors' layout is the header's: pointer, pointer, float, int, pointer / 50 floats, two pointers, int, two floats, three pointers / two pointers, two ints
    assert C.sizeof(_lib.MfNerfBgDesc) == 32 and C.sizeof(_lib.MfNerfOutDesc) == 24 and C.sizeof(_lib.MfNerfTorsoDesc) == 256
    assert _lib.MfNerfTorsoDesc.bg_coords.offset == 200 and _lib.MfNerfTorsoDesc.bg_out.offset == 232


@pytest.fixture()
def handle(lib_built):
    from mere_fusion_amd import _lib
    l, h = _lib.lib(), C.c_void_p()
    assert l.mf_nerf_frame_batch_create(3, 480, C.byref(h)) == 0 and h.value        # no device is touched: the ring comes with the first accepted call
    yield l, h
    l.mf_nerf_frame_batch_destroy(h)


def test_every_refusal_comes_by_name_before_anything_touches_a_device(handle):
    from mere_fusion_amd import _lib
    l, h = handle
    none = C.c_void_p()
    for frames, pixels, msg in ((0, 10, b"max_frames 0 (1..64)"), (65, 10, b"max_frames 65"), (2, 0, b"max_pixels 0")):
        assert l.mf_nerf_frame_batch_create(frames, pixels, C.byref(none)) == -1 and msg in l.mf_last_error() and not none.value
    assert l.mf_nerf_frame_batch_create(2, 10, None) == -1 and b"nerf_frame_batch_create" in l.mf_last_error()
    l.mf_nerf_frame_batch_destroy(None)                                              # a null handle is nothing to destroy

    bg, to, out = (_lib.MfNerfBgDesc * 4)(), (_lib.MfNerfTorsoDesc * 4)(), (_lib.MfNerfOutDesc * 4)()
    fake = 0x1000                                                                      # a pointer's worth of bits: no refusal below reads through it
    for d in bg:
        d.torso_rgba, d.bg_color = fake, fake
    for d in out:
        d.render, d.body_bgr = fake, fake

    def refused(rc, msg):
        assert rc == -1 and msg in l.mf_last_error(), (rc, l.mf_last_error())

    # ---- background
    refused(l.mf_nerf_frame_batch_background(None, bg, 1, 20, 24, None), b"nerf_frame_batch_background: null handle or descriptor table")
    refused(l.mf_nerf_frame_batch_background(h, None, 1, 20, 24, None), b"nerf_frame_batch_background: null handle or descriptor table")
    refused(l.mf_nerf_frame_batch_background(h, bg, 0, 20, 24, None), b"n_frames=0 (the handle holds 1..3)")
    refused(l.mf_nerf_frame_batch_background(h, bg, 4, 20, 24, None), b"n_frames=4 (the handle holds 1..3)")
    refused(l.mf_nerf_frame_batch_background(h, bg, 2, 20, 25, None), b"n_pixels=500 exceed the handle's max_pixels 480")
    refused(l.mf_nerf_frame_batch_background(h, bg, 2, 0, 24, None), b"nerf_frame_batch_background: frame 24 x 0")
    bg[1].bg_color = None
    refused(l.mf_nerf_frame_batch_background(h, bg, 2, 20, 24, None), b"frame 1: null torso_rgba or bg_color")
    bg[1].bg_color, bg[0].torso_rgba = fake, fake + 2
    refused(l.mf_nerf_frame_batch_background(h, bg, 2, 20, 24, None), b"frame 0: the RGBA image must be 4-byte aligned")
    # ---- torso (the batch handle's limits are checked before the torso handle is looked at)
    refused(l.mf_nerf_torso_forward_batch(None, None, to, 1, 64, None), b"nerf_torso_forward_batch: null handle or descriptor table")
    refused(l.mf_nerf_torso_forward_batch(None, h, None, 1, 64, None), b"nerf_torso_forward_batch: null handle or descriptor table")
    refused(l.mf_nerf_torso_forward_batch(None, h, to, 0, 64, None), b"n_frames=0 (the handle holds 1..3)")
    refused(l.mf_nerf_torso_forward_batch(None, h, to, 4, 64, None), b"n_frames=4 (the handle holds 1..3)")
    refused(l.mf_nerf_torso_forward_batch(None, h, to, 3, 481, None), b"n_pixels=481 (the handle's max_pixels is 480)")
    refused(l.mf_nerf_torso_forward_batch(None, h, to, 3, 0, None), b"n_pixels=0")
    refused(l.mf_nerf_torso_forward_batch(None, h, to, 3, 480, None), b"null torso handle")
    # ---- frame-out: render 16 x 12 -> 26 x 30 into 36 x 40 body frames
    args = (16, 12, 26, 30, 36, 40, 0)
    refused(l.mf_nerf_frame_batch_out(None, out, 1, *args, fake, None), b"nerf_frame_batch_out: null handle or descriptor table")
    refused(l.mf_nerf_frame_batch_out(h, None, 1, *args, fake, None), b"nerf_frame_batch_out: null handle or descriptor table")
    refused(l.mf_nerf_frame_batch_out(h, out, 0, *args, fake, None), b"n_frames=0 (the handle holds 1..3)")
    refused(l.mf_nerf_frame_batch_out(h, out, 4, *args, fake, None), b"n_frames=4 (the handle holds 1..3)")
    refused(l.mf_nerf_frame_batch_out(h, out, 2, *args, None, None), b"null output")
    refused(l.mf_nerf_frame_batch_out(h, out, 2, 24, 24, 26, 30, 36, 40, 0, fake, None), b"n_pixels=576 exceed the handle's max_pixels 480")
    # a body frame smaller than H x W at (x0, y0): one column, one row past the last legal corner (FW - W, FH - H) = (10, 10); a negative offset; a body too small
    for x0, y0 in ((11, 10), (10, 11), (-1, 0)):
        out[2].x0, out[2].y0 = x0, y0
        refused(l.mf_nerf_frame_batch_out(h, out, 3, *args, fake, None), b"frame 2: a 30 x 26 frame at (%d, %d) leaves the 40 x 36 body frame" % (x0, y0))
    out[2].x0, out[2].y0 = 0, 0
    refused(l.mf_nerf_frame_batch_out(h, out, 3, 16, 12, 26, 30, 25, 40, 0, fake, None), b"frame 0: a 30 x 26 frame at (0, 0) leaves the 40 x 25 body frame")
    out[1].render, out[1].body_bgr = None, None
    refused(l.mf_nerf_frame_batch_out(h, out, 3, *args, fake, None), b"frame 1: neither a render nor a body frame")
    out[1].render = fake                                                               # no body: the block's frames must be the GUI size, the offset 0
    refused(l.mf_nerf_frame_batch_out(h, out, 3, *args, fake, None), b"frame 1: no body frame, and the block's frames are 40 x 36, not 30 x 26")
    out[1].x0 = 1
    refused(l.mf_nerf_frame_batch_out(h, out, 3, *args, fake, None), b"frame 1: an offset (1, 0) without a body frame")


# ---- NerfBatcher's grouping, with stand-ins for the session, the model and the frame batch -----------------------------------------------------------
class _Model:
    FRAME_BATCH = True

    def __init__(self, log):
        self.log = log

    def render_frames(self, jobs, reserve_frames=0, torso_batch=False, **kw):
        self.log.append(("head", len(jobs), torso_batch))
        assert all(j["bg_color"] is not None for j in jobs)
        return [{"image": ("image", j["tag"])} for j in jobs]


class _Session:
    """what NerfBatcher reads of a NerfSession: `hw` the render size, `out` the output size; every frame of audio type (2, 2) is a custom-video frame"""

    def __init__(self, model, tag, hw, out, torso=True, frame_batch=True):
        self.model, self.tag, self.H, self.W, self.GH, self.GW = model, tag, hw[0], hw[1], out[0], out[1]
        self.fullbody_frames, self.custom_img_cycle, self.custom_index, self.render_kw = None, {}, {}, {}
        self.torso_imgs = object() if torso else None
        self.index, self.last_index = 0, None
        if frame_batch:
            self.out_key = lambda: (self.H, self.W, self.GH, self.GW, self.GH, self.GW, False)
            self.bg_key = lambda: (self.H, self.W)
            self.set_background = lambda job, bg: job.update(bg_color=bg)

    def begin(self, auds, audiotype=(0, 0), out=None, defer=False):
        self.last_index = self.index
        self.index += 1
        tag = (self.tag, self.last_index)
        if audiotype == (2, 2):
            if defer:
                return {"custom": ("custom", tag), "mi": self.last_index}
            self.model.log.append(("frame_out alone", tag))
            return out
        return {"rays_o": torch.zeros(self.H * self.W, 3), "bg_color": None if (defer and self.torso_imgs is not None) else "own", "mi": self.last_index, "body": None,
                "tag": tag, "bg_pending": defer and self.torso_imgs is not None}

    def end(self, job, image, out=None):
        self.model.log.append(("end alone", job["tag"]))

    def step(self, auds, audiotype=(0, 0), out=None):
        self.begin(auds, audiotype)
        self.model.log.append(("step", self.tag))

    def bind_aabb(self):
        pass


class _FrameBatch:
    max_frames = 5

    def __init__(self, log):
        self.log = log

    def background(self, sessions, mis):
        self.log.append(("background", [(s.tag, mi) for s, mi in zip(sessions, mis)]))
        return [("bg", s.tag, mi) for s, mi in zip(sessions, mis)]

    def frame_out(self, sessions, images, bodies, out):
        assert out.shape[0] == len(sessions) and all(tuple(out.shape[1:]) == (s.GH, s.GW, 3) for s in sessions)
        self.log.append(("frame_out", [s.tag for s in sessions], [i if i is None else i[1] for i in images], [b if b is None else b[1] for b in bodies], out.data_ptr()))


def _run(monkeypatch, sessions, types, switch=None, **kw):
    from mere_fusion_amd.nerf_serving import NerfBatcher
    if switch is None:
        monkeypatch.delenv("MF_NERF_BATCH", raising=False)
    else:
        monkeypatch.setenv("MF_NERF_BATCH", switch)
    log = sessions[0].model.log
    bat = NerfBatcher(sessions, batch_size=B, device="cpu", **kw)
    monkeypatch.setattr(bat, "_fb", _FrameBatch(log))
    out = bat.step([(torch.zeros(B, 8, 3, 16), types[k]) for k in range(len(sessions))])
    return bat, out, log


def test_batcher_puts_frames_of_unequal_size_in_different_calls(monkeypatch):
    log = []
    m = _Model(log)
    # a and c: 4 x 6 renders to 8 x 10 frames; b: the same ray count, 6 x 4, to 8 x 10; d: 4 x 6 to 9 x 10; e: no torso images; f: a session without the entry points
    ss = [_Session(m, "a", (4, 6), (8, 10)), _Session(m, "b", (6, 4), (8, 10)), _Session(m, "c", (4, 6), (8, 10)), _Session(m, "d", (4, 6), (9, 10)),
          _Session(m, "e", (4, 6), (8, 10), torso=False), _Session(m, "f", (4, 6), (8, 10), frame_batch=False)]
    types = [[(0, 0)] * B, [(0, 0)] * B, [(2, 2), (0, 0)], [(0, 0)] * B, [(0, 0)] * B, [(0, 0), (2, 2)]]
    bat, out, log = _run(monkeypatch, ss, types, torso_batch=True)
    bgs = [e[1] for e in log if e[0] == "background"]
    # one background call per render size: (4, 6) for a, c and d -- c's first frame is a custom-video one and has no background --, (6, 4) for b; e has none
    assert bgs == [[("a", 0), ("a", 1), ("c", 1), ("d", 0), ("d", 1)], [("b", 0), ("b", 1)]]
    assert [e for e in log if e[0] == "head"] == [("head", 10, True)]                 # the head call is grouped by ray count as before: all 24-ray frames
    outs = [e for e in log if e[0] == "frame_out"]
    # per output key one block; a, c and e share (4, 6) -> (8, 10), six frames in slot order cut at max_frames = 5; b and d are alone in theirs
    assert [(e[1], e[2], e[3]) for e in outs] == [
        (["a", "a", "c", "c", "e"], [("a", 0), ("a", 1), None, ("c", 1), ("e", 0)], [None, None, ("c", 0), None, None]),
        (["e"], [("e", 1)], [None]),
        (["b", "b"], [("b", 0), ("b", 1)], [None, None]),
        (["d", "d"], [("d", 0), ("d", 1)], [None, None])]
    # a size's sessions are views of ONE block, neighbours in it; the frame-out calls write where those views are
    fa, fc, fe = out[0][0], out[2][0], out[4][0]
    step = 8 * 10 * 3
    assert fc.data_ptr() == fa.data_ptr() + B * step and fe.data_ptr() == fa.data_ptr() + 2 * B * step and tuple(fa.shape) == (B, 8, 10, 3)
    assert outs[0][4] == fa.data_ptr() and outs[1][4] == fe.data_ptr() + step and outs[2][4] == out[1][0].data_ptr() and outs[3][4] == out[3][0].data_ptr()
    assert tuple(out[3][0].shape) == (B, 9, 10, 3)
    # the session without the entry points keeps its own launches, per frame
    assert ("frame_out alone", ("f", 1)) in log and ("end alone", ("f", 0)) in log and not any("f" in e[1] for e in outs)
    assert [o[1] for o in out] == [[0, 1]] * 6


@pytest.mark.parametrize("how", ["MF_NERF_BATCH=0", "frame_batch=False"])
def test_batcher_keeps_the_per_frame_calls_when_told_to(monkeypatch, how):
    log = []
    m = _Model(log)
    ss = [_Session(m, "a", (4, 6), (8, 10)), _Session(m, "b", (4, 6), (8, 10))]
    types = [[(0, 0)] * B, [(2, 2), (0, 0)]]
    if how == "MF_NERF_BATCH=0":
        _, out, log = _run(monkeypatch, ss, types, switch="0")
        assert log == [("step", "a"), ("step", "a"), ("frame_out alone", ("b", 0)), ("step", "b"), ("step", "b")]
    else:
        _, out, log = _run(monkeypatch, ss, types, frame_batch=False)
        assert log == [("frame_out alone", ("b", 0)), ("head", 3, False), ("end alone", ("a", 0)), ("end alone", ("a", 1)), ("end alone", ("b", 1))]
    assert out[0][0].data_ptr() != out[1][0].data_ptr() and [o[1] for o in out] == [[0, 1]] * 2
