"""PyTorch-ROCm custom ops over the C ABI (include/merefusion.h).

torch is plumbing here: it owns device memory and the current HIP stream; every op hands raw
device pointers to libmerefusion_hip.so.  Ops refuse CPU tensors -- there is no fallback path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _require_cuda(name, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                f"merefusion::{name}: tensor is on {t.device}; the MI355X path needs HIP device tensors "
                "(no CPU fallback is provided)")


@torch.library.custom_op("merefusion::wav2lip_forward", mutates_args=())
def wav2lip_forward(handle: int, mel: torch.Tensor, face: torch.Tensor) -> torch.Tensor:
    """pred = model(mel_batch, img_batch)  (lipreal.py:124-125).  mel [B,1,80,16], face [B,6,96,96]."""
    _require_cuda("wav2lip_forward", mel, face)
    if mel.dim() != 4 or tuple(mel.shape[1:]) != (1, 80, 16):
        raise RuntimeError(f"wav2lip_forward: mel must be [B,1,80,16], got {tuple(mel.shape)}")
    if face.dim() != 4 or tuple(face.shape[1:]) != (6, 96, 96) or face.shape[0] != mel.shape[0]:
        raise RuntimeError(f"wav2lip_forward: face must be [B,6,96,96] with B={mel.shape[0]}, got {tuple(face.shape)}")
    mel = mel.contiguous().float()
    face = face.contiguous().float()
    B = mel.shape[0]
    out = torch.empty((B, 3, 96, 96), dtype=torch.float32, device=mel.device)
    if B == 0:
        return out
    with torch.cuda.device(mel.device):
        _lib.check(_lib.lib().mf_wav2lip_forward(handle, mel.data_ptr(), face.data_ptr(), out.data_ptr(), B,
                                                 _lib.stream_ptr(mel.device)), "wav2lip_forward")
    return out


@wav2lip_forward.register_fake
def _(handle, mel, face):
    return mel.new_empty((mel.shape[0], 3, 96, 96), dtype=torch.float32)


@torch.library.custom_op("merefusion::wav2lip_forward_u8", mutates_args=())
def wav2lip_forward_u8(handle: int, mel: torch.Tensor, faces_u8: torch.Tensor) -> torch.Tensor:
    """lipreal.py:115-126 fused: uint8 [B,96,96,3] BGR crops + mel [B,1,80,16] -> fp32 [B,96,96,3] = pred*255."""
    _require_cuda("wav2lip_forward_u8", mel, faces_u8)
    if faces_u8.dtype != torch.uint8 or faces_u8.dim() != 4 or tuple(faces_u8.shape[1:]) != (96, 96, 3):
        raise RuntimeError(f"wav2lip_forward_u8: faces must be uint8 [B,96,96,3], got {faces_u8.dtype} {tuple(faces_u8.shape)}")
    if mel.dim() != 4 or tuple(mel.shape[1:]) != (1, 80, 16) or mel.shape[0] != faces_u8.shape[0]:
        raise RuntimeError(f"wav2lip_forward_u8: mel must be [B,1,80,16], got {tuple(mel.shape)}")
    mel = mel.contiguous().float()
    faces_u8 = faces_u8.contiguous()
    B = mel.shape[0]
    out = torch.empty((B, 96, 96, 3), dtype=torch.float32, device=mel.device)
    if B == 0:
        return out
    with torch.cuda.device(mel.device):
        _lib.check(_lib.lib().mf_wav2lip_forward_u8(handle, mel.data_ptr(), faces_u8.data_ptr(), out.data_ptr(), B,
                                                    _lib.stream_ptr(mel.device)), "wav2lip_forward_u8")
    return out


@wav2lip_forward_u8.register_fake
def _(handle, mel, faces_u8):
    return mel.new_empty((mel.shape[0], 96, 96, 3), dtype=torch.float32)


@torch.library.custom_op("merefusion::melspec", mutates_args=())
def melspec(wav: torch.Tensor, pad_mode: int) -> torch.Tensor:
    """audio.melspectrogram (wav2lip/audio.py:45-51): fp32 [n] -> fp32 [80, 1 + n//200]."""
    _require_cuda("melspec", wav)
    if wav.dim() != 1:
        raise RuntimeError(f"melspec: wav must be 1-D, got {tuple(wav.shape)}")
    wav = wav.contiguous().float()
    n = wav.shape[0]
    T = _lib.lib().mf_melspec_frames(n)
    out = torch.empty((80, T), dtype=torch.float32, device=wav.device)
    with torch.cuda.device(wav.device):
        _lib.check(_lib.lib().mf_melspec(wav.data_ptr(), n, out.data_ptr(), int(pad_mode), _lib.stream_ptr(wav.device)),
                   "melspec")
    return out


@melspec.register_fake
def _(wav, pad_mode):
    return wav.new_empty((80, 1 + wav.shape[0] // 200), dtype=torch.float32)


def wav2lip_forward_u8_rows(handle, mel, face_pool, rows):
    """wav2lip_forward_u8 with the faces picked from a pool: face_pool uint8 [n,96,96,3] on the device (every session's cached crops), rows the host list of
    pool rows, one per mel chunk -- batch row b is generated from face_pool[rows[b]] without a gather in between (mf_wav2lip_forward_u8_rows).  A plain
    function, not a custom op: `rows` is a host list that changes every step."""
    _require_cuda("wav2lip_forward_u8_rows", mel, face_pool)
    if face_pool.dtype != torch.uint8 or face_pool.dim() != 4 or tuple(face_pool.shape[1:]) != (96, 96, 3):
        raise RuntimeError(f"wav2lip_forward_u8_rows: the pool must be uint8 [n,96,96,3], got {face_pool.dtype} {tuple(face_pool.shape)}")
    rows = [int(r) for r in rows]
    if mel.dim() != 4 or tuple(mel.shape[1:]) != (1, 80, 16) or mel.shape[0] != len(rows):
        raise RuntimeError(f"wav2lip_forward_u8_rows: mel must be [B,1,80,16] with B = {len(rows)} rows, got {tuple(mel.shape)}")
    mel = mel.contiguous().float()
    face_pool = face_pool.contiguous()
    B = len(rows)
    out = torch.empty((B, 96, 96, 3), dtype=torch.float32, device=mel.device)
    if B == 0:
        return out
    with torch.cuda.device(mel.device):
        _lib.check(_lib.lib().mf_wav2lip_forward_u8_rows(handle, mel.data_ptr(), face_pool.data_ptr(), face_pool.shape[0], (C.c_int * B)(*rows),
                                                         out.data_ptr(), B, _lib.stream_ptr(mel.device)), "wav2lip_forward_u8_rows")
    return out


def melspec_windows(wav, starts, pad_mode, out=None):
    """The mel chunks of many LipASR.run_steps in one launch (lipasr.py:24-35): wav fp32 [n_windows, n] on the device, one sliding window per row; starts the
    host list lip_driver.mel_chunk_starts returns for n -> fp32 [n_windows * len(starts), 1, 80, 16], window-major (mf_melspec_windows)."""
    _require_cuda("melspec_windows", wav)
    if wav.dim() != 2:
        raise RuntimeError(f"melspec_windows: wav must be [n_windows, n], got {tuple(wav.shape)}")
    wav = wav.contiguous().float()
    nw, n = wav.shape
    starts = [int(v) for v in starts]
    shape = (nw * len(starts), 1, 80, 16)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=wav.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError(f"melspec_windows: out must be a contiguous fp32 device tensor {shape}, got {out.dtype} {tuple(out.shape)}")
    with torch.cuda.device(wav.device):
        _lib.check(_lib.lib().mf_melspec_windows(wav.data_ptr(), n, nw, (C.c_int * len(starts))(*starts), len(starts), out.data_ptr(), int(pad_mode),
                                                 _lib.stream_ptr(wav.device)), "melspec_windows")
    return out


def windows_push(buf, rows, new, out=None):
    """The sliding windows of one step's sessions, pushed by one launch (mf_windows_push, csrc/mf_window_push.hip): buf contiguous fp32 [N, n] on the device (every
    session's window), rows a host list of m distinct rows of it, new contiguous fp32 [m, n_new] on the device (n_new <= n) -> for every i
    buf[rows[i]] = concat(buf[rows[i]][n_new:], new[i]), and out fp32 [m, n] (created when None) holds the same m windows.  Rows that `rows` does not name keep
    their bytes.  The row list travels in the launch arguments: no index tensor.  Refuses before anything is enqueued."""
    for name, t in (("buf", buf), ("new", new)):
        if not torch.is_tensor(t):
            raise RuntimeError(f"windows_push: {name} must be a contiguous fp32 device tensor, got {type(t).__name__}")
    _require_cuda("windows_push", buf, new)
    rows = [int(r) for r in rows]
    m = len(rows)
    if m == 0:
        raise RuntimeError("windows_push: no rows (at least one window moves in a push)")
    if buf.dtype != torch.float32 or buf.dim() != 2 or not buf.is_contiguous():
        raise RuntimeError(f"windows_push: buf must be contiguous fp32 [N, n], got {buf.dtype} {tuple(buf.shape)}{'' if buf.is_contiguous() else ' (not contiguous)'}")
    N, n = int(buf.shape[0]), int(buf.shape[1])
    if new.dtype != torch.float32 or new.dim() != 2 or not new.is_contiguous() or new.shape[0] != m or not 1 <= new.shape[1] <= n or new.device != buf.device:
        raise RuntimeError(f"windows_push: new must be contiguous fp32 [{m}, n_new] with 1 <= n_new <= {n} on {buf.device}, got {new.dtype} {tuple(new.shape)} on "
                           f"{new.device}{'' if new.is_contiguous() else ' (not contiguous)'}")
    bad = [r for r in rows if not 0 <= r < N]
    if bad:
        raise RuntimeError(f"windows_push: rows {bad} are out of range: the pool has rows 0 to {N - 1}")
    if len(set(rows)) != m:
        raise RuntimeError(f"windows_push: a row appears twice in {rows}")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=buf.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_cuda and out.device == buf.device and out.is_contiguous() and tuple(out.shape) == (m, n)):
        what = f"{out.dtype} {tuple(out.shape)} on {out.device}" if torch.is_tensor(out) else type(out).__name__
        raise RuntimeError(f"windows_push: out must be a contiguous fp32 tensor {(m, n)} on {buf.device}, got {what}")
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().mf_windows_push(buf.data_ptr(), N, n, new.data_ptr(), int(new.shape[1]), (C.c_int * m)(*rows), m, out.data_ptr(),
                                              _lib.stream_ptr(buf.device)), "windows_push")
    return out


FRAME_ORDERS = {"bgr": 0, "rgb": 1}


def frames_to_i420(frames, order="bgr", out=None):
    """Finished packed frames as planar YUV 4:2:0 in one launch (mf_frames_to_i420; the integers are in csrc/mf_i420.hip): frames contiguous uint8 [B, H, W, 3] or
    [H, W, 3] on the device, channels in `order` ("bgr": the paste-back's frames, "rgb": ER-NeRF's) -> uint8 [B, H * 3 / 2, W] or [H * 3 / 2, W], per frame the
    array `VideoFrame.from_ndarray(a, format="yuv420p")` takes.  H and W must be even.  out: the contiguous uint8 device tensor of that shape to write."""
    if not torch.is_tensor(frames):
        raise RuntimeError(f"frames_to_i420: expected a uint8 device tensor, got {type(frames).__name__}")
    _require_cuda("frames_to_i420", frames)
    if order not in FRAME_ORDERS:
        raise RuntimeError(f"frames_to_i420: order must be 'bgr' or 'rgb', got {order!r}")
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise RuntimeError(f"frames_to_i420: frames must be contiguous uint8 [B, H, W, 3] or [H, W, 3], got {frames.dtype} {tuple(frames.shape)}"
                           f"{'' if frames.is_contiguous() else ' (not contiguous)'}")
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    B = int(frames.shape[0]) if frames.dim() == 4 else 1
    if H % 2 or W % 2:
        raise RuntimeError(f"frames_to_i420: frame size {H} x {W} (H x W) is odd; 4:2:0 chroma covers 2 x 2 blocks")
    if B < 1 or H < 2 or W < 2:
        raise RuntimeError(f"frames_to_i420: nothing to convert in {tuple(frames.shape)}")
    shape = ((B,) if frames.dim() == 4 else ()) + (H * 3 // 2, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.is_cuda and out.device == frames.device and out.is_contiguous() and tuple(out.shape) == shape):
        what = f"{out.dtype} {tuple(out.shape)} on {out.device}" if torch.is_tensor(out) else type(out).__name__
        raise RuntimeError(f"frames_to_i420: out must be a contiguous uint8 tensor {shape} on {frames.device}, got {what}")
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().mf_frames_to_i420(frames.data_ptr(), B, H, W, FRAME_ORDERS[order], out.data_ptr(), _lib.stream_ptr(frames.device)), "frames_to_i420")
    return out


FRAME_FORMATS = {"packed": 0, "i420": 1}


def gather_frames(sources, dst, out, fmt="packed", order="bgr"):
    """Finished frames from anywhere into chosen frames of one block, in one call (mf_frames_gather, csrc/mf_frame_gather.hip): sources a list of contiguous uint8
    [H, W, 3] device tensors or views -- a cached avatar frame, a frame of a custom cycle; they need not share an allocation -- and dst, one int per source: source i
    becomes frame dst[i] of `out`, contiguous uint8 [N, H, W, 3] (fmt "packed": a copy) or [N, H * 3 / 2, W] (fmt "i420": the bytes frames_to_i420 gives for the
    same pixels, channels in `order`; H and W even).  Frames of `out` that dst does not name keep their bytes; two sources with one dst are refused.  Returns out."""
    if fmt not in FRAME_FORMATS:
        raise RuntimeError(f"gather_frames: fmt must be 'packed' or 'i420', got {fmt!r}")
    if order not in FRAME_ORDERS:
        raise RuntimeError(f"gather_frames: order must be 'bgr' or 'rgb', got {order!r}")
    sources, dst = list(sources), [int(d) for d in dst]
    if not sources or len(sources) != len(dst):
        raise RuntimeError(f"gather_frames: {len(sources)} sources for {len(dst)} destination frames (at least one, and one dst per source)")
    if not torch.is_tensor(out):
        raise RuntimeError(f"gather_frames: out must be a uint8 device tensor, got {type(out).__name__}")
    _require_cuda("gather_frames", out)
    for i, t in enumerate(sources):
        if not torch.is_tensor(t):
            raise RuntimeError(f"gather_frames: source {i}: expected a uint8 device tensor, got {type(t).__name__}")
        _require_cuda("gather_frames", t)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous() or t.shape != sources[0].shape or t.device != out.device:
            raise RuntimeError(f"gather_frames: source {i} must be contiguous uint8 [H, W, 3] on {out.device} like source 0 {tuple(sources[0].shape)}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ' (not contiguous)'}")
    H, W = int(sources[0].shape[0]), int(sources[0].shape[1])
    if fmt == "i420" and (H % 2 or W % 2):
        raise RuntimeError(f"gather_frames: frame size {H} x {W} (H x W) is odd; 4:2:0 chroma covers 2 x 2 blocks")
    want = (H * 3 // 2, W) if fmt == "i420" else (H, W, 3)
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != len(want) + 1 or tuple(out.shape[1:]) != want or out.shape[0] < 1:
        raise RuntimeError(f"gather_frames: out must be a contiguous uint8 tensor [N, {', '.join(str(v) for v in want)}] for {H} x {W} frames as {fmt}, got {out.dtype} "
                           f"{tuple(out.shape)}{'' if out.is_contiguous() else ' (not contiguous)'}")
    N = int(out.shape[0])
    bad = [d for d in dst if not 0 <= d < N]
    if bad or len(set(dst)) != len(dst):
        raise RuntimeError(f"gather_frames: dst {dst} must name distinct frames of out, 0 to {N - 1}")
    srcs = (_lib.MfFrameSrc * len(sources))()
    for s, t, d in zip(srcs, sources, dst):
        s.frame, s.dst = t.data_ptr(), d
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().mf_frames_gather(srcs, len(sources), H, W, FRAME_FORMATS[fmt], FRAME_ORDERS[order], out.data_ptr(), N, _lib.stream_ptr(out.device)),
                   "frames_gather")
    return out


def lanczos4_tables(ssize, dsize):
    """One axis of cv::resize's INTER_LANCZOS4 tables for 8-bit images (imgproc/src/resize.cpp, OpenCV 4.x as published): -> (ofs int32 [dsize], coef int16
    [dsize, 8]).  Position fx = (float)((d + 0.5) * scale - 0.5), scale = 1 / (dsize / ssize) in double; s = floor(fx); tap k reads source index ofs + k with
    ofs = s - 3 (clamped to the image by whoever applies the table); coefficients from `interpolateLanczos4(fx - s)`: float32 values from the eight-entry cos / sin
    rotation table, 1e30 where the argument is (nearly) zero, normalised by their float32 sum, then saturate_cast<short>(c * 2048) (round half to even).
    Built on the host so that the device resampler is integer-only (mf_crop_resize.hip)."""
    f32, f64 = np.float32, np.float64
    ssize, dsize = int(ssize), int(dsize)
    if ssize < 1 or dsize < 1:
        raise ValueError(f"lanczos4_tables: sizes must be positive, got {ssize} -> {dsize}")
    scale = f64(1.0) / (f64(dsize) / f64(ssize))
    fx = ((np.arange(dsize, dtype=f64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(fx).astype(np.int64)
    x = (fx - s.astype(f32)).astype(f32)                                  # fx -= sx, in float
    s45 = 0.70710678118654752440084436210485
    cs = np.array([[1, 0], [-s45, -s45], [0, 1], [s45, -s45], [-1, 0], [s45, s45], [0, -1], [-s45, s45]], dtype=f64)
    x3 = (x + f32(3)).astype(f32)
    y0 = -x3.astype(f64) * np.pi * 0.25
    s0, c0 = np.sin(y0), np.cos(y0)
    coef = np.empty((dsize, 8), dtype=f32)
    total = np.zeros(dsize, dtype=f32)
    for i in range(8):
        yi = (x3 - f32(i)).astype(f32)
        y = -yi.astype(f64) * np.pi * 0.25
        with np.errstate(divide="ignore", invalid="ignore"):
            c = ((cs[i, 0] * s0 + cs[i, 1] * c0) / (y * y)).astype(f32)
        coef[:, i] = np.where(np.abs(yi) >= f32(1e-6), c, f32(1e30))
        total = (total + coef[:, i]).astype(f32)
    coef = (coef * (f32(1.0) / total).astype(f32)[:, None]).astype(f32)
    q = np.clip(np.rint((coef * f32(2048.0)).astype(f32)), -32768, 32767).astype(np.int16)
    return (s - 3).astype(np.int32), q


def crop_resize_u8(frames, boxes, size, mode="linear", frame_indices=None, out=None):
    """Batched crop + resize in one launch (mf_crop_resize_u8): frames contiguous uint8 [n, H, W, 3] on the device -> uint8 [n_jobs, dh, dw, 3].
    size: the destination as cv2.resize's dsize (dw, dh), or one int for a square.
    boxes: a host list of n_jobs (x1, y1, x2, y2) crops, box i cut from frame frame_indices[i] (default i); or a device int32 tensor [n_jobs, 5] of
    (frame_index, x1, y1, x2, y2) rows, as mf_avatar_lip_boxes writes (nothing is copied to the host; a row that is empty or outside the frame gives a zeroed crop).
    mode "linear": cv2.resize's default INTER_LINEAR (mf_blend.hip's arithmetic), coefficients formed on the device.  mode "lanczos4": cv2.resize(...,
    interpolation=cv2.INTER_LANCZOS4) as the integer two-pass on `lanczos4_tables`; the tables are built here from the boxes, which therefore must be host values.
    out: the contiguous uint8 device tensor [n_jobs, dh, dw, 3] to write (a slice of a larger block is fine)."""
    if not torch.is_tensor(frames):
        raise RuntimeError(f"crop_resize_u8: expected a uint8 device tensor, got {type(frames).__name__}")
    _require_cuda("crop_resize_u8", frames)
    if mode not in _lib.CROP_MODES:
        raise RuntimeError(f"crop_resize_u8: mode must be 'linear' or 'lanczos4', got {mode!r}")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise RuntimeError(f"crop_resize_u8: frames must be contiguous uint8 [n, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
    dw, dh = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    dev = frames.device
    n, H, W = (int(v) for v in frames.shape[:3])
    tables = [None] * 4
    if torch.is_tensor(boxes):
        if mode != "linear":
            raise RuntimeError("crop_resize_u8: lanczos4 builds its tables on the host from the boxes; pass them as a host list")
        if not (boxes.is_cuda and boxes.device == dev and boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 5 and boxes.is_contiguous()):
            raise RuntimeError(f"crop_resize_u8: a device job table must be contiguous int32 [n_jobs, 5] on {dev}, got {boxes.dtype} {tuple(boxes.shape)} on {boxes.device}")
        jobs_dev, jobs_host, n_jobs = boxes, None, int(boxes.shape[0])
    else:
        rows = [tuple(int(v) for v in b) for b in boxes]
        idx = list(range(len(rows))) if frame_indices is None else [int(i) for i in frame_indices]
        if len(idx) != len(rows) or any(len(r) != 4 for r in rows):
            raise RuntimeError("crop_resize_u8: one (x1, y1, x2, y2) box and one frame index per crop")
        n_jobs = len(rows)
        jobs_host = (_lib.MfCropJob * max(n_jobs, 1))()
        for k, (f, r) in enumerate(zip(idx, rows)):
            jobs_host[k].frame_index, jobs_host[k].x1, jobs_host[k].y1, jobs_host[k].x2, jobs_host[k].y2 = (f,) + r
        flat = np.array([(f,) + r for f, r in zip(idx, rows)], dtype=np.int32).reshape(n_jobs, 5)
        jobs_dev = torch.from_numpy(flat).to(dev)
        if mode == "lanczos4" and dh >= 1 and dw >= 1 and all(r[2] > r[0] and r[3] > r[1] for r in rows):
            memo = {}

            def axis(ssize, dsize):
                if (ssize, dsize) not in memo:
                    memo[(ssize, dsize)] = lanczos4_tables(ssize, dsize)
                return memo[(ssize, dsize)]

            xs = [axis(r[2] - r[0], dw) for r in rows]
            ys = [axis(r[3] - r[1], dh) for r in rows]
            tables = [torch.from_numpy(np.ascontiguousarray(np.stack(t))).to(dev) for t in ([a[0] for a in xs], [a[1] for a in xs], [a[0] for a in ys], [a[1] for a in ys])]
        elif mode == "lanczos4":                       # an argument the entry point refuses below, before any launch: it needs non-null tables to say so
            tables = [jobs_dev] * 4
    shape = (n_jobs, dh, dw, 3)
    if out is None:
        out = torch.empty(tuple(max(v, 0) for v in shape), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.is_cuda and out.device == dev and out.is_contiguous() and tuple(out.shape) == shape):
        what = f"{out.dtype} {tuple(out.shape)} on {out.device}" if torch.is_tensor(out) else type(out).__name__
        raise RuntimeError(f"crop_resize_u8: out must be a contiguous uint8 tensor {shape} on {dev}, got {what}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mf_crop_resize_u8(frames.data_ptr(), n, H, W, jobs_dev.data_ptr(), jobs_host, n_jobs, out.data_ptr(), dh, dw, _lib.CROP_MODES[mode],
                                                *[None if t is None else t.data_ptr() for t in tables], _lib.stream_ptr(dev)), "crop_resize_u8")
    return out


def _ints(v):
    v = [int(x) for x in v]
    return (C.c_int * len(v))(*v), len(v)


def _fp32_pool(name, what, t, tail):
    if not (t.dtype == torch.float32 and t.is_contiguous() and t.dim() == len(tail) + 1 and tuple(t.shape[1:]) == tuple(tail)):
        raise RuntimeError(f"{name}: {what} must be a contiguous fp32 tensor [N, {', '.join(str(v) for v in tail)}], got {t.dtype} {tuple(t.shape)}")


def nerf_feat_scatter(feats, left, right, rings, rows, starts):
    """nerfasr.py:119-124 for many sessions in one launch: rows [left, right) of feats[i] (the net's output [S, T, dim] for the S picked sessions) into ring
    rows starts[i]... of session rows[i] of rings [N, R, dim] (mf_nerf_feat_scatter).  rows / starts are host lists.  In place; returns nothing."""
    _require_cuda("nerf_feat_scatter", feats, rings)
    if feats.dim() != 3 or rings.dim() != 3 or feats.shape[2] != rings.shape[2]:
        raise RuntimeError(f"nerf_feat_scatter: feats [S, T, dim] and rings [N, R, dim] must share dim, got {tuple(feats.shape)} and {tuple(rings.shape)}")
    _fp32_pool("nerf_feat_scatter", "rings", rings, rings.shape[1:])
    feats = feats.contiguous().float()
    crows, S = _ints(rows)
    cstarts, n = _ints(starts)
    if S != feats.shape[0] or n != S:
        raise RuntimeError(f"nerf_feat_scatter: {S} rows and {n} starts for {feats.shape[0]} slices of the net output")
    with torch.cuda.device(rings.device):
        _lib.check(_lib.lib().mf_nerf_feat_scatter(feats.data_ptr(), S, feats.shape[1], feats.shape[2], int(left), int(right), rings.data_ptr(), rings.shape[0],
                                                   rings.shape[1], crows, cstarts, _lib.stream_ptr(rings.device)), "nerf_feat_scatter")


def nerf_feat_windows(rings, hist, rows, fronts, heads, n_new, att, out=None):
    """nerfasr.py:75-103 for many sessions in one launch (mf_nerf_feat_windows): rings [N, R, dim], hist [N, 8, dim, 16] (None with att == 0); rows, heads,
    n_new host lists, one value per picked session; fronts one list per session of the ring rows its 8 (or 1) windows start at, oldest first, -1 for a zero
    window -> fp32 [S, 8 or 1, dim, 16], the sessions' `auds`.  The history is updated in place."""
    _require_cuda("nerf_feat_windows", rings)
    if rings.dim() != 3:
        raise RuntimeError(f"nerf_feat_windows: rings must be [N, R, dim], got {tuple(rings.shape)}")
    N, R, dim = rings.shape
    _fp32_pool("nerf_feat_windows", "rings", rings, (R, dim))
    if att:
        if hist is None:
            raise RuntimeError("nerf_feat_windows: att > 0 needs the history [N, 8, dim, 16]")
        _require_cuda("nerf_feat_windows", hist)
        _fp32_pool("nerf_feat_windows", "hist", hist, (8, dim, 16))
        if hist.shape[0] != N:
            raise RuntimeError(f"nerf_feat_windows: {hist.shape[0]} histories for {N} rings")
    crows, S = _ints(rows)
    shape = (S, 8 if att else 1, dim, 16)
    fronts = [list(f) for f in fronts]
    if any(len(f) != shape[1] for f in fronts):
        raise RuntimeError(f"nerf_feat_windows: every session needs the fronts of its {shape[1]} windows")
    lists = [_ints(v for f in fronts for v in f), _ints(heads if att else [0] * S), _ints(n_new)]
    if [n for _, n in lists] != [S * shape[1], S, S]:
        raise RuntimeError(f"nerf_feat_windows: {S} rows, {len(fronts)} lists of fronts, {lists[1][1]} heads, {lists[2][1]} n_new")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rings.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise RuntimeError(f"nerf_feat_windows: out must be a contiguous fp32 device tensor {shape}, got {out.dtype} {tuple(out.shape)}")
    with torch.cuda.device(rings.device):
        _lib.check(_lib.lib().mf_nerf_feat_windows(rings.data_ptr(), hist.data_ptr() if att else None, N, R, dim, S, crows, lists[0][0], lists[1][0], lists[2][0],
                                                   int(bool(att)), out.data_ptr(), _lib.stream_ptr(rings.device)), "nerf_feat_windows")
    return out


def nerf_feat_rows_load(rings, hist, rows, src_ring=None, src_hist=None):
    """A session joins, starts again or is reset (mf_nerf_feat_rows_load): rows `rows` (a host list) of rings [N, R, dim] are written from src_ring [R, dim]
    and, where hist [N, 8, dim, 16] is not None, of hist from src_hist [8, dim, 16]; a source of None writes zeros.  ONE launch for all rows; a source may be a
    view of another row of the same tensors, not of a named one.  In place; returns nothing."""
    _require_cuda("nerf_feat_rows_load", rings)
    if rings.dim() != 3:
        raise RuntimeError(f"nerf_feat_rows_load: rings must be [N, R, dim], got {tuple(rings.shape)}")
    N, R, dim = rings.shape
    _fp32_pool("nerf_feat_rows_load", "rings", rings, (R, dim))
    if hist is None and src_hist is not None:
        raise RuntimeError("nerf_feat_rows_load: a history source without a history (att == 0 keeps none)")
    if hist is not None:
        _require_cuda("nerf_feat_rows_load", hist)
        _fp32_pool("nerf_feat_rows_load", "hist", hist, (8, dim, 16))
        if hist.shape[0] != N:
            raise RuntimeError(f"nerf_feat_rows_load: {hist.shape[0]} histories for {N} rings")
    for what, src, shape in (("src_ring", src_ring, (R, dim)), ("src_hist", src_hist, (8, dim, 16))):
        if src is None:
            continue
        _require_cuda("nerf_feat_rows_load", src)
        if not (src.dtype == torch.float32 and src.is_contiguous() and tuple(src.shape) == shape and src.device == rings.device):
            raise RuntimeError(f"nerf_feat_rows_load: {what} must be a contiguous fp32 tensor {shape} on {rings.device}, got {src.dtype} {tuple(src.shape)} on "
                               f"{src.device}")
    crows, S = _ints(rows)
    with torch.cuda.device(rings.device):
        _lib.check(_lib.lib().mf_nerf_feat_rows_load(rings.data_ptr(), None if hist is None else hist.data_ptr(), N, R, dim, S, crows,
                                                     None if src_ring is None else src_ring.data_ptr(), None if src_hist is None else src_hist.data_ptr(),
                                                     _lib.stream_ptr(rings.device)), "nerf_feat_rows_load")


# ---- MuseTalk / Whisper stages as custom ops too (the drop-in modules call these; handles are the C ABI's opaque pointers) ----------
@torch.library.custom_op("merefusion::unet_forward", mutates_args=())
def unet_forward(handle: int, latents: torch.Tensor, audio: torch.Tensor, add_pe: bool, out_channels: int) -> torch.Tensor:
    """unet.model(latent_batch, timesteps=[0], encoder_hidden_states=audio).sample (musereal.py:105-107): latents [B,8,S,S], audio [B,T,384]
    (+ the positional encoding of unet.py:12-27 when add_pe) -> [B,4,S,S] fp32."""
    _require_cuda("unet_forward", latents, audio)
    if latents.dim() != 4 or audio.dim() != 3 or audio.shape[0] != latents.shape[0]:
        raise RuntimeError(f"unet_forward: latents [B,C,S,S] and audio [B,T,D] expected, got {tuple(latents.shape)} / {tuple(audio.shape)}")
    lat, aud = latents.contiguous().float(), audio.contiguous().float()
    B = lat.shape[0]
    out = torch.empty((B, out_channels, lat.shape[2], lat.shape[3]), dtype=torch.float32, device=lat.device)
    if B == 0:
        return out
    with torch.cuda.device(lat.device):
        _lib.check(_lib.lib().mf_unet_forward(handle, lat.data_ptr(), aud.data_ptr(), int(add_pe), out.data_ptr(), B, _lib.stream_ptr(lat.device)),
                   "unet_forward")
    return out


@unet_forward.register_fake
def _(handle, latents, audio, add_pe, out_channels):
    return latents.new_empty((latents.shape[0], out_channels, latents.shape[2], latents.shape[3]), dtype=torch.float32)


@torch.library.custom_op("merefusion::vae_decode_latents", mutates_args=())
def vae_decode_latents(handle: int, latents: torch.Tensor) -> torch.Tensor:
    """VAE.decode_latents (musetalk/models/vae.py:96-108) up to the host copy: latents [B,4,S,S] -> uint8 BGR frames [B,8S,8S,3] on the device."""
    _require_cuda("vae_decode_latents", latents)
    if latents.dim() != 4:
        raise RuntimeError(f"vae_decode_latents: latents [B,4,S,S] expected, got {tuple(latents.shape)}")
    lat = latents.contiguous().float()
    B, S = lat.shape[0], lat.shape[2] * 8
    frames = torch.empty((B, S, S, 3), dtype=torch.uint8, device=lat.device)
    if B == 0:
        return frames
    with torch.cuda.device(lat.device):
        _lib.check(_lib.lib().mf_vae_decode_latents(handle, lat.data_ptr(), frames.data_ptr(), None, B, _lib.stream_ptr(lat.device)), "vae_decode_latents")
    return frames


@vae_decode_latents.register_fake
def _(handle, latents):
    return latents.new_empty((latents.shape[0], latents.shape[2] * 8, latents.shape[3] * 8, 3), dtype=torch.uint8)


@torch.library.custom_op("merefusion::whisper_encode_windows", mutates_args=())
def whisper_encode_windows(handle: int, wavs: torch.Tensor, ctx_tokens: int, n_layers1: int, n_state: int) -> torch.Tensor:
    """Audio2Feature.audio2feat for S windows in one encoder call (museasr.py:25-26 -> audio2feature.py:99-112): wavs fp32 [S, n] ->
    [S, n // 320, n_layer + 1, n_state].  The handle's workspace must hold S windows (mf_whisper_set_batch)."""
    _require_cuda("whisper_encode_windows", wavs)
    if wavs.dim() != 2:
        raise RuntimeError(f"whisper_encode_windows: wavs [S, n] expected, got {tuple(wavs.shape)}")
    w = wavs.contiguous().float()
    S, n = w.shape
    feat = torch.empty((S, n // 320, n_layers1, n_state), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(_lib.lib().mf_whisper_encode_windows(handle, w.data_ptr(), n, S, int(ctx_tokens), feat.data_ptr(), _lib.stream_ptr(w.device)),
                   "whisper_encode_windows")
    return feat


@whisper_encode_windows.register_fake
def _(handle, wavs, ctx_tokens, n_layers1, n_state):
    return wavs.new_empty((wavs.shape[0], wavs.shape[1] // 320, n_layers1, n_state), dtype=torch.float32)
